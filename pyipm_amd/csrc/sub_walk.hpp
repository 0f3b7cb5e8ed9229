// sub_walk.hpp -- the one walk over the sub-panels of a wide panel.  Plain C++: nothing of HIP or of the handle in it.
#pragma once
namespace pyipm {
// The sub-panels of a panel of pw columns at sub-width sw, first to last or last first: f(off, nbw) for the nbw columns at
// column offset off (the last sub-panel may be narrower).  f returns an int; the first non-zero one ends the walk.
template <class F>
inline int walk_sub(int pw, int sw, bool last_first, F f) {
    const int nsub = (pw + sw - 1) / sw;
    for (int i = 0; i < nsub; ++i) {
        const int off = (last_first ? nsub - 1 - i : i) * sw;
        const int rc = f(off, pw - off < sw ? pw - off : sw);
        if (rc) return rc;
    }
    return 0;
}
}  // namespace pyipm
