// fwd_range_plan.hpp -- who subtracts what from whom in the one-launch forward sweep over the panels [Pa, Pb) (k_fwd_range,
// kernels_solve.hpp), and what each side waits for.  Plain C++: nothing of HIP or of the handle in it; the functions are
// constexpr so that host code, the kernel and a stand-alone replay (tests/test_fwd_range_plan.py) all compile this one source.
// (k_fwd_prefix keeps its own, older text; with Pa = 0 inside the x block these functions state its rule, and the replay says so.)
#pragma once
#include <cstdint>
namespace pyipm {
constexpr int FWD_PLAN_TB = 64;          // rows of a chunk (= TB, ctx.hpp)
struct FwdPlanGeo { int64_t Npad, n, mi, me; int nb, skip; };

// can L[rows [r0, r1), columns [cA, cB) of one panel] be non-zero?  (active_ranges, pyipm_newton.hip: KKT order [x | s | lambda_e |
// lambda_i]; x columns have exact zeros in the s rows, s columns touch the matching lambda_i rows only)
constexpr bool fwd_plan_cols_active(const FwdPlanGeo& g, int64_t cA, int64_t cB, int64_t r0, int64_t r1) {
    if (!g.skip || g.mi == 0) return true;
    const int64_t s0 = g.n, s1 = g.n + g.mi, i0 = g.n + g.mi + g.me;
    if (cB <= s0) return (r0 < s0) || (r1 > s1);
    if (cA >= s0 && cB <= s1) return r1 > i0 + (cA - s0) && r0 < i0 + (cB - s0);
    return true;
}
// does panel s subtract anything from the 64-row chunk c?  The chunk lies below the panel and its 256-row launch block of
// k_fwd_gemv (blocks are counted from the panel's end) is not skipped there.
constexpr bool fwd_plan_visit(const FwdPlanGeo& g, int s, int c) {
    const int64_t row_begin = (int64_t)(s + 1) * g.nb, r0 = (int64_t)c * FWD_PLAN_TB;
    if (r0 < row_begin || r0 >= g.Npad) return false;
    const int64_t i0 = row_begin + (r0 - row_begin) / 256 * 256;
    return fwd_plan_cols_active(g, (int64_t)s * g.nb, row_begin, i0, i0 + 256);
}
// the last panel of [Pa, s) that subtracts from chunk c, or -1 where none does
constexpr int fwd_plan_last(const FwdPlanGeo& g, int Pa, int s, int c) {
    for (int p = s - 1; p >= Pa; --p) if (fwd_plan_visit(g, p, c)) return p;
    return -1;
}
// A launch over [Pa, Pb).  The chain, for chunk c of panel s: it waits for prog[c] >= fwd_plan_last(Pa, s, c) + 1, or not at all
// where that is -1.  The owner of chunk c, at panel s: the visit is FINAL -- the chunk goes to memory and prog[c] := s + 1 --
// where the chunk lies inside the range and s is the last panel that reaches it.
constexpr int fwd_plan_chain_waits(const FwdPlanGeo& g, int Pa, int s, int c) { return fwd_plan_last(g, Pa, s, c); }
constexpr bool fwd_plan_final(const FwdPlanGeo& g, int Pa, int Pb, int s, int c) {
    const int pc = c / (g.nb / FWD_PLAN_TB);
    return pc < Pb && fwd_plan_last(g, Pa, pc, c) == s;
}
// is chunk c owned in the launch over [Pa, Pb)?  Only chunks that some panel of the range reaches are numbered (ascending; number m
// goes to workgroup 1 + m mod (grid - 1)): a chunk nobody reaches has no owner, is waited for by nobody and keeps what memory holds.
constexpr bool fwd_plan_owned(const FwdPlanGeo& g, int Pa, int Pb, int c) {
    const int pc = c / (g.nb / FWD_PLAN_TB);
    return fwd_plan_last(g, Pa, pc < Pb ? pc : Pb, c) >= 0;
}
}  // namespace pyipm
