// bounds_csr.hpp -- the simple bounds of a bounded L-BFGS handle grouped by variable (include/pyipm_newton.h,
// pyipm_lbfgs_bounded_stage).  No HIP in here: tests/bounds_csr_replay.cpp compiles it under the host compiler alone.
//
// Bound j acts on variable var[j] with sign[j] = +1 (lower: x_k - l >= 0) or -1 (upper: u - x_k >= 0).  The weights kernel
// walks the bounds of ONE variable, so they are stored as a CSR by variable: the bounds of variable k are entries
// start[k] .. start[k+1] - 1 of ent, in the order the caller gave them (a stable counting sort: equal inputs sum in an
// equal order).  An entry carries the bound's index and its sign in one word: j for a lower bound, ~j for an upper one.
#pragma once
#include <stdint.h>
#include <vector>

namespace pyipm {

// The tail kernel walks a variable's segment once per bound of that variable, inside one thread: a box is two entries, and
// repeated bounds are allowed, but not without limit.
constexpr int64_t BD_MAX_PER_VAR = 64;

struct BoundsCsr {
    std::vector<int64_t> start;                  // n + 1
    std::vector<int64_t> ent;                    // mb

    static int64_t index_of(int64_t code) { return code >= 0 ? code : ~code; }
    static double sign_of(int64_t code) { return code >= 0 ? 1.0 : -1.0; }

    // nullptr: built.  Otherwise the reason for the refusal, and *this is what it was.
    const char* build(int64_t n, int64_t mb, const int64_t* var, const double* sign) {
        if (n < 1 || mb < 0) return "bad geometry";
        if (mb > 0 && (!var || !sign)) return "null var / sign with mb > 0";
        for (int64_t j = 0; j < mb; ++j) {
            if (var[j] < 0 || var[j] >= n) return "a variable index outside 0 .. n-1";
            if (!(sign[j] == 1.0 || sign[j] == -1.0)) return "a sign that is neither +1 nor -1";
        }
        std::vector<int64_t> st((size_t)n + 1, 0), en((size_t)mb);
        for (int64_t j = 0; j < mb; ++j) ++st[(size_t)var[j] + 1];
        for (int64_t k = 0; k < n; ++k) {
            if (st[(size_t)k + 1] > BD_MAX_PER_VAR) return "more than 64 bounds on one variable";
            st[(size_t)k + 1] += st[(size_t)k];
        }
        std::vector<int64_t> next(st.begin(), st.end() - 1);
        for (int64_t j = 0; j < mb; ++j) en[(size_t)next[(size_t)var[j]]++] = sign[j] > 0.0 ? j : ~j;
        start.swap(st);
        ent.swap(en);
        return nullptr;
    }
};

}  // namespace pyipm
