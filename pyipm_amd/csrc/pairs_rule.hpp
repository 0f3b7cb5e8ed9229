// pairs_rule.hpp -- the host half of the L-BFGS pair store (include/pyipm_newton.h, "pair store"): the accept / skip / reset
// decision of the reference's lbfgs_update (pyipm.py:1282-1371) and the SS / L / D bookkeeping, as
// pyipm_amd/loop.py:lbfgs_pair_update states them -- the same IEEE operations in the same order, so the two agree bit for
// bit on the same products.  No HIP in here: tests/pairs_rule_replay.cpp compiles it under the host compiler alone.
//
// The store holds m <= memory + 1 pairs (the reference lets the storage reach memory + 1, :1300).  An offer brings the
// products of the new (dx, dg) pair against the storage AS IT WOULD STAND with the pair appended -- the oldest pair left
// out when the store is full -- that is k = kept() + 1 entries each of
//     inner : S'dx (constrained) or Y'dg (unconstrained), the last entry being den = dx.dx or dg.dg,
//     cross : dx'Y (constrained) or S'dg (unconstrained), the last entry being curv = dg.dx,
// and curv, den themselves.  SS, L, D are m x m row-major and contiguous.
#pragma once
#include <math.h>
#include <stdint.h>
#include <vector>

namespace pyipm {

constexpr int PAIRS_ACCEPTED = 1, PAIRS_SKIPPED = 0, PAIRS_RESET = 2;

struct PairsRule {
    int memory = 0;
    bool constrained = false;
    double zeta0 = 1.0, zeta = 1.0;
    int m = 0;                       // stored pairs
    int64_t fail = 0;                // skipped pairs in a row
    std::vector<double> SS, L, D;    // m x m each

    void init(int memory_, bool constrained_, double zeta0_) {
        memory = memory_; constrained = constrained_; zeta0 = zeta0_;
        SS.reserve((size_t)(memory + 1) * (memory + 1)); L.reserve(SS.capacity()); D.reserve(SS.capacity());
        reset();
    }
    void reset() { zeta = zeta0; m = 0; fail = 0; SS.clear(); L.clear(); D.clear(); }     // lbfgs_init (:993-1005)

    bool drops() const { return m > memory; }             // an accepted pair pushes the oldest one out
    int kept() const { return drops() ? m - 1 : m; }      // columns of the present storage the products are taken against

    // Returns PAIRS_ACCEPTED (the caller appends the pair, dropping the oldest if drops() held BEFORE the call),
    // PAIRS_SKIPPED, or PAIRS_RESET (the rule has emptied itself; the caller forgets its columns).
    int offer(const double* inner, const double* cross, double curv, double den, double eps) {
        const double zeta_new = curv / (den + eps);
        const double root = sqrt(eps);
        if (curv > root && zeta_new > root) {
            const int k0 = kept(), off = drops() ? 1 : 0, k = k0 + 1;
            std::vector<double> s2((size_t)k * k, 0.0), l2(s2), d2(s2);
            for (int i = 0; i < k0; ++i)
                for (int j = 0; j < k0; ++j) {
                    const size_t src = (size_t)(i + off) * m + (j + off), dst = (size_t)i * k + j;
                    s2[dst] = SS[src]; l2[dst] = L[src]; d2[dst] = D[src];
                }
            for (int j = 0; j < k; ++j) s2[(size_t)j * k + k0] = s2[(size_t)k0 * k + j] = inner[j];
            if (constrained) {
                for (int j = 0; j < k; ++j) l2[(size_t)k0 * k + j] = cross[j];
                l2[(size_t)k0 * k + k0] = 0.0;
            } else {
                for (int j = 0; j < k; ++j) l2[(size_t)j * k + k0] = cross[j];
            }
            d2[(size_t)k0 * k + k0] = curv;
            SS.swap(s2); L.swap(l2); D.swap(d2);
            m = k; zeta = zeta_new; fail = 0;
            return PAIRS_ACCEPTED;
        }
        fail += 1;
        if (fail > memory && m > 0) { reset(); return PAIRS_RESET; }
        return PAIRS_SKIPPED;
    }
};

}  // namespace pyipm
