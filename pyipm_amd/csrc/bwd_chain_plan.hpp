// bwd_chain_plan.hpp -- the order in which workgroup 0 of the one-launch backward sweep (k_bwd_sweep, kernels_solve.hpp) walks the
// panels, and what that order means for the near specialists, the column owners and the progress words.  Plain C++: nothing of
// HIP or of the handle in it; the functions are constexpr so that host code, the kernel and a stand-alone replay
// (tests/test_bwd_chain_plan.py) all compile this one source.
//
// A panel that lies wholly inside the slack block [n, n + mi) is a CLOSED-FORM SLACK PANEL where the structural zeros are skipped:
// its diagonal block is diagonal, step t of such a panel reaches no column (x columns have exact zeros in the s rows, nothing else
// lies to its left) and what its own columns receive comes from the matching lambda_i rows, through their ordinary owners.  So
// x_s is what v holds once those owners are through, and the chain has nothing to do for it: it walks the CHAIN PANELS only, the
// near specialists of step t take the columns of pred(t), the next chain panel to the left, and the progress words count chain
// steps.  Such panels are one contiguous range [sa, sb) (empty: sa == sb == npanels), so everything below is O(1).
#pragma once
#include <cstdint>
namespace pyipm {
struct BwdChainGeo { int64_t Npad, n, mi; int nb, npanels, skip; };

// is panel p a closed-form slack panel?  [p nb, p nb + w) inside [n, n + mi), w the panel's width; never with skip == 0
constexpr bool bwd_chain_closed_form(const BwdChainGeo& g, int p) {
    if (!g.skip || g.mi == 0 || p < 0 || p >= g.npanels) return false;
    const int64_t c0 = (int64_t)p * g.nb;
    const int64_t w = g.Npad - c0 < g.nb ? g.Npad - c0 : (int64_t)g.nb;
    return c0 >= g.n && c0 + w <= g.n + g.mi;
}
struct BwdChain { int sa, sb, npanels; };     // the closed-form slack panels [sa, sb) of npanels panels
// slack_walk == 0 keeps every panel on the chain (PYIPM_BWD_SLACK=0)
constexpr BwdChain bwd_chain(const BwdChainGeo& g, int slack_walk) {
    const int64_t sa = (g.n + g.nb - 1) / g.nb, sb = (g.n + g.mi) / g.nb;
    if (!slack_walk || !g.skip || g.mi == 0 || sb <= sa || sb >= g.npanels) return BwdChain{g.npanels, g.npanels, g.npanels};
    return BwdChain{(int)sa, (int)sb, g.npanels};
}
constexpr bool bwd_chain_skipped(const BwdChain& ch, int p) { return p >= ch.sa && p < ch.sb; }
// the next chain panel to the left of chain panel t (-1: none), and its inverse (npanels: none)
constexpr int bwd_chain_pred(const BwdChain& ch, int t) { return bwd_chain_skipped(ch, t - 1) ? ch.sa - 1 : t - 1; }
constexpr int bwd_chain_succ(const BwdChain& ch, int q) { return bwd_chain_skipped(ch, q + 1) ? ch.sb : q + 1; }
// chain steps taken before chain panel t is resolved (the last panel: 0), and all of them
constexpr int bwd_chain_step(const BwdChain& ch, int t) { return ch.npanels - 1 - t - (t < ch.sa ? ch.sb - ch.sa : 0); }
constexpr int bwd_chain_steps(const BwdChain& ch) { return ch.npanels - (ch.sb - ch.sa); }
// Column owners.  A wave that has finished its groups of chain step t stores bwd_chain_step(t) + 1 in its progress word.  Before
// it resolves q = pred(t), the chain waits until the owners of q's groups have finished every chain step before t:
// progress >= bwd_chain_step(t), and nothing where t is the first chain panel (no step has been taken) or q < 0.
constexpr unsigned bwd_chain_published(const BwdChain& ch, int t) { return (unsigned)(bwd_chain_step(ch, t) + 1); }
constexpr unsigned bwd_chain_awaited(const BwdChain& ch, int t) { return (unsigned)bwd_chain_step(ch, t); }
}  // namespace pyipm
