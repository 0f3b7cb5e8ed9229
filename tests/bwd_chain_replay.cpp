// Replay of the hand-over protocol of k_bwd_sweep on the CPU (tests/test_bwd_chain_plan.py compiles and runs it with the address
// and undefined-behaviour sanitizers).  It includes the statement of the chain order the kernel compiles,
// pyipm_amd/csrc/bwd_chain_plan.hpp, and rebuilds the walk of workgroup 0, the steps of the near specialists and the visits of
// every owner wave the way the kernel does.
//
// stdin: lines "n me mi nb owners": owners = workgroups of column owners (16 waves each).  Per line, for skip in {0, 1} and the
// walk with and without the closed-form slack panels, it checks
//   * the panels the chain leaves out are exactly those wholly inside [n, n + mi), none with skip == 0; pred and succ are
//     inverse to each other, chain steps count the chain panels;
//   * where no panel is left out, the walk, the owners' visits and every awaited and published number are those of the walk over
//     all panels (written here from the kernel as it stood before, not from the header);
//   * every awaited (word, value) -- a progress word, a near count, a flag -- is stored by exactly one visit;
//   * a round-robin execution of chain, specialists and owners ends;
//   * every (chain panel t, column group) block left of t is visited exactly once: by the specialists if the group lies in
//     pred(t), otherwise by its owner; every block that can be non-zero is among them.  A block of a left-out panel t that
//     sweep_active does not rule out belongs to the panel that straddles n: x columns in slack rows and the slack block's
//     off-diagonal, exact zeros both;
//   * per column group the order of subtraction is descending t, complete when the chain reads it, with the near one last.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <utility>
#include <vector>
#include "bwd_chain_plan.hpp"

using namespace pyipm;
static long n_checked = 0;

#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "FAILED %s: ", #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

struct Geo { int64_t Npad, n, mi, me; int nb, P, skip; };
// sweep_active of kernels_solve.hpp, restated
static bool active(const Geo& g, int64_t cA, int64_t cB, int64_t r0, int64_t r1) {
    if (!g.skip || g.mi == 0) return true;
    const int64_t s0 = g.n, s1 = g.n + g.mi, i0 = g.n + g.mi + g.me;
    if (cB <= s0) return (r0 < s0) || (r1 > s1);
    if (cA >= s0 && cB <= s1) return r1 > i0 + (cA - s0) && r0 < i0 + (cB - s0);
    return true;
}
static int64_t width(const Geo& g, int p) { const int64_t w = g.Npad - (int64_t)p * g.nb; return w < g.nb ? w : g.nb; }
static bool wholly_slack(const Geo& g, int p) { return g.skip && g.mi > 0 && (int64_t)p * g.nb >= g.n && (int64_t)p * g.nb + width(g, p) <= g.n + g.mi; }
static bool block_active(const Geo& g, int t, int grp) {
    const int64_t cp = ((int64_t)grp * 8 / g.nb) * g.nb, r0 = (int64_t)t * g.nb;
    return active(g, cp, cp + g.nb, r0, r0 + width(g, t));
}

struct Visit { int t, grp; };                    // an owner wave's visit: chain step t, column group
struct Wave { std::vector<Visit> visits; std::vector<std::pair<int, unsigned>> publishes; };   // publishes: (visits made before it, value)

// the owner waves as the kernel builds them
static std::vector<Wave> owners_now(const Geo& g, const BwdChain& ch, int nwv) {
    const int gpp = g.nb / 8, P = g.P;
    std::vector<Wave> out((size_t)nwv);
    for (int gw = 0; gw < nwv; ++gw) {
        Wave& w = out[(size_t)gw];
        for (int t = P - 1, q; (q = bwd_chain_pred(ch, t)) >= 0; t = q) {
            const int glim = t * gpp, nlo = q * gpp, nhi = nlo + gpp, top = nhi == glim ? nlo : glim;
            if (gw >= top) break;
            for (int kk = (top - 1 - gw) / nwv; kk >= 0; --kk) {
                const int grp = gw + kk * nwv;
                if (grp >= nlo && grp < nhi) continue;
                w.visits.push_back(Visit{t, grp});
            }
            w.publishes.push_back({(int)w.visits.size(), bwd_chain_published(ch, t)});
        }
        w.publishes.push_back({(int)w.visits.size(), (unsigned)P});
    }
    return out;
}
// ... and as the walk over every panel built them
static std::vector<Wave> owners_before(const Geo& g, int nwv) {
    const int gpp = g.nb / 8, P = g.P;
    std::vector<Wave> out((size_t)nwv);
    for (int gw = 0; gw < nwv; ++gw) {
        Wave& w = out[(size_t)gw];
        for (int t = P - 1; t >= 1; --t) {
            const int glim = t * gpp;
            if (gw >= glim - gpp) break;
            for (int kk = (glim - gpp - 1 - gw) / nwv; kk >= 0; --kk) w.visits.push_back(Visit{t, gw + kk * nwv});
            w.publishes.push_back({(int)w.visits.size(), (unsigned)(P - t)});
        }
        w.publishes.push_back({(int)w.visits.size(), (unsigned)P});
    }
    return out;
}

static void replay(const Geo& g, int slack_walk, int owners) {
    const int P = g.P, gpp = g.nb / 8, nwv = owners * 16, ngroups = P * gpp;
    const BwdChainGeo cg{g.Npad, g.n, g.mi, g.nb, g.P, g.skip};
    const BwdChain ch = bwd_chain(cg, slack_walk);
    // ---- the order ----
    std::vector<int> walk;
    for (int s = P - 1; s >= 0; s = bwd_chain_pred(ch, s)) { CHECK((int)walk.size() < P, "the walk does not end"); walk.push_back(s); }
    std::vector<char> on_chain((size_t)P, 0);
    for (int s : walk) on_chain[(size_t)s] = 1;
    for (int p = 0; p < P; ++p) {
        CHECK(bwd_chain_closed_form(cg, p) == wholly_slack(g, p), "closed form of panel %d", p);
        CHECK(!on_chain[(size_t)p] == (slack_walk && wholly_slack(g, p)), "panel %d: on the chain %d, wholly slack %d", p, on_chain[(size_t)p], wholly_slack(g, p));
        CHECK(bwd_chain_skipped(ch, p) == !on_chain[(size_t)p], "skipped(%d)", p);
    }
    CHECK(on_chain[(size_t)(P - 1)], "the last panel is left out");
    CHECK((int)walk.size() == bwd_chain_steps(ch), "%zu chain panels, %d steps", walk.size(), bwd_chain_steps(ch));
    for (size_t i = 0; i < walk.size(); ++i) {
        CHECK(bwd_chain_step(ch, walk[i]) == (int)i, "chain step of panel %d", walk[i]);
        if (i + 1 < walk.size()) CHECK(bwd_chain_succ(ch, walk[i + 1]) == walk[i], "succ(pred(%d))", walk[i]);
    }
    CHECK(bwd_chain_succ(ch, P - 1) == P, "succ of the last panel");
    const bool all_panels = (int)walk.size() == P;
    if (!g.skip || !slack_walk) CHECK(all_panels, "skip %d, walk %d: %zu of %d panels", g.skip, slack_walk, walk.size(), P);
    // ---- the visits ----
    const std::vector<Wave> ow = owners_now(g, ch, nwv);
    if (all_panels) {
        const std::vector<Wave> was = owners_before(g, nwv);
        for (int w = 0; w < nwv; ++w) {
            const Wave &a = ow[(size_t)w], &b = was[(size_t)w];
            CHECK(a.visits.size() == b.visits.size() && a.publishes == b.publishes, "wave %d: %zu visits, before %zu", w, a.visits.size(), b.visits.size());
            for (size_t i = 0; i < a.visits.size(); ++i) CHECK(a.visits[i].t == b.visits[i].t && a.visits[i].grp == b.visits[i].grp, "wave %d, visit %zu", w, i);
        }
        for (int s : walk) { CHECK(bwd_chain_pred(ch, s) == s - 1, "pred(%d)", s); CHECK(bwd_chain_awaited(ch, s) == (unsigned)(P - (s + 1)), "awaited at %d", s); }
    }
    // who visits block (t, grp): 0 nobody, 1 + wave an owner, -1 the specialists
    std::map<std::pair<int, int>, int> who;
    for (int w = 0; w < nwv; ++w)
        for (const Visit& v : ow[(size_t)w].visits) {
            CHECK(v.grp % nwv == w, "group %d visited by wave %d", v.grp, w);
            CHECK(who.emplace(std::make_pair(v.t, v.grp), 1 + w).second, "block (%d, %d) visited twice", v.t, v.grp);
        }
    std::vector<int> near_of((size_t)P, -1);                     // panel -> the step whose specialists take its columns
    for (int t : walk) {
        const int q = bwd_chain_pred(ch, t);
        if (q < 0) continue;
        CHECK(on_chain[(size_t)q] && near_of[(size_t)q] < 0, "panel %d is the near panel of two steps", q);
        near_of[(size_t)q] = t;
        for (int j = 0; j < gpp; ++j) CHECK(who.emplace(std::make_pair(t, q * gpp + j), -1).second, "block (%d, %d): specialists and an owner", t, q * gpp + j);
    }
    for (int t = 0; t < P; ++t)
        for (int grp = 0; grp < t * gpp; ++grp) {
            const int by = who.count({t, grp}) ? who[{t, grp}] : 0;
            if (on_chain[(size_t)t]) {
                CHECK(by != 0, "block (%d, %d) of a chain step is visited by nobody", t, grp);
                CHECK((by == -1) == (grp / gpp == bwd_chain_pred(ch, t)), "block (%d, %d): specialists %d", t, grp, by == -1);
            } else {
                CHECK(by == 0, "block (%d, %d) of a left-out panel is visited", t, grp);
                const int64_t cp = ((int64_t)grp * 8 / g.nb) * g.nb;
                CHECK(!block_active(g, t, grp) || (cp < g.n && cp + g.nb > g.n), "block (%d, %d) of a left-out panel can be non-zero", t, grp);
            }
        }
    // ---- every awaited (word, value) is stored by exactly one visit ----
    for (size_t i = 1; i < walk.size(); ++i) {                  // after chain panel s = walk[i], before q = pred(s)
        const int s = walk[i], q = bwd_chain_pred(ch, s);
        if (q < 0) continue;
        for (int j = 0; j < gpp; ++j) {
            const Wave& w = ow[(size_t)((q * gpp + j) % nwv)];
            int nst = 0; unsigned last = 0;
            for (auto& pb : w.publishes) { CHECK(pb.second > last, "a progress word does not rise"); last = pb.second; nst += pb.second == bwd_chain_awaited(ch, s); }
            CHECK(nst == 1, "progress %u of wave %d, awaited at panel %d, is stored %d times", bwd_chain_awaited(ch, s), (q * gpp + j) % nwv, s, nst);
        }
    }
    for (int w = 0; w < nwv; ++w) for (const Visit& v : ow[(size_t)w].visits) CHECK(on_chain[(size_t)v.t], "an owner waits for the flag of panel %d", v.t);
    // ---- round-robin execution ----
    std::vector<unsigned> flag((size_t)P, 0u), nearc((size_t)P, 0u), prog((size_t)nwv, 0u);
    std::vector<std::vector<int>> seq((size_t)ngroups);        // per group: the steps subtracted from it, in order (near ones: by the chain)
    std::vector<char> near_there((size_t)ngroups, 0);
    std::vector<size_t> at((size_t)nwv, 0), pub((size_t)nwv, 0);
    std::vector<size_t> spec_at((size_t)gpp, 0);                // specialist wave j: index into walk of its next step
    size_t ci = 0; bool acked = true;                           // chain: next panel walk[ci]; acked: the wait behind the last flag is through
    auto expect = [&](int grp, int below) {                     // the chain steps right of the group's panel, descending, down to `below`
        std::vector<int> e; for (int t : walk) if (t > grp / gpp && t >= below) e.push_back(t); return e; };
    for (long turn = 0;; ++turn) {
        bool progress = false, done = ci == walk.size();
        if (!done) {
            const int s = walk[ci], up = ci ? walk[ci - 1] : P;
            if (!acked) {                                       // the progress words of the owners of this panel's columns
                bool ok = true;
                for (int j = 0; j < gpp; ++j) if (prog[(size_t)((s * gpp + j) % nwv)] < bwd_chain_awaited(ch, up)) ok = false;
                if (ok) { acked = true; progress = true; }
            }
            if (acked) {
                bool ready = true;
                if (up < P) for (int j = 0; j < gpp; ++j) if (!near_there[(size_t)(s * gpp + j)]) ready = false;
                if (ready) {
                    if (up < P) CHECK(nearc[(size_t)up] == (unsigned)gpp, "near count of step %d is %u", up, nearc[(size_t)up]);
                    for (int j = 0; j < gpp; ++j) {
                        std::vector<int>& sq = seq[(size_t)(s * gpp + j)];
                        if (up < P) { CHECK(expect(s * gpp + j, up + 1) == sq, "panel %d, group %d: far steps incomplete or out of order when the chain reads y", s, j); sq.push_back(up); }
                        CHECK(expect(s * gpp + j, 0) == sq, "panel %d, group %d: order of subtraction", s, j);
                    }
                    flag[(size_t)s] = 1u; ++ci; progress = true;
                    acked = !(up < P && bwd_chain_pred(ch, s) >= 0);
                }
            }
        }
        for (int j = 0; j < gpp; ++j) {                         // specialists: wave j at chain step t takes group j of pred(t)
            size_t& k = spec_at[(size_t)j];
            if (k >= walk.size() || bwd_chain_pred(ch, walk[k]) < 0) continue;
            done = false;
            const int t = walk[k];
            if (!flag[(size_t)t]) continue;
            const int grp = bwd_chain_pred(ch, t) * gpp + j;
            CHECK(!near_there[(size_t)grp], "near sum of group %d stored twice", grp);
            near_there[(size_t)grp] = 1; ++nearc[(size_t)t]; ++k; progress = true;
        }
        for (int w = 0; w < nwv; ++w) {
            const Wave& wv = ow[(size_t)w];
            while (pub[(size_t)w] < wv.publishes.size() && wv.publishes[pub[(size_t)w]].first == (int)at[(size_t)w]) {
                prog[(size_t)w] = wv.publishes[pub[(size_t)w]].second; ++pub[(size_t)w]; progress = true;
            }
            if (at[(size_t)w] == wv.visits.size()) continue;
            done = false;
            const Visit& v = wv.visits[at[(size_t)w]];
            if (!flag[(size_t)v.t]) continue;
            seq[(size_t)v.grp].push_back(v.t); ++at[(size_t)w]; progress = true;
        }
        if (done) break;
        CHECK(progress, "nobody can move: chain at panel %d", ci < walk.size() ? walk[ci] : -1);
    }
    for (int grp = 0; grp < ngroups; ++grp) CHECK(seq[(size_t)grp] == expect(grp, 0), "group %d: steps subtracted", grp);
    ++n_checked;
}

int main() {
    long long n, me, mi; int nb, owners;
    while (scanf("%lld %lld %lld %d %d", &n, &me, &mi, &nb, &owners) == 5) {
        CHECK(n > 0 && me >= 0 && mi >= 0 && nb >= 64 && nb % 64 == 0 && nb <= 256 && owners >= 1, "bad line");
        for (int skip = 0; skip < 2; ++skip)
            for (int slack_walk = 0; slack_walk < 2; ++slack_walk) {
                Geo g;
                const long long N = n + me + 2 * mi;
                g.Npad = (N + 127) / 128 * 128;
                g.n = n; g.mi = mi; g.me = me; g.nb = nb; g.skip = (skip && mi > 0) ? 1 : 0;
                g.P = (int)((g.Npad + nb - 1) / nb);
                if (g.P < 2) continue;                         // (sweeps_in_one_launch: the per-panel kernels)
                replay(g, slack_walk, owners);
            }
    }
    printf("%ld walks replayed\n", n_checked);
    return n_checked > 0 ? 0 : 1;
}
