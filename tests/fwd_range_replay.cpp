// Replay of the hand-over protocol of k_fwd_range and k_fwd_prefix on the CPU (tests/test_fwd_range_plan.py compiles and runs it
// with the address and undefined-behaviour sanitizers).  It includes the statement of the protocol k_fwd_range compiles,
// pyipm_amd/csrc/fwd_range_plan.hpp, and rebuilds every workgroup's visits the way fwd_range_owner does.  k_fwd_prefix keeps its
// own text: its numbering (every chunk below panel 0 but the slack hole), its visits and its rule (the chain waits prog[c] >= s,
// a visit is final at s + 1 == c / cpp) are restated here from that kernel and replayed for Pa = 0 inside the x block, where the
// header must give the same waits and final visits.
//
// stdin: lines "n me mi nb grid mode"; mode 0: every range [Pa, Pb) with Pb < npanels, 1: the ranges a handle can launch.
// Per case and range it checks
//   * every (word, value) the chain waits for is stored by exactly one owner visit;
//   * every flag an owner waits for is raised by the chain;
//   * a round-robin execution of all workgroups, each in its own visit order, ends, and the chain never reads a chunk that
//     memory does not hold in full;
//   * the (panel, chunk) updates are those of the per-panel kernels' active launch blocks, each once;
//   * for Pa = 0 inside the x block: the chain waits prog[c] >= s, a visit is final at s + 1 == c / cpp.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <utility>
#include <vector>
#include "fwd_range_plan.hpp"

using namespace pyipm;
static constexpr int RESIDENT = 16;      // FWDP_RESIDENT, kernels_solve.hpp
static long n_checked = 0;

#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "FAILED %s: ", #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

struct Visit { int s, c, k; };           // panel, chunk, the owner's k-th chunk

// the per-panel path, written from active_ranges / k_fwd_gemv and not from the header: (panel, chunk) pairs that are subtracted
static std::set<std::pair<int, int>> per_panel_updates(const FwdPlanGeo& g, int Pa, int Pb) {
    std::set<std::pair<int, int>> out;
    for (int s = Pa; s < Pb; ++s) {
        const int64_t cA = (int64_t)s * g.nb, cB = cA + g.nb, row_begin = cB;
        int64_t a0 = 0, a1 = g.Npad, b0 = 0, b1 = 0;
        if (g.skip && g.mi != 0) {
            const int64_t s0 = g.n, s1 = g.n + g.mi, i0 = g.n + g.mi + g.me;
            if (cB <= s0) { a0 = 0; a1 = s0; b0 = s1; b1 = g.Npad; }
            else if (cA >= s0 && cB <= s1) { a0 = i0 + (cA - s0); a1 = i0 + (cB - s0); b0 = 0; b1 = 0; }
        }
        for (int64_t i0 = row_begin; i0 < g.Npad; i0 += 256) {
            const int64_t i1 = i0 + 256;
            if (!((i1 > a0 && i0 < a1) || (i1 > b0 && i0 < b1))) continue;
            for (int64_t r = i0; r < i1 && r < g.Npad; r += FWD_PLAN_TB) out.insert({s, (int)(r / FWD_PLAN_TB)});
        }
    }
    return out;
}

// prefix_kernel: k_fwd_prefix's own numbering, visits and rule (Pa = 0, the range inside the x block) instead of the header's
static void replay(const FwdPlanGeo& g, int Pa, int Pb, int grid, bool prefix_kernel = false) {
    const int cpp = g.nb / FWD_PLAN_TB, nchunks = (int)(g.Npad / FWD_PLAN_TB), nown = grid - 1;
    std::vector<int> owned;
    std::vector<std::vector<Visit>> visits((size_t)nown);
    if (!prefix_kernel) {
        // numbering and visits, as fwd_range_owner builds them
        for (int c = (Pa + 1) * cpp; c < nchunks; ++c) if (fwd_plan_owned(g, Pa, Pb, c)) owned.push_back(c);
        for (int w = 0; w < nown; ++w)
            for (int s = Pa; s < Pb; ++s)
                for (size_t m = (size_t)w; m < owned.size(); m += (size_t)nown)
                    if (fwd_plan_visit(g, s, owned[m])) visits[(size_t)w].push_back(Visit{s, owned[m], (int)((m - (size_t)w) / (size_t)nown)});
    } else {
        // as fwd_prefix_owner builds them: the chunks below panel 0 without the hole; a visit where the chunk lies below the panel
        // and its launch block of k_fwd_gemv is active
        int h0 = nchunks, hl = 0;
        if (g.skip && g.mi >= 512) {
            const int a = (int)((g.n + 192 + FWD_PLAN_TB - 1) / FWD_PLAN_TB), b = (int)((g.n + g.mi - 256) / FWD_PLAN_TB) + 1;
            if (b > a) { h0 = a; hl = b - a; }
        }
        const int nlog = nchunks - cpp - hl;
        for (int m = 0; m < nlog; ++m) { const int c = cpp + m; owned.push_back(c >= h0 ? c + hl : c); }
        for (int w = 0; w < nown; ++w)
            for (int s = 0; s < Pb; ++s)
                for (int m = w; m < nlog; m += nown) {
                    const int c = owned[(size_t)m];
                    const int64_t row_begin = (int64_t)(s + 1) * g.nb, r0 = (int64_t)c * FWD_PLAN_TB;
                    if (r0 < row_begin) continue;
                    const int64_t i0 = row_begin + (r0 - row_begin) / 256 * 256;
                    bool act = true;
                    if (g.skip && g.mi != 0) act = (i0 < g.n) || (i0 + 256 > g.n + g.mi);      // x columns: not wholly inside the slack rows
                    if (act) visits[(size_t)w].push_back(Visit{s, c, (m - w) / nown});
                }
    }
    auto is_final = [&](int s, int c) { return prefix_kernel ? (c < Pb * cpp && s + 1 == c / cpp) : fwd_plan_final(g, Pa, Pb, s, c); };
    auto chain_waits = [&](int s, int c) { return prefix_kernel ? s - 1 : fwd_plan_chain_waits(g, Pa, s, c); };   // (-1 at s = 0: no wait)
    // the updates are the per-panel path's, each once; every update is some owner's visit
    std::multiset<std::pair<int, int>> got;
    for (auto& vw : visits) for (auto& v : vw) got.insert({v.s, v.c});
    const auto want = per_panel_updates(g, Pa, Pb);
    CHECK(got.size() == want.size(), "updates %zu, per panel %zu", got.size(), want.size());
    for (auto& u : want) CHECK(got.count(u) == 1, "update (panel %d, chunk %d) made %zu times", u.first, u.second, got.count(u));
    // what each visit stores: prog[c] := s + 1 where it is final or the chunk has no slot
    auto stores = [&](const Visit& v) { return v.k >= RESIDENT || is_final(v.s, v.c); };
    std::map<std::pair<int, unsigned>, int> raised;             // (word, value) -> visits that store it
    for (auto& vw : visits) for (auto& v : vw) if (stores(v)) raised[{v.c, (unsigned)(v.s + 1)}]++;
    for (int s = Pa; s < Pb; ++s)
        for (int t = 0; t < cpp; ++t) {
            const int c = s * cpp + t, p = chain_waits(s, c);
            if (p < 0) continue;                                 // (the execution below checks that memory holds the chunk in full)
            CHECK(p >= Pa && p < s, "chain waits for panel %d in front of the range or behind panel %d", p, s);
            const int nst = raised[std::make_pair(c, (unsigned)(p + 1))];
            CHECK(nst == 1, "prog[%d] = %d stored by %d visits", c, p + 1, nst);
            if (Pa == 0 && (int64_t)Pb * g.nb <= g.n) CHECK(p == s - 1, "x prefix: chain waits for %d at panel %d", p + 1, s);
        }
    if (Pa == 0 && (int64_t)Pb * g.nb <= g.n)
        for (auto& vw : visits) for (auto& v : vw)
            CHECK(fwd_plan_final(g, Pa, Pb, v.s, v.c) == (v.c < Pb * cpp && v.s + 1 == v.c / cpp), "x prefix: final at (%d, %d)", v.s, v.c);
    for (auto& vw : visits) for (auto& v : vw) CHECK(v.s >= Pa && v.s < Pb, "an owner waits for flag %d outside the range", v.s);
    // round-robin execution: the chain is workgroup 0, one step per turn where the word it waits for allows
    std::vector<unsigned> prog((size_t)nchunks, 0u), flag((size_t)(Pb - Pa), 0u);
    std::vector<int> applied((size_t)nchunks, 0), in_memory((size_t)nchunks, 0);   // updates made / updates memory holds
    std::vector<size_t> at((size_t)nown, 0);
    int chain_s = Pa;
    for (;;) {
        bool progress = false, done = chain_s == Pb;
        if (chain_s < Pb) {
            bool ready = true;
            for (int t = 0; t < cpp; ++t) {
                const int c = chain_s * cpp + t, p = chain_waits(chain_s, c);
                if (p >= 0 && prog[(size_t)c] < (unsigned)(p + 1)) ready = false;
            }
            if (ready) {
                for (int t = 0; t < cpp; ++t) {
                    const int c = chain_s * cpp + t;
                    int need = 0; for (int p = Pa; p < chain_s; ++p) need += want.count({p, c}) ? 1 : 0;
                    CHECK(in_memory[(size_t)c] == need, "chain reads chunk %d of panel %d with %d of %d updates in memory", c, chain_s, in_memory[(size_t)c], need);
                }
                flag[(size_t)(chain_s - Pa)] = 1u; ++chain_s; progress = true;
            }
        }
        for (int w = 0; w < nown; ++w) {
            if (at[(size_t)w] == visits[(size_t)w].size()) continue;
            done = false;
            const Visit& v = visits[(size_t)w][at[(size_t)w]];
            if (!flag[(size_t)(v.s - Pa)]) continue;
            ++applied[(size_t)v.c];
            if (stores(v)) {
                CHECK(prog[(size_t)v.c] < (unsigned)(v.s + 1), "prog[%d] does not rise", v.c);
                prog[(size_t)v.c] = (unsigned)(v.s + 1); in_memory[(size_t)v.c] = applied[(size_t)v.c];
            }
            if (++at[(size_t)w] == visits[(size_t)w].size())                      // the owner's end: what is still resident goes home
                for (auto& u : visits[(size_t)w]) in_memory[(size_t)u.c] = applied[(size_t)u.c];
            progress = true;
        }
        if (done) break;
        CHECK(progress, "no workgroup can move: chain at panel %d of [%d, %d)", chain_s, Pa, Pb);
    }
    for (int c = 0; c < nchunks; ++c) {
        int need = 0; for (int p = Pa; p < Pb; ++p) need += want.count({p, c}) ? 1 : 0;
        CHECK(in_memory[(size_t)c] == need, "chunk %d ends with %d of %d updates in memory", c, in_memory[(size_t)c], need);
    }
    ++n_checked;
}

int main() {
    long long n, me, mi; int nb, grid, mode;
    while (scanf("%lld %lld %lld %d %d %d", &n, &me, &mi, &nb, &grid, &mode) == 6) {
        for (int skip = 0; skip < 2; ++skip) {
            FwdPlanGeo g;
            const long long N = n + me + 2 * mi;
            g.Npad = (N + 127) / 128 * 128; if (g.Npad == 0) g.Npad = 128;
            g.n = n; g.mi = mi; g.me = me; g.nb = nb; g.skip = skip;
            const int np = (int)((g.Npad + nb - 1) / nb);
            if (mode == 0) {
                for (int Pa = 0; Pa < np; ++Pa) for (int Pb = Pa + 1; Pb < np; ++Pb) replay(g, Pa, Pb, grid);
                for (int Pb = 1; Pb < np && (long long)Pb * nb <= n; ++Pb) replay(g, 0, Pb, grid, true);   // k_fwd_prefix's own text
            } else {
                const int px = (int)(n / nb), sa = (int)((n + nb - 1) / nb), ea = (int)((n + mi + nb - 1) / nb), eb = (int)((n + mi + me) / nb);
                if (px >= 1 && px < np) { replay(g, 0, px, grid); replay(g, 0, px, grid, true); }
                for (int Pb = ea + 1; Pb <= eb && Pb < np; ++Pb) {              // (the kept lambda_e groups end at some group's border)
                    if (sa < Pb) replay(g, sa, Pb, grid);
                    replay(g, ea, Pb, grid);
                }
            }
        }
    }
    printf("%ld ranges replayed\n", n_checked);
    return n_checked > 0 ? 0 : 1;
}
