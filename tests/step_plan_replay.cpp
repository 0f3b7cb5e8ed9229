// What a reusing or recording step keeps, copies and skips, checked on the CPU (tests/test_step_plan.py compiles and runs this with
// the address and undefined-behaviour sanitizers).  It includes the one statement of it, pyipm_amd/csrc/step_plan.hpp, builds the
// full, recording and reusing plans of every geometry it is given -- with and without the lambda_e level, fuse_forward and the
// one-launch sweeps -- and checks them against the geometry, restated here from the column order [x | s | lambda_e | lambda_i]
// and from the order of factor_all's phases, not from the header.
//
// stdin: lines "n me mi nb group lookahead skip_zeros" (tail_group 4, not the user's; group_chain on: a handle's defaults).
// stdout: per line "n me mi nb group lookahead skip_zeros gB gS gE" (gS = gE = -1 without the level; gB = 0: no prefix), then
// "<count> lines replayed".
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "step_plan.hpp"

using namespace pyipm;
#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "FAILED %s: ", #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

static int64_t c0_of(const PlanGeo& g, const GroupSched& sc, int64_t grp) { return grp >= sc.ngroups() ? g.Npad : g.panel_c0(sc.first(grp)); }

// the matrix side of a recording or reusing plan that has a prefix
static void check_keeps(const PlanGeo& g, const GroupSched& sc, const StepPlan& p, bool lam_e, const char* tag) {
    const int64_t ng = sc.ngroups(), e0 = g.n + g.mi, e1 = e0 + g.me;
    CHECK(p.gB > 0 && p.gB < ng && p.cB <= g.n && p.cB == c0_of(g, sc, p.gB), "%s gB %lld cB %lld", tag, (long long)p.gB, (long long)p.cB);
    // the prefix: every group before gB ends at or before column n, group gB does not
    for (int64_t grp = 0; grp < p.gB; ++grp) CHECK(c0_of(g, sc, grp + 1) <= g.n, "%s group %lld of the prefix", tag, (long long)grp);
    CHECK(c0_of(g, sc, p.gB + 1) > g.n, "%s group gB = %lld ends inside x", tag, (long long)p.gB);
    const LamE& e = p.e;
    CHECK(lam_e || !e.ok, "%s the level was not asked for", tag);
    if (e.ok) {
        CHECK(p.gB < e.gS && e.gS < e.gE && e.gE < ng, "%s groups %lld %lld %lld", tag, (long long)p.gB, (long long)e.gS, (long long)e.gE);
        CHECK(e.cS == c0_of(g, sc, e.gS) && e.cE == c0_of(g, sc, e.gE) && e.cS >= e0 && e.cE <= e1 && e.cS < e.cE, "%s columns [%lld, %lld)", tag, (long long)e.cS, (long long)e.cE);
        auto inside = [&](int64_t grp) { return c0_of(g, sc, grp) >= e0 && c0_of(g, sc, grp + 1) <= e1; };
        for (int64_t grp = e.gS; grp < e.gE; ++grp) CHECK(inside(grp), "%s group %lld is kept", tag, (long long)grp);
        CHECK(!inside(e.gS - 1) && !inside(e.gE), "%s a whole lambda_e group is left out", tag);
        const size_t rows = (size_t)(g.Npad - e.cE);
        CHECK(p.snap_e_doubles == PX_HDR + rows * (size_t)(e.cE - e.cS) + rows * rows, "%s second snapshot %zu", tag, p.snap_e_doubles);
    } else {
        CHECK(p.snap_e_doubles == 0, "%s second snapshot without the level", tag);
    }
    // the first snapshot: disjoint ascending ranges, contiguous offsets, [cB, Npad) minus exactly the panels wholly inside the slack block
    CHECK(p.nranges >= 1 && p.nranges <= 2, "%s %d ranges", tag, p.nranges);
    size_t off = PX_HDR; int64_t prev = p.cB;
    std::vector<char> covered((size_t)g.Npad, 0);
    for (int k = 0; k < p.nranges; ++k) {
        const PxRange& r = p.ranges[k];
        CHECK(r.c0 >= prev && r.c1 > r.c0 && r.c1 <= g.Npad && (size_t)r.off == off, "%s range %d [%lld, %lld) at %lld", tag, k, (long long)r.c0, (long long)r.c1, (long long)r.off);
        for (int64_t c = r.c0; c < r.c1; ++c) covered[(size_t)c] = 1;
        off += (size_t)(r.c1 - r.c0) * (size_t)(g.Npad - r.c0); prev = r.c1;
    }
    CHECK(off == p.snap_doubles, "%s snapshot %zu against %zu", tag, p.snap_doubles, off);
    for (int64_t c = 0; c < g.Npad; ++c) {
        const int64_t q = c / g.nb, q0 = g.panel_c0(q), q1 = q0 + g.panel_w(q);
        const bool slack_panel = g.mi > 0 && q0 >= g.n && q1 <= g.n + g.mi;
        CHECK((covered[(size_t)c] != 0) == (c >= p.cB && !slack_panel), "%s column %lld", tag, (long long)c);
    }
    const PxRange& last = p.ranges[p.nranges - 1];
    CHECK(last.c1 == g.Npad && (!e.ok || last.c0 <= e.cE), "%s the last range [%lld, %lld)", tag, (long long)last.c0, (long long)last.c1);
}

// the forward substitution of a fused reusing step: every panel has one owner, whichever way the range launch went
static void check_forward(const PlanGeo& g, const GroupSched& sc, const StepPlan& p, bool sweeps, const char* tag) {
    const int64_t ng = sc.ngroups(), np = g.npanels;
    const bool cand = p.frB > p.frA;
    CHECK(p.pB == sc.first(p.gB) && p.pS == (p.e.ok ? sc.first(p.e.gS) : p.pB) && p.pE == (p.e.ok ? sc.first(p.e.gE) : p.pB), "%s panels", tag);
    CHECK(cand == (p.e.ok && sweeps) && p.fwd_prefix_launch == sweeps, "%s candidate [%lld, %lld)", tag, (long long)p.frA, (long long)p.frB);
    if (cand) {
        bool closed = p.slack_first;
        for (int64_t grp = p.gB; grp < p.e.gS; ++grp) closed = closed && sc.fast(grp);
        CHECK(p.frB == sc.first(p.e.gE) && p.frA == sc.first(closed ? p.gB : p.e.gS) && p.fr_slack == closed, "%s range [%lld, %lld)", tag, (long long)p.frA, (long long)p.frB);
        for (int64_t q = p.frA; q < p.frB; ++q)              // kept panels only: a kept lambda_e group's, or a slack panel enqueued up front
            CHECK(q >= p.pB && (q >= p.pS || (p.slack_first && sc.fast_panel(q))), "%s panel %lld is not kept", tag, (long long)q);
    }
    for (int used = 0; used < 2; ++used) {
        std::vector<int> owners((size_t)np, 0);
        for (int64_t q = 0; q < p.pB; ++q) owners[(size_t)q] += 1;                                  // the prefix launch or loop
        if (used && cand) for (int64_t q = p.frA; q < p.frB; ++q) owners[(size_t)q] += 1;           // the range launch
        for (int64_t q = p.pS; q < p.pE; ++q) owners[(size_t)q] += p.fwd_owner(q, used && cand) == FwdOwner::Kept;    // the kept groups' loop
        for (int64_t grp = p.gB; grp < ng; ++grp) {                                                  // panel_done: the groups that run
            if (p.e.ok && grp >= p.e.gS && grp < p.e.gE) continue;
            for (int64_t q = sc.first(grp); q < sc.first(grp + 1); ++q) owners[(size_t)q] += p.fwd_owner(q, used && cand) == FwdOwner::PanelDone;
        }
        for (int64_t q = 0; q < np; ++q) {
            CHECK(owners[(size_t)q] == 1, "%s panel %lld has %d owners (range %s)", tag, (long long)q, owners[(size_t)q], used ? "used" : "fallen back");
            const FwdOwner w = p.fwd_owner(q, used && cand);
            CHECK((w == FwdOwner::Prefix) == (q < p.pB) && (w == FwdOwner::Range) == (used && cand && q >= p.frA && q < p.frB), "%s owner of %lld", tag, (long long)q);
        }
    }
}

int main() {
    long long n, me, mi; int nb, group, lookahead, skip; long count = 0;
    while (scanf("%lld %lld %lld %d %d %d %d", &n, &me, &mi, &nb, &group, &lookahead, &skip) == 7) {
        PlanGeo g{n, me, mi, 0, nb, 0};
        g.Npad = (n + 2 * mi + me + 127) / 128 * 128; if (g.Npad == 0) g.Npad = 128;
        g.npanels = (g.Npad + nb - 1) / nb;
        const SchedOpts o{group, 4, false, skip != 0, lookahead, true};
        const GroupSched sc = plan_groups(g, o);
        const int64_t ng = sc.ngroups();
        bool any_fast = false; for (int64_t grp = 1; grp < ng; ++grp) any_fast = any_fast || sc.fast(grp);
        const bool slack_first = lookahead && !sc.fast(0) && any_fast;
        char tag[160];
        long long out_gB = 0, out_gS = -1, out_gE = -1;
        for (int kind = PX_FULL; kind <= PX_REUSE; ++kind) for (int lam_e = 0; lam_e < 2; ++lam_e) {
            StepPlan first;
            for (int v = 0; v < 4; ++v) {
                const bool fuse = (v & 1) != 0, sweeps = (v & 2) != 0;
                snprintf(tag, sizeof(tag), "(%lld %lld %lld nb %d group %d la %d skip %d) kind %d lam_e %d fuse %d sweeps %d:", n, me, mi, nb, group, lookahead, skip, kind, lam_e, (int)fuse, (int)sweeps);
                const StepPlan p = make_step_plan(g, sc, o, kind, lam_e != 0, fuse, sweeps);
                if (v == 0) first = p;
                CHECK(p == first, "%s what a step keeps depends on the forward substitution", tag);
                CHECK(p.kind == PX_FULL || p.kind == kind, "%s kind %d", tag, p.kind);
                if (p.kind == PX_FULL) {                      // keeps nothing, starts at group 0, panel_done owns every panel
                    CHECK(p.g0 == 0 && p.gB == 0 && p.cB == 0 && !p.e.ok && p.nranges == 0 && p.snap_doubles == 0 && p.snap_e_doubles == 0, "%s a full plan keeps something", tag);
                    CHECK(p.frB == p.frA && !p.fwd_prefix_launch && p.slack_first == slack_first, "%s a full plan's shortcuts", tag);
                    for (int64_t q = 0; q < g.npanels; ++q) CHECK(p.fwd_owner(q, true) == FwdOwner::PanelDone, "%s owner of %lld", tag, (long long)q);
                    continue;
                }
                check_keeps(g, sc, p, lam_e != 0, tag);
                CHECK(!p.early0, "%s early0 beside a prefix", tag);
                if (kind == PX_RECORD) {
                    CHECK(p.g0 == 0 && !p.slack_first && p.frB == p.frA && p.pE == 0, "%s a recording plan takes a shortcut", tag);
                    CHECK(p.snapshot_behind(p.gB - 1) == 1 && (!p.e.ok || p.snapshot_behind(p.e.gE - 1) == 2), "%s boundaries", tag);
                } else {
                    CHECK(p.g0 == (p.e.ok ? p.e.gE : p.gB) && p.slack_first == slack_first, "%s g0 %lld", tag, (long long)p.g0);
                    for (int64_t grp = 0; grp < ng; ++grp) CHECK(p.snapshot_behind(grp) == 0, "%s a reusing plan records", tag);
                    if (fuse) check_forward(g, sc, p, sweeps, tag);
                    else CHECK(p.frB == p.frA && !p.fwd_prefix_launch, "%s forward launches without fuse_forward", tag);
                    if (lam_e) { out_gB = p.gB; if (p.e.ok) { out_gS = p.e.gS; out_gE = p.e.gE; } }
                }
            }
        }
        printf("%lld %lld %lld %d %d %d %d %lld %lld %lld\n", n, me, mi, nb, group, lookahead, skip, out_gB, out_gS, out_gE);
        ++count;
    }
    printf("%ld lines replayed\n", count);
    return 0;
}
