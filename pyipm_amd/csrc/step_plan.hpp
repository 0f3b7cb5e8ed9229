// step_plan.hpp -- what one factorisation of the single-rank driver does, decided before its first launch: the group schedule
// (plan_groups) and the one statement of what a step keeps, copies and skips (make_step_plan).  Plain C++, nothing of HIP or of
// the handle: the assembly, the factorisation and the stand-alone replays (tests/test_step_plan.py, tests/test_step_plan_split.py) compile this one source.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>
namespace pyipm {
constexpr int PLAN_TB = 64;                   // the block-pivot tile (= TB, ctx.hpp)
constexpr int64_t TAIL_COLS = 24576;          // groups of tail_group panels once at most this many columns remain (plan_groups)
constexpr int PX_HDR = 32;                    // doubles in front of either snapshot: two records (SnapHeaders, pyipm_newton.hip), the
constexpr int PX_HDR_SECOND = 16;             // second one this many doubles behind the first

struct PlanGeo {                              // what of Geo (ctx.hpp) a plan depends on
    int64_t n, me, mi, Npad; int nb; int64_t npanels;
    int64_t panel_c0(int64_t p) const { return p * (int64_t)nb; }
    int64_t panel_w(int64_t p) const { const int64_t w = Npad - p * (int64_t)nb; return w < nb ? w : nb; }
};
struct SchedOpts { int group, tail_group; bool tail_group_user, skip_zeros; int lookahead; bool group_chain; };

// The group schedule of the single-rank driver as one value: which panels form a group (one bulk trailing update per group) and
// what the KKT structure says about each group.  plan_groups builds it for one geometry.  The accessors hold the fallback for a
// panel WITHOUT a schedule (per-panel phases, distributed driver): uniform groups of G panels, dense panels.
struct GroupSched {
    std::vector<int> of_, off_;           // per panel: group id and offset inside the group
    std::vector<int64_t> first_;          // per group: first panel (+ one past the last group)
    std::vector<char> fast_;              // per group: every panel of it lies inside the slack block: closed-form elimination (k_s_panel)
    std::vector<char> in_x_;              // per group: lies inside the x block (its chain kernels may skip the slack rows)
    bool active() const { return !of_.empty(); }
    void clear() { of_.clear(); off_.clear(); first_.clear(); fast_.clear(); in_x_.clear(); }   // the only way into per-panel mode
    bool has(int64_t p) const { return (size_t)p < of_.size(); }
    int64_t group_of(int64_t p, int64_t G) const { return has(p) ? of_[(size_t)p] : p / G; }
    int64_t offset_of(int64_t p, int64_t G) const { return has(p) ? off_[(size_t)p] : p % G; }
    bool fast_panel(int64_t p) const { return has(p) && fast(of_[(size_t)p]); }     bool in_x_panel(int64_t p) const { return has(p) && in_x(of_[(size_t)p]); }
    int64_t ngroups() const { return (int64_t)fast_.size(); }
    int64_t first(int64_t grp) const { return first_[(size_t)grp]; }      int64_t size(int64_t grp) const { return first(grp + 1) - first(grp); }
    bool fast(int64_t grp) const { return fast_[(size_t)grp] != 0; }      bool in_x(int64_t grp) const { return in_x_[(size_t)grp] != 0; }
};

// Three-level hierarchy: 64-wide block pivots inside nb-wide panels inside groups of `group` panels; the trailing matrix is
// updated ONCE per group with K = group*nb, which divides the C-tile read-modify-write traffic by `group`.  `group` panels per
// bulk update while it outlasts the panel chain; once at most TAIL_COLS columns remain the chain is the critical path and
// shorter groups end the factorisation sooner.  A pure function of its arguments.
inline GroupSched plan_groups(const PlanGeo& g, const SchedOpts& o) {
    GroupSched s;
    const int64_t np = g.npanels;
    const bool closed_form = o.skip_zeros && g.mi > 0;   // groups inside the slack block: closed-form elimination (k_s_panel)
    s.of_.assign((size_t)np, 0); s.off_.assign((size_t)np, 0);
    for (int64_t p = 0; p < np;) {
        const int64_t remaining = g.Npad - g.panel_c0(p);
        // (round 6: systems of at most 8192 rows take groups of 8 in the tail too -- with the chain of a group as ONE launch a group
        //  boundary costs more than the in-group updates of the longer group: config 2 2.25 against 2.29 ms; N = 32768: 4 stays)
        const int tg = (!o.tail_group_user && g.Npad <= 8192) ? 8 : o.tail_group;
        int64_t G = (tg > 0 && remaining <= TAIL_COLS) ? tg : o.group;
        if (G > o.group) G = o.group;
        if (p + G > np) G = np - p;
        // (round 5) the panels inside the slack block as ONE group: their kernels run up front (enqueue_slack_first) and what is left
        // of a slack group in the loop of factor_all is a head, a k_s_schur launch and four stream hops -- 56 us per group
        if (closed_form && o.lookahead && p > 0 && g.panel_c0(p) >= g.n && g.panel_c0(p + G - 1) + g.panel_w(p + G - 1) <= g.n + g.mi)
            while (p + G < np && g.panel_c0(p + G) + g.panel_w(p + G) <= g.n + g.mi) ++G;
        const int64_t ca = g.panel_c0(p), cb = g.panel_c0(p + G - 1) + g.panel_w(p + G - 1);      // the group's columns [ca, cb)
        for (int64_t q = 0; q < G; ++q) { s.of_[(size_t)(p + q)] = (int)s.first_.size(); s.off_[(size_t)(p + q)] = (int)q; }
        s.first_.push_back(p);
        s.in_x_.push_back(cb <= g.n ? 1 : 0);
        s.fast_.push_back((closed_form && ca >= g.n && cb <= g.n + g.mi) ? 1 : 0);
        p += G;
    }
    s.first_.push_back(np);
    return s;
}
// does group grp run as a tile chain (factor_group)?
inline bool chain_group(const PlanGeo& g, const GroupSched& sc, bool group_chain, int64_t grp) {
    return group_chain && !sc.fast(grp) && sc.size(grp) * (g.nb / PLAN_TB) <= 32 && g.nb % 128 == 0;
}

// ---- the reusable x-block prefix -------------------------------------------------------------------------
// Groups [0, gB) -- gB the first group that does not lie inside the x block -- are the prefix: they hold what stage_blocks staged
// and delta, nothing of s, lda or mu.  A RECORDING step is a full factorisation that copies the columns behind them, the statistics
// and the assembly's maximum into the snapshot once the prefix has been applied; a REUSING step re-assembles the slack columns,
// restores the rest from the snapshot, seeds the statistics and factors from group gB on.
enum { PX_FULL = 0, PX_RECORD = 1, PX_REUSE = 2 };
inline int64_t prefix_groups(const GroupSched& sc) { int64_t gB = 0; while (gB < sc.ngroups() && sc.in_x(gB)) ++gB; return gB; }
// The column ranges of the snapshot, [c0, c1) each with the rows [c0, Npad): what lies behind column cB except the panels wholly
// inside the slack block.  Returns the snapshot's doubles (header included).
struct PxRange { int64_t c0, c1, off; };
inline size_t prefix_ranges(const PlanGeo& g, int64_t cB, PxRange out[2], int* count) {
    int64_t s0 = 0, s1 = 0;                                  // the panels wholly inside the slack block: columns [s0, s1)
    if (g.mi > 0) { s0 = (g.n + g.nb - 1) / g.nb * g.nb; if (s0 < cB) s0 = cB; s1 = (g.n + g.mi) / g.nb * g.nb; }
    const int64_t cut[2][2] = {{cB, s1 > s0 ? s0 : g.Npad}, {s1 > s0 ? s1 : g.Npad, g.Npad}};
    size_t tot = PX_HDR; *count = 0;
    for (int k = 0; k < 2; ++k) {
        if (cut[k][1] <= cut[k][0]) continue;
        out[*count] = PxRange{cut[k][0], cut[k][1], (int64_t)tot};
        tot += (size_t)(cut[k][1] - cut[k][0]) * (size_t)(g.Npad - cut[k][0]); ++*count;
    }
    return tot;
}
// ---- the second level: the lambda_e groups -----------------------------------------------------------------
// The slack columns couple to lambda_i only, so the groups [gS, gE) that lie wholly inside the columns [n + mi, n + mi + me) are
// kept like the prefix.  gS is the first group behind the slack block, gE the first one that does not lie wholly inside lambda_e,
// cS / cE their first columns; a group that straddles either border is factored.  A reusing step applies the kept groups to the
// diagonal blocks behind cE (diag_update; the saved W) and takes everything else behind cE from the second snapshot.
struct LamE {
    bool ok = false; int64_t gS = 0, gE = 0, cS = 0, cE = 0;
    bool operator==(const LamE& o) const { return ok == o.ok && gS == o.gS && gE == o.gE && cS == o.cS && cE == o.cE; }
};
inline LamE lam_e_groups(const PlanGeo& g, const GroupSched& sc, int64_t gB) {
    LamE e;
    const int64_t ng = sc.ngroups(), e0 = g.n + g.mi, e1 = e0 + g.me;
    if (g.me <= 0 || g.mi <= 0 || gB <= 0 || gB >= ng) return e;
    auto c0 = [&](int64_t grp) { return grp >= ng ? g.Npad : g.panel_c0(sc.first(grp)); };
    int64_t gS = gB; while (gS < ng && c0(gS) < e0) ++gS;
    int64_t gE = gS; while (gE < ng && c0(gE + 1) <= e1) ++gE;
    if (gE == gS || gE >= ng) return e;                       // no whole group inside lambda_e, or none behind it
    e.ok = true; e.gS = gS; e.gE = gE; e.cS = c0(gS); e.cE = c0(gE);
    return e;
}
// The second snapshot: PX_HDR doubles, W of the columns [cS, cE) in the rows [cE, Npad) (leading dimension Npad - cE), the square.
inline size_t lam_e_doubles(const PlanGeo& g, const LamE& e) { const size_t rows = (size_t)(g.Npad - e.cE); return PX_HDR + rows * (size_t)(e.cE - e.cS) + rows * rows; }

// ---- the step plan: the assembly decides it (Held::plan), the factorisation derives it again and compares the two with == --------
// The forward substitution trails under the factorisation (fuse_forward; not part of ==: the factorisation alone knows it).  A
// reusing step has the kept panels' L at once: the prefix [0, pB) in one launch (fwd_prefix_launch) or panel by panel, the kept
// lambda_e groups [pS, pE) panel by panel -- or, a candidate the enqueue asks the device about (fwd_range_grid), the panels
// [frA, frB) in one launch: the slack panels too (fr_slack) where every group in [gB, gS) is closed-form and enqueued up front.
enum class FwdOwner { Prefix, Range, Kept, PanelDone };
struct StepPlan {
    int kind = PX_FULL;
    int64_t gB = 0, cB = 0; LamE e;       // the prefix: groups [0, gB), columns [0, cB); the lambda_e groups recorded / kept as well
    int64_t g0 = 0;                       // the first group of the lookahead loop
    bool early0 = false;                  // group 0 goes to the columns beyond it panel by panel (panel_done)
    bool slack_first = false;             // the closed-form panels of the slack block are enqueued up front (enqueue_slack_first)
    PxRange ranges[2] = {}; int nranges = 0; size_t snap_doubles = 0, snap_e_doubles = 0;   // the first snapshot's ranges, both sizes
    bool fuse_forward = false, fwd_prefix_launch = false, fr_slack = false;
    int64_t pB = 0, pS = 0, pE = 0, frA = 0, frB = 0;   // first panels of the groups gB, gS, gE (pS = pE = pB without the level)
    // The tail split (plan_tail_split; not part of ==, like the forward fields: the factorisation alone knows it).  Per group grp
    // of the lookahead loop: group grp + 1's chain starts behind group grp's chain launch -- which takes the rows of the next
    // diagonal block along -- and the diagonal block's share of the head; everything else of the hand-over runs beside it.
    std::vector<char> tail_split;
    bool split(int64_t grp) const { return grp >= 0 && (size_t)grp < tail_split.size() && tail_split[(size_t)grp] != 0; }
    bool operator==(const StepPlan& o) const {          // (what a step keeps: not the forward fields; the ranges follow from cB and the geometry)
        return kind == o.kind && gB == o.gB && cB == o.cB && e == o.e && g0 == o.g0 && early0 == o.early0 && slack_first == o.slack_first && snap_doubles == o.snap_doubles && snap_e_doubles == o.snap_e_doubles; }
    // a recording step, group grp complete: 1 -- the first snapshot follows it, 2 -- the second one, 0 -- neither
    int snapshot_behind(int64_t grp) const { return kind != PX_RECORD ? 0 : (e.ok && grp + 1 == e.gE) ? 2 : grp + 1 == gB ? 1 : 0; }
    FwdOwner fwd_owner(int64_t q, bool range_used) const {
        return q < pB ? FwdOwner::Prefix : range_used && q >= frA && q < frB ? FwdOwner::Range : q >= pS && q < pE ? FwdOwner::Kept : FwdOwner::PanelDone;
    }
};
// kind: what the caller asks for; the plan's own kind is PX_FULL where the schedule has no reusable prefix.  lam_e: the second
// level takes part.  sweeps: the one-launch forward sweeps apply to this handle (fwd_prefix_applies).
inline StepPlan make_step_plan(const PlanGeo& g, const GroupSched& sc, const SchedOpts& o, int kind, bool lam_e, bool fuse_forward, bool sweeps) {
    StepPlan p;
    const int64_t ng = sc.ngroups(), gB = prefix_groups(sc);
    if (kind != PX_FULL && gB > 0 && gB < ng && o.lookahead) {
        p.kind = kind; p.gB = gB; p.cB = g.panel_c0(sc.first(gB));
        if (lam_e) p.e = lam_e_groups(g, sc, gB);
        p.snap_doubles = prefix_ranges(g, p.cB, p.ranges, &p.nranges);
        if (p.e.ok) p.snap_e_doubles = lam_e_doubles(g, p.e);
    }
    const bool reuse = p.kind == PX_REUSE;
    p.g0 = reuse ? (p.e.ok ? p.e.gE : gB) : 0;
    p.early0 = p.kind == PX_FULL && o.lookahead >= 2 && ng > 2 && chain_group(g, sc, o.group_chain, 0) && sc.fast(1);
    if (p.kind != PX_RECORD && o.lookahead && !sc.fast(0)) for (int64_t gi = 1; gi < ng; ++gi) p.slack_first = p.slack_first || sc.fast(gi);
    p.fuse_forward = fuse_forward;          // (a recording step takes neither shortcut: both blur the point where the prefix is complete)
    if (!reuse) return p;
    p.pB = p.pS = p.pE = sc.first(gB); if (p.e.ok) { p.pS = sc.first(p.e.gS); p.pE = sc.first(p.e.gE); }
    p.fwd_prefix_launch = fuse_forward && sweeps && p.pB >= 1 && p.pB * g.nb <= g.n;
    if (p.e.ok && p.fwd_prefix_launch) {
        p.fr_slack = p.slack_first;
        for (int64_t grp = gB; grp < p.e.gS; ++grp) p.fr_slack = p.fr_slack && sc.fast(grp);
        p.frA = p.fr_slack ? p.pB : p.pS; p.frB = p.pE;
    }
    return p;
}

// ---- the tail split of a reusing step ----------------------------------------------------------------------
// Where the hand-over from group grp to group grp + 1 is split: a reusing step with lookahead, both groups tile chains, and the
// chain of group grp may take the rows of group grp + 1's diagonal block along (extra_ok(grp, rows): chain_extra_ok for the group
// seen as one block).  Recording and full steps, `pieces` (early0: full steps only) and `across` (the next group a slack group:
// no chain group) never qualify.  `on`: the handle's switch (PYIPM_TAIL_SPLIT).  tail_rows: only where at most this many rows are
// left from the next group's first column on (HEAD32_ROWS, ctx.hpp: where the chain is the bound) -- further up the moved head
// and the bulk update outlast the chains and queue on the main stream (first level alone at N = 32768: 11.3 -> 11.9 ms without it).
inline int64_t group_cols(const PlanGeo& g, const GroupSched& sc, int64_t grp) {
    int64_t w = 0; for (int64_t q = sc.first(grp); q < sc.first(grp + 1); ++q) w += g.panel_w(q); return w;
}
template <class ExtraOk>
inline void plan_tail_split(StepPlan& p, const PlanGeo& g, const GroupSched& sc, const SchedOpts& o, bool on, int64_t tail_rows, ExtraOk extra_ok) {
    const int64_t ng = sc.ngroups();
    p.tail_split.assign((size_t)ng, 0);
    if (!on || p.kind != PX_REUSE || !o.lookahead || p.early0) return;
    for (int64_t grp = p.g0; grp + 1 < ng; ++grp)
        p.tail_split[(size_t)grp] = chain_group(g, sc, o.group_chain, grp) && chain_group(g, sc, o.group_chain, grp + 1) &&
                                    g.Npad - g.panel_c0(sc.first(grp + 1)) <= tail_rows &&
                                    extra_ok(grp, group_cols(g, sc, grp + 1));
}
// ---- the enqueue items of the lookahead loop and what each waits for, as data (tests/step_plan_split_replay.cpp replays it) -------
// An item applies the columns of one source group `src` to rows [r0, r1) of the columns of one group `dst`: dst == src is the
// group's own factorisation (a stage), dst > src its update by src.  R(h): the rows of group h's diagonal block.
enum TailItem {
    TI_CHAIN,        // src = dst = h: R(h), the tile chain's launch (a group that is no chain group: all its rows, factor_panel)
    TI_XROWS,        // ... R(h + 1) in the same launch, where the hand-over h -> h + 1 is split
    TI_ROWS,         // ... the rows behind, the rows kernels (ctx->rest; the last sub-panel's on the chain's stream where h is not split)
    TI_HEAD_DIAG,    // src = h, dst = h + 1, split: R(h + 1) on the next chain's stream
    TI_HEAD_XROWS,   // ... R(h + 2) on the main stream, where h + 1 -> h + 2 is split too: the flag word is set behind it
    TI_HEAD_REST,    // ... the rows behind, on the main stream
    TI_HEAD_OLD,     // src = h, dst = h + 1, not split: head_from, all rows
    TI_BULK_NEXT,    // src = h, dst = h + 2, split: the next head's columns in a launch of their own (ev_main behind it)
    TI_BULK_REST,    // src = h, dst > h + 2 (split) or dst >= h + 2: the bulk update
    TI_COUNT
};
struct TailRegion { int item; int64_t src, dst, r0, r1; };
// rel 0: the reader's operands (L and W of group src) come from the writer, an item of src's own factorisation;
// rel 1: the writer is the stage before on the same entries (source src - 1, the same dst).
struct TailDep { int reader, writer, rel; const char* by; };
constexpr TailDep TAIL_DEPS[] = {
    {TI_XROWS, TI_CHAIN, 0, "same launch: the chain's progress words"},
    {TI_ROWS, TI_CHAIN, 0, "k_chain_wait on ctx->rest (pieces: ev_band); the last sub-panel where h is not split: ev_join"},
    {TI_HEAD_DIAG, TI_XROWS, 0, "stream order behind the chain's launch; ev_main where the source ran on the main stream"},
    {TI_HEAD_XROWS, TI_XROWS, 0, "ev_rows, recorded behind ev_chain_end"},
    {TI_HEAD_XROWS, TI_ROWS, 0, "ev_rows"},
    {TI_HEAD_REST, TI_XROWS, 0, "ev_rows, recorded behind ev_chain_end"},
    {TI_HEAD_REST, TI_ROWS, 0, "ev_rows"},
    {TI_HEAD_OLD, TI_ROWS, 0, "stream order: the last rows kernel runs on the chain's stream behind ev_join (ev_main behind group g0)"},
    {TI_HEAD_OLD, TI_CHAIN, 0, "stream order (a source that is no chain group)"},
    {TI_BULK_NEXT, TI_ROWS, 0, "ev_rows, then the main stream's order behind the head"},
    {TI_BULK_REST, TI_ROWS, 0, "split: as TI_BULK_NEXT; else ev_panel of the iteration before (ev_main / stream order behind g0)"},
    {TI_BULK_REST, TI_CHAIN, 0, "stream order / ev_panel (a source that is no chain group)"},
    {TI_CHAIN, TI_HEAD_DIAG, 1, "stream order (the chain's stream)"},
    {TI_CHAIN, TI_HEAD_OLD, 1, "stream order (the chain's stream; ev_head where the head ran on the main stream)"},
    {TI_XROWS, TI_HEAD_XROWS, 1, "the flag word, set behind that launch and enqueued before the chain that polls it"},
    {TI_XROWS, TI_HEAD_OLD, 1, "ev_head2 recorded on ctx->rest behind the old head, waited for by the chain's stream"},
    {TI_ROWS, TI_HEAD_REST, 1, "ev_head2"},
    {TI_ROWS, TI_HEAD_OLD, 1, "stream order on ctx->rest (ev_split), or the chain's stream"},
    {TI_HEAD_DIAG, TI_BULK_NEXT, 1, "ev_main, recorded behind that launch"},
    {TI_HEAD_DIAG, TI_BULK_REST, 1, "ev_main"},
    {TI_HEAD_XROWS, TI_BULK_NEXT, 1, "the main stream's order"},
    {TI_HEAD_XROWS, TI_BULK_REST, 1, "the main stream's order"},
    {TI_HEAD_REST, TI_BULK_NEXT, 1, "the main stream's order"},
    {TI_HEAD_REST, TI_BULK_REST, 1, "the main stream's order"},
    {TI_HEAD_OLD, TI_BULK_NEXT, 1, "ev_main, recorded behind that launch"},
    {TI_HEAD_OLD, TI_BULK_REST, 1, "ev_main"},
    {TI_BULK_NEXT, TI_BULK_REST, 1, "the main stream's order"},
    {TI_BULK_REST, TI_BULK_REST, 1, "the main stream's order"},
};
inline const TailDep* tail_dep(int reader, int writer, int rel) {
    for (const TailDep& d : TAIL_DEPS) if (d.reader == reader && d.writer == writer && d.rel == rel) return &d;
    return nullptr;
}
// The items of the groups [from, ngroups) as enqueue_groups, factor_block and head_split launch them for this plan (`from`: no
// slack group at or behind it; a head into or out of a slack group has forms of its own).
inline std::vector<TailRegion> tail_regions(const StepPlan& p, const PlanGeo& g, const GroupSched& sc, const SchedOpts& o, int64_t from) {
    std::vector<TailRegion> v;
    const int64_t ng = sc.ngroups();
    auto c0 = [&](int64_t h) { return h >= ng ? g.Npad : g.panel_c0(sc.first(h)); };
    for (int64_t h = from; h < ng; ++h) {
        const int64_t a = c0(h), b = c0(h + 1), x = p.split(h) ? c0(h + 2) : b;
        if (!chain_group(g, sc, o.group_chain, h)) { v.push_back({TI_CHAIN, h, h, a, g.Npad}); }
        else {
            v.push_back({TI_CHAIN, h, h, a, b});
            if (x > b) v.push_back({TI_XROWS, h, h, b, x});
            if (g.Npad > x) v.push_back({TI_ROWS, h, h, x, g.Npad});
        }
        if (h + 1 >= ng) continue;
        if (p.split(h)) {
            const int64_t t0 = b, t1 = c0(h + 2), xe = p.split(h + 1) ? c0(h + 3) : t1;
            v.push_back({TI_HEAD_DIAG, h, h + 1, t0, t1});
            if (xe > t1) v.push_back({TI_HEAD_XROWS, h, h + 1, t1, xe});
            if (g.Npad > xe) v.push_back({TI_HEAD_REST, h, h + 1, xe, g.Npad});
        } else v.push_back({TI_HEAD_OLD, h, h + 1, b, g.Npad});
        for (int64_t c = h + 2; c < ng; ++c)
            v.push_back({p.split(h) && c == h + 2 ? TI_BULK_NEXT : TI_BULK_REST, h, c, c0(c), g.Npad});
    }
    return v;
}
}  // namespace pyipm
