// The tail split of a reusing step, replayed on the CPU (tests/test_step_plan_split.py compiles and runs this with the address and
// undefined-behaviour sanitizers).  It includes pyipm_amd/csrc/step_plan.hpp, plans the reusing step of every geometry it is
// given with plan_tail_split, takes the enqueue items of the lookahead loop from tail_regions and checks, per geometry:
//   * every (rows, columns) region of every group is written by exactly one item per stage -- a stage is one source group applied
//     to one group's columns (the group's own factorisation included), the rows from the columns' first one to the end;
//   * every item's operands and the stage before it on the same entries come from items that TAIL_DEPS lists as waited for;
//   * where the split applies, restated here from the issue's conditions, not from the header.
// stdin: lines "n me mi nb group tail_group switch" (tail_group 0: the handle's default, not the user's; lookahead 2, skip_zeros on).
// stdout: per line "n me mi nb group tail_group switch g0 ngroups nsplit first_split", then "deps <bitmap of TAIL_DEPS used>",
// then "<count> lines replayed".
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "step_plan.hpp"

using namespace pyipm;
#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "FAILED %s: ", #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

// what the library's chain_extra_ok says for a group seen as one block, with a handle's defaults (one launch per chain where at most
// 12288 rows are left, 160 progress words, at most 16 extra row tiles, no hole behind the x block)
static bool extra_ok(const PlanGeo& g, const GroupSched& sc, int64_t grp, int64_t xrows) {
    const int64_t c0 = g.panel_c0(sc.first(grp)), c1 = grp + 1 >= sc.ngroups() ? g.Npad : g.panel_c0(sc.first(grp + 1));
    const int64_t nt = (c1 - c0) / 64, xr = xrows / 64;
    if (xrows <= 0 || xrows % 64 || xr > 16 || c1 + xrows > g.Npad) return false;
    if (nt < 2 || nt > 32 || g.Npad - c0 > 12288) return false;
    if (1 + 4 * (nt + xr) > 160) return false;
    return !sc.in_x(grp);
}

int main() {
    long long n, me, mi; int nb, group, tg, on; long count = 0;
    const int ndeps = (int)(sizeof(TAIL_DEPS) / sizeof(TAIL_DEPS[0]));
    std::vector<char> used((size_t)ndeps, 0);
    while (scanf("%lld %lld %lld %d %d %d %d", &n, &me, &mi, &nb, &group, &tg, &on) == 7) {
        PlanGeo g{n, me, mi, 0, nb, 0};
        g.Npad = (n + 2 * mi + me + 127) / 128 * 128; if (g.Npad == 0) g.Npad = 128;
        g.npanels = (g.Npad + nb - 1) / nb;
        const SchedOpts o{group, tg > 0 ? tg : 4, tg > 0, true, 2, true};
        const GroupSched sc = plan_groups(g, o);
        const int64_t ng = sc.ngroups();
        char tag[128]; snprintf(tag, sizeof(tag), "(%lld %lld %lld nb %d group %d tail %d switch %d)", n, me, mi, nb, group, tg, on);
        auto c0 = [&](int64_t h) { return h >= ng ? g.Npad : g.panel_c0(sc.first(h)); };
        auto ok = [&](int64_t grp, int64_t rows) { return extra_ok(g, sc, grp, rows); };
        // recording and full steps never split
        for (int kind = PX_FULL; kind <= PX_RECORD; ++kind) {
            StepPlan q = make_step_plan(g, sc, o, kind, true, true, true);
            plan_tail_split(q, g, sc, o, true, 6144, ok);
            for (int64_t h = 0; h < ng; ++h) CHECK(!q.split(h), "%s kind %d splits group %lld", tag, kind, (long long)h);
        }
        StepPlan p = make_step_plan(g, sc, o, PX_REUSE, true, true, true);
        plan_tail_split(p, g, sc, o, on != 0, 6144, ok);
        long long nsplit = 0, first_split = -1;
        if (p.kind != PX_REUSE) {
            for (int64_t h = 0; h < ng; ++h) CHECK(!p.split(h), "%s a full step splits", tag);
            printf("%lld %lld %lld %d %d %d %d -1 %lld 0 -1\n", n, me, mi, nb, group, tg, on, (long long)ng);
            ++count; continue;
        }
        // where the split applies: the issue's conditions
        for (int64_t h = 0; h < ng; ++h) {
            const bool want = on && h >= p.g0 && h + 1 < ng && chain_group(g, sc, true, h) && chain_group(g, sc, true, h + 1) &&
                              g.Npad - c0(h + 1) <= 6144 && extra_ok(g, sc, h, c0(h + 2) - c0(h + 1));
            CHECK(p.split(h) == want, "%s group %lld split %d", tag, (long long)h, (int)p.split(h));
            if (want) { ++nsplit; if (first_split < 0) first_split = h; CHECK(c0(h + 2) - c0(h + 1) <= 16 * 64, "%s extra rows", tag); }
        }
        // the part of the loop with no slack group in it
        int64_t from = p.g0; for (int64_t h = p.g0; h < ng; ++h) if (sc.fast(h)) from = h + 1;
        CHECK(first_split < 0 || first_split >= from, "%s a split in front of a slack group", tag);
        const std::vector<TailRegion> items = tail_regions(p, g, sc, o, from);
        // exactly one item per stage and row tile
        for (int64_t s = from; s < ng; ++s) for (int64_t d = s; d < ng; ++d) {
            std::vector<int> hits((size_t)((g.Npad - c0(d)) / 64), 0);
            for (const TailRegion& it : items) {
                if (it.src != s || it.dst != d) continue;
                CHECK(it.r0 >= c0(d) && it.r1 <= g.Npad && it.r0 < it.r1 && it.r0 % 64 == 0 && it.r1 % 64 == 0, "%s item %d rows [%lld, %lld)", tag, it.item, (long long)it.r0, (long long)it.r1);
                for (int64_t r = it.r0; r < it.r1; r += 64) ++hits[(size_t)((r - c0(d)) / 64)];
            }
            for (size_t k = 0; k < hits.size(); ++k) CHECK(hits[k] == 1, "%s stage %lld -> %lld row tile %zu written %d times", tag, (long long)s, (long long)d, k, hits[k]);
        }
        for (const TailRegion& it : items) CHECK(it.src >= from && it.dst >= it.src && it.dst < ng, "%s item %d of stage %lld -> %lld", tag, it.item, (long long)it.src, (long long)it.dst);
        // every reader's writers are in its wait list
        auto need = [&](const TailRegion& rd, int64_t s, int64_t d, int64_t r0, int64_t r1, int rel) {
            bool any = false;
            for (const TailRegion& w : items) {
                if (w.src != s || w.dst != d || w.r1 <= r0 || w.r0 >= r1 || &w == &rd) continue;
                any = true;
                const TailDep* dep = tail_dep(rd.item, w.item, rel);
                CHECK(dep != nullptr, "%s item %d (%lld -> %lld rows [%lld, %lld)) reads item %d (rel %d) and does not wait for it", tag, rd.item,
                      (long long)rd.src, (long long)rd.dst, (long long)rd.r0, (long long)rd.r1, w.item, rel);
                used[(size_t)(dep - TAIL_DEPS)] = 1;
            }
            CHECK(any, "%s item %d reads rows [%lld, %lld) of stage %lld -> %lld that nobody writes", tag, rd.item, (long long)r0, (long long)r1, (long long)s, (long long)d);
        };
        for (const TailRegion& it : items) {
            if (it.src == it.dst) {
                if (it.item != TI_CHAIN) need(it, it.src, it.src, c0(it.src), c0(it.src + 1), 0);       // the tiles and W of the diagonal block
            } else {
                need(it, it.src, it.src, it.r0, it.r1, 0);                                              // L of the source in my rows
                need(it, it.src, it.src, c0(it.dst), c0(it.dst + 1), 0);                                // W of the source in my columns' rows
            }
            if (it.src > from) need(it, it.src - 1, it.dst, it.r0, it.r1, 1);                           // the stage before on my entries
        }
        printf("%lld %lld %lld %d %d %d %d %lld %lld %lld %lld\n", n, me, mi, nb, group, tg, on, (long long)p.g0, (long long)ng, nsplit, first_split);
        ++count;
    }
    printf("deps ");
    for (int k = 0; k < ndeps; ++k) putchar(used[(size_t)k] ? '1' : '0');
    printf("\n%ld lines replayed\n", count);
    return 0;
}
