// pyipm_newton.hip — C-ABI of the MI355X Newton-step core (declared in include/pyipm_newton.h).
// gfx950 only; no CUDA path, no CPU fallback.  Host-side orchestration of the HIP kernels in
// kernels_*.hpp.  Replaces /root/reference/pyipm.py:1717-1725 (see the header for the mapping).
#include "driver.hpp"
#include "sub_walk.hpp"
#include "kernels_assemble.hpp"
#include "kernels_factor.hpp"
#include "kernels_panel.hpp"
#include "kernels_chain.hpp"
#include "kernels_solve.hpp"
#include "kernels_msolve.hpp"
#include "kernels_kmany.hpp"
#include "kernels_batched.hpp"
#include "kernels_merit.hpp"

using namespace pyipm;
using namespace pyipm::drv;

namespace pyipm { namespace drv {


// Workspace layout; returns total bytes.  When base != nullptr also sets the pointers.
size_t carve_workspace(Ctx* c, const Geo& g, char* base, bool provider_only = false) {
    Carve cv;
    const size_t D = sizeof(double);
    // (a provider-only handle -- pyipm_newton_create_provider: block products and residuals, no factorisation -- has no KKT
    //  storage, no W buffers, no tile inverses: N^2 x 8 bytes that an L-BFGS run never needs)
    const size_t oA = cv.take(provider_only ? 256 : (size_t)g.Npad * (size_t)(g.ncols_local > 0 ? g.ncols_local : 1) * D);
    const size_t oW = cv.take(provider_only ? 256 : 3 * (size_t)default_group(g.world, g.nb) * (size_t)g.Npad * g.nb * D);   // -W of a panel group, three rotating buffers (group g+1 is written while g is read)
    const size_t oL = cv.take(g.world > 1 ? (size_t)g.Npad * g.nb * D : 256);
    const size_t oD = cv.take(provider_only ? 256 : (size_t)(g.Npad / TB) * TB * TB * D);
    const size_t oT = cv.take(provider_only ? 256 : (size_t)(g.Npad / TB) * TB * TB * D);
    const size_t oTf = cv.take((size_t)(g.Npad / TB + 1) * D);
    const size_t orhs = cv.take((size_t)g.Npad * D);
    const size_t ov0 = cv.take((size_t)g.Npad * D);
    const size_t ov1 = cv.take((size_t)g.Npad * D);
    const size_t ov2 = cv.take((size_t)g.Npad * D);
    const size_t ov3 = cv.take((size_t)g.Npad * D);
    const size_t nchunk = (size_t)((g.Npad + ROWCHUNK - 1) / ROWCHUNK) + 1;
    size_t npart = nchunk * (size_t)g.nb;
    const size_t cd_chunks = 64;                       // column-dot partials for the mat-vec
    size_t maxcol = (size_t)(g.n > g.me ? g.n : g.me); if ((size_t)g.mi > maxcol) maxcol = g.mi;
    if (cd_chunks * maxcol > npart) npart = cd_chunks * maxcol;
    {   // one-pass symmetric product (k_symv_tiles): 64 chunks of column partials + one row partial per column segment
        const size_t nseg = ((size_t)g.n + SYMV_SEG - 1) / SYMV_SEG;
        if (((size_t)SYMV_CHUNKS + nseg) * (size_t)g.n > npart) npart = ((size_t)SYMV_CHUNKS + nseg) * (size_t)g.n;
        // ... and the same for a Jacobian block (k_jac_tiles: [SYMV_CHUNKS][m] column partials + [segments of m][n] row partials)
        const size_t mm = (size_t)(g.me > g.mi ? g.me : g.mi), jseg = (mm + SYMV_SEG - 1) / SYMV_SEG;
        if ((size_t)SYMV_CHUNKS * mm + jseg * (size_t)g.n > npart) npart = (size_t)SYMV_CHUNKS * mm + jseg * (size_t)g.n;
    }
    const size_t op = cv.take(npart * D);
    const size_t odf = cv.take((size_t)(g.n + 1) * D);
    const size_t oce = cv.take((size_t)(g.me + 1) * D);
    const size_t oci = cv.take((size_t)(g.mi + 1) * D);
    const size_t os = cv.take((size_t)(g.mi + 1) * D);
    const size_t ol = cv.take((size_t)(g.me + g.mi + 1) * D);
    const size_t ost = cv.take(sizeof(DevStats));
    const size_t ovc = cv.take((size_t)g.Npad * D);
    const size_t ovt = cv.take((size_t)(g.mi + 16) * D);
    const size_t oan = cv.take(64);
    const size_t own = cv.take((size_t)TB * TB * D);
    if (base) {
        c->Wnext = (double*)(base + own);
        c->vc = (double*)(base + ovc); c->vt = (double*)(base + ovt);
        c->anorm = (unsigned long long*)(base + oan);

        c->A = (double*)(base + oA); c->Wbuf = (double*)(base + oW); c->Lbuf = (double*)(base + oL);
        c->Dinv = (double*)(base + oD); c->Tsv = (double*)(base + oT); c->Tflag = (double*)(base + oTf); c->rhs = (double*)(base + orhs);
        c->v0 = (double*)(base + ov0); c->v1 = (double*)(base + ov1); c->v2 = (double*)(base + ov2);
        c->v3 = (double*)(base + ov3);
        c->partial = (double*)(base + op);
        c->df = (double*)(base + odf); c->ce = (double*)(base + oce); c->ci = (double*)(base + oci);
        c->s = (double*)(base + os); c->lda = (double*)(base + ol);
        c->dstats = (DevStats*)(base + ost);
    }
    return cv.off;
}

// Batched small-system handles: per problem A (Npad^2), tile inverses / tiles / flags, rhs and solution, the
// staged vectors; no W buffer (the upper blocks of A hold it) and no panel machinery.
size_t carve_batched(Ctx* c, const Geo& g, int64_t B, char* base) {
    Carve cv;
    const size_t D = sizeof(double), nt = (size_t)(g.Npad / TB);
    const size_t oA = cv.take((size_t)B * g.Npad * g.Npad * D);
    const size_t oD = cv.take((size_t)B * nt * TB * TB * D);
    const size_t oT = cv.take((size_t)B * nt * TB * TB * D);
    const size_t oTf = cv.take((size_t)B * nt * D);
    const size_t orhs = cv.take((size_t)B * g.Npad * D);
    const size_t ov0 = cv.take((size_t)B * g.Npad * D);
    const size_t ov2 = cv.take((size_t)B * g.N * D);
    const size_t odf = cv.take((size_t)B * (g.n + 1) * D);
    const size_t oce = cv.take((size_t)B * (g.me + 1) * D);
    const size_t oci = cv.take((size_t)B * (g.mi + 1) * D);
    const size_t os = cv.take((size_t)B * (g.mi + 1) * D);
    const size_t ol = cv.take((size_t)B * (g.me + g.mi + 1) * D);
    const size_t ost = cv.take((size_t)B * sizeof(DevStats));
    const size_t oan = cv.take((size_t)B * 2 * sizeof(unsigned long long));
    // condensed form (set_option("condensed", 1)): per problem the active set -- position, members, count -- and the backward errors
    const size_t ocp = cv.take((size_t)B * (size_t)(2 * g.mi + 2) * sizeof(int) + (size_t)B * sizeof(int));
    const size_t obe = cv.take((size_t)B * sizeof(double));
    const size_t osg = cv.take((size_t)B * (size_t)(g.mi + 1) * sizeof(double));
    // per-problem mu / delta / delta_c and activity flags, the landing place of host arrays for them, host step lengths
    const size_t opar = cv.take((size_t)B * 3 * D);
    const size_t oact = cv.take((size_t)B * sizeof(int));
    const size_t oin = cv.take((size_t)B * 3 * D);
    const size_t oia = cv.take((size_t)B * sizeof(int));
    const size_t oal = cv.take((size_t)B * 2 * D);
    if (base) {
        c->b_mu = (double*)(base + opar); c->b_delta = c->b_mu + B; c->b_delta_c = c->b_delta + B;
        c->b_act = (int*)(base + oact);
        c->b_in = (double*)(base + oin); c->b_in_act = (int*)(base + oia);
        c->b_alpha = (double*)(base + oal);
        c->WT = (double*)(base + osg);                  // (batched handle: Sigma of the eliminated pairs, the Gram operand's scaling)
        c->cond_pos = (int*)(base + ocp); c->cond_idx = c->cond_pos + (size_t)B * (size_t)(g.mi + 1);
        c->cond_cnt = c->cond_idx + (size_t)B * (size_t)(g.mi + 1);
        c->vt = (double*)(base + obe);
        c->anorm = (unsigned long long*)(base + oan);
        c->A = (double*)(base + oA); c->Dinv = (double*)(base + oD); c->Tsv = (double*)(base + oT);
        c->Tflag = (double*)(base + oTf); c->rhs = (double*)(base + orhs); c->v0 = (double*)(base + ov0);
        c->v2 = (double*)(base + ov2);
        c->df = (double*)(base + odf); c->ce = (double*)(base + oce); c->ci = (double*)(base + oci);
        c->s = (double*)(base + os); c->lda = (double*)(base + ol); c->dstats = (DevStats*)(base + ost);
    }
    return cv.off;
}

BatchPtrs batch_ptrs(Ctx* ctx) {
    const Geo& g = ctx->g;
    BatchPtrs bp;
    const int64_t nt = g.Npad / TB;
    bp.A = ctx->A; bp.sA = g.Npad * g.Npad;
    bp.Tinv = ctx->Dinv; bp.Tsave = ctx->Tsv; bp.sT = nt * TB * TB;
    bp.Tflag = ctx->Tflag; bp.sF = nt;
    bp.st = ctx->dstats;
    bp.rhs = ctx->rhs; bp.sol = ctx->v0; bp.sV = g.Npad;
    bp.d2L = ctx->d2L; bp.Je = ctx->Je; bp.Ji = ctx->Ji;
    bp.sH = ctx->b_sH; bp.sJe = ctx->b_sJe; bp.sJi = ctx->b_sJi;
    bp.ldh = ctx->ld_d2L; bp.ldje = ctx->ld_Je; bp.ldji = ctx->ld_Ji;
    bp.df = ctx->df; bp.ce = ctx->ce; bp.ci = ctx->ci; bp.s = ctx->s; bp.lda = ctx->lda;
    bp.anorm = ctx->anorm;
    bp.pmu = ctx->b_mu; bp.pdelta = ctx->b_delta; bp.pdelta_c = ctx->b_delta_c; bp.act = ctx->b_act;
    return bp;
}

BatchCond batch_cond(Ctx* ctx) {
    BatchCond bc;
    bc.pos = ctx->cond_pos; bc.idx = ctx->cond_idx; bc.cnt = ctx->cond_cnt; bc.sig = ctx->WT; bc.sP = ctx->g.mi + 1;
    bc.sigma_max = ctx->cond_sigma_max;
    return bc;
}


// copy `count` doubles from caller memory (host or device) into library device memory
int put_vec(Ctx* ctx, double* dst, const double* src, size_t count, int memkind) {
    if (count == 0) return 0;
    if (!src) { ctx->err = "null vector pointer"; return PYIPM_E_BADARG; }
    PYIPM_HIP(hipMemcpyAsync(dst, src, count * sizeof(double),
                             memkind == PYIPM_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice,
                             ctx->stream));
    if (memkind == PYIPM_MEM_HOST) PYIPM_HIP(hipStreamSynchronize(ctx->stream));   // host memory not retained
    return 0;
}

int stage_block(Ctx* ctx, const double* src, int64_t rows, int64_t cols, int64_t ld, int memkind,
                DevBuf<double>& stg, const double** out_ptr, int64_t* out_ld) {
    if (rows == 0 || cols == 0) { *out_ptr = nullptr; *out_ld = cols; return 0; }
    if (!src || ld < cols) { ctx->err = "bad block pointer / leading dimension"; return PYIPM_E_BADARG; }
    if (memkind == PYIPM_MEM_DEVICE) { *out_ptr = src; *out_ld = ld; return 0; }
    PYIPM_HIP(stg.reserve((size_t)rows * (size_t)cols));
    PYIPM_HIP(hipMemcpy2DAsync(stg.get(), (size_t)cols * sizeof(double), src, (size_t)ld * sizeof(double),
                               (size_t)cols * sizeof(double), (size_t)rows, hipMemcpyHostToDevice, ctx->stream));
    PYIPM_HIP(hipStreamSynchronize(ctx->stream));
    *out_ptr = stg.get(); *out_ld = cols;
    return 0;
}


// ---- per-panel building blocks -----------------------------------------------------------------

// Rows (= columns, by symmetry) on which a rank-K update with source columns [cA, cB) can be non-zero.
// KKT order [x | s | lambda_e | lambda_i] (pyipm.py:824-842): the (s,x) block is zero and nothing fills it, so
// while the source columns lie in the x block the s rows of L (and the s rows of W) are exact zeros; while they
// lie in the s block (diagonal Sigma, -I towards lambda_i) only the matching lambda_i rows are touched.
void active_ranges(const Ctx* ctx, int64_t cA, int64_t cB, int64_t* a0, int64_t* a1, int64_t* b0, int64_t* b1) {
    const Geo& g = ctx->g;
    *a0 = 0; *a1 = g.Npad; *b0 = 0; *b1 = 0;
    if (!ctx->skip_zeros || g.mi == 0) return;
    const int64_t s0 = g.n, s1 = g.n + g.mi, i0 = g.n + g.mi + g.me;
    if (cB <= s0)                { *a0 = 0; *a1 = s0; *b0 = s1; *b1 = g.Npad; }              // x-block sources
    else if (cA >= s0 && cB <= s1) { *a0 = i0 + (cA - s0); *a1 = i0 + (cB - s0); *b0 = 0; *b1 = 0; }   // s-block sources
}

// lower-triangle entries (i >= j) with i in rows, j in [j0, j1), both restricted to the active ranges
double active_area(int64_t row_begin, int64_t Npad, int64_t j0, int64_t j1, int64_t a0, int64_t a1, int64_t b0, int64_t b1) {
    double area = 0.0;
    const int64_t rng[2][2] = {{a0, a1}, {b0, b1}};
    for (int cj = 0; cj < 2; ++cj) {
        const int64_t ja = j0 > rng[cj][0] ? j0 : rng[cj][0], jb = j1 < rng[cj][1] ? j1 : rng[cj][1];
        if (jb <= ja) continue;
        for (int ri = 0; ri < 2; ++ri) {
            int64_t ia = rng[ri][0] > row_begin ? rng[ri][0] : row_begin, ib = rng[ri][1] < Npad ? rng[ri][1] : Npad;
            if (ib <= ia) continue;
            // sum over j in [ja,jb) of #{ i in [ia,ib) : i >= j }
            for (int64_t j = ja; j < jb; ++j) { const int64_t lo = ia > j ? ia : j; if (ib > lo) area += (double)(ib - lo); }
        }
    }
    return area;
}

// Compact, XCD-aware tile order of one swizzled launch.  The device decode (k_update, SWZ) is replayed here for
// every block; tiles that are out of range, above the diagonal or structurally zero are dropped, the eight
// per-XCD sequences (block b runs on XCD b % 8) are levelled by moving the tails of long ones to short ones,
// and the result is interleaved back into launch order.  Cached per geometry: it repeats every step.
// The list reaches the device WITHOUT a host synchronisation (round 4): built into pinned host memory, copied with
// hipMemcpyAsync on the stream of its first consumer (a plain hipMemcpy is ordered against the legacy default stream -- with
// torch's default stream as the handle's stream every list of a first factorisation waited for all the work enqueued so
// far: 35 lists, 98 ms of host time, the GPU idle behind the host for 25 ms of the first step of every solve); a consumer on
// another stream waits for the copy's event until it has been seen complete.  Device and host memory come from arenas.
int tile_list(Ctx* ctx, const UpdGeo& u, int64_t nsup, const unsigned** dev, unsigned* count, int bn = 128,
              hipStream_t consumer = nullptr) {
    if (ctx->debug_fault == 1 || ctx->debug_fault == 2) {   // test hook (tests/test_gpu_host_abi.py): the containers below can throw
        const int k = ctx->debug_fault; ctx->debug_fault = 0;
        if (k == 1) throw std::bad_alloc();
        throw std::runtime_error("injected fault");
    }
    std::vector<int64_t> key = {u.row_begin, u.Npad, u.first_lp, u.nrt, u.nct, u.a0, u.a1, u.b0, u.b1, u.nb, u.rt_min0, u.rt_step, bn, u.sub0};
    auto it = ctx->tile_lists.find(key);
    if (it != ctx->tile_lists.end()) {
        Ctx::TileList& t = it->second;
        if (t.ready && !t.seen_done) {
            if (hipEventQuery(t.ready) == hipSuccess) t.seen_done = true;
            else if (consumer != t.on) PYIPM_HIP(hipStreamWaitEvent(consumer, t.ready, 0));
        }
        *dev = t.dev; *count = t.count; return 0;
    }
    if (ctx->tile_lists.size() >= 1024) {              // geometries that keep changing (condensed option: |A| varies): start over
        PYIPM_HIP(hipDeviceSynchronize());
        ctx->tile_lists.clear();
        for (auto& a : ctx->tl_arenas) { a.used = 0; }
    }
    const auto t_build0 = std::chrono::steady_clock::now();
    struct BuildTimer { Ctx* c; std::chrono::steady_clock::time_point t0;
                        ~BuildTimer() { c->setup_lists_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); c->setup_lists_n++; } } bt_{ctx, t_build0};
    const int64_t rounds = (nsup + 7) / 8, nblocks = rounds * 8 * SUPER * SUPER;
    const int nsr = (u.nrt + SUPER - 1) >> 3, nsc = (u.nct + SUPER - 1) >> 3;
    std::vector<unsigned> seq[8];
    for (int64_t b = 0; b < nblocks; ++b) {
        const int xcd = (int)(b & 7);
        const int64_t slot = b >> 3;
        int sidx = (int)((slot >> 6) * 8) + xcd;
        const int within = (int)(slot & 63);
        int sJ = 0, sI = -1;
        for (; sJ < nsc; ++sJ) {
            const int mn = upd_super_min_row(u, sJ);
            const int cnt = mn < nsr ? nsr - mn : 0;
            if (sidx < cnt) { sI = mn + sidx; break; }
            sidx -= cnt;
        }
        if (sI < 0) continue;
        const int64_t rt = (int64_t)sI * SUPER + (within & (SUPER - 1)), ct = (int64_t)sJ * SUPER + (within >> 3);
        if (rt >= u.nrt || ct >= u.nct) continue;
        int64_t jglob, jloc;
        if (bn == 256) upd_col<256>(u, ct, jglob, jloc); else if (bn == 64) upd_col<64>(u, ct, jglob, jloc); else upd_col<128>(u, ct, jglob, jloc);
        if (jglob >= u.Npad) continue;
        const int64_t i0 = u.row_begin + rt * BM;
        if (i0 + BM <= jglob) continue;
        const bool ri = (i0 + BM > u.a0 && i0 < u.a1) || (i0 + BM > u.b0 && i0 < u.b1);
        const bool ci = (jglob + bn > u.a0 && jglob < u.a1) || (jglob + bn > u.b0 && jglob < u.b1);
        if (!(ri && ci)) continue;
        seq[xcd].push_back((unsigned)rt | ((unsigned)ct << 16));
    }
    size_t total = 0;
    for (auto& v : seq) total += v.size();
    const size_t target = (total + 7) / 8;
    std::vector<unsigned> spare;
    for (auto& v : seq) while (v.size() > target) { spare.push_back(v.back()); v.pop_back(); }
    for (auto& v : seq) while (v.size() < target && !spare.empty()) { v.push_back(spare.back()); spare.pop_back(); }
    std::vector<unsigned> list(8 * target, 0xffffffffu);
    for (int x = 0; x < 8; ++x) for (size_t j = 0; j < seq[x].size(); ++j) list[8 * j + x] = seq[x][j];
    Ctx::TileList tl;
    tl.count = (unsigned)list.size();
    if (tl.count) {
        // a slot in the arenas (device + pinned host, 1 Mi entries each; a list longer than that gets an arena of its own)
        const size_t need = (list.size() + 63) / 64 * 64;
        Ctx::TlArena* ar = nullptr;
        for (auto& a : ctx->tl_arenas) if (a.dev.capacity() - a.used >= need) { ar = &a; break; }
        if (!ar) {
            Ctx::TlArena a;
            const size_t cap = need > ((size_t)1 << 20) ? need : ((size_t)1 << 20);
            PYIPM_HIP(a.dev.reserve(cap));
            if (a.host.reserve(cap) != hipSuccess) { ctx->err = "no pinned host memory for the tile lists"; return PYIPM_E_NOMEM; }
            ctx->tl_arenas.push_back(std::move(a));
            ar = &ctx->tl_arenas.back();
        }
        tl.dev = ar->dev + ar->used;
        unsigned* hsrc = ar->host + ar->used;
        ar->used += need;
        memcpy(hsrc, list.data(), list.size() * sizeof(unsigned));
        PYIPM_HIP(hipMemcpyAsync(tl.dev, hsrc, list.size() * sizeof(unsigned), hipMemcpyHostToDevice, consumer));
        PYIPM_HIP(tl.ready.ensure(hipEventDisableTiming));
        PYIPM_HIP(hipEventRecord(tl.ready, consumer));
        tl.on = consumer;
    }
    *dev = tl.dev; *count = tl.count;
    ctx->tile_lists[key] = std::move(tl);
    return 0;
}

// Rank-K update of `n_lp` locally owned panels starting at local panel `first_lp` (UpdLaunch, driver.hpp: what a call may set).
int launch_update128(Ctx* ctx, hipStream_t stream, const double* Lop, int64_t ldl, const double* Wop, int K,
                     int64_t row_begin, int64_t first_lp, int64_t n_lp, const UpdLaunch& o) {
    const Geo& g = ctx->g;
    const int64_t ldw = o.ldw > 0 ? o.ldw : g.Npad;
    const int64_t row_end = o.row_end > 0 ? o.row_end : g.Npad;
    const int64_t col_end = o.col_end > 0 ? o.col_end : g.Npad;
    const bool bulk = o.bulk;
    const int waves = o.waves, ksplit = o.ksplit, nct_sub = o.nct_sub;
    const int64_t m = row_end - row_begin;
    if (m <= 0 || n_lp <= 0) return 0;
    UpdGeo u;
    u.row_begin = row_begin; u.Npad = col_end; u.first_lp = first_lp; u.sub0 = o.sub0;
    u.nb = g.nb; u.world = g.world; u.rank = g.rank;
    u.nrt = (int)(m / BM); u.nct = nct_sub > 0 ? nct_sub : (int)(n_lp * (g.nb / 128));
    u.dbg = ctx->dbg_buf;
    u.prio = o.prio >= 0 ? o.prio : (bulk ? 0 : SIDE_PRIO);
    u.rt_min0 = 0; u.rt_step = 0; u.tiles = nullptr; u.ks_cstride = 0; u.persist = 0;
    u.head_ct = 0; u.head_counter = nullptr;          // (the fused head of round 3: no launch uses it)
    if (o.src_c0 >= 0) active_ranges(ctx, o.src_c0, o.src_c0 + K, &u.a0, &u.a1, &u.b0, &u.b1);
    else { u.a0 = 0; u.a1 = g.Npad; u.b0 = 0; u.b1 = 0; }
    const int use_waves = waves ? waves : BULK_WAVES;
    if (o.tiles) {
        // The partial Gram launch (lbfgs_impl.hpp): the tiles the caller lists, on the bulk 128 x 128 instance.  Whatever instance
        // the full launch took, every entry receives its products k ascending in MFMA groups of 4: the same bits.
        if (o.ntiles == 0) return 0;
        if (o.ntiles % 8 != 0 || first_lp != 0 || o.sub0 != 0 || g.world != 1) { ctx->err = "bad caller tile list"; return PYIPM_E_BADARG; }
        u.tiles = o.tiles;
        if (ksplit > 1) u.ks_cstride = o.ks_cstride;
        hipLaunchKernelGGL((k_update<128, true, 8>), dim3(o.ntiles, (unsigned)ksplit), dim3(512), 0, stream, ctx->A, g.Npad, Lop, ldl, Wop, ldw, K, u);
        PYIPM_KCHECK();
        return 0;
    }
    // (col_end % 256: Npad is a multiple of 128 only -- a 256-wide tile at the last 128 columns would read and rewrite 128
    // columns past the storage, i.e. the first W slot, and W rows past Npad; such shapes keep 128 x 128 tiles)
    if (bulk && ctx->bulk_bn == 256 && use_waves == 8 && waves == 0 && ksplit == 1 && g.nb % 256 == 0 &&
        col_end % 256 == 0 && K >= BULK_BN_MIN_K && nct_sub == 0 && (ctx->reserve_cus <= 0 || m > (BULK_BN_ROWS > ctx->persist_rows ? BULK_BN_ROWS : ctx->persist_rows))) {
        // 128 x 256 tiles (the K = 1024 bulk launches of the single-rank schedule, the K = nb launches of the per-panel one)
        u.nct = (int)(n_lp * (g.nb / 256));
        upd_fill_affine<256>(u);
        const int64_t nsup = upd_super_count<256>(u);
        if (nsup <= 0) return 0;
        unsigned ntiles = 0;
        int rc = tile_list(ctx, u, nsup, &u.tiles, &ntiles, 256, stream); if (rc) return rc;
        if (o.used_bn) *o.used_bn = 256;
        if (ntiles == 0) return 0;
        hipLaunchKernelGGL((k_update<256, true, 8>), dim3(ntiles), dim3(512), 0, stream, ctx->A, g.Npad, Lop, ldl, Wop, ldw, K, u);
        PYIPM_KCHECK();
        return 0;
    }
    if (bulk && upd_swizzle_ok<128>(u)) {
        upd_fill_affine<128>(u);
        const int64_t nsup = upd_super_count<128>(u);
        if (nsup <= 0) return 0;
        unsigned ntiles = 0;
        int rc = tile_list(ctx, u, nsup, &u.tiles, &ntiles, 128, stream); if (rc) return rc;
        if (ntiles == 0) return 0;
        if (ctx->bulk_bn == 256 && use_waves == 8 && waves == 0 && ksplit == 1 && nct_sub == 0 &&
            ntiles <= (unsigned)(ctx->num_cus * 5 / 8) && upd_swizzle_ok<64>(u)) {
            // A launch that leaves most of the GPU idle (the last groups of a factorisation, the panel-by-panel updates of a small
            // system's first group): 128 x 64 tiles, twice as many blocks of half the length, no scratch.  (Config 2's K = 2048
            // launch of 136 tiles, 272 us: unchanged by itself -- 272 half tiles on 256 CUs end when 136 whole ones do -- but the K = 256
            // pieces of lookahead = 2 gain 2 %.  As the instance of EVERY narrow launch at N = 32768 it lost 1 %: tools/r06_bn64.sh.)
            // Every entry still receives its products k ascending in MFMA groups of 4: the same bits.
            UpdGeo v = u;
            v.nct = (int)(n_lp * (g.nb / 64)); v.tiles = nullptr;
            upd_fill_affine<64>(v);
            const int64_t nsup64 = upd_super_count<64>(v);
            unsigned nt64 = 0;
            if (nsup64 > 0) { rc = tile_list(ctx, v, nsup64, &v.tiles, &nt64, 64, stream); if (rc) return rc; }
            if (nt64 > 0) {
                hipLaunchKernelGGL((k_update<64, true, 8>), dim3(nt64), dim3(512), 0, stream, ctx->A, g.Npad, Lop, ldl, Wop, ldw, K, v);
                PYIPM_KCHECK();
                if (o.used_bn) *o.used_bn = 64;
                return 0;
            }
        }
        dim3 grid(ntiles, (unsigned)ksplit);             // K is the length of ONE split
        if (ksplit > 1) u.ks_cstride = o.ks_cstride;
        if (use_waves == 8 && waves == 0 && ksplit == 1 && ctx->reserve_cus > 0 &&
            m <= ctx->persist_rows) {
            // chain-bound phase: leave `reserve_cus` CUs without update blocks (two 8-wave blocks fill one)
            const unsigned slots = (unsigned)(2 * (ctx->num_cus - ctx->reserve_cus)) & ~7u;
            if (slots >= 8 && ntiles > slots) { u.persist = ntiles; grid.x = slots; }
        }
        if (use_waves == 8)
            hipLaunchKernelGGL((k_update<128, true, 8>), grid, dim3(512), 0, stream, ctx->A, g.Npad, Lop, ldl, Wop, ldw, K, u);
        else
            hipLaunchKernelGGL((k_update<128, true>), grid, dim3(256), 0, stream, ctx->A, g.Npad, Lop, ldl, Wop, ldw, K, u);
    } else {
        // a panel-chain launch, or a panel width the tile-list decode does not cover: plain grid order
        if (ksplit > 1) { ctx->err = "split-K launches need the tile-list order"; return PYIPM_E_BADARG; }
        dim3 grid((unsigned)u.nrt, (unsigned)u.nct);
        hipLaunchKernelGGL((k_update<128, false>), grid, dim3(256), 0, stream, ctx->A, g.Npad, Lop, ldl, Wop, ldw, K, u);
    }
    PYIPM_KCHECK();
    return 0;
}

// Per-panel mode (no group schedule: the multi-rank driver): a panel inside the slack block needs no tile chain,
// no message and no update launch (k_s_panel / k_s_schur_sigma).
bool panel_in_s(const Ctx* ctx, int64_t p) {
    const Geo& g = ctx->g;
    if (!ctx->skip_zeros || g.mi == 0 || ctx->sched.active() || ctx->held.cond_active) return false;
    const int64_t c0 = g.panel_c0(p);
    return c0 >= g.n && c0 + g.panel_w(p) <= g.n + g.mi;
}

// Per-panel mode: rows [h0, h1) of a panel that lies inside the x block are whole 128-row tiles of slack rows --
// exact zeros that no update launch with these source columns ever reads (active_ranges).  The owner's chain
// kernels skip them and the panel message leaves them out.  Empty range when nothing can be skipped.
// Rows of exact zeros (whole slack rows of x-block columns) that the chain kernels neither compute nor WRITE into W.  Whole
// HOLEG-row blocks only, HOLEG = the widest column tile of an update launch: a 128 x 256 tile whose columns straddled the edge of
// a 128-aligned hole read W rows nobody had written -- stale memory, silently wrong factors whenever n or n + mi is an odd
// multiple of 128 and the workspace is not fresh (found by tests/test_gpu_configs.py::test_oracle_lu_where_the_headline_runs,
// round 4; the benchmark shapes are 256-aligned and were never affected).
constexpr int64_t HOLEG = 256;
inline void slack_hole(const Geo& g, int64_t* h0, int64_t* h1) {
    *h0 = (g.n + HOLEG - 1) / HOLEG * HOLEG; *h1 = (g.n + g.mi) / HOLEG * HOLEG;
    if (*h1 < *h0) *h1 = *h0;
}

void panel_hole(const Ctx* ctx, int64_t p, int64_t* h0, int64_t* h1) {
    const Geo& g = ctx->g;
    *h0 = 0; *h1 = 0;
    if (!ctx->skip_zeros || g.mi == 0 || ctx->sched.active() || ctx->held.cond_active) return;
    if (g.panel_c0(p) + g.panel_w(p) > g.n) return;
    int64_t a, b;
    slack_hole(g, &a, &b);
    if (b > a) { *h0 = a; *h1 = b; }
}

int factor_wide_panel(Ctx* ctx, int64_t p, hipStream_t stream);
int launch_tile_steps(Ctx* ctx, hipStream_t chain, int64_t gc0, int64_t glc0, int nT, int ta, int tb, double* Wg, double* Dv, double* Ts,
                      int nX = 0, const unsigned* xword = nullptr, unsigned xwant = 0);

// Factor panel p on `stream`.  apply_pending: first apply the earlier panels of p's group to p's columns
// (grouped single-rank driver; their bulk update is deferred to the end of the group).
int factor_panel(Ctx* ctx, int64_t p, hipStream_t stream, bool apply_pending) {
    const Geo& g = ctx->g;
    if (p < 0 || p >= g.npanels || g.owner(p) != g.rank) { ctx->err = "factor_panel: not the owner"; return PYIPM_E_BADARG; }
    const int64_t c0 = g.panel_c0(p), lc0 = g.local_c0(p);
    const int nbw = (int)g.panel_w(p);
    const int nt = nbw / TB;
    const int64_t lp = p / g.world;
    if (ctx->sched.fast_panel(p) || panel_in_s(ctx, p)) {
        // the whole group (or, per-panel mode, the panel) lies inside the slack block: closed form, no W, no updates
        hipLaunchKernelGGL(k_s_panel, dim3(1), dim3(256), 0, stream, ctx->A, g.Npad, c0, lc0, nt,
                           ctx->Dinv + (c0 / TB) * (int64_t)(TB * TB), ctx->Tsv + (c0 / TB) * (int64_t)(TB * TB),
                           ctx->Tflag + c0 / TB, ctx->refine_cond, ctx->block_refine, ctx->dstats,
                           g.n, g.n + g.mi + g.me, ctx->pivtol_rel, ctx->anorm);
        PYIPM_KCHECK();
        return 0;
    }
    double* W = wbuf(ctx, p);
    const int64_t poff = ctx->sched.offset_of(p, ctx->group);
    if (apply_pending && poff != 0) {
        const int64_t p0 = p - poff;
        const int K = (int)((p - p0) * g.nb);
        if (g.Npad - c0 <= PENDING32_ROWS) {
            int64_t pa0, pa1, pb0, pb1;
            active_ranges(ctx, g.panel_c0(p0), g.panel_c0(p0) + K, &pa0, &pa1, &pb0, &pb1);
            hipLaunchKernelGGL(k_inpanel_update, dim3((unsigned)((g.Npad - c0) / 32), (unsigned)(nbw / TB)), dim3(256), 0, stream,
                               ctx->A, g.Npad, lc0, ctx->A + g.local_c0(p0) * g.Npad, g.Npad, wbuf(ctx, p0), g.Npad, c0, K, c0,
                               g.Npad, pa0, pa1, pb0, pb1, SIDE_PRIO);
            PYIPM_KCHECK();
        } else {
            int rc = launch_update128(ctx, stream, ctx->A + g.local_c0(p0) * g.Npad, g.Npad, wbuf(ctx, p0),
                                      K, c0, lp, 1, {.bulk = false, .src_c0 = g.panel_c0(p0)});
            if (rc) return rc;
        }
    }
    // Panels inside the x block: the slack rows of the panel are exact zeros (active_ranges), whole 128-row tiles of
    // them are skipped by the scalings (single rank only: a receiver rebuilds L from W).
    int64_t hole0 = 0, hole1 = 0;
    // Only when the whole GROUP lies in the x block: a group's bulk update reads every W row the structure of its
    // source columns allows, so a mixed group needs all of them written.
    if (ctx->skip_zeros && g.world == 1 && g.mi > 0 && ctx->sched.in_x_panel(p)) slack_hole(g, &hole0, &hole1);
    else panel_hole(ctx, p, &hole0, &hole1);            // per-panel mode (any number of ranks)
    if (ctx->tile_step && !ctx->sched.active() && panel_is_wide(ctx, p) && nt <= 32 && c0 + nbw < g.Npad)
        return factor_wide_panel(ctx, p, stream);
    if (ctx->tile_step && nt <= 16) {
        // stepped schedule: launch t inverts tile t (after eliminating tile t - 1 from the rows of the diagonal block), one
        // more launch runs all stages for the rows below the diagonal block
        double* Dv = ctx->Dinv + (c0 / TB) * (int64_t)(TB * TB);
        double* Ts = ctx->Tsv + (c0 / TB) * (int64_t)(TB * TB);
        { int r0 = launch_tile_steps(ctx, stream, c0, lc0, nt, 0, nt, W, Dv, Ts); if (r0) return r0; }
        const int64_t rb = c0 + nbw;
        if (g.Npad > rb) {
            hipLaunchKernelGGL(k_panel_rest, dim3((unsigned)((g.Npad - rb) / TB)), dim3(256), 0, stream, ctx->A, g.Npad, c0, lc0, nt, rb,
                               W, g.Npad, Dv, Ts, ctx->Tflag + c0 / TB, ctx->block_refine, hole0, hole1, &ctx->dstats->growth_bits);
            PYIPM_KCHECK();
        }
        return 0;
    }
    // panels of more than 16 tiles: one inversion and one scaling launch per tile; the scaling launch also updates the next
    // tile's column block with the tiles before it (NextUpd): two dependent launches per tile instead of three
    for (int t = 0; t < nt; ++t) {
        const int64_t j0 = c0 + (int64_t)t * TB, lcol = lc0 + (int64_t)t * TB;
        const int64_t below = g.Npad - (j0 + TB);
        const bool next = t + 1 < nt && below > 0;   // the scaling launch below carries the update of tile t + 1
        hipLaunchKernelGGL(k_tile_invert, dim3(1), dim3(256), 0, stream, ctx->A, g.Npad, j0, lcol,
                           ctx->Dinv + (j0 / TB) * (int64_t)(TB * TB), ctx->Tsv + (j0 / TB) * (int64_t)(TB * TB),
                           ctx->Tflag + j0 / TB, ctx->refine_cond, ctx->dstats, g.N, ctx->pivtol_rel, ctx->anorm,
                           g.n + g.mi, ctx->dbg_buf, next ? ctx->Wnext : (double*)nullptr, ctx->tile_blocked);
        PYIPM_KCHECK();
        if (below > 0) {
            NextUpd nu; memset(&nu, 0, sizeof(nu));
            if (next) {
                nu.on = 1; nu.C = ctx->A; nu.ldc = g.Npad; nu.ccol = lcol + TB;
                nu.Lop = ctx->A + lc0 * g.Npad; nu.ldl = g.Npad;
                nu.Wop = W; nu.ldw = g.Npad; nu.cglob = j0 + TB; nu.Wnext = ctx->Wnext; nu.K = t * TB;
            }
            hipLaunchKernelGGL(k_panel_scale, dim3((unsigned)(below / TB)), dim3(256), 0, stream,
                               ctx->A, g.Npad, lcol, ctx->A, g.Npad, lcol, W, g.Npad, (int64_t)t * TB,
                               ctx->Dinv + (j0 / TB) * (int64_t)(TB * TB), ctx->Tsv + (j0 / TB) * (int64_t)(TB * TB),
                               ctx->Tflag + j0 / TB, ctx->block_refine, j0 + TB, hole0, hole1, &ctx->dstats->growth_bits, 1.0, nu);
            PYIPM_KCHECK();
        }
    }
    return 0;
}

int ensure_rest_stream(Ctx* ctx) {
    PYIPM_HIP(ctx->rest.ensure_highest(hipStreamNonBlocking));
    return 0;
}

// One block of adjacent sub-panels owned by this rank, chained tile to tile (kernels_panel.hpp): a GROUP of panels of the
// single-rank schedule (factor_group) or ONE wide panel of the per-panel schedule cut into sub-panels (factor_wide_panel).
// The diagonal block of the WHOLE block runs as one sequence of k_tile_step launches on `chain`: a tile waits for nothing
// but the tile before it, and what a per-panel schedule does between two panels (the pending update of the next panel's
// columns, the scaling of all rows below) no longer sits between two tile inversions.  The rows below the diagonal block
// follow on ctx->rest, sub-panel by sub-panel: all stages of the sub-panel (k_panel_rest), then its contribution to the
// later sub-panels of the block (right-looking: the pending update, one source at a time -- the same products in the same
// order).  on_done(id, stream): sub-panel `id` is complete once `stream` reaches this point.
// Tile steps [ta, tb) of a diagonal block of nT tiles on `chain`: one k_tile_step launch per tile.
// does the diagonal block at global column gc0 (nT tiles) take k_tile_chain (kernels_chain.hpp)?
static bool chain_applies(const Ctx* ctx, int64_t gc0, int nT) {
    const Geo& g = ctx->g;
    const bool exposed = !ctx->sched.active() || gc0 == 0 || g.Npad - gc0 <= ctx->tile8_rows;   // (where the chain is what the step waits for)
    return ctx->tile_chain && nT >= 2 && nT <= 32 && (ctx->tile_chain >= 2 || exposed);
}
// nX > 0 (k_tile_chain only, ta = 0, tb = nT): nX row tiles right below the diagonal block take every stage in the same launch,
// once *xword has reached xwant (chain_extra_ok says whether a caller may ask for it).
int launch_tile_steps(Ctx* ctx, hipStream_t chain, int64_t gc0, int64_t glc0, int nT, int ta, int tb, double* Wg, double* Dv, double* Ts,
                      int nX, const unsigned* xword, unsigned xwant) {
    const Geo& g = ctx->g;
    if (tb <= ta) return 0;
    if (tb - ta >= 2 && chain_applies(ctx, gc0, nT)) {
        // the steps [ta, tb) as ONE launch of persistent workgroups (kernels_chain.hpp): no launch boundary between two tiles
        PollWords& cw = ctx->chain_words;
        if (!cw.buf) {                                   // once per handle: every word, the error word too
            PYIPM_HIP(cw.allocate());
            PYIPM_HIP(cw.zero_and_wait(cw.words + 1));
            ctx->chain_epoch = 0;
        }
        if (ctx->chain_epoch >= (1u << 24)) {            // the words' epochs must stay ordered: start over (every 16 M launches)
            PYIPM_HIP(hipDeviceSynchronize());
            PYIPM_HIP(cw.zero_and_wait(cw.words));
            ctx->chain_epoch = 0;
        }
        ChainGeo cg;
        cg.ta = ta; cg.tb = tb; cg.nT = nT; cg.cpy = ctx->chain_cpy > 0 ? ctx->chain_cpy : 5;
        cg.nR = nT + ((ta == 0 && tb == nT) ? nX : 0); cg.xword = xword; cg.xwant = xwant;
        ctx->chain_epoch += 1;
        cg.base = ctx->chain_epoch * 64u;
        cg.sync = cw.buf + (size_t)(ctx->chain_epoch % Ctx::CHAIN_SLOTS) * Ctx::CHAIN_WORDS;
        cg.err = cw.err();
        cg.timeout = POLL_TIMEOUT;
        cg.dbg = nullptr;
        if (ctx->chain_dbg && ctx->chain_dbg_launch < 64) cg.dbg = ctx->chain_dbg + (size_t)(ctx->chain_dbg_launch++) * CHAIN_DBG_WORDS;
        const unsigned nblk = 1u + (unsigned)chain_units(ta, nT, cg.cpy, cg.nR);
        // dynamic shared memory nobody touches: with it a workgroup of the chain has its compute unit to itself (single-rank
        // schedule only: beside the bulk updates of the per-panel schedule it would wait for a whole CU to drain)
        size_t pad = (ctx->chain_lds_kb > 0 && ctx->sched.active()) ? (size_t)ctx->chain_lds_kb * 1024 : 0;
        if (pad && !ctx->chain_lds_set) {
            if (hipFuncSetAttribute((const void*)k_tile_chain, hipFuncAttributeMaxDynamicSharedMemorySize, 110 * 1024) != hipSuccess) { (void)hipGetLastError(); ctx->chain_lds_kb = 0; pad = 0; }
            ctx->chain_lds_set = true;
        }
        hipLaunchKernelGGL(k_tile_chain, dim3(nblk), dim3(256), pad, chain, ctx->A, g.Npad, gc0, glc0, Wg, g.Npad, Dv, Ts,
                           ctx->Tflag + gc0 / TB, ctx->refine_cond, ctx->block_refine, ctx->dstats, g.N, ctx->pivtol_rel, ctx->anorm,
                           g.n + g.mi, ctx->tile_blocked, cg, ctx->dbg_buf);
        PYIPM_KCHECK();
        cw.used = true;
        ctx->chain_last = cg;
        return 0;
    }
    if (nX > 0) { ctx->err = "launch_tile_steps: extra rows need the one-launch chain (chain_extra_ok)"; return PYIPM_E_BADARG; }
    for (int j = ta; j < tb; ++j) {
        int ny = (nT - j + 4) / 5; if (ny < 1) ny = 1; if (ny > 4) ny = 4;     // <= ~5 column tiles per block
        // the critical block on eight waves (chain + helpers) where a whole CU is to be had: a 512-thread block owns the
        // registers of its CU, so beside an ordinary bulk launch it would wait for BOTH resident bulk blocks of a CU to retire
        // (all launches: exposed panel 7.1 -> 10.9 ms at N = 32768; the per-panel schedule, whose ranks run their bulk updates
        // beside every chain: owners' chain path 31.0 -> 32.1 ms in the replay -- it keeps the 256-thread kernel)
        const int64_t m_left = g.Npad - gc0;
        if (ctx->tile_waves == 8 && ctx->sched.active() && (gc0 == 0 || m_left <= ctx->tile8_rows)) {
            const int units = (nT - j - 1) * ny;
            const int free_cus = (gc0 == 0 || ctx->reserve_cus <= 0) ? ctx->num_cus : TILE_FREE_CUS;
            const int upb = units + 1 <= free_cus ? 1 : 2;          // (row tile, y) units per 512-thread block
            const unsigned nblk = 1u + (unsigned)((units + upb - 1) / upb);
            hipLaunchKernelGGL(k_tile_step8, dim3(nblk), dim3(512), 0, chain, ctx->A, g.Npad, gc0, glc0, j, nT, ny, upb,
                               Wg, g.Npad, Dv, Ts, ctx->Tflag + gc0 / TB, ctx->refine_cond, ctx->block_refine, ctx->dstats, g.N,
                               ctx->pivtol_rel, ctx->anorm, g.n + g.mi, ctx->dbg_buf, ctx->tile_blocked);
            PYIPM_KCHECK();
            continue;
        }
        hipLaunchKernelGGL(k_tile_step, dim3((unsigned)(nT - j), (unsigned)ny), dim3(256), 0, chain, ctx->A, g.Npad, gc0, glc0, j,
                           Wg, g.Npad, Dv, Ts, ctx->Tflag + gc0 / TB, ctx->refine_cond, ctx->block_refine, ctx->dstats, g.N,
                           ctx->pivtol_rel, ctx->anorm, g.n + g.mi, ctx->dbg_buf, ctx->tile_blocked);
        PYIPM_KCHECK();
    }
    return 0;
}

struct SubPanel { int64_t c0, lc0; int nt; double* W; int64_t id; };
// The tail split seen from one block (single-rank reusing step; StepPlan::tail_split, enqueue_groups decides):
//   xrows > 0: the block hands over split -- its chain launch takes the `xrows` rows right below the diagonal block along (the
//   next group's diagonal block; released by *xword reaching xwant, NULL: at once), the rows kernels start behind them and ALL of
//   them run on ctx->rest, nothing follows the chain's launch on its stream; every panel is done (on_done) and ctx->ev_rows is
//   recorded on ctx->rest once the chain's launch has ended too.
//   rows_behind: the rows kernels wait for it (the rest of the head into this block's columns ran on another stream).
struct TailHand { int64_t xrows = 0; const unsigned* xword = nullptr; unsigned xwant = 0; hipEvent_t rows_behind = nullptr; };
struct BlockDesc {
    std::vector<SubPanel> sp;              // adjacent in global AND local columns; W adjacent too (sp[k].W = sp[0].W + (c0_k - c0_0) * Npad)
    bool wide = false;                     // sub-panels of local panel `lp` (column tiles addressed inside it) instead of whole panels
    int64_t lp = 0;                        // wide: the local panel index; else: sp[k].id is the (local = global) panel index
    int64_t hole0 = 0, hole1 = 0;          // rows of exact zeros the rows kernels skip (KKT structure)
    TailHand hand;                         // the tail split's part in this block (none: all zero)
};
int factor_block(Ctx* ctx, const BlockDesc& bd, hipStream_t chain, const std::function<int(int64_t, hipStream_t)>& on_done) {
    const Geo& g = ctx->g;
    const int64_t n0 = (int64_t)bd.sp.size();
    std::vector<int> toff((size_t)n0 + 1, 0);           // first tile of each sub-panel inside the block (the matrix's last panel may be narrower)
    for (int64_t k = 0; k < n0; ++k) toff[(size_t)k + 1] = toff[(size_t)k] + bd.sp[(size_t)k].nt;
    const int nT = toff[(size_t)n0];
    const int64_t gc0 = bd.sp[0].c0, glc0 = bd.sp[0].lc0, gend = gc0 + (int64_t)nT * TB;
    const int64_t TT = (int64_t)TB * TB;
    { int r0 = ensure_rest_stream(ctx); if (r0) return r0; }
    PYIPM_HIP(ctx->ev_join.ensure(hipEventDisableTiming));
    PYIPM_HIP(ensure_events(ctx->ev_band, (size_t)n0, hipEventDisableTiming));
    double* Wg = bd.sp[0].W;
    double* Dv = ctx->Dinv + (gc0 / TB) * TT;
    double* Ts = ctx->Tsv + (gc0 / TB) * TT;
    // update of the block's own columns, rows from `row_begin`: target sub-panels [k1, k1 + cnt)
    auto upd = [&](hipStream_t st, const double* Lop, const double* Wop, int K, int64_t row_begin, int64_t k1, int64_t cnt,
                   int64_t src_c0) -> int {
        if (!bd.wide)
            return launch_update128(ctx, st, Lop, g.Npad, Wop, K, row_begin, bd.sp[(size_t)k1].id, cnt, {.bulk = false, .src_c0 = src_c0});
        const int s0 = (int)((bd.sp[(size_t)k1].c0 - g.panel_c0(bd.lp * g.world + g.rank)) / 128);
        const int nc = (int)((int64_t)(toff[(size_t)(k1 + cnt)] - toff[(size_t)k1]) * TB / 128);
        return launch_update128(ctx, st, Lop, g.Npad, Wop, K, row_begin, bd.lp, 1,
                                {.bulk = false, .src_c0 = src_c0, .sub0 = s0, .nct_sub = nc});
    };
    // sub-panel q's columns are final inside the diagonal block once the first tile of sub-panel q + 1 has applied its last
    // stage: the tile steps run in pieces that END with that step, an event after each
    // (k_tile_chain: the whole diagonal block is ONE launch; the rows of sub-panel q wait on their own stream for the chain's
    //  progress words instead -- k_chain_wait below)
    const bool one_launch = ctx->chain_whole && chain_applies(ctx, gc0, nT);
    const bool hand = bd.hand.xrows > 0;
    const int64_t rbeg = gend + bd.hand.xrows;          // the rows kernels' first row
    if (hand && !one_launch) { ctx->err = "factor_block: the tail split needs the one-launch chain (group_extra_ok)"; return PYIPM_E_BADARG; }
    if (bd.hand.rows_behind) PYIPM_HIP(hipStreamWaitEvent(ctx->rest, bd.hand.rows_behind, 0));
    ChainGeo cgw; memset(&cgw, 0, sizeof(cgw));
    if (one_launch) {
        // (the rows stream polls the chain's progress with a bounded wait: it must not start polling before the chain can start --
        //  behind a Gram launch of seconds, the condensed form at n = 65536, the bound ran out while the chain's stream was still busy)
        PYIPM_HIP(hipEventRecord(ctx->ev_band[0], chain));
        PYIPM_HIP(hipStreamWaitEvent(ctx->rest, ctx->ev_band[0], 0));
        int r0 = launch_tile_steps(ctx, chain, gc0, glc0, nT, 0, nT, Wg, Dv, Ts, (int)(bd.hand.xrows / TB), bd.hand.xword, bd.hand.xwant); if (r0) return r0;
        cgw = ctx->chain_last;
        if (hand) PYIPM_HIP(hipEventRecord(ctx->ev_chain_end, chain));
    }
    for (int kp = 1, ta = 0; kp <= n0 && !one_launch; ++kp) {
        const int tb = kp < n0 ? toff[(size_t)kp] + 1 : nT;
        int r0 = launch_tile_steps(ctx, chain, gc0, glc0, nT, ta, tb, Wg, Dv, Ts); if (r0) return r0;
        if (kp < n0) PYIPM_HIP(hipEventRecord(ctx->ev_band[(size_t)(kp - 1)], chain));
        ta = tb;
    }
    for (int64_t k = 0; k < n0; ++k) {
        const SubPanel& q = bd.sp[(size_t)k];
        const int64_t c0 = q.c0, lc0 = q.lc0;
        const int nt = q.nt;
        // the last sub-panel's rows are what the next block waits for: they stay on the chain's stream (a dependency across
        // streams costs 10-30 us when the waiting side is idle), behind the other sub-panels' work on ctx->rest
        hipStream_t rs = ctx->rest;
        // (the tail split: what the next block waits for left with the chain's launch; these rows go to ctx->rest like the others)
        if (k + 1 == n0 && !hand) {
            PYIPM_HIP(hipEventRecord(ctx->ev_join, ctx->rest));
            PYIPM_HIP(hipStreamWaitEvent(chain, ctx->ev_join, 0));
            rs = chain;
        } else if (one_launch) {
            // sub-panel k's tiles are inverted (the chain has passed tile toff[k + 1] - 1) and every later row tile has the stages
            // up to the sub-panel's last tile but one: W of the sub-panel's columns is final inside the diagonal block
            hipLaunchKernelGGL(k_chain_wait, dim3(1), dim3(64), 0, ctx->rest, cgw, toff[(size_t)k + 1], toff[(size_t)k + 1], toff[(size_t)k + 1]);
            PYIPM_KCHECK();
        } else {
            PYIPM_HIP(hipStreamWaitEvent(ctx->rest, ctx->ev_band[(size_t)k], 0));
        }
        // Where the bulk update is the bound (many rows below), the in-block updates of the rows below the diagonal block
        // are applied LEFT-looking -- all earlier sub-panels at once (K up to 768), right before the sub-panel's own
        // stages -- instead of one by one: half the read-modify-write passes over those rows and longer K per launch.
        // In the tail the one-by-one form keeps only the last sub-panel's stages behind the chain.  Same bits either way.
        const bool left = g.Npad - gend > PENDING_LEFT_ROWS;
        if (g.Npad > rbeg && left && k > 0) {
            const int K = toff[(size_t)k] * TB;
            int rc = upd(rs, ctx->A + glc0 * g.Npad, Wg, K, rbeg, k, 1, gc0);
            if (rc) return rc;
        }
        if (g.Npad > rbeg) {
            hipLaunchKernelGGL(k_panel_rest, dim3((unsigned)((g.Npad - rbeg) / TB)), dim3(256), 0, rs, ctx->A, g.Npad, c0, lc0, nt,
                               rbeg, q.W, g.Npad, ctx->Dinv + (c0 / TB) * TT, ctx->Tsv + (c0 / TB) * TT, ctx->Tflag + c0 / TB,
                               ctx->block_refine, bd.hole0, bd.hole1, &ctx->dstats->growth_bits);
            PYIPM_KCHECK();
            if (k + 1 < n0 && !left) {
                // this sub-panel's contribution to the later ones of the block, rows below the diagonal block
                const int K = nt * TB;
                const SubPanel& nx = bd.sp[(size_t)k + 1];
                const int64_t tc0 = nx.c0, ncols = (int64_t)(nT - toff[(size_t)k + 1]) * TB;
                if (g.Npad - tc0 <= PENDING32_ROWS) {
                    int64_t pa0, pa1, pb0, pb1;
                    active_ranges(ctx, c0, c0 + K, &pa0, &pa1, &pb0, &pb1);
                    hipLaunchKernelGGL(k_inpanel_update, dim3((unsigned)((g.Npad - rbeg) / 32), (unsigned)(ncols / TB)), dim3(256), 0,
                                       rs, ctx->A, g.Npad, nx.lc0, ctx->A + lc0 * g.Npad, g.Npad, q.W, g.Npad,
                                       tc0, K, rbeg, g.Npad, pa0, pa1, pb0, pb1, SIDE_PRIO);
                    PYIPM_KCHECK();
                } else {
                    int rc = upd(rs, ctx->A + lc0 * g.Npad, q.W, K, rbeg, k + 1, n0 - 1 - k, c0);
                    if (rc) return rc;
                }
            }
        }
        // One launch for the whole chain: the rows stream ran ahead of it on progress words that say what the ROWS kernels read (W,
        // inv(T)) is there.  Whoever reads panel q as a whole (the forward substitution that trails the factorisation) needs L of its
        // columns inside the diagonal block too, i.e. the state after the tile step of the next sub-panel's first tile (what an event
        // behind that launch used to say): a second wait, behind the rows kernels.  L, like W and inv(T), is written through.
        if (one_launch && k + 1 < n0 && !hand) {
            const int tq = toff[(size_t)k + 1] + 1;
            hipLaunchKernelGGL(k_chain_wait, dim3(1), dim3(64), 0, ctx->rest, cgw, tq, tq, tq);
            PYIPM_KCHECK();
        }
        if (hand) continue;
        int rc = on_done(q.id, rs); if (rc) return rc;
    }
    if (hand) {
        // a panel as a whole -- L inside the diagonal block, the extra rows -- is there when the chain's launch has ended
        PYIPM_HIP(hipStreamWaitEvent(ctx->rest, ctx->ev_chain_end, 0));
        for (int64_t k = 0; k < n0; ++k) { int rc = on_done(bd.sp[(size_t)k].id, ctx->rest); if (rc) return rc; }
        PYIPM_HIP(hipEventRecord(ctx->ev_rows, ctx->rest));
    }
    return 0;
}

// A group of panels of the single-rank schedule: panels [p0, p0 + n0).
int factor_group(Ctx* ctx, int64_t p0, int64_t n0, hipStream_t chain, const std::function<int(int64_t, hipStream_t)>& on_done, const TailHand& hand = {}) {
    const Geo& g = ctx->g;
    BlockDesc bd; bd.hand = hand;
    for (int64_t k = 0; k < n0; ++k) {
        const int64_t q = p0 + k;
        bd.sp.push_back(SubPanel{g.panel_c0(q), g.local_c0(q), (int)(g.panel_w(q) / TB), wbuf(ctx, q), q});
    }
    if (ctx->skip_zeros && g.mi > 0 && ctx->sched.in_x_panel(p0)) slack_hole(g, &bd.hole0, &bd.hole1);
    return factor_block(ctx, bd, chain, on_done);
}

// Per-panel schedule, a panel wider than `wide_sub` columns (nb = 512 / 1024): the owner factors it like the single-rank
// schedule factors a group -- one tile chain over the panel's diagonal block, the rows below it sub-panel by sub-panel on
// ctx->rest with the in-panel updates as MFMA launches of K up to nb - wide_sub (k_panel_rest with all nt stages in one
// launch is right-looking 64 columns at a time through L2: 120 tile passes per strip at nt = 16).  The same products in the
// same order: the same bits.  What the other ranks see does not change (one message, one rank-nb update per panel), only
// that the message is 4 x larger and 4 x rarer than at nb = 256 and the owner's chain is the single-rank one.
int factor_wide_panel(Ctx* ctx, int64_t p, hipStream_t stream) {
    const Geo& g = ctx->g;
    const int64_t c0 = g.panel_c0(p), lc0 = g.local_c0(p);
    const int nt = (int)(g.panel_w(p) / TB), snt = ctx->wide_sub / TB;
    BlockDesc bd;
    bd.wide = true; bd.lp = p / g.world;
    double* W = wbuf(ctx, p);
    for (int t = 0; t < nt; t += snt) {
        const int w = nt - t < snt ? nt - t : snt;
        bd.sp.push_back(SubPanel{c0 + (int64_t)t * TB, lc0 + (int64_t)t * TB, w, W + (int64_t)t * TB * g.Npad, p});
    }
    panel_hole(ctx, p, &bd.hole0, &bd.hole1);
    return factor_block(ctx, bd, stream, [](int64_t, hipStream_t) { return 0; });
}

// ---- per-panel schedule, a panel in pieces (round 5: the two-message protocol of the distributed driver, dist_impl.hpp) ------
// The owner of panel p + 1 starts that panel's tile chain as soon as the rows of panel p that meet ITS diagonal block have
// arrived (a slice message, nb x nb); the rows below follow when their operands do.  A panel's rows below its diagonal block
// do not interact, so factoring it in pieces -- the tile chain, then the stages of any row range -- runs the same kernels on
// every entry in the same order as factor_panel does in one go: the same bits (tests/test_gpu_dist.py, tools/rank_replay.py).
// is panel p wider than `wide_sub` columns (factored and swept as a block of sub-panels that wide)?  The width alone: every
// site adds what else it needs (factor_panel: per-panel mode, at most 32 tiles, rows below; panel_piecewise_ok: 32 against 16
// tiles; panel_rows: nothing; the distributed driver's classic head, plan_slot: also the slack block and the 32-row grid).
bool panel_is_wide(const Ctx* ctx, int64_t p) {
    return ctx->wide_sub >= 128 && ctx->wide_sub % 128 == 0 && ctx->g.panel_w(p) > ctx->wide_sub;
}
bool panel_piecewise_ok(const Ctx* ctx, int64_t p) {
    if (!ctx->tile_step || panel_in_s(ctx, p)) return false;
    const int nt = (int)ctx->g.panel_w(p) / TB;
    return panel_is_wide(ctx, p) ? (nt <= 32) : (nt <= 16);
}
// the tile steps of panel p's diagonal block (all that needs is the diagonal block up to date)
int panel_chain(Ctx* ctx, int64_t p, hipStream_t stream, int64_t xrows, const unsigned* xword, unsigned xwant) {
    const Geo& g = ctx->g;
    const int64_t c0 = g.panel_c0(p), lc0 = g.local_c0(p);
    const int nt = (int)(g.panel_w(p) / TB);
    return launch_tile_steps(ctx, stream, c0, lc0, nt, 0, nt, wbuf(ctx, p), ctx->Dinv + (c0 / TB) * (int64_t)(TB * TB),
                             ctx->Tsv + (c0 / TB) * (int64_t)(TB * TB), (int)(xrows / TB), xword, xwant);
}
// may panel p's chain take the `xrows` rows right below its diagonal block along (every stage of theirs in the chain's launch
// instead of panel_rows behind it)?  The one-launch chain, whole tiles -- at most 16 of them: a wide panel's (nb = 1024) rows for
// the next owner are 16 row tiles of 16 stages each, units that keep the chain's pace like the block's own far rows --, none of
// them inside the panel's hole of structural zeros (k_panel_rest leaves those alone), progress words enough.
// (the diagonal block of nt tiles at column c0, its hole [h0, h1): a panel, or a group of the single-rank schedule seen as one block)
static bool block_extra_ok(const Ctx* ctx, int64_t c0, int nt, int64_t xrows, int64_t h0, int64_t h1) {
    const Geo& g = ctx->g;
    const int64_t nbw = (int64_t)nt * TB;
    if (xrows <= 0 || xrows % TB != 0 || xrows / TB > 16 || c0 + nbw + xrows > g.Npad) return false;
    if (!(nt >= 2 && chain_applies(ctx, c0, nt))) return false;
    if (1 + 4 * (nt + (int)(xrows / TB)) > Ctx::CHAIN_WORDS) return false;
    const int64_t r0 = c0 + nbw, r1 = r0 + xrows;
    return !(h1 > h0 && r1 > h0 && r0 < h1);
}
bool chain_extra_ok(const Ctx* ctx, int64_t p, int64_t xrows) {
    int64_t h0 = 0, h1 = 0;
    panel_hole(ctx, p, &h0, &h1);
    return block_extra_ok(ctx, ctx->g.panel_c0(p), (int)ctx->g.panel_w(p) / TB, xrows, h0, h1);
}
// ... and group grp of the single-rank schedule (the tail split, StepPlan::tail_split): the group's whole diagonal block is one launch
static bool group_extra_ok(const Ctx* ctx, int64_t grp, int64_t xrows) {
    const Geo& g = ctx->g;
    const int64_t p0 = ctx->sched.first(grp), p1 = ctx->sched.first(grp + 1);
    int64_t cols = 0, h0 = 0, h1 = 0;
    for (int64_t q = p0; q < p1; ++q) cols += g.panel_w(q);
    if (ctx->skip_zeros && g.mi > 0 && ctx->sched.in_x_panel(p0)) slack_hole(g, &h0, &h1);
    return ctx->chain_whole && cols / TB <= 32 && block_extra_ok(ctx, g.panel_c0(p0), (int)(cols / TB), xrows, h0, h1);
}
// every stage of panel p for the rows [r0, r1) below its diagonal block (128-aligned), the chain complete on `stream` before
int panel_rows(Ctx* ctx, int64_t p, int64_t r0, int64_t r1, hipStream_t stream) {
    const Geo& g = ctx->g;
    if (r1 > g.Npad) r1 = g.Npad;
    if (r1 <= r0) return 0;
    const int64_t c0 = g.panel_c0(p), lc0 = g.local_c0(p), TT = (int64_t)TB * TB;
    const int nbw = (int)g.panel_w(p), nt = nbw / TB;
    double* W = wbuf(ctx, p);
    int64_t hole0 = 0, hole1 = 0;
    panel_hole(ctx, p, &hole0, &hole1);
    if (!panel_is_wide(ctx, p)) {
        hipLaunchKernelGGL(k_panel_rest, dim3((unsigned)((r1 - r0) / TB)), dim3(256), 0, stream, ctx->A, g.Npad, c0, lc0, nt, r0,
                           W, g.Npad, ctx->Dinv + (c0 / TB) * TT, ctx->Tsv + (c0 / TB) * TT, ctx->Tflag + c0 / TB,
                           ctx->block_refine, hole0, hole1, &ctx->dstats->growth_bits);
        PYIPM_KCHECK();
        return 0;
    }
    // a wide panel: sub-panel by sub-panel as factor_block does below a diagonal block (left-looking MFMA in-panel updates while
    // many rows remain below the panel, right-looking one source at a time in the tail: decided by the PANEL, so every row range
    // of it takes the same kernels)
    const int snt = ctx->wide_sub / TB;
    const int64_t gend = c0 + nbw, lp = p / g.world;
    const bool left = g.Npad - gend > PENDING_LEFT_ROWS;
    for (int t = 0; t < nt; t += snt) {
        const int w = nt - t < snt ? nt - t : snt;
        const int64_t sc0 = c0 + (int64_t)t * TB, slc0 = lc0 + (int64_t)t * TB;
        double* sW = W + (int64_t)t * TB * g.Npad;
        if (left && t > 0) {
            int rc = launch_update128(ctx, stream, ctx->A + lc0 * g.Npad, g.Npad, W, t * TB, r0, lp, 1,
                                      {.bulk = false, .row_end = r1, .src_c0 = c0, .sub0 = (t * TB) / 128, .nct_sub = (w * TB) / 128});
            if (rc) return rc;
        }
        hipLaunchKernelGGL(k_panel_rest, dim3((unsigned)((r1 - r0) / TB)), dim3(256), 0, stream, ctx->A, g.Npad, sc0, slc0, w, r0,
                           sW, g.Npad, ctx->Dinv + (sc0 / TB) * TT, ctx->Tsv + (sc0 / TB) * TT, ctx->Tflag + sc0 / TB,
                           ctx->block_refine, hole0, hole1, &ctx->dstats->growth_bits);
        PYIPM_KCHECK();
        if (!left && t + w < nt) {
            const int K = w * TB;
            const int64_t tc0 = sc0 + K, ncols = (int64_t)(nt - t - w) * TB;
            if (g.Npad - tc0 <= PENDING32_ROWS) {
                int64_t pa0, pa1, pb0, pb1;
                active_ranges(ctx, sc0, sc0 + K, &pa0, &pa1, &pb0, &pb1);
                hipLaunchKernelGGL(k_inpanel_update, dim3((unsigned)((r1 - r0) / 32), (unsigned)(ncols / TB)), dim3(256), 0, stream,
                                   ctx->A, g.Npad, slc0 + K, ctx->A + slc0 * g.Npad, g.Npad, sW, g.Npad, tc0, K, r0, g.Npad,
                                   pa0, pa1, pb0, pb1, SIDE_PRIO);
                PYIPM_KCHECK();
            } else {
                int rc = launch_update128(ctx, stream, ctx->A + slc0 * g.Npad, g.Npad, sW, K, r0, lp, 1,
                                          {.bulk = false, .row_end = r1, .src_c0 = sc0, .sub0 = ((t + w) * TB) / 128, .nct_sub = (int)(ncols / 128)});
                if (rc) return rc;
            }
        }
    }
    return 0;
}

// Slice j (1 or 2) of panel p: the rows of panel p + j, i.e. W rows [c0(p + j), c0(p + j) + w(p + j)) of all the panel's columns
// (leading dimension = the slice's rows); slice 1 also carries the panel's tile inverses, tiles and flags.
int64_t slice_rows(const Geo& g, int64_t p, int j, int64_t* r0) {
    if (p + j >= g.npanels) { *r0 = g.Npad; return 0; }
    *r0 = g.panel_c0(p + j);
    return g.panel_w(p + j);
}
size_t slice_numel(const Geo& g, int64_t p, int j) {
    int64_t r0; const int64_t E = slice_rows(g, p, j, &r0), nbw = g.panel_w(p);
    if (E <= 0) return 0;
    return (size_t)(E * nbw + (j == 1 ? 2 * (nbw / TB) * TB * TB + nbw / TB : 0));
}
int pack_slice(Ctx* ctx, int64_t p, int j, double* buf, hipStream_t st) {
    const Geo& g = ctx->g;
    int64_t r0; const int64_t E = slice_rows(g, p, j, &r0), nbw = g.panel_w(p), c0 = g.panel_c0(p);
    if (E <= 0) return 0;
    const int64_t total = (int64_t)slice_numel(g, p, j);
    int64_t blocks = (total + 1023) / 1024; if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(k_slice_pack, dim3((unsigned)blocks), dim3(256), 0, st, buf, E, nbw, wbuf(ctx, p) + r0, g.Npad,
                       ctx->Dinv + (c0 / TB) * (int64_t)(TB * TB), ctx->Tsv + (c0 / TB) * (int64_t)(TB * TB), ctx->Tflag + c0 / TB,
                       j == 1 ? 1 : 0);
    PYIPM_KCHECK();
    return 0;
}
// receiver: L = W inv(T) of the slice's rows into `EL` (E x nbw, leading dimension E), in ONE launch straight from the message:
// the tile inverses are read where slice 1 carries them (`tiles` = the tail of the slice-1 buffer), and slice 1's W rows --
// the columns of the panel this rank factors next: the W operand of every update of those columns -- are copied to where the
// panel message would put them by the same launch.  (Slice 2's W rows are the column positions of a panel this rank does not
// own: nobody here reads them.)
int unpack_slice(Ctx* ctx, int64_t p, int j, const double* buf, const double* tiles, double* EL, hipStream_t st) {
    const Geo& g = ctx->g;
    int64_t r0; const int64_t E = slice_rows(g, p, j, &r0), nbw = g.panel_w(p);
    if (E <= 0) return 0;
    const int64_t tb = (nbw / TB) * (int64_t)(TB * TB);
    int64_t h0, h1;
    panel_hole(ctx, p, &h0, &h1);
    NextUpd nu_off; memset(&nu_off, 0, sizeof(nu_off));
    hipLaunchKernelGGL(k_panel_scale, dim3((unsigned)(E / TB), (unsigned)(nbw / TB)), dim3(256), 0, st,
                       EL - r0, E, (int64_t)0, buf - r0, E, (int64_t)0, j == 1 ? wbuf(ctx, p) : (double*)nullptr, g.Npad, (int64_t)0,
                       tiles, tiles + tb, tiles + 2 * tb, ctx->block_refine, r0, h0, h1, (unsigned long long*)nullptr, -1.0, nu_off);
    PYIPM_KCHECK();
    return 0;
}
// ... and the panel's tile inverses, tiles and flags from the slice-1 buffer into the handle's arrays (what the rest of the
// panel's unpacking and nothing on the chain path reads)
int unpack_slice_tiles(Ctx* ctx, int64_t p, const double* tiles, hipStream_t st) {
    const Geo& g = ctx->g;
    const int64_t nbw = g.panel_w(p), c0 = g.panel_c0(p);
    const size_t tb = (size_t)(nbw / TB) * TB * TB;
    PYIPM_HIP(hipMemcpyAsync(ctx->Dinv + (c0 / TB) * (int64_t)(TB * TB), tiles, tb * sizeof(double), hipMemcpyDeviceToDevice, st));
    PYIPM_HIP(hipMemcpyAsync(ctx->Tsv + (c0 / TB) * (int64_t)(TB * TB), tiles + tb, tb * sizeof(double), hipMemcpyDeviceToDevice, st));
    PYIPM_HIP(hipMemcpyAsync(ctx->Tflag + c0 / TB, tiles + 2 * tb, (size_t)(nbw / TB) * sizeof(double), hipMemcpyDeviceToDevice, st));
    return 0;
}
// The panel message of p on a receiver, rows from `row_from` on only (the rows before it came as slices), tiles optional.
int unpack_panel_from(Ctx* ctx, int64_t p, const double* buf, int64_t row_from, bool with_tiles, hipStream_t st) {
    const Geo& g = ctx->g;
    int64_t h0, h1;
    panel_hole(ctx, p, &h0, &h1);
    const int64_t nbw = g.panel_w(p), c0 = g.panel_c0(p), c1 = c0 + nbw, m = g.Npad - c1 - (h1 - h0);
    double* dinv = ctx->Dinv + (c0 / TB) * (int64_t)(TB * TB);
    double* tsv = ctx->Tsv + (c0 / TB) * (int64_t)(TB * TB);
    if (with_tiles) {
        const size_t tbytes = (size_t)(nbw / TB) * TB * TB * sizeof(double);
        PYIPM_HIP(hipMemcpyAsync(dinv, buf + m * nbw, tbytes, hipMemcpyDeviceToDevice, st));
        PYIPM_HIP(hipMemcpyAsync(tsv, buf + m * nbw + (nbw / TB) * TB * TB, tbytes, hipMemcpyDeviceToDevice, st));
        PYIPM_HIP(hipMemcpyAsync(ctx->Tflag + c0 / TB, buf + m * nbw + 2 * (nbw / TB) * TB * TB, (size_t)(nbw / TB) * sizeof(double),
                                 hipMemcpyDeviceToDevice, st));
    }
    const int64_t rf = row_from > c1 ? row_from : c1;
    if (m <= 0 || rf >= g.Npad) return 0;
    // rows [c1, Npad) without the hole [h0, h1) sit in the message with leading dimension m.  One launch per segment at or beyond
    // rf reads -S straight from the message, rebuilds L = S inv(T) into Lbuf and leaves -S where the update launches read it
    // (round 6; until then: a strided copy of the segment into the W slot, then the product from there -- the panel's 8 nb bytes per
    // row read twice and written twice on every receiver, 57-70 ms per rank of the N = 131072 replay).  The tile columns of a
    // received panel are independent (L_t = W_t inv(T_t)): grid.y walks them.
    const int64_t segs[2][2] = {{c1, (h1 > h0) ? h0 : g.Npad}, {(h1 > h0) ? h1 : g.Npad, g.Npad}};
    NextUpd nu_off; memset(&nu_off, 0, sizeof(nu_off));
    for (int k = 0; k < 2; ++k) {
        const int64_t a = segs[k][0] > rf ? segs[k][0] : rf, b = segs[k][1];
        if (b <= a) continue;
        const int64_t mrow = a - c1 - ((h1 > h0 && a >= h1) ? (h1 - h0) : 0);      // the message row of matrix row a
        hipLaunchKernelGGL(k_panel_scale, dim3((unsigned)((b - a) / TB), (unsigned)(nbw / TB)), dim3(256), 0, st,
                           ctx->Lbuf, g.Npad, (int64_t)0, buf + mrow - a, m, (int64_t)0,
                           wbuf(ctx, p), g.Npad, (int64_t)0, dinv, tsv, ctx->Tflag + c0 / TB, ctx->block_refine, a, (int64_t)0, (int64_t)0,
                           (unsigned long long*)nullptr, -1.0, nu_off);
        PYIPM_KCHECK();
    }
    return 0;
}

// One bulk k_update<128> launch: panels [p0, p0+np) (contiguous, same rank) applied with K = their total
// width to local panels [first_lp, first_lp+n_lp); timed with HIP events on the handle's stream.
int timed_update(Ctx* ctx, int64_t p0, int64_t np, int64_t first_lp, int64_t n_lp, const UpdTimed& o) {
    const Geo& g = ctx->g;
    hipStream_t stream = o.stream ? o.stream : ctx->stream;
    if (n_lp <= 0) return 0;
    int K = 0;
    for (int64_t q = p0; q < p0 + np; ++q) K += (int)g.panel_w(q);
    if (ctx->sched.fast_panel(p0)) {
        // slack-block sources: each column updates one diagonal entry (k_s_schur), here for the target columns
        // of this launch -- on the update stream, where the dense launch would have run
        const int64_t tq0 = first_lp, tq1 = first_lp + n_lp;                       // single rank: local = global panels
        const int64_t tc0 = g.panel_c0(tq0), tc1 = tq1 >= g.npanels ? g.Npad : g.panel_c0(tq1);
        hipLaunchKernelGGL(k_s_schur, grid1(K), dim3(256), 0, stream, ctx->A, g.Npad, g.panel_c0(p0), (int64_t)K,
                           g.n, g.n + g.mi + g.me, tc0, tc1);
        PYIPM_KCHECK();
        return 0;
    }
    if (np == 1 && panel_in_s(ctx, p0)) {
        // per-panel mode, slack-block source panel: every rank updates the diagonal entries it owns, from s / lambda
        const int64_t tp0 = first_lp * g.world + g.rank, tp1 = (first_lp + n_lp - 1) * g.world + g.rank + 1;
        hipLaunchKernelGGL(k_s_schur_sigma, dim3((unsigned)(K / TB)), dim3(64), 0, stream, ctx->A, g.Npad, g.panel_c0(p0),
                           g.n, g.n + g.mi + g.me, ctx->s, ctx->lda + g.me, ctx->eps, ctx->refine_cond, ctx->block_refine,
                           ctx->pivtol_rel, g.nb, g.world, g.rank, tp0, tp1, ctx->anorm);
        PYIPM_KCHECK();
        return 0;
    }
    const bool mine = g.owner(p0) == g.rank;
    const double* Lop = mine ? ctx->A + g.local_c0(p0) * g.Npad : ctx->Lbuf;
    const int64_t q0 = first_lp * g.world + g.rank;           // first global panel updated
    const int64_t row_begin = g.panel_c0(q0);
    if (row_begin >= g.Npad) return 0;
    // A launch on another stream than the handle's is a lookahead head riding the chain's stream: it overlaps the bulk launch
    // on the main stream, so its duration says nothing about the kernel's rate -- it is not part of the "trailing" figures
    // (time, flops, launches), and it uses the 4-wave instance of the kernel so that a kernel trace keeps the two apart.
    const bool chain_side = stream != ctx->stream && ctx->sched.active() && !o.as_bulk;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int used_bn = 128;
    if (ctx->profile && !chain_side) {
        if ((size_t)ctx->n_trailing >= ctx->ev_trailing.size()) {
            std::pair<Event, Event> pr;
            PYIPM_HIP(pr.first.ensure(hipEventDefault)); PYIPM_HIP(pr.second.ensure(hipEventDefault));
            ctx->ev_trailing.push_back(std::move(pr));
        }
        e0 = ctx->ev_trailing[ctx->n_trailing].first; e1 = ctx->ev_trailing[ctx->n_trailing].second;
        PYIPM_HIP(hipEventRecord(e0, stream));
    }
    if (!ctx->sched.active() && n_lp == 1 && g.Npad - row_begin <= HEAD32_ROWS_DIST) {
        // one panel of columns (the head of the per-panel schedule): 32 x 64 blocks instead of a handful of 128 x 128 tiles
        int64_t pa0, pa1, pb0, pb1;
        active_ranges(ctx, g.panel_c0(p0), g.panel_c0(p0) + K, &pa0, &pa1, &pb0, &pb1);
        hipLaunchKernelGGL(k_inpanel_update, dim3((unsigned)((g.Npad - row_begin) / 32), (unsigned)(g.panel_w(q0) / TB)), dim3(256), 0,
                           stream, ctx->A, g.Npad, first_lp * (int64_t)g.nb, Lop, g.Npad, wbuf(ctx, p0), g.Npad, row_begin, K,
                           row_begin, g.Npad, pa0, pa1, pb0, pb1, SIDE_PRIO);
        PYIPM_KCHECK();
    } else {
        int rc = launch_update128(ctx, stream, Lop, g.Npad, wbuf(ctx, p0), K, row_begin, first_lp, n_lp,
                                  {.src_c0 = g.panel_c0(p0), .waves = chain_side ? HEAD_WAVES : 0, .used_bn = &used_bn});
        if (rc) return rc;
    }
    if (chain_side) return 0;
    if (ctx->profile) PYIPM_HIP(hipEventRecord(e1, stream));
    // algorithmic flops of this launch: 2*K per lower-triangle entry of the updated local columns
    // (entries the KKT block structure leaves at zero are not counted: the launch skips their tiles)
    double fl = 0.0;
    int64_t a0, a1, b0, b1;
    active_ranges(ctx, g.panel_c0(p0), g.panel_c0(p0) + K, &a0, &a1, &b0, &b1);
    for (int64_t k = 0; k < n_lp; ++k) {
        const int64_t qq = (first_lp + k) * g.world + g.rank;
        if (qq >= g.npanels) break;
        fl += 2.0 * K * active_area(g.panel_c0(qq), g.Npad, g.panel_c0(qq), g.panel_c0(qq) + g.panel_w(qq), a0, a1, b0, b1);
    }
    ctx->trailing_flops += fl;
    ctx->trailing_area += fl / (2.0 * K);
    if ((size_t)ctx->n_trailing >= ctx->trailing_tag.size()) ctx->trailing_tag.resize((size_t)ctx->n_trailing + 64);
    // algorithmic bytes of the launch: the C tiles read and written once (16 B per updated entry) + the two operand panels
    // read once (K columns over the rows below the first updated column)
    ctx->trailing_tag[(size_t)ctx->n_trailing] = {used_bn, fl, 16.0 * (fl / (2.0 * K)) + 16.0 * (double)K * (double)(g.Npad - row_begin),
                                                  16.0 * (fl / (2.0 * K))};
    ctx->n_trailing++;
    return 0;
}

// Rank-nb update of every locally owned panel to the right of panel p.
int trailing_update(Ctx* ctx, int64_t p) {
    const Geo& g = ctx->g;
    if (g.panel_c0(p) + g.panel_w(p) >= g.Npad) return 0;
    int64_t q = p + 1;
    while (q < g.npanels && g.owner(q) != g.rank) ++q;
    if (q >= g.npanels) return 0;
    const int64_t local_panels = (g.ncols_local + g.nb - 1) / g.nb;
    return timed_update(ctx, p, 1, q / g.world, local_panels - q / g.world);
}

// Reset of the device-side statistics, on `st` (the stream the first tile kernels of this factorisation run on; default: the
// handle's).  A kernel, not a copy from a stack temporary followed by a host synchronisation (rounds 1-3): the host must be
// able to enqueue the first group's chain while the assembly is still running.
int factor_begin(Ctx* ctx, hipStream_t st) {
    if (!st) st = ctx->stream;
    hipLaunchKernelGGL(k_init_stats, dim3(1), dim3(64), 0, st, ctx->dstats);
    PYIPM_KCHECK();
    ctx->n_trailing = 0; ctx->trailing_flops = 0.0; ctx->trailing_area = 0.0;
    return 0;
}

// the statistics record as the C-ABI hands it out (growth travels as the bit pattern of a non-negative double)
pyipm_factor_stats to_stats(const DevStats& z) {
    pyipm_factor_stats s;
    s.n_neg = z.n_neg; s.n_zero = z.n_zero; s.n_2x2 = z.n_2x2; s.n_pos = z.n_pos;
    s.d_min = z.d_min; s.d_max = z.d_max;
    memcpy(&s.growth, &z.growth_bits, sizeof(s.growth));
    s.nonfinite = z.nonfinite;
    return s;
}

int factor_end(Ctx* ctx, pyipm_factor_stats* stats) {
    DevStats z;
    PYIPM_HIP(hipMemcpyAsync(&z, ctx->dstats, sizeof(z), hipMemcpyDeviceToHost, ctx->stream));
    // the error words of the device-driven launches, in the order they are reported in.  (prefix and range sweeps: the main stream has joined
    // ctx->fwd by now, this step's launch is behind us.)  `used` falls once the word has been read, whatever it held.
    constexpr int NPW = 4;
    PollWords* const pw[NPW] = {&ctx->chain_words, &ctx->sweep_words, &ctx->fwdp_words, &ctx->fwdr_words};
    int perr[NPW] = {0, 0, 0, 0};
    for (int k = 0; k < NPW; ++k) if (pw[k]->used && pw[k]->buf) PYIPM_HIP(pw[k]->fetch_err(&perr[k], ctx->stream));
    PYIPM_HIP(hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < NPW; ++k) pw[k]->used = false;
    for (int k = 0; k < NPW; ++k) {
        if (!perr[k]) continue;
        PYIPM_HIP(pw[k]->clear_err(ctx->stream));
        if (pw[k] == &ctx->chain_words) ctx->held.factor_invalid();
        ctx->err = pw[k]->message; return PYIPM_E_HIP;
    }
    if (ctx->profile) {
        // time during which SOME update launch ran: the launches of the main stream are serial, a lookahead head on the
        // side stream may overlap the bulk update that follows it -- union of the intervals, not their sum
        std::vector<std::pair<float, float>> iv;
        for (int64_t i = 0; i < ctx->n_trailing; ++i) {
            float a = 0.f, d = 0.f;
            PYIPM_HIP(hipEventElapsedTime(&a, ctx->ev_trailing[0].first, ctx->ev_trailing[i].first));
            PYIPM_HIP(hipEventElapsedTime(&d, ctx->ev_trailing[i].first, ctx->ev_trailing[i].second));
            iv.push_back({a, a + d});
        }
        std::sort(iv.begin(), iv.end());
        double uni = 0.0, sum = 0.0; float hi = -1.0e30f;
        int64_t nreal = 0;
        for (auto& x : iv) {
            sum += x.second - x.first;
            if (x.second - x.first > 0.03f) ++nreal;           // (a launch whose tile list came out empty leaves two events a few
                                                               //  microseconds apart; the shortest real launch takes 70 us)
            if (x.second <= hi) continue;
            uni += x.second - (x.first > hi ? x.first : hi);
            hi = x.second;
        }
        for (int k = 0; k < 2; ++k) { ctx->inst_ms[k] = 0.0; ctx->inst_flops[k] = 0.0; ctx->inst_area[k] = 0.0; ctx->inst_cbytes[k] = 0.0; ctx->inst_n[k] = 0; }
        for (int64_t i = 0; i < ctx->n_trailing && (size_t)i < ctx->trailing_tag.size(); ++i) {
            float d = 0.f;
            PYIPM_HIP(hipEventElapsedTime(&d, ctx->ev_trailing[i].first, ctx->ev_trailing[i].second));
            if (d <= 0.03f) continue;                            // (empty tile list: see above)
            const int k = ctx->trailing_tag[(size_t)i].bn == 256 ? 1 : 0;
            ctx->inst_ms[k] += d; ctx->inst_flops[k] += ctx->trailing_tag[(size_t)i].flops; ctx->inst_area[k] += ctx->trailing_tag[(size_t)i].area;
            ctx->inst_cbytes[k] += ctx->trailing_tag[(size_t)i].cbytes;
            ctx->inst_n[k]++;
        }
        ctx->t_trailing = sum;                               // what a kernel trace adds up for the same launches
        ctx->t_trailing_union = uni;
        ctx->n_trailing_real = nreal;
    }
    ctx->held.factor_read_back(z.nonfinite != 0);
    if (stats) *stats = to_stats(z);
    if (z.nonfinite) { ctx->err = "NaN/Inf met during factorisation"; return PYIPM_E_NONFINITE; }
    return 0;
}

// nrhs right-hand sides at stride vstride (doubles) share every launch (last grid dimension); the single-vector
// callers use the defaults.
// A panel wider than wide_sub columns is swept in sub-panels of that width (the in-panel kernels are one workgroup with nt - 1
// dependent steps: at nb = 1024 the sweeps took 5.9 ms instead of 2.1): the launches of the same matrix at nb = wide_sub.
static int sub_width(const Ctx* ctx, int pw) {
    return (ctx->wide_sub >= TB && ctx->wide_sub % TB == 0 && pw > ctx->wide_sub) ? ctx->wide_sub : pw;
}
// One sub-panel of a walk: nbw columns at global column c0 (local lc0), `below` rows under them and, where there are any, the row
// ranges in which L of these columns can be non-zero (active_ranges).  for_sub_panels: body(SweepSub) for the sub-panels of panel p
// at sub-width sw, first to last or last first (walk_sub, sub_walk.hpp); the first non-zero return ends the walk.
struct SweepSub { int64_t c0, lc0; int nbw; int64_t below, a0, a1, b0, b1; };
template <class F>
static int for_sub_panels(const Ctx* ctx, int64_t p, int sw, bool last_first, F body) {
    const Geo& g = ctx->g;
    return walk_sub((int)g.panel_w(p), sw, last_first, [&](int off, int nbw) {
        SweepSub s = {g.panel_c0(p) + off, g.local_c0(p) + off, nbw, g.Npad - (g.panel_c0(p) + off + nbw), 0, 0, 0, 0};
        if (s.below > 0) active_ranges(ctx, s.c0, s.c0 + nbw, &s.a0, &s.a1, &s.b0, &s.b1);
        return body(s);
    });
}
int fwd_panel(Ctx* ctx, int64_t p, double* v, hipStream_t stream, int nrhs, int64_t vstride) {
    if (!stream) stream = ctx->stream;
    const Geo& g = ctx->g;
    return for_sub_panels(ctx, p, sub_width(ctx, (int)g.panel_w(p)), false, [&](const SweepSub& s) {
        hipLaunchKernelGGL(k_fwd_diag, dim3(1, nrhs), dim3(s.nbw), s.nbw * sizeof(double), stream, ctx->A, g.Npad, s.lc0, s.c0, s.nbw, v, vstride);
        PYIPM_KCHECK();
        if (s.below > 0) {
            hipLaunchKernelGGL(k_fwd_gemv, dim3(grid1(s.below).x, nrhs), dim3(256), s.nbw * sizeof(double), stream, ctx->A, g.Npad, s.lc0, s.c0,
                               s.nbw, s.c0 + s.nbw, g.Npad, v, vstride, s.a0, s.a1, s.b0, s.b1);
            PYIPM_KCHECK();
        }
        return 0;
    });
}

int diag_panel(Ctx* ctx, int64_t p, double* v, hipStream_t stream, int nrhs, int64_t vstride) {
    if (!stream) stream = ctx->stream;
    const Geo& g = ctx->g;
    const int64_t c0 = g.panel_c0(p);
    const int nbw = (int)g.panel_w(p);
    hipLaunchKernelGGL(k_diag_apply, dim3(nbw / TB, nrhs), dim3(64), 0, stream, ctx->Dinv, ctx->Tsv, ctx->Tflag, ctx->block_refine,
                       c0 / TB, c0, v, vstride);
    PYIPM_KCHECK();
    return 0;
}

// part / pstride: partial-sum buffer for several right-hand sides (>= nchunk*nb doubles each); default = the handle's own
int bwd_panel(Ctx* ctx, int64_t p, double* v, int nrhs, int64_t vstride, double* part, int64_t pstride) {
    const Geo& g = ctx->g;
    if (!part) part = ctx->partial;
    return for_sub_panels(ctx, p, sub_width(ctx, (int)g.panel_w(p)), true, [&](const SweepSub& s) {      // last first (see fwd_panel)
        int nchunk = 0;
        if (s.below > 0) {
            nchunk = (int)((s.below + ROWCHUNK - 1) / ROWCHUNK);
            hipLaunchKernelGGL(k_bwd_dot, dim3(s.nbw, nchunk, nrhs), dim3(256), 0, ctx->stream, ctx->A, g.Npad, s.lc0, g.nb,
                               s.c0 + s.nbw, g.Npad, v, part, vstride, pstride, s.a0, s.a1, s.b0, s.b1);
            PYIPM_KCHECK();
        }
        if (s.nbw <= 4 * TB)                                // on 1024 threads through shared memory; wider panels: thread k walks down column k
            hipLaunchKernelGGL(k_bwd_diag4, dim3(1, nrhs), dim3(1024), 0, ctx->stream, ctx->A, g.Npad, s.lc0, s.c0, s.nbw,
                               g.nb, part, nchunk, v, vstride, pstride);
        else
            hipLaunchKernelGGL(k_bwd_diag, dim3(1, nrhs), dim3(s.nbw), s.nbw * sizeof(double), ctx->stream, ctx->A, g.Npad, s.lc0, s.c0, s.nbw,
                               g.nb, part, nchunk, v, vstride, pstride);
        PYIPM_KCHECK();
        return 0;
    });
}

// ---- the one-launch sweeps: k_fwd_sweep, k_bwd_sweep (solve_plain), k_fwd_prefix (a reusing step) -------------------------------
// what the three ask of the handle and its geometry; each caller adds its own terms
static bool sweeps_in_one_launch(const Ctx* ctx) {
    const Geo& g = ctx->g;
    return ctx->sweep_persist && g.world == 1 && g.nb <= 4 * TB && g.nb % TB == 0 && g.npanels >= 2 && g.npanels <= 4096 &&
           g.Npad % 8 == 0 && g.Npad / TB <= 8192;
}
static SweepGeo sweep_geo(const Ctx* ctx) {
    const Geo& g = ctx->g;
    SweepGeo sg;
    sg.Npad = g.Npad; sg.ld = g.Npad; sg.n = g.n; sg.mi = g.mi; sg.me = g.me; sg.nb = g.nb; sg.npanels = (int)g.npanels;
    sg.skip = (ctx->skip_zeros && g.mi > 0) ? 1 : 0;
    return sg;
}
// Every workgroup of a sweep must be resident (they wait for each other): the grid comes from an occupancy query of THIS build of
// the kernel, not from an assumption about its registers / shared memory.  *occ: resident workgroups per CU, cached.
// must_fit: the message of the error where none fits (NULL: the caller clamps).
template <class K>
static int resident_per_cu(Ctx* ctx, int* occ, K kernel, int threads, const char* must_fit) {
    if (*occ <= 0) PYIPM_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(occ, kernel, threads, 0));
    if (*occ < 1 && must_fit) { ctx->err = must_fit; return PYIPM_E_HIP; }
    return 0;
}
// ... `want` workgroups, at most `resident` per CU, at most `cap`, at most the test hook's, at least `floor`
static unsigned sweep_grid(const Ctx* ctx, int64_t want, int resident, int64_t floor, int64_t cap = INT64_MAX) {
    int64_t blocks = std::min(std::min(want, (int64_t)resident * ctx->num_cus), cap);
    if (ctx->sweep_max_blocks > 0 && blocks > ctx->sweep_max_blocks) blocks = ctx->sweep_max_blocks;      // (test hook: several chunks per owner)
    return (unsigned)std::max(blocks, floor);
}

// forward sweep in one launch (k_fwd_sweep: workgroup 0 on the diagonal blocks, the others on their 64-row chunks), then
// inv(T) y for all tiles at once
static int fwd_sweep(Ctx* ctx, double* v) {
    const Geo& g = ctx->g;
    PollWords& sw = ctx->sweep_words;
    PYIPM_HIP(sw.ensure(ctx->stream));
    PYIPM_HIP(sw.arm((size_t)(g.npanels + g.Npad / TB), ctx->stream));
    { int rc = resident_per_cu(ctx, &ctx->occ_fwd_sweep, k_fwd_sweep, 512, nullptr); if (rc) return rc; }
    const int occ = ctx->occ_fwd_sweep < 1 ? 1 : (ctx->occ_fwd_sweep > 2 ? 2 : ctx->occ_fwd_sweep);
    hipLaunchKernelGGL(k_fwd_sweep, dim3(sweep_grid(ctx, 1 + (g.Npad / TB - g.nb / TB), occ, 2)), dim3(512), 0, ctx->stream,
                       ctx->A, sweep_geo(ctx), v, sw.buf.get(), sw.err(), POLL_TIMEOUT);
    PYIPM_KCHECK();
    hipLaunchKernelGGL(k_diag_apply, dim3((unsigned)(g.Npad / TB), 1), dim3(64), 0, ctx->stream, ctx->Dinv, ctx->Tsv, ctx->Tflag,
                       ctx->block_refine, (int64_t)0, (int64_t)0, v, (int64_t)0);
    PYIPM_KCHECK();
    sw.used = true;
    return 0;
}
// the whole backward sweep in one launch (k_bwd_sweep): workgroup 0 on the diagonal blocks, every other wave on its columns
static int bwd_sweep(Ctx* ctx, double* v) {
    const Geo& g = ctx->g;
    PollWords& sw = ctx->sweep_words;
    PYIPM_HIP(ctx->sweep_buf.reserve((size_t)g.Npad));
    PYIPM_HIP(sw.ensure(ctx->stream));
    PYIPM_HIP(sw.arm((size_t)(2 * g.npanels + 4096), ctx->stream));     // flags, near counts, a progress word per owner wave
    PYIPM_HIP(hipMemsetAsync(ctx->sweep_buf, 0xFF, (size_t)g.Npad * sizeof(double), ctx->stream));      // NaN: "not there yet"
    const int64_t nearb = (g.nb / 8 + 15) / 16;                  // workgroups that only do the next panel's columns
    { int rc = resident_per_cu(ctx, &ctx->occ_bwd_sweep, k_bwd_sweep, 1024, "k_bwd_sweep does not fit a compute unit"); if (rc) return rc; }
    // one workgroup per CU by design, whatever would fit.  The cap: a progress word per owner WAVE, (blocks - 1 - nearb) x 16 of them,
    // inside the 4096 words zeroed above (on a part with more than 257 CUs the words beyond them would keep last sweep's
    // counts and workgroup 0 would stop waiting)
    const unsigned blocks = sweep_grid(ctx, 1 + nearb + (g.Npad / 8 + 15) / 16, 1, 2 + nearb, 1 + nearb + 4096 / 16);
    // workgroup 0 leaves the closed-form slack panels out of its walk (bwd_chain_plan.hpp)
    const SweepGeo sg = sweep_geo(ctx);
    const BwdChain ch = bwd_chain(BwdChainGeo{sg.Npad, sg.n, sg.mi, sg.nb, sg.npanels, sg.skip}, ctx->bwd_slack);
    hipLaunchKernelGGL(k_bwd_sweep, dim3(blocks), dim3(1024), 0, ctx->stream, ctx->A, sg, ch, v, sw.buf.get(), sw.err(),
                       POLL_TIMEOUT, ctx->sweep_buf.get(), ctx->dbg_buf);
    PYIPM_KCHECK();
    sw.used = true;
    return 0;
}

// x := M^{-1} x in place for the factored matrix of the current geometry (single-rank path)
int solve_plain(Ctx* ctx, double* v, bool forward_done, int nrhs, int64_t vstride, double* part, int64_t pstride) {
    const Geo& g = ctx->g;
    const bool one_launch = sweeps_in_one_launch(ctx) && nrhs == 1;
    if (!forward_done && one_launch) {
        int rc = fwd_sweep(ctx, v); if (rc) return rc;
    } else if (!forward_done) {
        for (int64_t p = 0; p < g.npanels; ++p) { int rc = fwd_panel(ctx, p, v, nullptr, nrhs, vstride); if (rc) return rc; }
        for (int64_t p = 0; p < g.npanels; ++p) { int rc = diag_panel(ctx, p, v, nullptr, nrhs, vstride); if (rc) return rc; }
    }
    if (one_launch) return bwd_sweep(ctx, v);
    for (int64_t p = g.npanels - 1; p >= 0; --p) { int rc = bwd_panel(ctx, p, v, nrhs, vstride, part, pstride); if (rc) return rc; }
    return 0;
}

// The forward substitution of a reusing step through the kept panels [0, P0) (k_fwd_prefix + one k_diag_apply over their tiles) on
// `stream`, in place of P0 x (k_fwd_diag, k_fwd_gemv, k_diag_apply): the same bits.  Applies where solve_plain's one-launch sweeps
// do; the caller keeps the per-panel loop otherwise.  The words are this launch's own (a solve may still be running on the main
// stream with ctx->sweep_words): flags and a progress word per chunk, zeroed on the same stream in front of every launch.
// (the plan adds what depends on the prefix: at least one panel, all of them inside the x block)
static bool fwd_prefix_applies(const Ctx* ctx) {
    const Geo& g = ctx->g;
    return ctx->fwd_prefix && sweeps_in_one_launch(ctx) && g.nb % (2 * TB) == 0 && sub_width(ctx, (int)g.nb) == (int)g.nb;
}
static int fwd_prefix(Ctx* ctx, int64_t P0, double* v, hipStream_t stream) {
    const Geo& g = ctx->g;
    PollWords& fw = ctx->fwdp_words;
    const int64_t nchunks = g.Npad / TB;
    PYIPM_HIP(fw.ensure(stream));
    PYIPM_HIP(fw.arm((size_t)(P0 + nchunks), stream));
    { int rc = resident_per_cu(ctx, &ctx->occ_fwd_prefix, k_fwd_prefix, 256, "k_fwd_prefix does not fit a compute unit"); if (rc) return rc; }
    // a guest beside the factorisation, whose chains and heads run meanwhile: fwd_prefix_wgs workgroups (profiles/fwd_prefix_resident_ab.json)
    const unsigned blocks = sweep_grid(ctx, 1 + (nchunks - g.nb / TB), ctx->occ_fwd_prefix, 2, ctx->fwd_prefix_wgs);
    hipLaunchKernelGGL(k_fwd_prefix, dim3(blocks), dim3(256), 0, stream, ctx->A, sweep_geo(ctx), (int)P0, v, fw.buf.get(), fw.err(),
                       POLL_TIMEOUT);
    PYIPM_KCHECK();
    hipLaunchKernelGGL(k_diag_apply, dim3((unsigned)(P0 * g.nb / TB), 1), dim3(64), 0, stream, ctx->Dinv, ctx->Tsv, ctx->Tflag,
                       ctx->block_refine, (int64_t)0, (int64_t)0, v, (int64_t)0);
    PYIPM_KCHECK();
    fw.used = true;
    return 0;
}

// The other kept panels of a reusing step, [Pa, Pb) behind the prefix -- the closed-form slack panels and the kept lambda_e groups --
// in one launch of their own (k_fwd_range + one k_diag_apply over their tiles) in place of (Pb - Pa) x 3 dependent launches: the
// same bits (panels ascending, k_fwd_gemv's sums).  Its words are its own: the prefix launch in front of it may still be polling its.
// fwd_range_grid: the workgroups of that launch, 0 where it does not apply (every owner must be able to number its chunks).
static unsigned fwd_range_grid(Ctx* ctx, int64_t Pa, int64_t Pb) {
    const Geo& g = ctx->g;
    if (!ctx->fwd_range || Pb <= Pa || Pb >= g.npanels) return 0;
    if (resident_per_cu(ctx, &ctx->occ_fwd_range, k_fwd_range, 256, nullptr) || ctx->occ_fwd_range < 1) return 0;
    const SweepGeo sg = sweep_geo(ctx);
    // the owned chunks of the range: a function of the geometry and the range alone, counted once and kept (the enqueue path of
    // every reusing step comes through here)
    const int64_t key[8] = {sg.Npad, sg.n, sg.mi, sg.me, sg.nb, sg.skip, Pa, Pb};
    if (memcmp(key, ctx->fwd_range_key, sizeof(key)) != 0) {
        const FwdPlanGeo pg{sg.Npad, sg.n, sg.mi, sg.me, sg.nb, sg.skip};
        int64_t owned = 0;
        for (int64_t c = (Pa + 1) * (g.nb / TB); c < g.Npad / TB; ++c) owned += fwd_plan_owned(pg, (int)Pa, (int)Pb, (int)c) ? 1 : 0;
        memcpy(ctx->fwd_range_key, key, sizeof(key)); ctx->fwd_range_owned = owned;
    }
    const int64_t owned = ctx->fwd_range_owned;
    const unsigned blocks = sweep_grid(ctx, 1 + owned, ctx->occ_fwd_range, 2, ctx->fwd_range_wgs);
    // (k_fwd_range's owners hold the numbers of at most FWDR_MAXOWN chunks each: a grid that would give one more is not launched)
    return (owned + blocks - 2) / (blocks - 1) <= FWDR_MAXOWN ? blocks : 0;
}
static int fwd_range(Ctx* ctx, int64_t Pa, int64_t Pb, unsigned blocks, double* v, hipStream_t stream) {
    const Geo& g = ctx->g;
    PollWords& fw = ctx->fwdr_words;
    PYIPM_HIP(fw.ensure(stream));
    PYIPM_HIP(fw.arm((size_t)((Pb - Pa) + g.Npad / TB), stream));
    hipLaunchKernelGGL(k_fwd_range, dim3(blocks), dim3(256), 0, stream, ctx->A, sweep_geo(ctx), (int)Pa, (int)Pb, v, fw.buf.get(), fw.err(),
                       POLL_TIMEOUT);
    PYIPM_KCHECK();
    hipLaunchKernelGGL(k_diag_apply, dim3((unsigned)((Pb - Pa) * g.nb / TB), 1), dim3(64), 0, stream, ctx->Dinv, ctx->Tsv, ctx->Tflag,
                       ctx->block_refine, Pa * g.nb / TB, Pa * g.nb, v, (int64_t)0);
    PYIPM_KCHECK();
    fw.used = true;
    return 0;
}

// ---- condensed option: right-hand side reduction and solution expansion --------------------------
// vc <- [ b_x + Ji (Sigma b_i + b_s) ; b_e ; 0 ]   from a full-order right-hand side b
// (every rank of a distributed run does both over ALL rows: the vectors are replicated and the blocks fully staged)
static RowMap all_rows(const Geo& g) { Geo g1 = g; g1.world = 1; g1.rank = 0; return make_rowmap(g1, 0); }

int cond_reduce(Ctx* ctx, const double* b, double* vc) {
    const Geo& g = ctx->g;
    hipLaunchKernelGGL(k_cond_t, grid1(g.mi), dim3(256), 0, ctx->stream, ctx->vt, b, g, ctx->s, ctx->lda + g.me, ctx->eps,
                       ctx->cond_pos);
    PYIPM_KCHECK();
    hipLaunchKernelGGL(k_rowdot2, grid1(g.n, 4), dim3(256), 0, ctx->stream, vc, b, g.n,
                       (const double*)nullptr, (int64_t)0, (const double*)nullptr, (int64_t)0,
                       ctx->Ji, ctx->ld_Ji, ctx->vt, g.mi, 0, 0, all_rows(g));
    PYIPM_KCHECK();
    if (ctx->gc.Npad > g.n) {
        hipLaunchKernelGGL(k_cond_gather, grid1(ctx->gc.Npad - g.n), dim3(256), 0, ctx->stream, vc, b, g, ctx->gc.Npad,
                           ctx->cond_idx, ctx->cond_na, ctx->s, ctx->lda + g.me, ctx->eps);
        PYIPM_KCHECK();
    }
    return 0;
}

// v (holding the full right-hand side) <- [dx ; ds ; dle ; dli] from the condensed solution vc
int cond_expand(Ctx* ctx, const double* vc, double* v) {
    const Geo& g = ctx->g;
    const int nchunk = 64;
    const int64_t rpc = (g.n + nchunk - 1) / nchunk;
    hipLaunchKernelGGL(k_coldot_partial, dim3((unsigned)((g.mi + 255) / 256), nchunk), dim3(256), 0, ctx->stream,
                       ctx->partial, ctx->Ji, ctx->ld_Ji, g.n, g.mi, vc, rpc, 0, all_rows(g));
    PYIPM_KCHECK();
    hipLaunchKernelGGL(k_coldot_reduce, grid1(g.mi), dim3(256), 0, ctx->stream, ctx->vt, ctx->partial, g.mi, nchunk, 0);
    PYIPM_KCHECK();
    hipLaunchKernelGGL(k_cond_expand, grid1(g.Npad), dim3(256), 0, ctx->stream, v, vc, ctx->vt, g, ctx->s, ctx->lda + g.me, ctx->eps,
                       ctx->cond_pos);
    PYIPM_KCHECK();
    return 0;
}

// x := Hc^{-1} x  in place on a full-order Npad device vector (single-rank path).  With the condensed
// factor: reduce, solve the (n+me) system, expand.  forward_done: the fused pass already ran (on v, or on
// ctx->vc for the condensed factor, in which case v still holds the right-hand side).
int solve_inplace(Ctx* ctx, double* v, bool forward_done) {
    if (!ctx->held.cond_active) return solve_plain(ctx, v, forward_done);
    int rc;
    if (!forward_done) { rc = cond_reduce(ctx, v, ctx->vc); if (rc) return rc; }
    { GeoSwap sw(ctx, ctx->gc); rc = solve_plain(ctx, ctx->vc, forward_done); }
    if (rc) return rc;
    return cond_expand(ctx, ctx->vc, v);
}

// ---- many right-hand sides: pyipm_newton_solve_many (kernels_msolve.hpp) --------------------------------------------
// V := M^{-1} V in place for kpad columns at stride ldv (the current geometry's Npad), kpad a multiple of MS_KB, single
// rank: the per-panel structure of solve_plain (wide_sub sub-panels, active_ranges) with every GEMV a product over
// column blocks.  part: >= (ceil(Npad / MS_RCH) + 1) * kpad * MS_SUBW doubles (the partials, then their sums).
void solve_many_sizes(int64_t Npad, int64_t k, int64_t* kpad, size_t* part_doubles) {
    *kpad = (k + MS_KB - 1) / MS_KB * MS_KB;
    *part_doubles = (size_t)((Npad + MS_RCH - 1) / MS_RCH + 1) * (size_t)*kpad * (size_t)MS_SUBW;      // partials + their sums
}
int solve_many_plain(Ctx* ctx, double* V, int64_t ldv, int64_t kpad, double* part) {
    const Geo& g = ctx->g;
    const hipStream_t st = ctx->stream;
    auto ms_width = [&](int64_t p) { return std::min(sub_width(ctx, (int)g.panel_w(p)), (int)MS_SUBW); };     // (the in-panel kernels' limit)
    for (int64_t p = 0; p < g.npanels; ++p) {
        int rc = for_sub_panels(ctx, p, ms_width(p), false, [&](const SweepSub& s) {
            hipLaunchKernelGGL(k_ms_fwd_diag, dim3((unsigned)(kpad / MS_CW)), dim3(512), 0, st,
                               ctx->A, g.Npad, s.lc0, s.c0, s.nbw, V, ldv);
            PYIPM_KCHECK();
            if (s.below > 0) {
                hipLaunchKernelGGL(k_ms_fwd_gemm, dim3((unsigned)(kpad / MS_KB), (unsigned)(s.below / TB)), dim3(256), 0, st,
                                   ctx->A, g.Npad, s.lc0, s.c0, s.nbw, s.c0 + s.nbw, V, ldv, s.a0, s.a1, s.b0, s.b1);
                PYIPM_KCHECK();
            }
            return 0;
        });
        if (rc) return rc;
    }
    hipLaunchKernelGGL(k_ms_diag, dim3((unsigned)(kpad / MS_CW), (unsigned)(g.Npad / TB)), dim3(256), 0, st, ctx->Dinv, ctx->Tsv,
                       ctx->Tflag, ctx->block_refine, V, ldv);
    PYIPM_KCHECK();
    for (int64_t p = g.npanels - 1; p >= 0; --p) {
        int rc = for_sub_panels(ctx, p, ms_width(p), true, [&](const SweepSub& s) {
            const double* sums = nullptr;
            if (s.below > 0) {
                const int nchunk = (int)((s.below + MS_RCH - 1) / MS_RCH);
                hipLaunchKernelGGL(k_ms_bwd_part, dim3((unsigned)(kpad / MS_KB), (unsigned)(s.nbw / TB), (unsigned)nchunk), dim3(256), 0, st,
                                   ctx->A, g.Npad, s.lc0, s.nbw, s.c0 + s.nbw, g.Npad, V, ldv, part, kpad, s.a0, s.a1, s.b0, s.b1);
                PYIPM_KCHECK();
                const int64_t nelem = kpad * s.nbw;
                double* red = part + (size_t)nchunk * (size_t)nelem;
                hipLaunchKernelGGL(k_ms_bwd_reduce, dim3((unsigned)(nelem / 64)), dim3(256), 0, st, part, nchunk, nelem, red);
                PYIPM_KCHECK();
                sums = red;
            }
            hipLaunchKernelGGL(k_ms_bwd_diag, dim3((unsigned)(kpad / MS_CW)), dim3(512), 0, st,
                               ctx->A, g.Npad, s.lc0, s.c0, s.nbw, sums, V, ldv);
            PYIPM_KCHECK();
            return 0;
        });
        if (rc) return rc;
    }
    return 0;
}

// X := Hc^{-1} X for full-order columns (ld = Npad; k real columns, the rest of kpad zero).  With the condensed factor the
// columns are reduced into Xc (ld = gc.Npad) one by one, solved together, expanded one by one (cond_reduce / cond_expand
// are O(N) per column apart from the Ji products).
int solve_many_inplace(Ctx* ctx, double* X, int64_t k, int64_t kpad, double* part, double* Xc) {
    const Geo& g = ctx->g;
    if (!ctx->held.cond_active) return solve_many_plain(ctx, X, g.Npad, kpad, part);
    const int64_t ldc = ctx->gc.Npad;
    int rc;
    if (kpad > k) PYIPM_HIP(hipMemsetAsync(Xc + k * ldc, 0, (size_t)((kpad - k) * ldc) * sizeof(double), ctx->stream));
    for (int64_t j = 0; j < k; ++j) { rc = cond_reduce(ctx, X + j * g.Npad, Xc + j * ldc); if (rc) return rc; }
    { GeoSwap sw(ctx, ctx->gc); rc = solve_many_plain(ctx, Xc, ldc, kpad, part); }
    if (rc) return rc;
    for (int64_t j = 0; j < k; ++j) { rc = cond_expand(ctx, Xc + j * ldc, X + j * g.Npad); if (rc) return rc; }
    return 0;
}

// Y = Hc V for k columns (column j at V + j * ldv, Y + j * ldy) from the staged blocks, the handle's current shifts, in ONE launch
// (kernels_kmany.hpp); single rank.  Rows 0 .. N-1 of every column are written, with pad also rows N .. Npad-1 (y = v there, as
// kkt_matvec_dev leaves them; ldv, ldy >= Npad then).  Writes nothing but Y: no work vector, nothing of Held.
int kkt_matvec_many_dev(Ctx* ctx, int64_t k, const double* V, int64_t ldv, double* Y, int64_t ldy, bool pad) {
    const Geo& g = ctx->g;
    if (!ctx->held.have_blocks || !ctx->held.have_vectors) { ctx->err = "kkt_matvec_many: stage blocks and vectors first"; return PYIPM_E_BADARG; }
    if (k <= 0) return 0;
    KmArgs a;
    a.U = ctx->d2L; a.ldu = ctx->ld_d2L; a.Je = ctx->Je; a.lde = ctx->ld_Je; a.Ji = ctx->Ji; a.ldi = ctx->ld_Ji;
    a.s = ctx->s; a.lda = ctx->lda; a.eps = ctx->eps; a.delta = ctx->delta; a.delta_c = ctx->delta_c;
    a.n = g.n; a.me = g.me; a.mi = g.mi; a.N = g.N; a.rows_out = pad ? g.Npad : g.N;
    a.V = V; a.ldv = ldv; a.Y = Y; a.ldy = ldy; a.k = k;
    a.tx = (int)((g.n + KM_TR - 1) / KM_TR); a.te = (int)((g.me + KM_TR - 1) / KM_TR); a.ti = (int)((g.mi + KM_TR - 1) / KM_TR);
    a.ts = a.ti;
    const int tiles = a.tx + a.te + a.ti + a.ts + (a.rows_out > a.N ? 1 : 0);
    hipLaunchKernelGGL(k_kmany, dim3((unsigned)((k + KM_KB - 1) / KM_KB), (unsigned)tiles), dim3(256), 0, ctx->stream, a);
    PYIPM_KCHECK();
    return 0;
}

// The whole call after argument checks.  Device pointers: the launch reads v and writes y where they are.  Host pointers: packed
// (ld = N) through ctx->km_buf, outside the workspace.
int kkt_matvec_many(Ctx* ctx, int64_t k, const double* v, int64_t ld_v, double* y, int64_t ld_y, int memkind) {
    const Geo& g = ctx->g;
    const hipStream_t st = ctx->stream;
    if (memkind == PYIPM_MEM_DEVICE) return kkt_matvec_many_dev(ctx, k, v, ld_v, y, ld_y, false);
    const size_t col = (size_t)g.N * (size_t)k, need = 2 * col;
    if (ctx->km_buf.capacity() < need) {
        PYIPM_HIP(ctx->km_buf.reserve(need));
        if (getenv("PYIPM_POISON_WORKSPACE")) PYIPM_HIP(hipMemsetAsync(ctx->km_buf, 0xFF, need * sizeof(double), st));   // as the workspace
    }
    double* Vd = ctx->km_buf;
    double* Yd = Vd + col;
    PYIPM_HIP(hipMemcpy2DAsync(Vd, (size_t)g.N * sizeof(double), v, (size_t)ld_v * sizeof(double), (size_t)g.N * sizeof(double),
                               (size_t)k, hipMemcpyHostToDevice, st));
    PYIPM_HIP(hipStreamSynchronize(st));                                     // host memory not retained
    int rc = kkt_matvec_many_dev(ctx, k, Vd, g.N, Yd, g.N, false); if (rc) return rc;
    PYIPM_HIP(hipMemcpy2DAsync(y, (size_t)ld_y * sizeof(double), Yd, (size_t)g.N * sizeof(double), (size_t)g.N * sizeof(double),
                               (size_t)k, hipMemcpyDeviceToHost, st));
    PYIPM_HIP(hipStreamSynchronize(st));
    return 0;
}

// The whole call after argument checks: stage, solve, refine, flip, copy out.  Every vector lives in ctx->ms_buf: v0 - v3,
// vc, the kept residual and the factor are not touched, so a pending fused forward pass and the last direction survive.
int solve_many(Ctx* ctx, int64_t k, const double* rhs, int64_t ld_rhs, double* dz, int64_t ld_dz, int flip, int refine,
               int memkind) {
    const Geo& g = ctx->g;
    const hipStream_t st = ctx->stream;
    refine = refine_steps(ctx, refine);                 // (the buffers below depend on it)
    const bool adaptive = refine < 0;
    const int64_t Np = g.Npad, Nc = ctx->held.cond_active ? ctx->gc.Npad : 0;
    int64_t kpad; size_t n_part;
    solve_many_sizes(Np, k, &kpad, &n_part);
    const size_t col = (size_t)Np * (size_t)kpad;
    size_t need = col + (size_t)Nc * (size_t)kpad + n_part;                    // X, Xc, partials
    if (refine != 0) need += 2 * col;                                           // B, R
    if (adaptive) need += col + 2 * (size_t)kpad;                               // the spare iterate, per-column sums
    if (ctx->ms_buf.capacity() < need) {
        PYIPM_HIP(ctx->ms_buf.reserve(need));
        if (getenv("PYIPM_POISON_WORKSPACE")) PYIPM_HIP(hipMemsetAsync(ctx->ms_buf, 0xFF, need * sizeof(double), st));   // as the workspace
    }
    double* X = ctx->ms_buf;
    double* Xc = X + col;
    double* part = Xc + (size_t)Nc * (size_t)kpad;
    double* B = part + n_part;
    double* R = B + col;
    double* Xp = R + col;
    double* ss_dev = Xp + col;
    // right-hand sides into X: rows N .. Npad and columns k .. kpad zero
    PYIPM_HIP(hipMemcpy2DAsync(X, (size_t)Np * sizeof(double), rhs, (size_t)ld_rhs * sizeof(double), (size_t)g.N * sizeof(double),
                               (size_t)k, memkind == PYIPM_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, st));
    if (Np > g.N) PYIPM_HIP(hipMemset2DAsync(X + g.N, (size_t)Np * sizeof(double), 0, (size_t)(Np - g.N) * sizeof(double), (size_t)k, st));
    if (kpad > k) PYIPM_HIP(hipMemsetAsync(X + k * Np, 0, (size_t)((kpad - k) * Np) * sizeof(double), st));
    if (memkind == PYIPM_MEM_HOST) PYIPM_HIP(hipStreamSynchronize(st));      // host memory not retained
    if (refine != 0) {
        PYIPM_HIP(hipMemcpyAsync(B, X, col * sizeof(double), hipMemcpyDeviceToDevice, st));
        PYIPM_HIP(hipMemsetAsync(R, 0, col * sizeof(double), st));             // (its pad columns stay zero)
    }
    int rc = solve_many_inplace(ctx, X, k, kpad, part, Xc); if (rc) return rc;
    // refinement: column by column for the product, all columns at once for the solve; the adaptive loop follows the WORST
    // column's backward error
    std::vector<double> ss(adaptive ? 2 * (size_t)k : 0);
    rc = refine_loop(ctx, refine,
        [&]() -> int {                                          // R = B - Hc X
            if (ctx->ms_matvec_many) { int r2 = kkt_matvec_many_dev(ctx, k, X, Np, R, Np, true); if (r2) return r2; }   // all columns in one launch
            else for (int64_t j = 0; j < k; ++j) { int r2 = kkt_matvec_dev(ctx, X + j * Np, R + j * Np); if (r2) return r2; }
            hipLaunchKernelGGL(k_axpby, grid1((int64_t)col), dim3(256), 0, st, R, B, R, 1.0, -1.0, (int64_t)col);
            PYIPM_KCHECK();
            return 0;
        },
        [&](double* worst) -> int {
            hipLaunchKernelGGL(k_ms_sumsq2, dim3((unsigned)k), dim3(1024), 0, st, ss_dev, R, B, Np, g.N);
            PYIPM_KCHECK();
            PYIPM_HIP(hipMemcpyAsync(ss.data(), ss_dev, 2 * (size_t)k * sizeof(double), hipMemcpyDeviceToHost, st));
            PYIPM_HIP(hipStreamSynchronize(st));
            double berr = 0.0;
            for (int64_t j = 0; j < k; ++j) {
                const double b = ss[2 * j + 1] > 0.0 ? sqrt(ss[2 * j] / ss[2 * j + 1]) : sqrt(ss[2 * j]);
                if (!(b <= berr) && berr == berr) berr = b;                        // (a NaN column makes the worst NaN)
            }
            *worst = berr;
            return 0;
        },
        [&]() -> int { PYIPM_HIP(hipMemcpyAsync(Xp, X, col * sizeof(double), hipMemcpyDeviceToDevice, st)); return 0; },
        [&]() -> int { PYIPM_HIP(hipMemcpyAsync(X, Xp, col * sizeof(double), hipMemcpyDeviceToDevice, st)); return 0; },
        [&]() -> int {                                          // X += Hc^{-1} R
            int r2 = solve_many_inplace(ctx, R, k, kpad, part, Xc); if (r2) return r2;
            hipLaunchKernelGGL(k_axpby, grid1((int64_t)col), dim3(256), 0, st, X, X, R, 1.0, 1.0, (int64_t)col);
            PYIPM_KCHECK();
            return 0;
        });
    if (rc) return rc;
    const int64_t from = g.n + g.mi;
    if (flip && g.N > from) {
        hipLaunchKernelGGL(k_ms_flip, grid1((g.N - from) * k), dim3(256), 0, st, X, Np, from, g.N, k);
        PYIPM_KCHECK();
    }
    PYIPM_HIP(hipMemcpy2DAsync(dz, (size_t)ld_dz * sizeof(double), X, (size_t)Np * sizeof(double), (size_t)g.N * sizeof(double),
                               (size_t)k, memkind == PYIPM_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, st));
    if (memkind == PYIPM_MEM_HOST) PYIPM_HIP(hipStreamSynchronize(st));
    return 0;
}

// y[0:n) = sym(triu(d2L)) v + delta v for the rows / columns this rank works on: one pass over the upper triangle
// (k_symv_tiles + k_symv_finish; ctx->partial holds the partials)
int symv_dev(Ctx* ctx, const double* v, double* y, double delta, const RowMap& rm) {
    const Geo& g = ctx->g;
    const int64_t n = g.n;
    const int nchunk = SYMV_CHUNKS;
    int64_t rpc = ((rm.nloc + nchunk - 1) / nchunk + 63) / 64 * 64; if (rpc < 64) rpc = 64;
    const int nch = (int)((rm.nloc + rpc - 1) / rpc);
    const int nseg = (int)((n + SYMV_SEG - 1) / SYMV_SEG);
    double* part_col = ctx->partial;
    double* part_row = ctx->partial + (size_t)nchunk * (size_t)n;
    if (nch > 0) {
        hipLaunchKernelGGL(k_symv_tiles, dim3((unsigned)nseg, (unsigned)nch), dim3(256), 0, ctx->stream, part_row, part_col,
                           ctx->d2L, ctx->ld_d2L, n, v, rpc, rm);
        PYIPM_KCHECK();
    }
    hipLaunchKernelGGL(k_symv_finish, grid1(n), dim3(256), 0, ctx->stream, y, part_row, part_col, n, v, delta, nseg, nch, rm);
    PYIPM_KCHECK();
    return 0;
}

// y = Hc v from the staged blocks (Npad vectors on the device).  With several ranks every rank adds the terms of the
// KKT columns it owns (row j of triu(d2L) | Je | Ji is column j of the lower triangle), rank 0 the element-wise s /
// multiplier part; the caller sums y over the ranks (dist_impl.hpp).
int kkt_matvec_dev(Ctx* ctx, const double* v, double* y) {
    const Geo& g = ctx->g;
    const int64_t n = g.n, me = g.me, mi = g.mi;
    if (!ctx->held.have_blocks || !ctx->held.have_vectors) { ctx->err = "matvec: stage blocks and vectors first"; return PYIPM_E_BADARG; }
    const RowMap rm = make_rowmap(g, ctx->sharded);
    const int64_t nl = rm.nloc;
    if (g.world > 1) { hipLaunchKernelGGL(k_fill, grid1(g.Npad), dim3(256), 0, ctx->stream, y, 0.0, g.Npad); PYIPM_KCHECK(); }
    if (nl > 0) {
        // x block: sym(triu(d2L)) v + delta v, one pass over the upper triangle (row sums and mirrored column sums together)
        { int r2 = symv_dev(ctx, v, y, ctx->delta, rm); if (r2) return r2; }
    }
    // s, lambda_e, lambda_i, pad: element-wise parts (one rank)
    if (g.Npad > n && g.rank == 0) {                   // (nothing beyond the x block when me = mi = 0 and n is a multiple of 128)
        hipLaunchKernelGGL(k_matvec_tail, grid1(g.Npad - n), dim3(256), 0, ctx->stream, y, v, g, ctx->s, ctx->lda,
                           ctx->eps, ctx->delta_c);
        PYIPM_KCHECK();
    }
    // + Je v_e, Ji v_i into the x rows and + Je' v_x, Ji' v_x into the multiplier rows: each Jacobian block is passed over ONCE
    // (round 4: k_jac_tiles -- row sums and column sums from the same loads, as for the triangle of d2L; was k_rowdot2 + k_coldot_*,
    // two passes)
    if (nl > 0) {
        int64_t rpc = ((nl + SYMV_CHUNKS - 1) / SYMV_CHUNKS + 63) / 64 * 64; if (rpc < 64) rpc = 64;
        const int nch = (int)((nl + rpc - 1) / rpc);
        for (int blk = 0; blk < 2; ++blk) {
            const int64_t m = blk == 0 ? me : mi;
            if (m <= 0) continue;
            const double* M = blk == 0 ? ctx->Je : ctx->Ji;
            const int64_t ldm = blk == 0 ? ctx->ld_Je : ctx->ld_Ji;
            const int64_t off = n + mi + (blk == 0 ? 0 : me);                 // the multiplier rows of this block
            const int nseg = (int)((m + SYMV_SEG - 1) / SYMV_SEG);
            double* part_col = ctx->partial;
            double* part_row = ctx->partial + (size_t)SYMV_CHUNKS * (size_t)m;
            hipLaunchKernelGGL(k_jac_tiles, dim3((unsigned)nseg, (unsigned)nch), dim3(256), 0, ctx->stream, part_row, part_col,
                               M, ldm, m, v + off, v, rpc, rm);
            PYIPM_KCHECK();
            hipLaunchKernelGGL(k_jac_finish_rows, grid1(nl), dim3(256), 0, ctx->stream, y, part_row, nseg, rm);
            PYIPM_KCHECK();
            hipLaunchKernelGGL(k_coldot_reduce, grid1(m), dim3(256), 0, ctx->stream, y + off, part_col, m, nch, 1);
            PYIPM_KCHECK();
        }
    }
    return 0;
}

// g = -grad into ctx->rhs.  With several ranks: the x rows this rank owns and (rank 0) the s / multiplier rows, zero
// elsewhere; the distributed driver sums it over the ranks.
int residual_dev(Ctx* ctx) {
    const Geo& g = ctx->g;
    if (!ctx->held.have_blocks || !ctx->held.have_vectors) { ctx->err = "residual: stage blocks and vectors first"; return PYIPM_E_BADARG; }
    const RowMap rm = make_rowmap(g, ctx->sharded);
    if (g.world > 1) { hipLaunchKernelGGL(k_fill, grid1(g.Npad), dim3(256), 0, ctx->stream, ctx->rhs, 0.0, g.Npad); PYIPM_KCHECK(); }
    if (rm.nloc > 0) {
        hipLaunchKernelGGL(k_rowdot2, grid1(rm.nloc, 4), dim3(256), 0, ctx->stream, ctx->rhs, ctx->df, rm.nloc,
                           ctx->Je, ctx->ld_Je, ctx->lda, g.me, ctx->Ji, ctx->ld_Ji, ctx->lda + g.me, g.mi, 0, 1, rm);
        PYIPM_KCHECK();
    }
    if (g.Npad > g.n && g.rank == 0) {
        hipLaunchKernelGGL(k_residual_tail, grid1(g.Npad - g.n), dim3(256), 0, ctx->stream, ctx->rhs, g, ctx->ce, ctx->ci,
                           ctx->s, ctx->lda, ctx->mu, ctx->eps);
        PYIPM_KCHECK();
    }
    ctx->held.residual_formed();
    return 0;
}

// Condensed assembly.  Split the inequalities by Sigma (k_active_scan), then
//   A (ld = gc.Npad) <- tril [[H + delta I, Jx], [Jx', D]]   by K1 on the condensed geometry, Jx = [Je | Ji_A],
//                        D = diag(-delta_c I, -1/Sigma_A);
//   += Ji_I Sigma_I Ji_I'   as ONE rank-mi launch of the MFMA update kernel (C += JT * WT').
void asm_grid(const Geo& g, dim3* grid, int* tri);
int assemble_condensed(Ctx* ctx, double delta, double delta_c) {
    const Geo& g = ctx->g;
    const int64_t nx = (g.n + BM - 1) / BM * BM;                 // rows / columns of the x-x block the Gram launch touches
    const int64_t mi_pad = (g.mi + BKU - 1) / BKU * BKU, ldt = nx;
    if (ctx->JT.reserve(2 * (size_t)ldt * (size_t)mi_pad) != hipSuccess) { ctx->err = "condensed: no memory for the Ji' operands"; return PYIPM_E_NOMEM; }
    if (!ctx->cond_pos) {
        if (ctx->cond_store.reserve((size_t)(2 * g.mi + 4)) != hipSuccess) { ctx->err = "condensed: no memory"; return PYIPM_E_NOMEM; }
        ctx->cond_pos = ctx->cond_store;
        ctx->cond_idx = ctx->cond_pos + g.mi;
        ctx->cond_cnt = ctx->cond_idx + g.mi;
    }
    // active rows: Sigma_k > cond_sigma_max  (one scalar comes back to size the system)
    hipLaunchKernelGGL(k_active_scan, dim3(1), dim3(1024), 0, ctx->stream, ctx->cond_pos, ctx->cond_idx, ctx->cond_cnt,
                       ctx->s, ctx->lda + g.me, ctx->eps, ctx->cond_sigma_max, g.mi);
    PYIPM_KCHECK();
    int na = 0;
    PYIPM_HIP(hipMemcpyAsync(&na, ctx->cond_cnt, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    PYIPM_HIP(hipStreamSynchronize(ctx->stream));
    ctx->cond_na = na;
    ctx->gc = make_geo(g.n, g.me + na, 0, g.nb, g.world, g.rank);     // (several ranks: the same 1-D block-cyclic map, fewer panels)
    const Geo& gc = ctx->gc;
    const int64_t mx = g.me + na;
    ctx->WT = ctx->JT + (size_t)ldt * (size_t)mi_pad;
    const double* Jx = ctx->Je; int64_t ldx = ctx->ld_Je;
    if (na > 0) {
        if (ctx->Jx.reserve((size_t)g.n * (size_t)(g.me + g.mi)) != hipSuccess) { ctx->err = "condensed: no memory for [Je | Ji_A]"; return PYIPM_E_NOMEM; }
        dim3 grid((unsigned)g.n, (unsigned)((mx + 255) / 256));
        hipLaunchKernelGGL(k_cond_gather_J, grid, dim3(256), 0, ctx->stream, ctx->Jx, mx, ctx->Je, ctx->ld_Je, g.me,
                           ctx->Ji, ctx->ld_Ji, ctx->cond_idx, (int64_t)na);
        PYIPM_KCHECK();
        Jx = ctx->Jx; ldx = mx;
    }
    {
        dim3 grid; int tri = 0;
        asm_grid(gc, &grid, &tri);
        PYIPM_HIP(hipMemsetAsync(ctx->anorm, 0, sizeof(unsigned long long), ctx->stream));
        hipLaunchKernelGGL(k_assemble, grid, dim3(256), 0, ctx->stream, ctx->A, gc.Npad, gc, ctx->d2L, ctx->ld_d2L,
                           Jx, ldx, (const double*)nullptr, (int64_t)0, ctx->s, ctx->lda, ctx->eps, delta, delta_c, ctx->anorm, 0, 0, 0, (int64_t)0, tri, (int64_t)0, gc.Npad);
        PYIPM_KCHECK();
        if (na > 0) {
            hipLaunchKernelGGL(k_cond_fix_diag, grid1(na), dim3(256), 0, ctx->stream, ctx->A, gc.Npad, g.n + g.me,
                               ctx->cond_idx, (int64_t)na, ctx->s, ctx->lda + g.me, ctx->eps, gc);
            PYIPM_KCHECK();
        }
    }
    {
        dim3 grid((unsigned)((ldt + 31) / 32), (unsigned)((mi_pad + 31) / 32));
        hipLaunchKernelGGL(k_transpose_scale, grid, dim3(256), 0, ctx->stream, ctx->JT, ctx->WT, ldt, ctx->Ji, ctx->ld_Ji,
                           g.n, g.mi, mi_pad, ctx->s, ctx->lda + g.me, ctx->eps, ctx->cond_pos);
        PYIPM_KCHECK();
    }
    if (ctx->profile) PYIPM_HIP(hipEventRecord(ctx->ev[6], ctx->stream));
    {
        GeoSwap sw(ctx, gc);
        // Gram update of the x-x block: the panels below column nx, of which a rank holds every world-th (its local panels
        // 0 .. ceil(#panels / world) - 1; a local panel past the block is cut off by col_end)
        const int64_t npx = (nx + gc.nb - 1) / gc.nb;
        int rc = launch_update128(ctx, ctx->stream, ctx->JT, ldt, ctx->WT, (int)mi_pad, 0, 0, (npx + gc.world - 1) / gc.world,
                                  {.ldw = ldt, .row_end = nx, .col_end = nx});
        if (rc) return rc;
    }
    if (ctx->profile) PYIPM_HIP(hipEventRecord(ctx->ev[7], ctx->stream));
    return 0;
}

// Grid of a whole-matrix k_assemble launch.  Single rank, Npad a multiple of 512: a 1-D grid over the 512 x 16 patches on or
// below the diagonal only (round 4: the 2-D grid started as many workgroups above the diagonal that returned at once --
// 65000 of them at N = 32768 cost 0.5 of K1's 1.5 ms; with them gone K1 moves its algorithmic bytes at 6.5 TB/s).
void asm_grid(const Geo& g, dim3* grid, int* tri) {
    *grid = dim3((unsigned)((g.Npad + 511) / 512), (unsigned)((g.ncols_local + 15) / 16));
    *tri = 0;
    if (g.world == 1 && g.Npad % 512 == 0) {
        const int64_t nbx = g.Npad / 512, ngrp = (g.ncols_local / 16 + 31) / 32;          // column patches in groups of 32
        int64_t tot = 0;
        for (int64_t G = 0; G < ngrp; ++G) tot += 32 * (nbx - G);
        if (ngrp <= nbx && tot < (int64_t)1 << 31) { *grid = dim3((unsigned)tot, 1); *tri = (int)nbx; }
    }
}

int assemble_dev(Ctx* ctx, double delta, double delta_c) {
    const Geo& g = ctx->g;
    if (ctx->provider_only) { ctx->err = "a provider-only handle has no KKT storage: block products and residuals only"; return PYIPM_E_BADARG; }
    if (!ctx->held.have_blocks || !ctx->held.have_vectors) { ctx->err = "assemble: stage blocks and vectors first"; return PYIPM_E_BADARG; }
    if (delta != ctx->delta || delta_c != ctx->delta_c) ctx->held.rc_warm_cold();      // a shifted matrix
    ctx->delta = delta; ctx->delta_c = delta_c;
    if (ctx->condensed && g.mi > 0 && g.world > 1 && ctx->sharded) {
        ctx->err = "condensed option across ranks needs the full blocks on every rank (stage_blocks, not stage_blocks_owned): "
                   "a column of Ji Sigma Ji' takes every row of Ji";
        return PYIPM_E_BADARG;
    }
    const bool condensed = ctx->condensed && g.mi > 0;
    ctx->held.assemble_begun(condensed);
    if (condensed) {
        int rc = assemble_condensed(ctx, delta, delta_c); if (rc) return rc;
        ctx->held.assemble_done(true, g.world == 1);
        return 0;
    }
    PYIPM_HIP(hipMemsetAsync(ctx->anorm, 0, sizeof(unsigned long long), ctx->stream));
    if (g.ncols_local > 0) {
        const int zip = (ctx->keep_zeros && !ctx->held.storage_exported && ctx->held.zeros_clean && g.world == 1 && g.mi > 0) ? 1 : 0;
        dim3 grid; int tri = 0;
        asm_grid(g, &grid, &tri);
        hipLaunchKernelGGL(k_assemble, grid, dim3(256), 0, ctx->stream, ctx->A, g.Npad, g, ctx->d2L, ctx->ld_d2L,
                           ctx->Je, ctx->ld_Je, ctx->Ji, ctx->ld_Ji, ctx->s, ctx->lda, ctx->eps, delta, delta_c, ctx->anorm, 0, ctx->sharded,
                           zip, (int64_t)0, tri, (int64_t)0, g.Npad);
        PYIPM_KCHECK();
    }
    ctx->held.assemble_done(false, g.world == 1);
    return 0;
}

// ---- single-rank factorisation: the plan (step_plan.hpp: plan_groups, make_step_plan; plan_step), then the enqueue (factor_all) ---
#include "reuse_impl.hpp"

// diagnostics (PYIPM_GROUP_TRACE=1): where each group's chain, head and bulk update begin and end on the device, without a
// tracer's per-call cost on the host (tools/group_trace.py)
struct GroupTrace {
    std::vector<std::pair<std::string, Event>> marks;
    static bool on() { static const bool v = getenv("PYIPM_GROUP_TRACE") != nullptr; return v; }
    void mark(const char* what, int64_t grp, hipStream_t st) {
        Event e; if (!on() || e.ensure(hipEventDefault) != hipSuccess) return;
        hipEventRecord(e, st);
        char buf[64]; snprintf(buf, sizeof(buf), "%s g%lld", what, (long long)grp);
        marks.emplace_back(buf, std::move(e));
    }
    void report(hipEvent_t t0, hipEvent_t t1, float total_ms) {
        if (!on()) return;
        hipEventSynchronize(t1);
        for (auto& m : marks) {
            float t = 0.f;
            if (hipEventSynchronize(m.second) == hipSuccess && hipEventElapsedTime(&t, t0, m.second) == hipSuccess)
                fprintf(stderr, "[pyipm group trace] %9.1f us  %s\n", 1e3 * t, m.first.c_str());
        }
        fprintf(stderr, "[pyipm group trace] %9.1f us  factorisation end\n", 1e3 * total_ms);
    }
};

// does group grp run as a tile chain (factor_group)?
static bool chain_group(const Ctx* ctx, int64_t grp) { return pyipm::chain_group(ctx->g, ctx->sched, ctx->group_chain != 0, grp); }

struct FactorRun {                     // one whole factorisation: its plan, and what the plan does not hold
    const StepPlan plan;
    unsigned fr_blocks = 0;            // workgroups of the range launch over the plan's [frA, frB) (fwd_range_grid); 0: the fallback owners
    GroupTrace tr;
    bool across_prev = false;          // the lookahead loop: the iteration before this one looked across the slack block
    bool done_early(const Ctx* ctx, int64_t q) const { return plan.slack_first && ctx->sched.fast_panel(q); }   // panel q was enqueued up front
};
// the forward substitution of the panels [q0, q1), whose L is complete on the forward stream, there
static int fwd_panels(Ctx* ctx, int64_t q0, int64_t q1) {
    int rc = 0;
    for (int64_t q = q0; q < q1 && !rc; ++q) { rc = fwd_panel(ctx, q, ctx->fwd_vec, ctx->fwd); if (!rc) rc = diag_panel(ctx, q, ctx->fwd_vec, ctx->fwd); }
    return rc;
}

// Panel q of group grp is complete once `used` reaches this point.  The fused forward substitution takes it up.
// Group 0 right-looking panel by panel (early0): where the x block is ONE group followed by the slack block
// every panel of group 0 goes to the columns beyond the group as soon as it is complete -- a K = nb launch on the side stream
// behind the panel's event, under the chain of the panels that follow; neither a head nor a bulk update is left for group 0.
// Every entry receives the same products in the same order.  Measured (tools/r06_early.sh): config 2 2.225 -> 2.165 ms; where
// the next group is an ordinary one the lookahead already hides the bulk update and the pieces lose: not applied there.
static int panel_done(Ctx* ctx, const FactorRun& run, int64_t grp, int64_t q, hipStream_t used) {
    if (run.plan.fuse_forward && run.plan.fwd_owner(q, run.fr_blocks != 0) == FwdOwner::PanelDone) {
        const bool early = run.done_early(ctx, q);                     // its kernel ran up front: complete at ev_sfast, or (per-panel
        if (!early) PYIPM_HIP(hipEventRecord(ctx->ev_done[q], used));  // launches) at the record behind its own kernel
        PYIPM_HIP(hipStreamWaitEvent(ctx->fwd, early && ctx->slack_one ? ctx->ev_sfast : ctx->ev_done[q], 0));
        const int r2 = fwd_panels(ctx, q, q + 1); if (r2) return r2;
    }
    if (!(run.plan.early0 && grp == 0)) return 0;
    const int64_t p1 = ctx->sched.first(1);
    PYIPM_HIP(hipEventRecord(ctx->ev_early, used));
    PYIPM_HIP(hipStreamWaitEvent(ctx->side, ctx->ev_early, 0));
    return timed_update(ctx, q, 1, p1, ctx->g.npanels - p1, {.stream = ctx->side, .as_bulk = true});
}

// all panels of one group on stream S
static int run_group(Ctx* ctx, const FactorRun& run, int64_t grp, hipStream_t S, const TailHand& hand = {}) {
    const int64_t pA = ctx->sched.first(grp), nA = ctx->sched.size(grp);
    auto done = [&](int64_t q, hipStream_t used) { return panel_done(ctx, run, grp, q, used); };
    if (chain_group(ctx, grp)) return factor_group(ctx, pA, nA, S, done, hand);
    for (int64_t q = pA; q < pA + nA; ++q) {
        if (!run.done_early(ctx, q)) { int r2 = factor_panel(ctx, q, S, true); if (r2) return r2; }
        int r2 = done(q, S); if (r2) return r2;
    }
    return 0;
}

// (round 5) The closed-form panels of the slack block depend on nothing but the assembly: they are enqueued
// up front on the rows stream; what READS them (k_s_schur on the update stream, the forward sweep) keeps its place and waits
// for one event.  Statistics are atomic sums / minima / maxima: the same numbers.
static int enqueue_slack_first(Ctx* ctx, const FactorRun& run, hipStream_t after) {
    { int r0 = ensure_rest_stream(ctx); if (r0) return r0; }
    PYIPM_HIP(hipEventRecord(ctx->ev_sfast, after));                  // the assembly and the reset of the statistics
    PYIPM_HIP(hipStreamWaitEvent(ctx->rest, ctx->ev_sfast, 0));
    const Geo& g = ctx->g;
    for (int64_t q = 0; q < g.npanels; ++q) {
        if (!ctx->sched.fast_panel(q)) continue;
        if (!ctx->slack_one) {                                        // (PYIPM_SLACK_ONE=0) a launch and an event per panel
            int r2 = factor_panel(ctx, q, ctx->rest, true); if (r2) return r2;
            if (run.plan.fuse_forward) PYIPM_HIP(hipEventRecord(ctx->ev_done[q], ctx->rest));
            continue;
        }
        // One launch per contiguous run of them (k_s_panels: a workgroup per panel, each what factor_panel's k_s_panel launch
        // does): 24 launches with a record behind each were 0.43 ms in front of a reusing step's first chain at N = 32768.
        // Their forward substitution waits for ev_sfast (panel_done).
        int64_t q1 = q + 1;
        while (q1 < g.npanels && ctx->sched.fast_panel(q1)) ++q1;
        hipLaunchKernelGGL(k_s_panels, dim3((unsigned)(q1 - q)), dim3(256), 0, ctx->rest, ctx->A, g.Npad, q, g.nb, ctx->Dinv, ctx->Tsv,
                           ctx->Tflag, ctx->refine_cond, ctx->block_refine, ctx->dstats, g.n, g.n + g.mi + g.me, ctx->pivtol_rel,
                           ctx->anorm);
        PYIPM_KCHECK();
        q = q1 - 1;
    }
    PYIPM_HIP(hipEventRecord(ctx->ev_sfast, ctx->rest));              // every closed-form panel is done
    return 0;
}

// Head on hs: panels [q0, q0 + nq) of a complete group applied to the columns of panels [tp, tp + tn) (the target's chain waits for it)
static int head_from(Ctx* ctx, bool fast_src, int64_t q0, int64_t nq, int64_t tp, int64_t tn, hipStream_t hs, bool split) {
    const Geo& g = ctx->g;
    const int64_t tc0 = g.panel_c0(tp);
    if (fast_src || g.Npad - tc0 > HEAD32_ROWS) return timed_update(ctx, q0, nq, tp, tn, {.stream = hs});   // (else, where the chain is the bound: 32 x 64 blocks)
    int K = 0; int64_t cols = 0;
    for (int64_t q = q0; q < q0 + nq; ++q) K += (int)g.panel_w(q);
    for (int64_t q = tp; q < tp + tn; ++q) cols += g.panel_w(q);
    const int64_t tend = tc0 + cols;
    int64_t pa0, pa1, pb0, pb1;
    active_ranges(ctx, g.panel_c0(q0), g.panel_c0(q0) + K, &pa0, &pa1, &pb0, &pb1);
    // split: the chain of the target group needs the head only inside that group's diagonal block (rows [tc0, tend));
    // the rows below it are first read by the group's rows stream.  Two launches: the block on the chain's
    // stream, the rest on ctx->rest behind it -- the same entries, the same operations.
    const bool below = split && tend < g.Npad;
    if (below) {
        int r2 = ensure_rest_stream(ctx); if (r2) return r2;
        PYIPM_HIP(hipEventRecord(ctx->ev_split, hs));          // the source group is complete, the main stream's
        PYIPM_HIP(hipStreamWaitEvent(ctx->rest, ctx->ev_split, 0));   // earlier updates of these columns are ordered
    }
    // W of a panel inside its group's buffer: wbuf(q0) addresses it (column offset of q0 in the group)
    const int64_t rows = split ? cols : g.Npad - tc0;
    hipLaunchKernelGGL(k_inpanel_update, dim3((unsigned)(rows / 32), (unsigned)(cols / TB)), dim3(256), 0,
                       hs, ctx->A, g.Npad, g.local_c0(tp), ctx->A + g.local_c0(q0) * g.Npad, g.Npad,
                       wbuf(ctx, q0), g.Npad, tc0, K, tc0, g.Npad, pa0, pa1, pb0, pb1, SIDE_PRIO);
    PYIPM_KCHECK();
    if (below && g.Npad - tend <= HEAD32_ROWS) {
        hipLaunchKernelGGL(k_inpanel_update, dim3((unsigned)((g.Npad - tend) / 32), (unsigned)(cols / TB)), dim3(256), 0,
                           ctx->rest, ctx->A, g.Npad, g.local_c0(tp), ctx->A + g.local_c0(q0) * g.Npad, g.Npad,
                           wbuf(ctx, q0), g.Npad, tc0, K, tend, g.Npad, pa0, pa1, pb0, pb1, SIDE_PRIO);
        PYIPM_KCHECK();
    } else if (below) {
        return launch_update128(ctx, ctx->rest, ctx->A + g.local_c0(q0) * g.Npad, g.Npad, wbuf(ctx, q0), K, tend, tp, tn,
                                {.src_c0 = g.panel_c0(q0), .waves = HEAD_WAVES});
    }
    return 0;
}

// The tail split's head (StepPlan::tail_split): the complete group of panels [q0, q0 + nq) applied to the columns
// of panels [tp, tp + tn) in two k_update launches of the same K.  The target's diagonal block on ds, the next chain's stream, behind
// the source's chain launch; the rows behind it on the main stream in front of the bulk update, behind the source's rows kernels
// (ev_rows).  release: the flag word takes the next token behind the second launch -- the next chain's extra rows wait for it.
// ev_head2: the second launch is through (the target's rows kernels wait for it).  Every entry is written by one launch.
__global__ __launch_bounds__(64) void k_tail_mark(unsigned* p, unsigned v) { if (threadIdx.x == 0) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
static int head_split(Ctx* ctx, GroupTrace& tr, int64_t grp, int64_t q0, int64_t nq, int64_t tp, int64_t tn, hipStream_t ds, int64_t xnext) {
    const Geo& g = ctx->g; const bool release = xnext > 0;
    int K = 0; int64_t cols = 0;
    for (int64_t q = q0; q < q0 + nq; ++q) K += (int)g.panel_w(q);
    for (int64_t q = tp; q < tp + tn; ++q) cols += g.panel_w(q);
    const int64_t tc0 = g.panel_c0(tp), tend = tc0 + cols, src = g.panel_c0(q0);
    const double* Lop = ctx->A + g.local_c0(q0) * g.Npad;
    // (36 tiles of 128 x 128 at the default sizes.  With the default options -- reserve_cus > 0, so no 128 x 256 tiles over so
    //  few rows -- launch_update128 halves such a narrow launch into 128 x 64 tiles, k_update<64, true, 8>: the instance the
    //  kernel statistics show and the one measured; as 128 x 128 tiles on four waves the step took 5.67 against 5.48 ms.  Any
    //  instance gives the same bits.)
    int rc = launch_update128(ctx, ds, Lop, g.Npad, wbuf(ctx, q0), K, tc0, tp, tn, {.row_end = tend, .src_c0 = src, .prio = SIDE_PRIO}); if (rc) return rc;
    tr.mark("diag head end", grp, ds);
    PYIPM_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_rows, 0));
    // (the rows the next chain takes along first, in a launch of their own: the word behind it releases them while the rest runs)
    const int64_t xend = release ? tend + xnext : tend;
    if (xend > tend) { rc = launch_update128(ctx, ctx->stream, Lop, g.Npad, wbuf(ctx, q0), K, tend, tp, tn, {.row_end = xend, .src_c0 = src}); if (rc) return rc; }
    if (release) { hipLaunchKernelGGL(k_tail_mark, dim3(1), dim3(64), 0, ctx->stream, ctx->tail_flag.get(), ++ctx->tail_token); PYIPM_KCHECK(); }
    if (xend < g.Npad) { rc = launch_update128(ctx, ctx->stream, Lop, g.Npad, wbuf(ctx, q0), K, xend, tp, tn, {.src_c0 = src}); if (rc) return rc; }
    PYIPM_HIP(hipEventRecord(ctx->ev_head2, ctx->stream));
    tr.mark("rest of head end", grp, ctx->stream);
    return 0;
}

// One iteration of the lookahead loop, decided (group grp is complete, group grp + 1 runs next)
struct GroupStep {
    bool fast_src, nxt_fast;      // group grp / group grp + 1 lies inside the slack block
    bool across; int64_t pT, nT;  // the lookahead target and its panels: group grp + 1, or (across) group grp + 2 BEHIND the slack group
    bool pieces, head, split;     // (early0) grp's contribution is applied already, panel by panel: no head, no bulk; a head is launched; in two launches
    hipStream_t cs, hs;           // where group grp + 1 runs; where the head runs
};
static GroupStep plan_step(const Ctx* ctx, const FactorRun& run, int64_t grp) {
    const GroupSched& sc = ctx->sched;
    GroupStep st; st.fast_src = sc.fast(grp); st.nxt_fast = sc.fast(grp + 1);
    // Streams.  The next group runs on cs: the side stream, except a group inside the slack block -- a handful of
    // microsecond launches (closed form) that stay on the main stream, head included (sending them through the side
    // stream cost two stream crossings per group, 50-240 us each time for 30 us of work; config 2: 0.6 of 3.6 ms).
    st.cs = st.nxt_fast ? ctx->stream : ctx->side;
    // (round 5) Lookahead ACROSS the slack block, whose panels ran up front: the group after the slack group is
    // the lookahead target -- a split head applies this group's contribution to its columns, the bulk update starts beyond them
    // (its chain used to wait for the whole bulk launch: 1.6 + 0.3 ms at N = 32768).  The same products in the same order per entry.
    st.across = run.plan.slack_first && st.nxt_fast && !st.fast_src && grp > 0 && grp + 2 < sc.ngroups() &&
                !sc.fast(grp + 2) && chain_group(ctx, grp + 2);
    st.pT = sc.first(grp + (st.across ? 2 : 1)); st.nT = sc.size(grp + (st.across ? 2 : 1));
    // The head runs on hs: the stream of the chain it follows, i.e. the side stream for every group but the first, so that
    // chain -> head -> next chain never cross streams.  There it waits for ev_main: the bulk update of the group before touched
    // its columns on the main stream.  (The FIRST head stays on the main stream: nothing runs beside it either way, and as a
    // main-stream launch it takes the bulk instance and is part of the trailing figures, as in rounds 1-3.)
    st.hs = (grp > 0 && (st.cs == ctx->side || st.across)) ? ctx->side : ctx->stream;
    st.pieces = run.plan.early0 && grp == 0;
    // (a head INTO the slack block is structurally empty: no x column reaches an s column, and a slack column's only
    //  update is a diagonal entry of the multiplier block -- no launch, 10-15 us of the chain's path each)
    st.head = !st.pieces && (st.across || !st.nxt_fast);
    st.split = st.across || (chain_group(ctx, grp + 1) && st.cs != ctx->stream);
    return st;
}

// ---- the phases of the enqueue: each carries out its part of the plan (run.plan) and is empty where the plan has none -------------
// begin: streams and events, the forward stream behind the right-hand side's copy, the statistics reset or (reusing) seeded
static int enqueue_begin(Ctx* ctx, FactorRun& run) {
    const StepPlan& plan = run.plan;
    if (!ctx->side) {
        // panel kernels are latency-critical and tiny: highest dispatch priority, so they take the first
        // CU slot a retiring bulk-update block frees instead of queueing behind the whole bulk grid
        for (Event* e : {&ctx->ev_main, &ctx->ev_early, &ctx->ev_split, &ctx->ev_sfast, &ctx->ev_rows, &ctx->ev_head2, &ctx->ev_chain_end})      // the events of the schedule below
            PYIPM_HIP(e->ensure(hipEventDisableTiming));
        PYIPM_HIP(ctx->side.ensure_highest(hipStreamNonBlocking));
    }
    PYIPM_HIP(hipEventRecord(ctx->ev[0], ctx->stream));
    ctx->held.factor_begun();
    if (plan.fuse_forward) {
        PYIPM_HIP(ctx->fwd.ensure(hipStreamNonBlocking));
        PYIPM_HIP(ensure_events(ctx->ev_done, (size_t)ctx->g.npanels, hipEventDisableTiming));
        PYIPM_HIP(hipEventRecord(ctx->ev_head, ctx->stream));          // v0 = rhs copy was enqueued on the main stream
        PYIPM_HIP(hipStreamWaitEvent(ctx->fwd, ctx->ev_head, 0));
    }
    if (plan.kind != PX_REUSE) return factor_begin(ctx);
    const SnapHeaders hdr = snap_headers(ctx);                          // the statistics as the prefix left them, not zero
    PYIPM_HIP(hipMemcpyAsync(ctx->dstats, hdr.at_boundary, sizeof(DevStats), hipMemcpyDeviceToDevice, ctx->stream));
    if (plan.e.ok) { hipLaunchKernelGGL(k_merge_stats, dim3(1), dim3(64), 0, ctx->stream, ctx->dstats, (const DevStats*)hdr.of_lam_e); PYIPM_KCHECK(); }
    ctx->n_trailing = 0; ctx->trailing_flops = 0.0; ctx->trailing_area = 0.0;
    return 0;
}
// the new right-hand side through the prefix panels (reusing, fused) in one launch (k_fwd_prefix) or panel by panel; the range
// launch follows at once where it takes the slack panels (complete at ev_sfast) with the kept lambda_e groups
static int enqueue_fwd_kept(Ctx* ctx, FactorRun& run) {
    const StepPlan& plan = run.plan;
    if (plan.kind != PX_REUSE || !plan.fuse_forward) return 0;
    int rc = plan.fwd_prefix_launch ? fwd_prefix(ctx, plan.pB, ctx->fwd_vec, ctx->fwd) : fwd_panels(ctx, 0, plan.pB); if (rc) return rc;
    run.tr.mark("fwd prefix end (before group)", plan.gB, ctx->fwd);
    if (!(run.fr_blocks && plan.fr_slack)) return 0;
    PYIPM_HIP(hipStreamWaitEvent(ctx->fwd, ctx->ev_sfast, 0));
    rc = fwd_range(ctx, plan.frA, plan.frB, run.fr_blocks, ctx->fwd_vec, ctx->fwd); if (rc) return rc;
    run.tr.mark("fwd kept range end", plan.gB, ctx->fwd);
    return 0;
}
// The groups between the prefix and the kept lambda_e groups (the slack group, a group that straddles a border) on the main stream.
// What they reach behind themselves that this step still needs: the columns in front of cS and the diagonal blocks behind cE.
static int enqueue_between(Ctx* ctx, FactorRun& run) {
    const StepPlan& plan = run.plan; const GroupSched& sc = ctx->sched;
    if (plan.kind != PX_REUSE || !plan.e.ok) return 0;
    for (int64_t grp = plan.gB; grp < plan.e.gS; ++grp) {
        const int64_t p0 = sc.first(grp), n0 = sc.size(grp);
        if (plan.slack_first && sc.fast(grp)) PYIPM_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_sfast, 0));
        run.tr.mark("chain+rows begin", grp, ctx->stream);
        int rc = run_group(ctx, run, grp, ctx->stream); if (rc) return rc;
        run.tr.mark("chain+rows end", grp, ctx->stream);
        if (sc.fast(grp)) { rc = timed_update(ctx, p0, n0, p0 + n0, ctx->g.npanels - (p0 + n0)); if (rc) return rc; continue; }   // (k_s_schur: diagonal entries)
        for (int64_t t = grp + 1; t < plan.e.gS; ++t)
            if (!sc.fast(t)) { rc = timed_update(ctx, p0, n0, sc.first(t), sc.size(t)); if (rc) return rc; }
        rc = diag_update_group(ctx, grp, wbuf(ctx, p0), 0, ctx->g.Npad, plan.e.cE); if (rc) return rc;
    }
    return 0;
}
// ... the kept groups: their forward substitution waits for nothing, their products go to the diagonal blocks
static int enqueue_kept_diag(Ctx* ctx, FactorRun& run) {
    const StepPlan& plan = run.plan; const LamE& le = plan.e;
    if (plan.kind != PX_REUSE || !le.ok) return 0;
    run.tr.mark("diagonal blocks begin", le.gS, ctx->stream);
    if (run.fr_blocks && !plan.fr_slack) {
        const int rc = fwd_range(ctx, plan.frA, plan.frB, run.fr_blocks, ctx->fwd_vec, ctx->fwd); if (rc) return rc;
        run.tr.mark("fwd kept range end", le.gS, ctx->fwd);
    }
    for (int64_t grp = le.gS; grp < le.gE; ++grp) {
        const int64_t p0 = ctx->sched.first(grp);
        const bool mine = plan.fuse_forward && plan.fwd_owner(p0, run.fr_blocks != 0) == FwdOwner::Kept;
        int rc = mine ? fwd_panels(ctx, p0, ctx->sched.first(grp + 1)) : 0; if (rc) return rc;
        rc = diag_update_group(ctx, grp, lam_e_w(ctx, le, ctx->g.panel_c0(p0)), le.cE, ctx->g.Npad - le.cE, le.cE); if (rc) return rc;
    }
    run.tr.mark("diagonal blocks end", le.gE, ctx->stream);
    return 0;
}
// A recording step, group grp complete on the main stream.  A lambda_e group: its W in the rows behind cE goes to the second
// snapshot before the buffer is recycled.  which = 1, the last group of the prefix, or 2, the last lambda_e group: no lookahead
// -- one update of everything behind the group, the snapshot, then the next group, all on the main stream.  0: no boundary.
static int record_behind(Ctx* ctx, FactorRun& run, int64_t grp, int which) {
    const Geo& g = ctx->g; const StepPlan& plan = run.plan; const LamE& le = plan.e;
    const int64_t p0 = ctx->sched.first(grp), n0 = ctx->sched.size(grp); int rc = 0;
    if (plan.kind == PX_RECORD && le.ok && grp >= le.gS && grp < le.gE) {
        const int64_t c0 = g.panel_c0(p0), rows = g.Npad - le.cE;
        rc = copy_cols(ctx, lam_e_w(ctx, le, c0), rows, wbuf(ctx, p0) + le.cE, g.Npad, rows, g.panel_c0(p0 + n0) - c0); if (rc) return rc;
    }
    if (!which) return 0;
    run.tr.mark("bulk begin", grp, ctx->stream);
    rc = timed_update(ctx, p0, n0, p0 + n0, g.npanels - (p0 + n0)); if (rc) return rc;
    run.tr.mark("bulk end", grp, ctx->stream);
    if (which == 2) {
        const SnapHeaders hdr = snap_headers(ctx);
        PYIPM_HIP(hipMemcpyAsync(hdr.of_lam_e, ctx->dstats, sizeof(DevStats), hipMemcpyDeviceToDevice, ctx->stream));
        hipLaunchKernelGGL(k_merge_stats, dim3(1), dim3(64), 0, ctx->stream, ctx->dstats, (const DevStats*)hdr.before_lam_e); PYIPM_KCHECK();
        rc = copy_square(ctx, lam_e_square(ctx, le), le.cE, true); if (rc) return rc;
    } else {
        rc = prefix_copy(ctx, plan, true); if (rc) return rc;
    }
    run.tr.mark(which == 2 ? "second snapshot end" : "snapshot end", grp, ctx->stream);
    rc = run_group(ctx, run, grp + 1, ctx->stream); if (rc) return rc;
    PYIPM_HIP(hipEventRecord(ctx->ev_main, ctx->stream));
    run.across_prev = false; return 0;
}
// The lookahead loop: group g0 on the main stream; then per group grp, as plan_step decided: head (grp -> the lookahead target) on
// hs, group grp + 1 on cs, bulk update (grp -> everything behind the target) on the main stream beside it.  lookahead = 0: all on it.
static int enqueue_groups(Ctx* ctx, FactorRun& run) {
    const StepPlan& plan = run.plan; const GroupSched& sc = ctx->sched; GroupTrace& tr = run.tr;
    const int64_t np = ctx->g.npanels, ngroups = sc.ngroups(), g0 = plan.g0; const bool reuse = plan.kind == PX_REUSE;
    if (reuse && plan.slack_first && sc.fast(g0)) PYIPM_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_sfast, 0));   // (as in front of any slack group)
    // The tail split, as the plan states it per hand-over.  What group h's block takes along and waits for:
    // gated -- the head into h's columns is split too, its second launch releases the extra rows through the flag word.
    auto hand_of = [&](int64_t h, bool gated) {
        TailHand th;
        if (plan.split(h)) { th.xrows = group_cols(ctx->g, sc, h + 1); if (gated) { th.xword = ctx->tail_flag.get(); th.xwant = ctx->tail_token; } }
        if (gated) th.rows_behind = ctx->ev_head2;
        return th;
    };
    tr.mark("chain+rows begin", g0, ctx->stream);
    int rc = run_group(ctx, run, g0, ctx->stream, hand_of(g0, false)); if (rc) return rc;     // (what its extra rows read is ordered on the main stream)
    tr.mark("chain+rows end", g0, ctx->stream);
    if (reuse) PYIPM_HIP(hipEventRecord(ctx->ev_main, ctx->stream));       // group g0 ran on the main stream: its head on the side stream waits for this
    if (tr.on()) fprintf(stderr, "[pyipm group trace] %lld groups\n", (long long)ngroups);
    for (int64_t grp = g0; grp + 1 < ngroups; ++grp) {
        const int64_t p0 = sc.first(grp), n0 = sc.size(grp);            // the source: its contribution goes to everything behind it
        const int snapshot = plan.snapshot_behind(grp);
        rc = record_behind(ctx, run, grp, snapshot); if (rc) return rc;
        if (snapshot) continue;
        if (!ctx->lookahead) {
            rc = timed_update(ctx, p0, n0, p0 + n0, np - (p0 + n0)); if (rc) return rc;
            rc = run_group(ctx, run, grp + 1, ctx->stream); if (rc) return rc;
            continue;
        }
        const GroupStep st = plan_step(ctx, run, grp);
        if (st.hs == ctx->side) {
            // (recorded at the end of the iteration before.  Behind an `across` iteration the source is the slack group: its
            //  head is the diagonal update of the target's columns, ordered behind the x group's head on this stream, and the
            //  x group's bulk update -- what the event would wait for -- no longer touches those columns)
            if (!run.across_prev) PYIPM_HIP(hipStreamWaitEvent(ctx->side, ctx->ev_main, 0));
            if (plan.slack_first && st.fast_src) PYIPM_HIP(hipStreamWaitEvent(ctx->side, ctx->ev_sfast, 0));   // (k_s_schur reads the slack columns)
        }
        if (st.pieces) {
            PYIPM_HIP(hipEventRecord(ctx->ev_early, ctx->side));          // the last piece
            PYIPM_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_early, 0)); // (later updates of those columns; cs, if it is the main stream)
            if (ctx->rest) PYIPM_HIP(hipStreamWaitEvent(ctx->rest, ctx->ev_early, 0));
        } else if (plan.split(grp)) {
            tr.mark("head begin", grp, st.cs);
            rc = head_split(ctx, tr, grp, p0, n0, st.pT, st.nT, st.cs, plan.split(grp + 1) ? group_cols(ctx->g, sc, grp + 2) : 0); if (rc) return rc;
        } else {
            tr.mark("head begin", grp, st.hs);
            if (st.head) { rc = head_from(ctx, st.fast_src, p0, n0, st.pT, st.nT, st.hs, st.split); if (rc) return rc; }
            tr.mark("head end (its first launch's stream)", grp, st.hs);
            if (plan.split(grp + 1)) {        // the next chain's extra rows read the whole head: its second launch ran on ctx->rest
                PYIPM_HIP(hipEventRecord(ctx->ev_head2, ctx->rest));
                PYIPM_HIP(hipStreamWaitEvent(st.cs, ctx->ev_head2, 0));
            }
        }
        if (st.hs == ctx->stream && st.cs == ctx->side) {
            PYIPM_HIP(hipEventRecord(ctx->ev_head, ctx->stream));
            PYIPM_HIP(hipStreamWaitEvent(ctx->side, ctx->ev_head, 0));
        }
        tr.mark("chain+rows begin", grp + 1, st.cs);
        if (plan.slack_first && st.nxt_fast)                             // its kernels ran up front: whoever follows on cs (= the main
            PYIPM_HIP(hipStreamWaitEvent(st.cs, ctx->ev_sfast, 0));      // stream: k_s_schur too) is ordered behind them
        if (plan.kind == PX_RECORD && plan.e.ok && grp + 1 == plan.e.gS) {   // stats_aside: the record so far is set aside and reset in
            PYIPM_HIP(hipMemcpyAsync(snap_headers(ctx).before_lam_e, ctx->dstats, sizeof(DevStats), hipMemcpyDeviceToDevice, st.cs));   // front of
            hipLaunchKernelGGL(k_init_stats, dim3(1), dim3(64), 0, st.cs, ctx->dstats); PYIPM_KCHECK();   // group gS, merged back behind gE - 1
        }
        rc = run_group(ctx, run, grp + 1, st.cs, hand_of(grp + 1, plan.split(grp))); if (rc) return rc;
        tr.mark("chain+rows end", grp + 1, st.cs);
        PYIPM_HIP(hipEventRecord(ctx->ev_panel, st.cs));
        tr.mark("bulk begin", grp, ctx->stream);
        // bulk (overlaps the side stream): everything behind the target, whose columns the head above took
        // (the tail split: the next head's columns -- group grp + 2's -- in a launch of their own, so that the head waits for them alone;
        //  each entry still takes this group's products from one launch, behind the groups before it)
        const int64_t nA = plan.split(grp) && grp + 2 < ngroups ? sc.size(grp + 2) : 0;
        if (nA > 0) {
            rc = timed_update(ctx, p0, n0, st.pT + st.nT, nA); if (rc) return rc;
            PYIPM_HIP(hipEventRecord(ctx->ev_main, ctx->stream));
            tr.mark("bulk, next head's columns end", grp, ctx->stream);
        }
        if (!st.pieces) { rc = timed_update(ctx, p0, n0, st.pT + st.nT + nA, np - (st.pT + st.nT + nA)); if (rc) return rc; }
        tr.mark("bulk end", grp, ctx->stream);
        // what the next head must not overtake on the main stream: this group's bulk update -- recorded
        // BEFORE the main stream starts waiting for the side stream (the head would otherwise wait for its own stream,
        // two stream crossings for nothing)
        if (nA == 0) PYIPM_HIP(hipEventRecord(ctx->ev_main, ctx->stream));
        PYIPM_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_panel, 0));
        run.across_prev = st.across;
    }
    return 0;
}
// join: the main stream continues after the forward pass; the statistics come back, the timings are taken
static int enqueue_end(Ctx* ctx, FactorRun& run, pyipm_factor_stats* stats, std::chrono::steady_clock::time_point t_host0) {
    if (run.plan.fuse_forward) {
        run.tr.mark("fwd stream end (before group)", ctx->sched.ngroups(), ctx->fwd);
        PYIPM_HIP(hipEventRecord(ctx->ev_fwd, ctx->fwd));
        PYIPM_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_fwd, 0));
        ctx->held.forward_fused_under_factor();
    }
    PYIPM_HIP(hipEventRecord(ctx->ev[1], ctx->stream));
    ctx->held.factor_enqueued();
    if (getenv("PYIPM_SETUP_TRACE")) {
        const double host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_host0).count();
        fprintf(stderr, "[pyipm] factor_all: host enqueue %.2f ms (tile lists built so far: %d in %.2f ms)\n", host_ms,
                ctx->setup_lists_n, ctx->setup_lists_ms);
    }
    const int rc = factor_end(ctx, stats);
    float ms = 0.f;
    PYIPM_HIP(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
    run.tr.report(ctx->ev[0], ctx->ev[1], ms);
    ctx->t_factor = ms;
    ctx->t_panel = ctx->profile ? (ms - ctx->t_trailing_union) : 0.0;    // exposed panel time: no update launch running
    return rc;
}

// The enqueue: the schedule and the plan of this step (px: pyipm_newton_step and factor_planned alone pass one), which must be the
// one its assembly decided; then the phases above in order.  The same products in the same order per entry: the same bits.
int factor_all(Ctx* ctx, pyipm_factor_stats* stats, bool fuse_forward = false, int px = PX_FULL) {
    const Geo& g = ctx->g;
    if (g.world != 1) { ctx->err = "factor(): single-rank entry point; use the per-panel phases when world > 1"; return PYIPM_E_BADARG; }
    if (!ctx->held.assembled) { ctx->err = "factor: assemble first"; return PYIPM_E_BADARG; }
    const auto t_host0 = std::chrono::steady_clock::now();
    const SchedOpts o = sched_opts(ctx); ctx->sched = plan_groups(g, o);
    StepPlan decided = make_step_plan(g, ctx->sched, o, px, px && ctx->held.plan.e.ok, fuse_forward, fwd_prefix_applies(ctx));
    plan_tail_split(decided, g, ctx->sched, o, ctx->tail_split != 0, HEAD32_ROWS, [&](int64_t grp, int64_t rows) { return group_extra_ok(ctx, grp, rows); });
    FactorRun run{std::move(decided)};
    const StepPlan& plan = run.plan;
    if (px && plan.kind == PX_FULL) { ctx->err = "factor: no reusable prefix in this schedule"; return PYIPM_E_BADARG; }
    if (px && !(plan == ctx->held.plan && (!plan.e.ok || ctx->snap_e))) {
        const char* const what = plan.e.ok || ctx->held.plan.e.ok ? "lambda_e groups" : "x prefix";
        ctx->err = "factor: the schedule changed behind the assembly of a step that keeps the " + std::string(what); return PYIPM_E_BADARG;
    }
    if (plan.frB > plan.frA) run.fr_blocks = fwd_range_grid(ctx, plan.frA, plan.frB);      // (0: the occupancy query says no -- the fallback owners)
    if (run.tr.on()) {
        const bool rec = plan.kind == PX_RECORD, reuse = plan.kind == PX_REUSE;
        fprintf(stderr, "[pyipm group trace] %s step%s\n", rec ? "recording" : reuse ? "reusing" : "full",
                reuse ? ": the x-block prefix is kept" : "");
        if (px) fprintf(stderr, "[pyipm group trace] %s %lld groups: x prefix [0, %lld), lambda_e [%lld, %lld)\n", rec ? "records" : "keeps",
                        (long long)(plan.gB + (plan.e.ok ? plan.e.gE - plan.e.gS : 0)), (long long)plan.gB, (long long)plan.e.gS, (long long)plan.e.gE);
    }
    int rc = enqueue_begin(ctx, run); if (rc) return rc;
    if (plan.slack_first) { rc = enqueue_slack_first(ctx, run, ctx->stream); if (rc) return rc; }
    rc = enqueue_fwd_kept(ctx, run); if (rc) return rc;
    rc = enqueue_between(ctx, run); if (rc) return rc;
    rc = enqueue_kept_diag(ctx, run); if (rc) return rc;
    rc = enqueue_groups(ctx, run); if (rc) return rc;
    return enqueue_end(ctx, run, stats, t_host0);
}

// factor_all on whichever system assemble() built; inertia reported for the FULL KKT matrix either way:
// every eliminated (s_k, lambda_i_k) pair [[Sigma_k, -1], [-1, 0]] has determinant -1, i.e. one positive
// and one negative eigenvalue whatever the sign of Sigma_k.
int factor_dispatch(Ctx* ctx, pyipm_factor_stats* stats, bool fuse_forward, int px) {
    if (!ctx->held.cond_active) { ctx->fwd_vec = ctx->v0; return factor_all(ctx, stats, fuse_forward, px); }
    pyipm_factor_stats local; if (!stats) stats = &local;
    int rc;
    ctx->fwd_vec = ctx->vc;
    { GeoSwap sw(ctx, ctx->gc); rc = factor_all(ctx, stats, fuse_forward); }
    // eliminated pairs (I) carry one negative and one positive eigenvalue each; an active row kept in the
    // system already counts its negative one there, the positive one is its eliminated Sigma_k pivot
    stats->n_neg += ctx->g.mi - ctx->cond_na; stats->n_pos += ctx->g.mi;
    if (ctx->profile) { float ms = 0.f; PYIPM_HIP(hipEventElapsedTime(&ms, ctx->ev[6], ctx->ev[7])); ctx->t_gram = ms; }
    return rc;
}

// kernels of this translation unit on behalf of the others (a kernel is launched from the unit that defines it)
int launch_mask_owned(Ctx* ctx, hipStream_t st, double* v, const double* b) {
    hipLaunchKernelGGL(k_mask_owned, grid1(ctx->g.Npad), dim3(256), 0, st, v, b, ctx->g); PYIPM_KCHECK(); return 0; }
int launch_inpanel_update(Ctx* ctx, hipStream_t st, dim3 grid, double* Cm, int64_t ldc, int64_t ccol, const double* Lop, int64_t ldl,
                          const double* Wop, int64_t ldw, int64_t cglob, int K, int64_t row_begin, int64_t row_end,
                          int64_t a0, int64_t a1, int64_t b0, int64_t b1, int prio) {
    hipLaunchKernelGGL(k_inpanel_update, grid, dim3(256), 0, st, Cm, ldc, ccol, Lop, ldl, Wop, ldw, cglob, K, row_begin, row_end, a0, a1, b0, b1, prio);
    PYIPM_KCHECK(); return 0; }

int copy_out(Ctx* ctx, double* dst, const double* src_dev, size_t count, int memkind) {
    if (!dst || count == 0) return 0;
    PYIPM_HIP(hipMemcpyAsync(dst, src_dev, count * sizeof(double),
                             memkind == PYIPM_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, ctx->stream));
    if (memkind == PYIPM_MEM_HOST) PYIPM_HIP(hipStreamSynchronize(ctx->stream));
    return 0;
}

// load the right-hand side into v1 (kept for refinement) and v0 (solved in place)
int solve_prepare(Ctx* ctx, const double* rhs, int memkind, bool for_fused_forward) {
    const Geo& g = ctx->g;
    if (rhs) {
        hipLaunchKernelGGL(k_fill, grid1(g.Npad), dim3(256), 0, ctx->stream, ctx->v1, 0.0, g.Npad); PYIPM_KCHECK();
        int rc = put_vec(ctx, ctx->v1, rhs, g.N, memkind); if (rc) return rc;
    } else {
        if (!ctx->held.have_rhs) { ctx->err = "solve: no right-hand side (call residual or pass rhs)"; return PYIPM_E_BADARG; }
        PYIPM_HIP(hipMemcpyAsync(ctx->v1, ctx->rhs, g.Npad * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    }
    PYIPM_HIP(hipMemcpyAsync(ctx->v0, ctx->v1, g.Npad * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    if (for_fused_forward && ctx->held.cond_active) return cond_reduce(ctx, ctx->v0, ctx->vc);   // the fused pass runs on vc
    return 0;
}

// The tail of every solve: v1 = b and v0 = b (solve_prepare) -> x in v0, refined against the blocks (v2 the residual, v3 the spare
// iterate), flipped into v2 and copied out.  Events 4 (the caller) and 5 bracket it.
int solve_finish(Ctx* ctx, const SolveOps& ops, double* dz, int flip, int refine, int memkind, bool forward_done) {
    const Geo& g = ctx->g;
    int rc = ops.solve(ctx, ctx->v1, ctx->v0, forward_done); if (rc) return rc;
    const size_t vbytes = (size_t)g.Npad * sizeof(double);
    rc = refine_loop(ctx, refine,
        [&]() -> int {                                          // v2 = b - Hc v0
            int r2 = ops.matvec(ctx, ctx->v0, ctx->v2); if (r2) return r2;
            hipLaunchKernelGGL(k_axpby, grid1(g.Npad), dim3(256), 0, ctx->stream, ctx->v2, ctx->v1, ctx->v2, 1.0, -1.0, g.Npad);
            PYIPM_KCHECK();
            return 0;
        },
        [&](double* berr) -> int {
            double ss[2];
            hipLaunchKernelGGL(k_sumsq2, dim3(1), dim3(1024), 0, ctx->stream, ctx->partial, ctx->v2, ctx->v1, g.N);
            PYIPM_KCHECK();
            PYIPM_HIP(hipMemcpyAsync(ss, ctx->partial, 2 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
            PYIPM_HIP(hipStreamSynchronize(ctx->stream));
            *berr = ss[1] > 0.0 ? sqrt(ss[0] / ss[1]) : sqrt(ss[0]);
            return 0;
        },
        [&]() -> int { PYIPM_HIP(hipMemcpyAsync(ctx->v3, ctx->v0, vbytes, hipMemcpyDeviceToDevice, ctx->stream)); return 0; },
        [&]() -> int { PYIPM_HIP(hipMemcpyAsync(ctx->v0, ctx->v3, vbytes, hipMemcpyDeviceToDevice, ctx->stream)); return 0; },
        [&]() -> int {                                          // v0 += Hc^{-1} v2
            int r2 = ops.solve(ctx, ctx->v2, ctx->v2, false); if (r2) return r2;
            hipLaunchKernelGGL(k_axpby, grid1(g.Npad), dim3(256), 0, ctx->stream, ctx->v0, ctx->v0, ctx->v2, 1.0, 1.0, g.Npad);
            PYIPM_KCHECK();
            return 0;
        });
    if (rc) return rc;
    // flip + copy out (device staging through v2 so host copies stay contiguous)
    hipLaunchKernelGGL(k_copy_flip, grid1(g.N), dim3(256), 0, ctx->stream, ctx->v2, ctx->v0, g.N, g.n + g.mi,
                       (flip && (g.me + g.mi) > 0) ? 1 : 0);
    PYIPM_KCHECK();
    PYIPM_HIP(hipEventRecord(ctx->ev[5], ctx->stream));
    rc = copy_out(ctx, dz, ctx->v2, g.N, memkind); if (rc) return rc;
    ctx->held.solved((flip != 0) || (g.me + g.mi == 0), ops.ray_survives);
    return PYIPM_OK;
}

static int solve_local(Ctx* ctx, const double*, double* x, bool forward_done) { return solve_inplace(ctx, x, forward_done); }
static const SolveOps kLocalOps = {solve_local, kkt_matvec_dev, false};

// events 2 and 3 around the assembly (last_timings)
int assemble_timed(Ctx* ctx, double delta, double delta_c) {
    PYIPM_HIP(hipEventRecord(ctx->ev[2], ctx->stream));
    int rc = assemble_dev(ctx, delta, delta_c); if (rc) return rc;
    PYIPM_HIP(hipEventRecord(ctx->ev[3], ctx->stream));
    ctx->held.assemble_timed();
    return PYIPM_OK;
}

// y = Hc v for the caller.  The product goes through vc (free outside a condensed solve), so v2 -- the direction of the last
// solve, which step_lengths() reads -- survives a backward-error check; v1 takes the operand.
int kkt_matvec_io(Ctx* ctx, const SolveOps& ops, const double* v, double* y, int memkind) {
    const Geo& g = ctx->g;
    ctx->held.borrowed(Held::V1);
    hipLaunchKernelGGL(k_fill, grid1(g.Npad), dim3(256), 0, ctx->stream, ctx->v1, 0.0, g.Npad); PYIPM_KCHECK();
    int rc = put_vec(ctx, ctx->v1, v, g.N, memkind); if (rc) return rc;
    rc = ops.matvec(ctx, ctx->v1, ctx->vc); if (rc) return rc;
    return copy_out(ctx, y, ctx->vc, g.N, memkind);
}

} }  // namespace pyipm::drv

// =================================================================================================
#pragma GCC visibility push(default)
extern "C" {

size_t pyipm_newton_workspace_bytes(int64_t n, int64_t me, int64_t mi, int nb, int world, int rank) try {
    if (n <= 0 || me < 0 || mi < 0 || world < 1 || rank < 0 || rank >= world) return 0;
    if (nb == 0) nb = 256;
    if (nb % 128 != 0 || nb > 1024) return 0;
    Geo g = make_geo(n, me, mi, nb, world, rank);
    return carve_workspace(nullptr, g, nullptr);
} PYIPM_CATCH_SIZE

// The one way a handle comes to be.  args_ok: the entry point's checks of its own arguments;  set(ctx): the fields of this kind of
// handle (its device is current);  carve(ctx, base): the workspace layout (both NULL: only its size);  anorm_words: what of
// ctx->anorm starts at zero;  schedule_events: the provider and lookahead events of a single-system handle beside the eight
// timing events every handle has.  An early return releases whatever the handle owns by then (~Ctx).
static int create_handle(pyipm_newton_ctx** out, bool args_ok, int device, void* workspace, size_t workspace_bytes, void* stream,
                         const std::function<void(Ctx*)>& set, const std::function<size_t(Ctx*, char*)>& carve, size_t anorm_words,
                         bool schedule_events) {
    if (!out) return PYIPM_E_BADARG;
    *out = nullptr;
    if (!args_ok) return PYIPM_E_BADARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return PYIPM_E_NODEVICE;
    std::unique_ptr<Ctx> ctx(new Ctx());
    ctx->device = device;
    ctx->stream = (hipStream_t)stream;
    if (hipSetDevice(device) != hipSuccess) return PYIPM_E_NODEVICE;
    set(ctx.get());
    const size_t need = carve(nullptr, nullptr);
    if (workspace) {
        if (workspace_bytes < need) return PYIPM_E_NOMEM;
        ctx->ws.adopt((char*)workspace, need);
    } else {
        if (ctx->ws.reserve(need) != hipSuccess) return PYIPM_E_NOMEM;
        if (getenv("PYIPM_POISON_WORKSPACE")) hipMemset(ctx->ws, 0xFF, need);      // test hook: NaN wherever nothing is written before it is read
    }
    carve(ctx.get(), ctx->ws.get());
    if (hipMemset(ctx->anorm, 0, anorm_words * sizeof(unsigned long long)) != hipSuccess) return PYIPM_E_HIP;
    for (Event& e : ctx->ev) if (e.ensure(hipEventDefault) != hipSuccess) return PYIPM_E_HIP;
    if (ctx->tail_split) {            // the flag word of the tail split, zero before any stream can poll it (PollWords::zero_and_wait: why the wait)
        if (ctx->tail_flag.reserve(1) != hipSuccess) return PYIPM_E_NOMEM;
        if (hipMemset(ctx->tail_flag.get(), 0, sizeof(unsigned)) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return PYIPM_E_HIP;
    }
    if (schedule_events) {
        for (Event& e : ctx->ev_prov) if (e.ensure(hipEventDefault) != hipSuccess) return PYIPM_E_HIP;
        for (Event* e : {&ctx->ev_fwd, &ctx->ev_head, &ctx->ev_panel}) if (e->ensure(hipEventDisableTiming) != hipSuccess) return PYIPM_E_HIP;
    }
    *out = reinterpret_cast<pyipm_newton_ctx*>(ctx.release());
    return PYIPM_OK;
}

static int create_impl(pyipm_newton_ctx** out, int64_t n, int64_t me, int64_t mi, int nb, int device,
                       int world, int rank, void* workspace, size_t workspace_bytes, void* stream, bool provider_only) {
    if (nb == 0) nb = 256;
    const bool args_ok = n > 0 && me >= 0 && mi >= 0 && world >= 1 && rank >= 0 && rank < world && nb % 128 == 0 && nb <= 1024;
    const Geo g = args_ok ? make_geo(n, me, mi, nb, world, rank) : Geo{};
    return create_handle(out, args_ok, device, workspace, workspace_bytes, stream,
        [&](Ctx* ctx) {
            ctx->g = g;
            ctx->gc = make_geo(n, me, 0, nb, 1, 0);          // re-derived by every condensed assemble
            ctx->group = default_group(world, nb);
            { int ncu = 0; if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && ncu > 0) ctx->num_cus = ncu; }
            ctx->provider_only = provider_only;
            { const char* e = getenv("PYIPM_REUSE_X"); if (e && e[0] == '0') ctx->reuse_x = 0; }
            { const char* e = getenv("PYIPM_REUSE_LAM_E"); if (e && e[0] == '0') ctx->reuse_lam_e = 0; }
            { const char* e = getenv("PYIPM_FWD_PREFIX"); if (e) { const int w = atoi(e); if (w <= 0) ctx->fwd_prefix = 0; else if (w >= 2) ctx->fwd_prefix_wgs = w; } }
            { const char* e = getenv("PYIPM_FWD_RANGE"); if (e) { const int w = atoi(e); if (w <= 0) ctx->fwd_range = 0; else if (w >= 2) ctx->fwd_range_wgs = w; } }
            { const char* e = getenv("PYIPM_SLACK_ONE"); if (e && atoi(e) <= 0) ctx->slack_one = 0; }
            { const char* e = getenv("PYIPM_BWD_SLACK"); if (e && e[0] == '0') ctx->bwd_slack = 0; }
            { const char* e = getenv("PYIPM_TAIL_SPLIT"); if (e && e[0] == '0') ctx->tail_split = 0; }
            { const char* e = getenv("PYIPM_MS_MATVEC_MANY"); if (e && atoi(e) > 0) ctx->ms_matvec_many = 1; }
        },
        [&](Ctx* ctx, char* base) { return carve_workspace(ctx, g, base, provider_only); },
        2 /* [0] max |entry|, [1] "assembly pending" */, true);
}

int pyipm_newton_create(pyipm_newton_ctx** out, int64_t n, int64_t me, int64_t mi, int nb, int device,
                        int world, int rank, void* workspace, size_t workspace_bytes, void* stream) try {
    return create_impl(out, n, me, mi, nb, device, world, rank, workspace, workspace_bytes, stream, false);
} PYIPM_CATCH_NOH

size_t pyipm_newton_workspace_bytes_provider(int64_t n, int64_t me, int64_t mi) try {
    if (n <= 0 || me < 0 || mi < 0) return 0;
    Geo g = make_geo(n, me, mi, 256, 1, 0);
    return carve_workspace(nullptr, g, nullptr, true);
} PYIPM_CATCH_SIZE

int pyipm_newton_create_provider(pyipm_newton_ctx** out, int64_t n, int64_t me, int64_t mi, int device,
                                 void* workspace, size_t workspace_bytes, void* stream) try {
    return create_impl(out, n, me, mi, 256, device, 1, 0, workspace, workspace_bytes, stream, true);
} PYIPM_CATCH_NOH

size_t pyipm_newton_workspace_bytes_batched(int64_t n, int64_t me, int64_t mi, int batch) try {
    if (n <= 0 || me < 0 || mi < 0 || batch < 1) return 0;
    Geo g = make_geo(n, me, mi, 128, 1, 0);
    if (g.Npad > 1024) return 0;
    return carve_batched(nullptr, g, batch, nullptr);
} PYIPM_CATCH_SIZE

int pyipm_newton_create_batched(pyipm_newton_ctx** out, int64_t n, int64_t me, int64_t mi, int batch, int device,
                                void* workspace, size_t workspace_bytes, void* stream) try {
    bool args_ok = n > 0 && me >= 0 && mi >= 0 && batch >= 1;
    const Geo g = args_ok ? make_geo(n, me, mi, 128, 1, 0) : Geo{};
    args_ok = args_ok && g.Npad <= 1024;               // one workgroup per problem: Npad threads in the substitutions
    return create_handle(out, args_ok, device, workspace, workspace_bytes, stream,
        [&](Ctx* ctx) {
            ctx->g = g; ctx->gc = g;
            ctx->batch = batch;
            ctx->group = 1;
            ctx->batched = true;
            ctx->tile_blocked = 1;       // the blocked inversion in both forms since round 6 (512 x N = 768, full form: 3.24 against 3.44 ms;
                                         // condensed: 0.99 against 1.10; round 3 measured the opposite for the full form, before the per-problem
                                         // Gram kernel and the eight-wave-free register budget of today's k_b_factor)
        },
        [&](Ctx* ctx, char* base) { return carve_batched(ctx, g, batch, base); },
        (size_t)batch * 2, false);
} PYIPM_CATCH_NOH

// the statistics records of the last step_batched (waits for it) and its time
static int fetch_batched_stats(Ctx* ctx, pyipm_factor_stats* stats) {
    const int B = ctx->batch;
    std::vector<DevStats> z((size_t)B);
    PYIPM_HIP(hipMemcpyAsync(z.data(), ctx->dstats, (size_t)B * sizeof(DevStats), hipMemcpyDeviceToHost, ctx->stream));
    PYIPM_HIP(hipStreamSynchronize(ctx->stream));
    int rc = PYIPM_OK;
    for (int b = 0; b < B; ++b) {
        stats[b] = to_stats(z[b]);
        if (z[b].nonfinite) { ctx->err = "NaN/Inf met during factorisation"; rc = PYIPM_E_NONFINITE; }
    }
    float ms = 0.f;
    PYIPM_HIP(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
    ctx->t_factor = ms;
    return rc;
}

int pyipm_newton_stage_blocks_batched(pyipm_newton_ctx* h, const double* d2L, int64_t ld_d2L, int64_t stride_d2L,
                                      const double* Je, int64_t ld_Je, int64_t stride_Je,
                                      const double* Ji, int64_t ld_Ji, int64_t stride_Ji) try {
    PYIPM_ENTER("stage_blocks_batched", G_BATCHED) const Geo& g = ctx->g;
    if (!d2L || ld_d2L < g.n || (g.me && (!Je || ld_Je < g.me)) || (g.mi && (!Ji || ld_Ji < g.mi))) {
        ctx->err = "stage_blocks_batched: bad block pointer / leading dimension (device pointers only)"; return PYIPM_E_BADARG; }
    ctx->d2L = d2L; ctx->ld_d2L = ld_d2L; ctx->b_sH = stride_d2L;
    ctx->Je = g.me ? Je : nullptr; ctx->ld_Je = ld_Je; ctx->b_sJe = stride_Je;
    ctx->Ji = g.mi ? Ji : nullptr; ctx->ld_Ji = ld_Ji; ctx->b_sJi = stride_Ji;
    ctx->held.blocks_staged();              // (nothing on a batched handle ever forms the products it forgets)
    return PYIPM_OK;
} PYIPM_CATCH_H(h)

// The launches of one batched step, for both entries: k_b_begin (who takes part, with which mu / delta / delta_c), residual or
// condensed prep, assembly, factorisation, substitutions.  A problem whose flag is 0 costs a workgroup that returns at once
// in each of them; its matrix, factor, statistics record, anorm words and row of dz stay as its last step left them.
static int step_batched_enqueue(Ctx* ctx, const BatchEach& in, double* dz, int memkind) {
    const Geo& g = ctx->g;
    const int B = ctx->batch;
    BatchPtrs bp = batch_ptrs(ctx);
    BatchCond bc = batch_cond(ctx);
    const int cond = (ctx->condensed && g.mi > 0) ? 1 : 0;
    ctx->held.step_batched_begun(cond != 0);
    if (ctx->b_form.capacity() < (size_t)B) {               // first step of the handle: no problem holds a factor yet
        PYIPM_HIP(ctx->b_form.reserve((size_t)B));
        PYIPM_HIP(hipMemsetAsync(ctx->b_form, 0xFF, (size_t)B * sizeof(int), ctx->stream));
    }
    if (cond) ctx->b_any_cond = true;
    PYIPM_HIP(hipEventRecord(ctx->ev[0], ctx->stream));
    hipLaunchKernelGGL(k_b_begin, grid1(B), dim3(256), 0, ctx->stream, bp, in, B, ctx->b_form.get(), cond);
    PYIPM_KCHECK();
    if (cond) {
        // condensed form: per problem n + me + |A| columns instead of n + 2 mi + me (config 5: 256 instead of 768) -- the
        // (s, lambda_i) pairs with Sigma <= condensed_sigma_max eliminated analytically (pyipm.py:824-842's block structure)
        hipLaunchKernelGGL(k_bc_prep, dim3(B), dim3(256), 0, ctx->stream, bp, g, ctx->eps, bc);
        PYIPM_KCHECK();
        const int nt0 = (int)((g.n + g.me + TB - 1) / TB);
        const int nx = (g.n % TB == 0 && g.n >= TB && g.n <= 4 * TB && g.mi % 32 == 0 && ctx->bc_per_problem) ? (int)(g.n / TB) : 0;
        // one workgroup per problem while the Jacobian chunk of all n columns fits shared memory twice (n <= 256), else a tile each
        if (nx == 4)      hipLaunchKernelGGL((k_bc_assemble_p<4>), dim3((unsigned)B), dim3(512), 0, ctx->stream, bp, g, ctx->eps, bc);
        else if (nx == 3) hipLaunchKernelGGL((k_bc_assemble_p<3>), dim3((unsigned)B), dim3(384), 0, ctx->stream, bp, g, ctx->eps, bc);
        else if (nx == 2) hipLaunchKernelGGL((k_bc_assemble_p<2>), dim3((unsigned)B), dim3(256), 0, ctx->stream, bp, g, ctx->eps, bc);
        else if (nx == 1) hipLaunchKernelGGL((k_bc_assemble_p<1>), dim3((unsigned)B), dim3(128), 0, ctx->stream, bp, g, ctx->eps, bc);
        else
            hipLaunchKernelGGL(k_bc_assemble, dim3((unsigned)(nt0 * (nt0 + 1) / 2 + 1), (unsigned)B), dim3(256), 0, ctx->stream, bp, g,
                               ctx->eps, bc, nt0);
        PYIPM_KCHECK();
    } else {
        hipLaunchKernelGGL(k_b_residual, dim3(B), dim3(256), 0, ctx->stream, bp, g, ctx->eps);
        PYIPM_KCHECK();
        dim3 grid((unsigned)((g.Npad + 511) / 512), (unsigned)((g.Npad + 15) / 16), (unsigned)B);
        hipLaunchKernelGGL(k_b_assemble, grid, dim3(256), 0, ctx->stream, bp, g, ctx->eps);
        PYIPM_KCHECK();
    }
    PYIPM_HIP(hipEventRecord(ctx->ev[2], ctx->stream));
    hipLaunchKernelGGL(k_b_factor, dim3(B), dim3(256), 0, ctx->stream, bp, g, ctx->refine_cond, ctx->block_refine, ctx->pivtol_rel, ctx->tile_blocked,
                       cond ? (const int*)ctx->cond_cnt : (const int*)nullptr);
    PYIPM_KCHECK();
    PYIPM_HIP(hipEventRecord(ctx->ev[3], ctx->stream));
    double* out_dev = (memkind == PYIPM_MEM_DEVICE) ? dz : ctx->v2;
    hipLaunchKernelGGL(k_b_solve, dim3(B), dim3((unsigned)g.Npad), 2 * g.Npad * sizeof(double), ctx->stream, bp, g,
                       ctx->block_refine, (g.me + g.mi) > 0 ? 1 : 0, out_dev, bc, cond, ctx->eps);
    PYIPM_KCHECK();
    PYIPM_HIP(hipEventRecord(ctx->ev[1], ctx->stream));
    ctx->held.step_batched_enqueued(memkind == PYIPM_MEM_HOST);
    return PYIPM_OK;
}

int pyipm_newton_step_batched(pyipm_newton_ctx* h, double delta, double delta_c, double* dz,
                              pyipm_factor_stats* stats, int memkind) try {
    PYIPM_ENTER("step_batched", G_BATCHED | G_DEVICE) const Geo& g = ctx->g;
    if (!ctx->held.have_blocks || !ctx->held.have_vectors) { ctx->err = "step_batched: stage blocks and vectors first"; return PYIPM_E_BADARG; }
    if (!dz) { ctx->err = "step_batched: null output"; return PYIPM_E_BADARG; }
    const int B = ctx->batch;
    ctx->delta = delta; ctx->delta_c = delta_c;
    // one mu (stage_vectors') and one pair of shifts for every problem, all of them active
    const BatchEach in = {nullptr, nullptr, nullptr, nullptr, ctx->mu, delta, delta_c};
    { int rc = step_batched_enqueue(ctx, in, dz, memkind); if (rc) return rc; }
    if (memkind == PYIPM_MEM_HOST)
        PYIPM_HIP(hipMemcpyAsync(dz, ctx->v2, (size_t)B * g.N * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (stats) return fetch_batched_stats(ctx, stats);
    if (memkind == PYIPM_MEM_HOST) PYIPM_HIP(hipStreamSynchronize(ctx->stream));
    return PYIPM_OK;
} PYIPM_CATCH_H(h)

// A step with each problem's own mu, delta, delta_c (after the first barrier update, pyipm.py:1804-1814, and the first reghess,
// pyipm.py:1373-1406, no two problems of a multi-start batch share them) for the problems `active` selects.
int pyipm_newton_step_batched_each(pyipm_newton_ctx* h, const double* mu, const double* delta, const double* delta_c,
                                   const int32_t* active, double* dz, int memkind) try {
    PYIPM_ENTER("step_batched_each", G_BATCHED | G_DEVICE) const Geo& g = ctx->g;
    if (!ctx->held.have_blocks || !ctx->held.have_vectors) { ctx->err = "step_batched_each: stage blocks and vectors first"; return PYIPM_E_BADARG; }
    if (!mu || !delta || !delta_c) { ctx->err = "step_batched_each: null mu / delta / delta_c"; return PYIPM_E_BADARG; }
    if (!dz) { ctx->err = "step_batched_each: null output"; return PYIPM_E_BADARG; }
    if (memkind != PYIPM_MEM_DEVICE && memkind != PYIPM_MEM_HOST) { ctx->err = "step_batched_each: bad memkind"; return PYIPM_E_BADARG; }
    const size_t B = (size_t)ctx->batch;
    BatchEach in = {mu, delta, delta_c, (const int*)active, 0.0, 0.0, 0.0};
    if (memkind == PYIPM_MEM_HOST) {
        // host arrays land in the handle first; k_b_begin then moves the entries of the problems that take part
        PYIPM_HIP(hipMemcpyAsync(ctx->b_in, mu, B * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        PYIPM_HIP(hipMemcpyAsync(ctx->b_in + B, delta, B * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        PYIPM_HIP(hipMemcpyAsync(ctx->b_in + 2 * B, delta_c, B * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        if (active) PYIPM_HIP(hipMemcpyAsync(ctx->b_in_act, active, B * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
        in.mu = ctx->b_in; in.delta = ctx->b_in + B; in.delta_c = ctx->b_in + 2 * B; in.active = active ? ctx->b_in_act : nullptr;
    }
    { int rc = step_batched_enqueue(ctx, in, dz, memkind); if (rc) return rc; }
    if (memkind == PYIPM_MEM_HOST) {
        // only the rows of the problems that took part, run by run
        const size_t row = (size_t)g.N;
        for (size_t b0 = 0; b0 < B;) {
            if (active && !active[b0]) { ++b0; continue; }
            size_t b1 = b0 + 1;
            while (b1 < B && (!active || active[b1])) ++b1;
            PYIPM_HIP(hipMemcpyAsync(dz + b0 * row, ctx->v2 + b0 * row, (b1 - b0) * row * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
            b0 = b1;
        }
        PYIPM_HIP(hipStreamSynchronize(ctx->stream));
    }
    return PYIPM_OK;
} PYIPM_CATCH_H(h)

// alpha[b] = (alpha_s, alpha_l) of every problem for the staged s, lda and the directions dz (k_b_step_lengths)
int pyipm_newton_step_lengths_batched(pyipm_newton_ctx* h, double tau, const double* dz, double* alpha, int memkind) try {
    PYIPM_ENTER("step_lengths_batched", G_BATCHED | G_DEVICE) const Geo& g = ctx->g;
    if (!alpha) { ctx->err = "step_lengths_batched: null output"; return PYIPM_E_BADARG; }
    if (memkind != PYIPM_MEM_DEVICE && memkind != PYIPM_MEM_HOST) { ctx->err = "step_lengths_batched: bad memkind"; return PYIPM_E_BADARG; }
    if (!ctx->held.have_vectors) { ctx->err = "step_lengths_batched: stage vectors first"; return PYIPM_E_BADARG; }
    if (!dz && !ctx->held.have_direction) {
        ctx->err = "step_lengths_batched: the handle keeps the directions of a step with host output only -- pass dz"; return PYIPM_E_BADARG; }
    const int B = ctx->batch;
    double* dev = (memkind == PYIPM_MEM_DEVICE) ? alpha : ctx->b_alpha;
    hipLaunchKernelGGL(k_b_step_lengths, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, ctx->stream, dev, ctx->s, ctx->lda,
                       dz ? dz : ctx->v2, g, B, tau);
    PYIPM_KCHECK();
    if (memkind == PYIPM_MEM_HOST) {
        PYIPM_HIP(hipMemcpyAsync(alpha, ctx->b_alpha, (size_t)B * 2 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        PYIPM_HIP(hipStreamSynchronize(ctx->stream));
    }
    return PYIPM_OK;
} PYIPM_CATCH_H(h)

// The per-problem statistics of the last step_batched, fetched when the caller wants them: a step called with stats = NULL
// returns as soon as its five launches are enqueued (round 6: the copy of 512 statistics records and the synchronisation in
// front of it were 0.3 of the 1.4 ms a batch step took on the host's clock).
int pyipm_newton_stats_batched(pyipm_newton_ctx* h, pyipm_factor_stats* stats) try {
    PYIPM_ENTER("stats_batched", G_BATCHED | G_DEVICE)
    if (!stats) return PYIPM_E_BADARG;
    if (!ctx->held.have_rhs) { ctx->err = "stats_batched: step_batched first"; return PYIPM_E_BADARG; }
    return fetch_batched_stats(ctx, stats);
} PYIPM_CATCH_H(h)

// out[b] = |g - Hc raw_b| / |g| of every problem, Hc applied from the blocks with the problem's own shifts (k_b_berr)
int pyipm_newton_backward_error_batched(pyipm_newton_ctx* h, const double* dz, double* out, int memkind) try {
    PYIPM_ENTER("backward_error_batched", G_BATCHED | G_DEVICE) const Geo& g = ctx->g;
    if (!dz || !out) return PYIPM_E_BADARG;
    if (!ctx->held.have_blocks || !ctx->held.have_vectors || !ctx->held.have_rhs) { ctx->err = "backward_error_batched: step_batched first"; return PYIPM_E_BADARG; }
    BatchPtrs bp = batch_ptrs(ctx);
    double* dev = (memkind == PYIPM_MEM_DEVICE) ? out : ctx->vt;
    hipLaunchKernelGGL(k_b_berr, dim3(ctx->batch), dim3(256), 0, ctx->stream, bp, g, dz, ctx->eps, dev);
    PYIPM_KCHECK();
    if (memkind == PYIPM_MEM_HOST) {
        PYIPM_HIP(hipMemcpyAsync(out, ctx->vt, (size_t)ctx->batch * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        PYIPM_HIP(hipStreamSynchronize(ctx->stream));
    }
    return PYIPM_OK;
} PYIPM_CATCH_H(h)

// ---- the batch as a solver: provider products and merit pieces of every problem (kernels_batched.hpp) ----
// Scratch of the four entries below, outside the workspace (as solve_many's): the fixed part and room for K candidates.
struct BatchMerit { double *info, *gq, *dce, *dci, *nu, *mu, *quad, *alphas, *out; };
static int batch_merit_scratch(Ctx* ctx, int K, BatchMerit* m) {
    const Geo& g = ctx->g;
    const size_t B = (size_t)ctx->batch, fixed = B * (size_t)(MERIT_NQ + 2 + g.me + g.mi + 3);
    const size_t need = fixed + 2 * B * (size_t)K;
    if (ctx->b_merit_buf.capacity() < need) {
        PYIPM_HIP(ctx->b_merit_buf.reserve(need));
        if (getenv("PYIPM_POISON_WORKSPACE")) PYIPM_HIP(hipMemsetAsync(ctx->b_merit_buf, 0xFF, need * sizeof(double), ctx->stream));   // as the workspace
    }
    double* p = ctx->b_merit_buf;
    m->info = p; p += B * MERIT_NQ;
    m->gq = p; p += B * 2;
    m->dce = p; p += B * (size_t)g.me;
    m->dci = p; p += B * (size_t)g.mi;
    m->nu = p; p += B; m->mu = p; p += B; m->quad = p; p += B;
    m->alphas = p; p += B * (size_t)K; m->out = p;
    return 0;
}
static size_t batch_products_lds(const Geo& g) { return (size_t)(2 * g.n + 4 * (g.n + g.me + g.mi)) * sizeof(double); }

int pyipm_newton_block_products_batched(pyipm_newton_ctx* h, const double* v, double* Qv, double* JeTv, double* JiTv) try {
    PYIPM_ENTER("block_products_batched", G_BATCHED | G_DEVICE) const Geo& g = ctx->g;
    if (!v) { ctx->err = "block_products_batched: null v"; return PYIPM_E_BADARG; }
    if (!ctx->held.have_blocks) { ctx->err = "block_products_batched: stage blocks first"; return PYIPM_E_BADARG; }
    if (!Qv && !(JeTv && g.me) && !(JiTv && g.mi)) return PYIPM_OK;
    hipLaunchKernelGGL(k_b_products, dim3((unsigned)ctx->batch), dim3(256), batch_products_lds(g), ctx->stream, batch_ptrs(ctx), g, v, Qv, JeTv, JiTv);
    PYIPM_KCHECK();
    return PYIPM_OK;
} PYIPM_CATCH_H(h)

int pyipm_newton_block_products_t_batched(pyipm_newton_ctx* h, const double* le, const double* li, double* out) try {
    PYIPM_ENTER("block_products_t_batched", G_BATCHED | G_DEVICE) const Geo& g = ctx->g;
    if (!out) { ctx->err = "block_products_t_batched: null output"; return PYIPM_E_BADARG; }
    if (!ctx->held.have_blocks) { ctx->err = "block_products_t_batched: stage blocks first"; return PYIPM_E_BADARG; }
    hipLaunchKernelGGL(k_b_products_t, dim3((unsigned)ctx->batch), dim3(256), 0, ctx->stream, batch_ptrs(ctx), g, le, li, out);
    PYIPM_KCHECK();
    return PYIPM_OK;
} PYIPM_CATCH_H(h)

int pyipm_newton_merit_info_batched(pyipm_newton_ctx* h, const double* dz, double* out, int memkind) try {
    PYIPM_ENTER("merit_info_batched", G_BATCHED | G_DEVICE) const Geo& g = ctx->g;
    if (!out) { ctx->err = "merit_info_batched: null output"; return PYIPM_E_BADARG; }
    if (memkind != PYIPM_MEM_DEVICE && memkind != PYIPM_MEM_HOST) { ctx->err = "merit_info_batched: bad memkind"; return PYIPM_E_BADARG; }
    if (!ctx->held.have_vectors) { ctx->err = "merit_info_batched: stage vectors first"; return PYIPM_E_BADARG; }
    const int B = ctx->batch;
    BatchMerit m;
    if (memkind == PYIPM_MEM_HOST) { int rc = batch_merit_scratch(ctx, 0, &m); if (rc) return rc; }
    const double* d = dz ? dz : (ctx->held.have_direction ? ctx->v2 : nullptr);
    double* dev = (memkind == PYIPM_MEM_DEVICE) ? out : m.info;
    hipLaunchKernelGGL(k_b_merit_info, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, ctx->stream, dev, batch_ptrs(ctx), g, d,
                       ctx->held.have_rhs ? 1 : 0, ctx->eps, B);
    PYIPM_KCHECK();
    if (memkind == PYIPM_MEM_HOST) {
        PYIPM_HIP(hipMemcpyAsync(out, dev, (size_t)B * MERIT_NQ * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        PYIPM_HIP(hipStreamSynchronize(ctx->stream));
    }
    return PYIPM_OK;
} PYIPM_CATCH_H(h)

int pyipm_newton_merit_ray_batched(pyipm_newton_ctx* h, const double* dz, const double* nu, const double* mu, const double* quad,
                                   const double* alphas, int K, double* out, int memkind) try {
    PYIPM_ENTER("merit_ray_batched", G_BATCHED | G_DEVICE) const Geo& g = ctx->g;
    if (!nu || !mu || !alphas || !out) { ctx->err = "merit_ray_batched: null nu / mu / alphas / out"; return PYIPM_E_BADARG; }
    if (K < 1 || K > 1024) { ctx->err = "merit_ray_batched: 1 <= K <= 1024"; return PYIPM_E_BADARG; }
    if (memkind != PYIPM_MEM_DEVICE && memkind != PYIPM_MEM_HOST) { ctx->err = "merit_ray_batched: bad memkind"; return PYIPM_E_BADARG; }
    if (!ctx->held.have_vectors || !ctx->held.have_blocks) { ctx->err = "merit_ray_batched: stage blocks and vectors first"; return PYIPM_E_BADARG; }
    const double* d = dz ? dz : (ctx->held.have_direction ? ctx->v2 : nullptr);
    if (!d) { ctx->err = "merit_ray_batched: the handle keeps the directions of a step with host output only -- pass dz"; return PYIPM_E_BADARG; }
    const size_t B = (size_t)ctx->batch;
    const bool host = memkind == PYIPM_MEM_HOST;
    BatchMerit m;
    { int rc = batch_merit_scratch(ctx, host ? K : 0, &m); if (rc) return rc; }
    if (host) {
        PYIPM_HIP(hipMemcpyAsync(m.nu, nu, B * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        PYIPM_HIP(hipMemcpyAsync(m.mu, mu, B * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        if (quad) PYIPM_HIP(hipMemcpyAsync(m.quad, quad, B * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        PYIPM_HIP(hipMemcpyAsync(m.alphas, alphas, B * (size_t)K * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        nu = m.nu; mu = m.mu; if (quad) quad = m.quad; alphas = m.alphas;
    }
    const BatchPtrs bp = batch_ptrs(ctx);
    // the products of the direction with the blocks, formed for every call: nothing of a direction is kept between two calls
    hipLaunchKernelGGL(k_b_ray_prep, dim3((unsigned)B), dim3(256), batch_products_lds(g), ctx->stream, bp, g, d, quad, m.gq, m.dce, m.dci);
    PYIPM_KCHECK();
    double* dev = host ? m.out : out;
    hipLaunchKernelGGL(k_b_merit_ray, dim3((unsigned)((K + 3) / 4), (unsigned)B), dim3(256), 0, ctx->stream, dev, alphas, K, bp, g,
                       m.gq, m.dce, m.dci, d, nu, mu);
    PYIPM_KCHECK();
    if (host) {
        PYIPM_HIP(hipMemcpyAsync(out, dev, B * (size_t)K * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        PYIPM_HIP(hipStreamSynchronize(ctx->stream));
    }
    return PYIPM_OK;
} PYIPM_CATCH_H(h)

// ---- the kept factors of a batch as a solver (kernels_bsolve.hpp) ----------------------------------------
// Scratch of the three entries below, the library's own buffer outside the workspace (as b_merit_buf): `count` doubles behind
// the staged mask.  Growing drops the contents: nothing in it outlives a call.
static int batch_solve_scratch(Ctx* ctx, size_t count, int** mask, double** p) {
    const size_t B = (size_t)ctx->batch, head = (B * sizeof(int) + sizeof(double) - 1) / sizeof(double), need = head + count;
    if (ctx->b_solve_buf.capacity() < need) {
        PYIPM_HIP(ctx->b_solve_buf.reserve(need));
        if (getenv("PYIPM_POISON_WORKSPACE")) PYIPM_HIP(hipMemsetAsync(ctx->b_solve_buf, 0xFF, need * sizeof(double), ctx->stream));   // as the workspace
    }
    *mask = reinterpret_cast<int*>(ctx->b_solve_buf.get());
    *p = ctx->b_solve_buf.get() + head;
    return 0;
}
// the mask as the kernels read it: the caller's device array, or the host one staged
static int batch_mask(Ctx* ctx, const int32_t* active, int memkind, int* stage, const int** out) {
    *out = nullptr;
    if (!active) return 0;
    if (memkind == PYIPM_MEM_HOST) {
        PYIPM_HIP(hipMemcpyAsync(stage, active, (size_t)ctx->batch * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
        *out = stage;
    } else *out = (const int*)active;
    return 0;
}
static int batch_solve_launch(Ctx* ctx, const BSolveIO& io) {
    const Geo& g = ctx->g;
    const int64_t rows = g.Npad + (ctx->b_any_cond ? TB : 0);        // (a condensed problem keeps its Ji-sided vector behind the sweep's rows)
    const dim3 grid((unsigned)ctx->batch, (unsigned)((io.k + BS_W - 1) / BS_W)), block(64 * BS_NW);
    const BatchPtrs bp = batch_ptrs(ctx);
    const BatchCond bc = batch_cond(ctx);
    if (rows <= 320)      hipLaunchKernelGGL((k_b_solve_many<320>), grid, block, 0, ctx->stream, bp, g, ctx->block_refine, io, bc, ctx->eps);
    else if (rows <= 576) hipLaunchKernelGGL((k_b_solve_many<576>), grid, block, 0, ctx->stream, bp, g, ctx->block_refine, io, bc, ctx->eps);
    else if (rows <= 832) hipLaunchKernelGGL((k_b_solve_many<832>), grid, block, 0, ctx->stream, bp, g, ctx->block_refine, io, bc, ctx->eps);
    else                  hipLaunchKernelGGL((k_b_solve_many<1088>), grid, block, 0, ctx->stream, bp, g, ctx->block_refine, io, bc, ctx->eps);
    PYIPM_KCHECK();
    return 0;
}
static int batch_matvec_launch(Ctx* ctx, const BMatvecIO& io) {
    const dim3 grid((unsigned)ctx->batch, (unsigned)((io.k + BMV_NC - 1) / BMV_NC));
    hipLaunchKernelGGL(k_b_kkt_matvec, grid, dim3(256), 0, ctx->stream, batch_ptrs(ctx), ctx->g, ctx->eps, io);
    PYIPM_KCHECK();
    return 0;
}
// k columns of every problem between caller memory (leading dimension ld, batch stride) and a packed device block ([B][k][N])
static int batch_cols_copy(Ctx* ctx, double* dst, const double* src, int64_t k, int64_t ld, int64_t stride, bool to_device,
                           const int32_t* active_host) {
    const size_t N = (size_t)ctx->g.N;
    for (int b = 0; b < ctx->batch; ++b) {
        if (active_host && !active_host[b]) continue;
        if (to_device)
            PYIPM_HIP(hipMemcpy2DAsync(dst + (size_t)b * (size_t)k * N, N * sizeof(double), src + (size_t)b * (size_t)stride, (size_t)ld * sizeof(double),
                                       N * sizeof(double), (size_t)k, hipMemcpyHostToDevice, ctx->stream));
        else
            PYIPM_HIP(hipMemcpy2DAsync(dst + (size_t)b * (size_t)stride, (size_t)ld * sizeof(double), src + (size_t)b * (size_t)k * N, N * sizeof(double),
                                       N * sizeof(double), (size_t)k, hipMemcpyDeviceToHost, ctx->stream));
    }
    return 0;
}

int pyipm_newton_solve_batched(pyipm_newton_ctx* h, int64_t k, const double* rhs, int64_t ld_rhs, int64_t stride_rhs,
                               double* x, int64_t ld_x, int64_t stride_x, const int32_t* active, int flip, int refine, int memkind) try {
    PYIPM_ENTER("solve_batched", G_BATCHED | G_DEVICE) const Geo& g = ctx->g;
    if (k < 0) { ctx->err = "solve_batched: k < 0"; return PYIPM_E_BADARG; }
    if (refine < 0) { ctx->err = "solve_batched: refine < 0 (no adaptive counts on a batched handle: a column's bits never depend on its neighbours)"; return PYIPM_E_BADARG; }
    if (memkind != PYIPM_MEM_DEVICE && memkind != PYIPM_MEM_HOST) { ctx->err = "solve_batched: bad memkind"; return PYIPM_E_BADARG; }
    if (k == 0) return PYIPM_OK;
    if (k > 65535) { ctx->err = "solve_batched: k > 65535"; return PYIPM_E_BADARG; }
    if (!ctx->held.batch_stepped) { ctx->err = "solve_batched: no step yet (the factors are a step's)"; return PYIPM_E_BADARG; }
    if (!rhs || !x) { ctx->err = "solve_batched: null right-hand side or output"; return PYIPM_E_BADARG; }
    if (ld_rhs < g.N || ld_x < g.N) { ctx->err = "solve_batched: leading dimension below N"; return PYIPM_E_BADARG; }
    const size_t B = (size_t)ctx->batch, blk = B * (size_t)k * (size_t)g.N;
    const bool host = memkind == PYIPM_MEM_HOST;
    // device pointers: x may BE rhs (same ld and stride -- a refined solve then keeps a copy of the right-hand sides for its
    // residuals); any other overlap of the two blocks is refused
    bool inplace = false;
    if (!host) {
        const double* r1 = rhs + (B - 1) * (size_t)stride_rhs + (size_t)(k - 1) * (size_t)ld_rhs + (size_t)g.N;
        const double* x1 = x + (B - 1) * (size_t)stride_x + (size_t)(k - 1) * (size_t)ld_x + (size_t)g.N;
        inplace = rhs == x && ld_rhs == ld_x && stride_rhs == stride_x;
        if (!inplace && rhs < x1 && x < r1) { ctx->err = "solve_batched: x overlaps rhs (it may only BE rhs, with the same ld and stride)"; return PYIPM_E_BADARG; }
    }
    const bool keep_b = inplace && refine > 0;
    int* mstage; double* buf;
    { int rc = batch_solve_scratch(ctx, (host ? 2 * blk : 0) + (refine ? blk : 0) + (keep_b ? blk : 0), &mstage, &buf); if (rc) return rc; }
    const int* act;
    { int rc = batch_mask(ctx, active, memkind, mstage, &act); if (rc) return rc; }
    const int64_t kN = k * g.N;
    BSolveIO io = {rhs, ld_rhs, stride_rhs, x, ld_x, stride_x, k, act, ctx->b_form.get(), flip ? 1 : 0};
    double* r = buf;                                      // the residual of a refinement step, solved in place
    if (host) {
        double* rd = buf; double* xd = buf + blk; r = buf + 2 * blk;
        { int rc = batch_cols_copy(ctx, rd, rhs, k, ld_rhs, stride_rhs, true, active); if (rc) return rc; }
        io.rhs = rd; io.ld_rhs = g.N; io.stride_rhs = kN; io.x = xd; io.ld_x = g.N; io.stride_x = kN;
    }
    const dim3 gcols((unsigned)B, (unsigned)k, (unsigned)((g.N + 255) / 256));
    const double* bsub = io.rhs; int64_t ld_b = io.ld_rhs, stride_b = io.stride_rhs;     // B of the residuals
    if (keep_b) {
        double* keep = buf + blk;
        hipLaunchKernelGGL(k_b_copy_cols, gcols, dim3(256), 0, ctx->stream, keep, rhs, ld_rhs, stride_rhs, g.N);
        PYIPM_KCHECK();
        bsub = keep; ld_b = g.N; stride_b = kN;
    }
    // refinement works on the raw solution: the flip of the multiplier rows is the last thing done to x
    const int flip_last = io.flip;
    if (refine) io.flip = 0;
    { int rc = batch_solve_launch(ctx, io); if (rc) return rc; }
    for (int it = 0; it < refine; ++it) {
        // R = B - Hc X from the blocks;  X += solve(R)
        const BMatvecIO mv = {io.x, io.ld_x, io.stride_x, r, g.N, kN, bsub, ld_b, stride_b, k, act};
        { int rc = batch_matvec_launch(ctx, mv); if (rc) return rc; }
        const BSolveIO cor = {r, g.N, kN, r, g.N, kN, k, act, ctx->b_form.get(), 0};
        { int rc = batch_solve_launch(ctx, cor); if (rc) return rc; }
        hipLaunchKernelGGL(k_b_add_cols, gcols, dim3(256), 0, ctx->stream,
                           io.x, io.ld_x, io.stride_x, r, g.N, kN, g.N, act, it + 1 == refine ? flip_last : 0, g.n + g.mi);
        PYIPM_KCHECK();
    }
    if (host) {
        { int rc = batch_cols_copy(ctx, x, io.x, k, ld_x, stride_x, false, active); if (rc) return rc; }
        PYIPM_HIP(hipStreamSynchronize(ctx->stream));
    }
    return PYIPM_OK;
} PYIPM_CATCH_H(h)

int pyipm_newton_kkt_matvec_batched(pyipm_newton_ctx* h, int64_t k, const double* v, int64_t ld_v, int64_t stride_v,
                                    double* y, int64_t ld_y, int64_t stride_y, int memkind) try {
    PYIPM_ENTER("kkt_matvec_batched", G_BATCHED | G_DEVICE) const Geo& g = ctx->g;
    if (k < 0) { ctx->err = "kkt_matvec_batched: k < 0"; return PYIPM_E_BADARG; }
    if (memkind != PYIPM_MEM_DEVICE && memkind != PYIPM_MEM_HOST) { ctx->err = "kkt_matvec_batched: bad memkind"; return PYIPM_E_BADARG; }
    if (k == 0) return PYIPM_OK;
    if (k > 65535) { ctx->err = "kkt_matvec_batched: k > 65535"; return PYIPM_E_BADARG; }
    if (!ctx->held.have_blocks || !ctx->held.have_vectors || !ctx->held.batch_stepped) {
        ctx->err = "kkt_matvec_batched: stage blocks and vectors and take a step first (the step supplies the shifts)"; return PYIPM_E_BADARG; }
    if (!v || !y) { ctx->err = "kkt_matvec_batched: null v or y"; return PYIPM_E_BADARG; }
    if (ld_v < g.N || ld_y < g.N) { ctx->err = "kkt_matvec_batched: leading dimension below N"; return PYIPM_E_BADARG; }
    const size_t B = (size_t)ctx->batch, blk = B * (size_t)k * (size_t)g.N;
    const bool host = memkind == PYIPM_MEM_HOST;
    const int64_t kN = k * g.N;
    BMatvecIO io = {v, ld_v, stride_v, y, ld_y, stride_y, nullptr, 0, 0, k, nullptr};
    if (host) {
        int* mstage; double* buf;
        { int rc = batch_solve_scratch(ctx, 2 * blk, &mstage, &buf); if (rc) return rc; }
        { int rc = batch_cols_copy(ctx, buf, v, k, ld_v, stride_v, true, nullptr); if (rc) return rc; }
        io.v = buf; io.ld_v = g.N; io.stride_v = kN; io.y = buf + blk; io.ld_y = g.N; io.stride_y = kN;
    }
    { int rc = batch_matvec_launch(ctx, io); if (rc) return rc; }
    if (host) {
        { int rc = batch_cols_copy(ctx, y, io.y, k, ld_y, stride_y, false, nullptr); if (rc) return rc; }
        PYIPM_HIP(hipStreamSynchronize(ctx->stream));
    }
    return PYIPM_OK;
} PYIPM_CATCH_H(h)

// The quantities of pyipm_newton_rcond for every problem, the iterations of the whole batch in lockstep: every launch below
// takes all problems through one step of theirs, nothing comes back to the host in between.
int pyipm_newton_rcond_batched(pyipm_newton_ctx* h, int it_inv, int it_pow, const int32_t* active, double* out, int memkind) try {
    PYIPM_ENTER("rcond_batched", G_BATCHED | G_DEVICE) const Geo& g = ctx->g;
    if (!out) { ctx->err = "rcond_batched: null output"; return PYIPM_E_BADARG; }
    if (it_inv < 0 || it_pow < 0) { ctx->err = "rcond_batched: negative (adaptive) iteration counts are not part of the batched estimate"; return PYIPM_E_BADARG; }
    if (memkind != PYIPM_MEM_DEVICE && memkind != PYIPM_MEM_HOST) { ctx->err = "rcond_batched: bad memkind"; return PYIPM_E_BADARG; }
    if (!ctx->held.have_blocks || !ctx->held.have_vectors || !ctx->held.batch_stepped) {
        ctx->err = "rcond_batched: stage blocks and vectors and take a step first"; return PYIPM_E_BADARG; }
    if (ctx->held.cond_active) {
        ctx->err = "rcond_batched: the last step was condensed -- the estimate works on the factor of the full form only"; return PYIPM_E_BADARG; }
    if (it_inv < 1) it_inv = 3;
    if (it_pow < 1) it_pow = 6;
    const int B = ctx->batch;
    const size_t BN = (size_t)B * (size_t)g.N;
    int* mstage; double* buf;
    { int rc = batch_solve_scratch(ctx, 2 * BN + 9 * (size_t)B, &mstage, &buf); if (rc) return rc; }
    const int* act;
    { int rc = batch_mask(ctx, active, memkind, mstage, &act); if (rc) return rc; }
    double *wa = buf, *wb = buf + BN, *est = buf + 2 * BN, *alive = est + 2 * B, *res = alive + B;    // est: [2][B] (power, inverse); res: [B][4]
    double* fix = res + 4 * B;                               // [B]: the corrected min|w| estimate of the problems with static pivots
    int* mask2 = reinterpret_cast<int*>(fix + B);            // [B]: those problems
    const dim3 gstart((unsigned)B, (unsigned)((g.N + 255) / 256)), gwave((unsigned)((B + 3) / 4));
    for (int phase = 0; phase < 2; ++phase) {
        double* e = est + (size_t)phase * B;
        hipLaunchKernelGGL(k_b_rc_start, gstart, dim3(256), 0, ctx->stream, wb, e, alive, g.N, (unsigned long long)(17 + phase));
        PYIPM_KCHECK();
        hipLaunchKernelGGL(k_b_rc_norm, gwave, dim3(256), 0, ctx->stream, wb, wa, e, alive, act, g.N, B, 0);
        PYIPM_KCHECK();
        const int its = phase == 0 ? it_pow : it_inv;
        for (int it = 0; it < its; ++it) {
            if (phase == 0) {                                 // wb = Hc (v / |v|)
                const BMatvecIO mv = {wa, g.N, g.N, wb, g.N, g.N, nullptr, 0, 0, 1, act};
                int rc = batch_matvec_launch(ctx, mv); if (rc) return rc;
            } else {                                          // wb = inv(factored) (v / |v|)
                const BSolveIO io = {wa, g.N, g.N, wb, g.N, g.N, 1, act, ctx->b_form.get(), 0};
                int rc = batch_solve_launch(ctx, io); if (rc) return rc;
            }
            hipLaunchKernelGGL(k_b_rc_norm, gwave, dim3(256), 0, ctx->stream, wb, it + 1 < its ? wa : (double*)nullptr, e, alive, act, g.N, B, 1);
            PYIPM_KCHECK();
        }
    }
    {   // static pivots: the last inverse iterate (wb) taken back to the unperturbed matrix (k_b_rc_fix_begin, kernels_bsolve.hpp)
        hipLaunchKernelGGL(k_b_rc_fix_begin, grid1(B), dim3(256), 0, ctx->stream, mask2, fix, alive, act, ctx->b_form.get(), ctx->dstats, B);
        PYIPM_KCHECK();
        const BMatvecIO mv = {wa, g.N, g.N, wb, g.N, g.N, nullptr, 0, 0, 1, mask2};
        const BSolveIO sv = {wb, g.N, g.N, wb, g.N, g.N, 1, mask2, ctx->b_form.get(), 0};
        hipLaunchKernelGGL(k_b_rc_norm, gwave, dim3(256), 0, ctx->stream, wb, wa, fix, alive, mask2, g.N, B, 0);      // wa = x / |x|
        PYIPM_KCHECK();
        { int rc = batch_matvec_launch(ctx, mv); if (rc) return rc; }                                                 // wb = Hc wa
        { int rc = batch_solve_launch(ctx, sv); if (rc) return rc; }                                                  // wb = inv(factored) wb
        hipLaunchKernelGGL(k_b_rc_sub, gstart, dim3(256), 0, ctx->stream, wb, wa, mask2, g.N);                        // wb = x'
        PYIPM_KCHECK();
        hipLaunchKernelGGL(k_b_rc_norm, gwave, dim3(256), 0, ctx->stream, wb, wa, fix, alive, mask2, g.N, B, 0);      // wa = x' / |x'|
        PYIPM_KCHECK();
        { int rc = batch_matvec_launch(ctx, mv); if (rc) return rc; }
        hipLaunchKernelGGL(k_b_rc_norm, gwave, dim3(256), 0, ctx->stream, wb, (double*)nullptr, fix, alive, mask2, g.N, B, 1);   // fix = |Hc x'| / |x'|
        PYIPM_KCHECK();
    }
    double* dev = (memkind == PYIPM_MEM_DEVICE) ? out : res;
    hipLaunchKernelGGL(k_b_rc_finish, grid1(B), dim3(256), 0, ctx->stream, dev, est, est + B, fix, ctx->anorm, act, ctx->b_form.get(), B);
    PYIPM_KCHECK();
    if (memkind == PYIPM_MEM_HOST) {
        for (int b0 = 0; b0 < B;) {                           // only the rows of the problems that took part, run by run
            if (active && !active[b0]) { ++b0; continue; }
            int b1 = b0 + 1;
            while (b1 < B && (!active || active[b1])) ++b1;
            PYIPM_HIP(hipMemcpyAsync(out + 4 * (size_t)b0, res + 4 * (size_t)b0, (size_t)(b1 - b0) * 4 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
            b0 = b1;
        }
        PYIPM_HIP(hipStreamSynchronize(ctx->stream));
    }
    return PYIPM_OK;
} PYIPM_CATCH_H(h)

// Adaptive refinement of a batch of directions, every problem by the rule of drv::refine_loop(refine < 0) applied to it alone
// (refine_each_plan.hpp; kernels_brefine.hpp).  max_steps + 1 rounds are enqueued whatever the problems do: a problem that has
// stopped costs workgroups that return at once.
int pyipm_newton_refine_batched(pyipm_newton_ctx* h, double* dz, int64_t ld, int64_t stride, const int32_t* active, int flip,
                                double target, int max_steps, double* info, int memkind) try {
    PYIPM_ENTER("refine_batched", G_BATCHED | G_DEVICE) const Geo& g = ctx->g;
    if (memkind != PYIPM_MEM_DEVICE && memkind != PYIPM_MEM_HOST) { ctx->err = "refine_batched: bad memkind"; return PYIPM_E_BADARG; }
    if (!ctx->held.have_blocks || !ctx->held.have_vectors || !ctx->held.batch_stepped) {
        ctx->err = "refine_batched: no step since the blocks / vectors were staged (the factors, the shifts and the residual are a step's)"; return PYIPM_E_BADARG; }
    if (!dz || !info) { ctx->err = "refine_batched: null direction or info"; return PYIPM_E_BADARG; }
    if (ld < g.N || (ctx->batch > 1 && stride < g.N)) { ctx->err = "refine_batched: leading dimension / batch stride below N"; return PYIPM_E_BADARG; }
    if (!(target > 0.0)) target = ctx->refine_target;
    if (max_steps < 0) max_steps = ctx->refine_max;
    const int B = ctx->batch;
    const size_t BN = (size_t)B * (size_t)g.N;
    int* mstage; double* buf;
    { int rc = batch_solve_scratch(ctx, 2 * BN + 7 * (size_t)B, &mstage, &buf); if (rc) return rc; }
    const int* act;
    { int rc = batch_mask(ctx, active, memkind, mstage, &act); if (rc) return rc; }
    double* res = buf + 2 * BN;                              // [B][4]: info of a call with host output
    double* prev = res + 4 * (size_t)B;                      // [B]
    int* words = reinterpret_cast<int*>(prev + B);           // go [B], it [B]
    const bool host = memkind == PYIPM_MEM_HOST;
    const BRefine rf = {dz, stride, buf, buf + BN, words, words + B, prev, host ? res : info, max_steps, target};
    const BatchPtrs bp = batch_ptrs(ctx);
    const dim3 gadd((unsigned)B, (unsigned)((g.N + 255) / 256));
    if (host) PYIPM_HIP(hipMemsetAsync(res, 0xFF, 4 * (size_t)B * sizeof(double), ctx->stream));     // (a problem without a factor: NaN)
    hipLaunchKernelGGL(k_b_ref_begin, grid1(B), dim3(256), 0, ctx->stream, rf, act, ctx->b_form.get(), B);
    PYIPM_KCHECK();
    for (int round = 0; round <= max_steps; ++round) {
        if (flip) hipLaunchKernelGGL((k_b_ref_round<true>), dim3((unsigned)B), dim3(256), 0, ctx->stream, bp, g, ctx->eps, rf);
        else      hipLaunchKernelGGL((k_b_ref_round<false>), dim3((unsigned)B), dim3(256), 0, ctx->stream, bp, g, ctx->eps, rf);
        PYIPM_KCHECK();
        if (round == max_steps) break;                       // (a problem with max_steps steps behind it never goes on)
        const BSolveIO cor = {rf.r, g.N, g.N, rf.r, g.N, g.N, 1, rf.go, ctx->b_form.get(), 0};
        { int rc = batch_solve_launch(ctx, cor); if (rc) return rc; }
        hipLaunchKernelGGL(k_b_ref_add, gadd, dim3(256), 0, ctx->stream, rf, g.N, flip ? 1 : 0, g.n + g.mi);
        PYIPM_KCHECK();
    }
    if (host) {
        for (int b0 = 0; b0 < B;) {                           // only the rows of the problems that took part, run by run
            if (active && !active[b0]) { ++b0; continue; }
            int b1 = b0 + 1;
            while (b1 < B && (!active || active[b1])) ++b1;
            PYIPM_HIP(hipMemcpyAsync(info + 4 * (size_t)b0, res + 4 * (size_t)b0, (size_t)(b1 - b0) * 4 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
            b0 = b1;
        }
        PYIPM_HIP(hipStreamSynchronize(ctx->stream));
    }
    return PYIPM_OK;
} PYIPM_CATCH_H(h)

// Teardown is an order, not a list: stuck collectives aborted, every stream of the handle drained, the communicators gone --
// after that nothing on the device refers to what the handle owns, and ~Ctx may release its members in any order.
int pyipm_newton_destroy(pyipm_newton_ctx* h) try {
    PYIPM_ENTER("destroy", 0)
    hipSetDevice(ctx->device);
    dist_abort_broken(ctx);
    hipStreamSynchronize(ctx->stream);
    dist_sync(ctx);
    ctx->side.sync(); ctx->fwd.sync(); ctx->rest.sync();
    dist_comm_destroy(ctx);
    delete ctx;
    return PYIPM_OK;
} PYIPM_CATCH_H(h)

int pyipm_newton_set_stream(pyipm_newton_ctx* h, void* stream) try {
    PYIPM_ENTER("set_stream", 0)
    if (ctx->stream != (hipStream_t)stream) {                // (what the old stream still runs is not ordered before the new one)
        PYIPM_HIP(hipSetDevice(ctx->device));
        const int rc = storage_whole(ctx); if (rc) return rc;
    }
    ctx->stream = (hipStream_t)stream;
    return PYIPM_OK;
} PYIPM_CATCH_H(h)

const char* pyipm_newton_last_error(pyipm_newton_ctx* h) {
    Ctx* ctx;
    return enter(h, "last_error", 0, &ctx) ? "null handle" : ctx->err.c_str();
}

int pyipm_newton_geometry(pyipm_newton_ctx* h, int64_t out[8]) try {
    PYIPM_ENTER("geometry", 0) const Geo& g = ctx->g;
    if (!out) return PYIPM_E_BADARG;
    out[0] = g.N; out[1] = g.Npad; out[2] = g.nb; out[3] = g.npanels; out[4] = g.ncols_local;
    out[5] = g.world; out[6] = g.rank; out[7] = (int64_t)ctx->ws.capacity();
    return PYIPM_OK;
} PYIPM_CATCH_H(h)

int pyipm_newton_stage_blocks(pyipm_newton_ctx* h, const double* d2L, int64_t ld_d2L, const double* Je,
                              int64_t ld_Je, const double* Ji, int64_t ld_Ji, int memkind) try {
    PYIPM_ENTER("stage_blocks", G_SINGLE | G_DEVICE) const Geo& g = ctx->g;
    int rc;
    if (!d2L && ctx->provider_only) { ctx->d2L = nullptr; ctx->ld_d2L = g.n; }     // (a factored Hessian model: only the Jacobian products)
    else { rc = stage_block(ctx, d2L, g.n, g.n, ld_d2L, memkind, ctx->stg_d2L, &ctx->d2L, &ctx->ld_d2L); if (rc) return rc; }
    rc = stage_block(ctx, Je, g.me ? g.n : 0, g.me, ld_Je, memkind, ctx->stg_Je, &ctx->Je, &ctx->ld_Je); if (rc) return rc;
    rc = stage_block(ctx, Ji, g.mi ? g.n : 0, g.mi, ld_Ji, memkind, ctx->stg_Ji, &ctx->Ji, &ctx->ld_Ji); if (rc) return rc;
    ctx->held.blocks_staged();
    return PYIPM_OK;
} PYIPM_CATCH_H(h)

int pyipm_newton_stage_vectors(pyipm_newton_ctx* h, const double* df, const double* ce, const double* ci,
                               const double* s, const double* lda, double mu, double eps, int memkind) try {
    PYIPM_ENTER("stage_vectors", G_DEVICE) const Geo& g = ctx->g;
    int rc;
    if (ctx->held.partial()) { rc = storage_whole(ctx); if (rc) return rc; }      // (a pending partial assembly is completed from the vectors it was made of)
    const size_t B = (size_t)ctx->batch;          // batched handles: every vector is [batch][len], contiguous
    rc = put_vec(ctx, ctx->df, df, B * g.n, memkind); if (rc) return rc;
    rc = put_vec(ctx, ctx->ce, ce, B * g.me, memkind); if (rc) return rc;
    rc = put_vec(ctx, ctx->ci, ci, B * g.mi, memkind); if (rc) return rc;
    rc = put_vec(ctx, ctx->s, s, B * g.mi, memkind); if (rc) return rc;
    rc = put_vec(ctx, ctx->lda, lda, B * (g.me + g.mi), memkind); if (rc) return rc;
    ctx->mu = mu; ctx->eps = eps;
    ctx->held.vectors_staged();
    return PYIPM_OK;
} PYIPM_CATCH_H(h)

int pyipm_newton_residual(pyipm_newton_ctx* h, double* g_out, int memkind) try {
    PYIPM_ENTER("residual", G_SINGLE | G_DEVICE)
    int rc = residual_dev(ctx); if (rc) return rc;
    return copy_out(ctx, g_out, ctx->rhs, ctx->g.N, memkind);
} PYIPM_CATCH_H(h)

int pyipm_newton_assemble(pyipm_newton_ctx* h, double delta, double delta_c) try {
    PYIPM_ENTER("assemble", G_SINGLE | G_DEVICE)
    return assemble_planned(ctx, delta, delta_c);
} PYIPM_CATCH_H(h)

int pyipm_newton_factor(pyipm_newton_ctx* h, pyipm_factor_stats* stats) try {
    PYIPM_ENTER("factor", G_SINGLE | G_DEVICE)
    // a residual is pending (pyipm.py:1717 precedes :1718): let its forward substitution trail the
    // factorisation; solve(rhs = NULL) then only runs the block-diagonal and backward parts
    const bool fuse = ctx->fuse_forward && ctx->held.have_rhs && ctx->g.world == 1 && ctx->held.assembled;
    if (fuse) { int rc = solve_prepare(ctx, nullptr, PYIPM_MEM_DEVICE, true); if (rc) return rc; }
    int rc = factor_planned(ctx, stats, fuse);
    ctx->held.factor_returned(rc, fuse);
    return rc;
} PYIPM_CATCH_H(h)

int pyipm_newton_solve(pyipm_newton_ctx* h, const double* rhs, double* dz, int flip, int refine, int memkind) try {
    PYIPM_ENTER("solve", G_SINGLE | G_ONE_RANK | G_FACTORED | G_DEVICE) const Geo& g = ctx->g;
    if (!dz) { ctx->err = "solve: null output"; return PYIPM_E_BADARG; }
    PYIPM_HIP(hipEventRecord(ctx->ev[4], ctx->stream));
    const bool pending = ctx->held.forward_pending && rhs == nullptr;      // v0 already holds the forward-substituted residual
    ctx->held.borrowed(Held::V0 | Held::V1);                               // consumed (or overwritten) either way
    if (!pending) { int rc = solve_prepare(ctx, rhs, memkind); if (rc) return rc; }
    return solve_finish(ctx, kLocalOps, dz, flip, refine, memkind, pending);
} PYIPM_CATCH_H(h)

int pyipm_newton_kkt_matvec(pyipm_newton_ctx* h, const double* v, double* y, int memkind) try {
    PYIPM_ENTER("kkt_matvec", G_SINGLE | G_DEVICE)
    if (!v || !y) return PYIPM_E_BADARG;
    return kkt_matvec_io(ctx, kLocalOps, v, y, memkind);
} PYIPM_CATCH_H(h)

int pyipm_newton_kkt_matvec_many(pyipm_newton_ctx* h, int64_t k, const double* v, int64_t ld_v, double* y, int64_t ld_y,
                                 int memkind) try {
    PYIPM_ENTER("kkt_matvec_many", G_SINGLE | G_ONE_RANK) const Geo& g = ctx->g;
    if (k < 0) { ctx->err = "kkt_matvec_many: k < 0"; return PYIPM_E_BADARG; }
    if (memkind != PYIPM_MEM_DEVICE && memkind != PYIPM_MEM_HOST) { ctx->err = "kkt_matvec_many: bad memkind"; return PYIPM_E_BADARG; }
    if (k == 0) return PYIPM_OK;
    if (!ctx->held.have_blocks || !ctx->held.have_vectors) { ctx->err = "kkt_matvec_many: stage blocks and vectors first"; return PYIPM_E_BADARG; }
    if (!v || !y) { ctx->err = "kkt_matvec_many: null v or y"; return PYIPM_E_BADARG; }
    if (ld_v < g.N || ld_y < g.N) { ctx->err = "kkt_matvec_many: leading dimension below N"; return PYIPM_E_BADARG; }
    {   // the launch reads v while it writes y
        const double* v1 = v + (k - 1) * ld_v + g.N; const double* y1 = y + (k - 1) * ld_y + g.N;
        if ((uintptr_t)v < (uintptr_t)y1 && (uintptr_t)y < (uintptr_t)v1) { ctx->err = "kkt_matvec_many: y overlaps v"; return PYIPM_E_BADARG; }
    }
    PYIPM_HIP(hipSetDevice(ctx->device));
    return kkt_matvec_many(ctx, k, v, ld_v, y, ld_y, memkind);
} PYIPM_CATCH_H(h)

int pyipm_newton_solve_info(pyipm_newton_ctx* h, double out[4]) try {
    PYIPM_ENTER("solve_info", 0)
    if (!out) return PYIPM_E_BADARG;
    out[0] = (double)ctx->info_steps; out[1] = ctx->info_berr0; out[2] = ctx->info_berr; out[3] = (double)ctx->info_converged;
    return PYIPM_OK;
} PYIPM_CATCH_H(h)

int pyipm_newton_solve_many(pyipm_newton_ctx* h, int64_t k, const double* rhs, int64_t ld_rhs, double* dz, int64_t ld_dz,
                            int flip, int refine, int memkind) try {
    PYIPM_ENTER("solve_many", G_SINGLE | G_FACTOR_ABLE | G_ONE_RANK) const Geo& g = ctx->g;
    if (k < 0) { ctx->err = "solve_many: k < 0"; return PYIPM_E_BADARG; }
    if (k == 0) return PYIPM_OK;                             // (an empty sweep needs no factor)
    { int rc = need_factor(ctx, "solve_many"); if (rc) return rc; }
    if (!rhs || !dz) { ctx->err = "solve_many: null right-hand side or output"; return PYIPM_E_BADARG; }
    if (ld_rhs < g.N || ld_dz < g.N) { ctx->err = "solve_many: leading dimension below N"; return PYIPM_E_BADARG; }
    if (memkind != PYIPM_MEM_DEVICE && memkind != PYIPM_MEM_HOST) { ctx->err = "solve_many: bad memkind"; return PYIPM_E_BADARG; }
    PYIPM_HIP(hipSetDevice(ctx->device));
    return solve_many(ctx, k, rhs, ld_rhs, dz, ld_dz, flip, refine, memkind);
} PYIPM_CATCH_H(h)

// Restates the quantity reghess tests, rcond = min|w| / max|w| over the eigenvalues of Hc (pyipm.py:1379-1381), without
// an eigendecomposition: max|w| by power iteration on Hc applied from the blocks, min|w| by inverse iteration with
// the factor (each step one substitution sweep).  Few iterations suffice for a threshold test at eps: a singular
// direction dominates inv(Hc) by many orders of magnitude.
int pyipm_newton_rcond(pyipm_newton_ctx* h, int it_inv, int it_pow, double out[4]) try {
    PYIPM_ENTER("rcond", G_SINGLE | G_ONE_RANK | G_FACTORED | G_DEVICE) const Geo& g = ctx->g;
    if (!out) return PYIPM_E_BADARG;
    // it_inv / it_pow >= 1: that many iterations of each; 0 = the defaults of rounds 2-3 (3 and 6).  < 0 = ADAPTIVE (round 4): an estimate for a
    // THRESHOLD test does not need the converged value.  Power iteration stops when two successive estimates agree to 10 %
    // (at most 6); inverse iteration stops when converged likewise (at most 3) -- or as soon as even a pessimistic correction
    // of the running estimate cannot reach the threshold: from a random start one step already finds 1 / |w|_min to within
    // the start vector's component along that eigenvector (~1/sqrt(N)), so min|w| >= 1 / (64 sqrt(N) est_1) is safe; if
    // that is still far above eps max|w| (x 100), the matrix is not singular to working precision and the other two
    // substitution sweeps (2.6 ms each at N = 32768) change nothing.  Late in an interior-point run this estimate is taken at
    // every iterate (Sigma spreads the pivots by itself): 18 -> ~7 ms.
    const bool adaptive_inv = it_inv < 0, adaptive_pow = it_pow < 0;
    if (it_inv < 1) it_inv = 3;
    if (it_pow < 1) it_pow = 6;
    // work vectors: v3 (the adaptive refinement's spare iterate) and vc (free outside a condensed solve), so that v0 / v1 -- a
    // right-hand side already forward-substituted under the factorisation -- and v2, the last direction, survive: the solve
    // that follows starts at the backward sweep (1.3 ms at N = 32768, at every suspect iterate).  With the condensed system
    // the substitution itself goes through vc: v0 / v1 as before, the pending forward pass is redone (and the direction in v2,
    // which nothing here writes, has always been dropped with them).
    double* wa = ctx->held.cond_active ? ctx->v0 : ctx->v3;
    double* wb = ctx->held.cond_active ? ctx->v1 : ctx->vc;
    if (ctx->held.cond_active) ctx->held.borrowed(Held::V0 | Held::V1 | Held::V2);
    double ss[2], lmax = 0.0, linv = 0.0;
    int used_pow = 0, used_inv = 0;
    const bool trace = getenv("PYIPM_RCOND_TRACE") != nullptr;
    auto norm_of = [&](const double* v, double* nrm) -> int {
        hipLaunchKernelGGL(k_sumsq2, dim3(1), dim3(1024), 0, ctx->stream, ctx->partial, v, v, g.N);
        PYIPM_KCHECK();
        PYIPM_HIP(hipMemcpyAsync(ss, ctx->partial, 2 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        PYIPM_HIP(hipStreamSynchronize(ctx->stream));
        *nrm = sqrt(ss[0]);
        return 0;
    };
    // Warm start (round 5, adaptive mode only): late in an interior-point run this estimate is taken at EVERY iterate, on a matrix
    // that changes little from one iterate to the next -- and so do its extreme eigenvectors.  Starting each iteration from the
    // vector the previous estimate ended with (instead of a hashed one) the first two estimates already agree: two substitution
    // sweeps instead of three, two products instead of up to six (-5 ms per late iterate at N = 32768).  Any start vector with a
    // component along the extreme eigenvector is valid; the stopping rules are unchanged; a hashed start is taken whenever the
    // stored vector is missing, of another size, or not finite.  stage_blocks forgets it.
    const bool warm_ok = (adaptive_inv || adaptive_pow) && !ctx->held.cond_active && getenv("PYIPM_RCOND_COLD") == nullptr;
    if (warm_ok && ctx->rc_warm_buf.capacity() < 2 * (size_t)g.Npad) {      // (no memory: no warm start, asked for again next time)
        const bool got = ctx->rc_warm_buf.reserve(2 * (size_t)g.Npad) == hipSuccess;
        ctx->rc_warm[0] = ctx->rc_warm_buf; ctx->rc_warm[1] = got ? ctx->rc_warm[0] + g.Npad : nullptr;
        ctx->held.rc_warm_cold();
    }
    for (int phase = 0; phase < 2; ++phase) {
        const bool adaptive_phase = phase == 0 ? adaptive_pow : adaptive_inv;
        const bool warm = warm_ok && adaptive_phase && ctx->rc_warm[0] && ctx->held.rc_warm_valid[phase];
        // The start vector is hashed; a warm start ADDS the stored iterate to it, both normalised: the stored vector
        // has been through inverse (power) iterations on every earlier call, so along a direction that has only just become
        // (nearly) singular -- or a Sigma entry that has only just become dominant -- it holds rounding noise, and the stopping
        // rules below (two estimates agree; the pessimistic bound from the start vector's ~1/sqrt(N) component along every
        // eigenvector) would read the OLD extreme eigenvalue off it.  The hashed half keeps that component for every direction.
        hipLaunchKernelGGL(k_hash_vector, grid1(g.Npad), dim3(256), 0, ctx->stream, wb, g.N, g.Npad, (unsigned long long)(17 + phase));
        PYIPM_KCHECK();
        double nrm = 0.0, est = 0.0, prev_est = 0.0;
        int rc = norm_of(wb, &nrm); if (rc) return rc;
        if (warm && nrm > 0.0) {
            double wn = 0.0;
            rc = norm_of(ctx->rc_warm[phase], &wn); if (rc) return rc;
            if (wn > 0.0 && wn <= 1.0e300) {                             // (a stored vector that went bad is ignored)
                hipLaunchKernelGGL(k_axpby, grid1(g.Npad), dim3(256), 0, ctx->stream, wb, wb, ctx->rc_warm[phase], 1.0 / nrm, 1.0 / wn, g.Npad);
                PYIPM_KCHECK();
                rc = norm_of(wb, &nrm); if (rc) return rc;
            }
        }
        const int its = phase == 0 ? it_pow : it_inv;
        for (int it = 0; it < its; ++it) {
            if (!(nrm > 0.0) || !(nrm <= 1.0e300)) break;
            if (phase == 0) {
                hipLaunchKernelGGL(k_scale_copy, grid1(g.Npad), dim3(256), 0, ctx->stream, wa, wb, 1.0 / nrm, g.Npad); PYIPM_KCHECK();
                rc = kkt_matvec_dev(ctx, wa, wb); if (rc) return rc;          // v1 = Hc (v / |v|)
            } else {
                hipLaunchKernelGGL(k_scale_copy, grid1(g.Npad), dim3(256), 0, ctx->stream, wa, wb, 1.0 / nrm, g.Npad); PYIPM_KCHECK();
                rc = solve_inplace(ctx, wa); if (rc) return rc;                     // v0 = inv(factored) (v / |v|)
                PYIPM_HIP(hipMemcpyAsync(wb, wa, g.Npad * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
            }
            rc = norm_of(wb, &nrm); if (rc) return rc;
            prev_est = est; est = nrm;
            (phase == 0 ? used_pow : used_inv) = it + 1;
            if (trace) fprintf(stderr, "[pyipm rcond] %s iteration %d: %.6e\n", phase == 0 ? "power" : "inverse", it + 1, est);
            if (phase == 0 && adaptive_pow && it >= 1 && est <= 1.1 * prev_est) break;
            if (phase == 1 && adaptive_inv) {
                if (it >= 1 && est <= 1.1 * prev_est) break;
                // 1 / (pessimistic min|w|) = 64 sqrt(N) est; not singular by a factor 100:  that < 1 / (100 eps max|w|)
                const double pess = 64.0 * sqrt((double)g.N) * est;
                if (lmax > 0.0 && pess * (100.0 * 2.220446049250313e-16 * lmax) < 1.0) break;
            }
        }
        if (phase == 0) lmax = est; else linv = est;
        if (warm_ok && adaptive_phase && ctx->rc_warm[0]) {
            // keep the iterate (unnormalised: the next call normalises it) -- if it is finite
            const bool good = nrm > 0.0 && nrm <= 1.0e300;
            if (good) PYIPM_HIP(hipMemcpyAsync(ctx->rc_warm[phase], wb, g.Npad * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
            ctx->held.rc_warm_kept(phase, good);
        }
    }
    ctx->rcond_its[0] = used_pow; ctx->rcond_its[1] = used_inv;
    const double lmin = linv > 0.0 ? 1.0 / linv : 0.0;
    out[0] = lmin; out[1] = lmax; out[2] = (lmax > 0.0) ? lmin / lmax : 0.0;
    double an = 0.0;
    PYIPM_HIP(hipMemcpy(&an, ctx->anorm, sizeof(double), hipMemcpyDeviceToHost));
    out[3] = 1.4901161193847656e-08 * ((an > 0.0 && an <= 1.0e300) ? an : 1.0);      // magnitude of a static pivot
    return PYIPM_OK;
} PYIPM_CATCH_H(h)

int pyipm_newton_anorm(pyipm_newton_ctx* h, double** dev_ptr) try {
    PYIPM_ENTER("anorm", 0)
    if (!dev_ptr) return PYIPM_E_BADARG;
    *dev_ptr = reinterpret_cast<double*>(ctx->anorm);        // bits of a non-negative double ARE that double
    return PYIPM_OK;
} PYIPM_CATCH_H(h)

// ---- QP family: the derivative provider's products on the device ------------------------------
// The reference evaluates df = Q x + c, ce = A x - b, ci = G x - h and the Jacobian-transpose products of the KKT report
// through compiled Aesara functions on the host (pyipm.py:855-954).  For a QP the blocks are constant and already staged,
// so these are passes over the staged d2L (its UPPER triangle, as everywhere), Je and Ji.
static int block_products_dev(Ctx* ctx, const double* v, double* Qv, double* JeTv, double* JiTv);
int pyipm_newton_block_products(pyipm_newton_ctx* h, const double* v, double* Qv, double* JeTv, double* JiTv) try {
    PYIPM_ENTER("block_products", G_SINGLE | G_DEVICE)
    if (!v) return PYIPM_E_BADARG;
    return block_products_dev(ctx, v, Qv, JeTv, JiTv);
} PYIPM_CATCH_H(h)

static int block_products_dev(Ctx* ctx, const double* v, double* Qv, double* JeTv, double* JiTv) {
    const Geo& g = ctx->g;
    if (g.world != 1 || ctx->sharded) { ctx->err = "block_products: single-rank handles with fully staged blocks"; return PYIPM_E_BADARG; }
    if (!ctx->held.have_blocks) { ctx->err = "block_products: stage blocks first"; return PYIPM_E_BADARG; }
    if (Qv && !ctx->d2L) { ctx->err = "block_products: no d2L block staged on this provider-only handle (pass Qv = NULL)"; return PYIPM_E_BADARG; }
    const RowMap rm = make_rowmap(g, 0);
    const int64_t n = g.n, me = g.me, mi = g.mi;
    const int nchunk = 64;
    const int64_t rpc = (n + nchunk - 1) / nchunk;
    if (ctx->profile) PYIPM_HIP(hipEventRecord(ctx->ev_prov[0], ctx->stream));
    double bytes = 0.0;
    if (Qv) {            // sym(triu(d2L)) v: ONE pass over the upper triangle (round 4: was a row pass + a mirrored pass)
        int r2 = symv_dev(ctx, v, Qv, 0.0, rm); if (r2) return r2;
        bytes += 4.0 * (double)n * (double)n;
    }
    if (JeTv && me > 0) {
        hipLaunchKernelGGL(k_coldot_partial, dim3((unsigned)((me + 255) / 256), nchunk), dim3(256), 0, ctx->stream,
                           ctx->partial, ctx->Je, ctx->ld_Je, n, me, v, rpc, 0, rm);
        PYIPM_KCHECK();
        hipLaunchKernelGGL(k_coldot_reduce, grid1(me), dim3(256), 0, ctx->stream, JeTv, ctx->partial, me, nchunk, 0);
        PYIPM_KCHECK();
        bytes += 8.0 * (double)n * (double)me;
    }
    if (JiTv && mi > 0) {
        hipLaunchKernelGGL(k_coldot_partial, dim3((unsigned)((mi + 255) / 256), nchunk), dim3(256), 0, ctx->stream,
                           ctx->partial, ctx->Ji, ctx->ld_Ji, n, mi, v, rpc, 0, rm);
        PYIPM_KCHECK();
        hipLaunchKernelGGL(k_coldot_reduce, grid1(mi), dim3(256), 0, ctx->stream, JiTv, ctx->partial, mi, nchunk, 0);
        PYIPM_KCHECK();
        bytes += 8.0 * (double)n * (double)mi;
    }
    if (ctx->profile) { PYIPM_HIP(hipEventRecord(ctx->ev_prov[1], ctx->stream)); ctx->prov_valid[0] = true; }
    ctx->prov_bytes[0] = bytes;
    return PYIPM_OK;
}

// out (n) = Je le + Ji li  (either may be NULL): the Jacobian terms of dL/dx (pyipm.py:655-668)
int pyipm_newton_block_products_t(pyipm_newton_ctx* h, const double* le, const double* li, double* out) try {
    PYIPM_ENTER("block_products_t", G_SINGLE | G_DEVICE) const Geo& g = ctx->g;
    if (!out) return PYIPM_E_BADARG;
    if (g.world != 1 || ctx->sharded) { ctx->err = "block_products_t: single-rank handles with fully staged blocks"; return PYIPM_E_BADARG; }
    if (!ctx->held.have_blocks) { ctx->err = "block_products_t: stage blocks first"; return PYIPM_E_BADARG; }
    const int64_t me = le ? g.me : 0, mi = li ? g.mi : 0;
    if (ctx->profile) PYIPM_HIP(hipEventRecord(ctx->ev_prov[2], ctx->stream));
    hipLaunchKernelGGL(k_rowdot2, grid1(g.n, 4), dim3(256), 0, ctx->stream, out, (const double*)nullptr, g.n,
                       ctx->Je, ctx->ld_Je, le, me, ctx->Ji, ctx->ld_Ji, li, mi, 2, 0, make_rowmap(g, 0));
    PYIPM_KCHECK();
    if (ctx->profile) { PYIPM_HIP(hipEventRecord(ctx->ev_prov[3], ctx->stream)); ctx->prov_valid[1] = true; }
    ctx->prov_bytes[1] = 8.0 * (double)g.n * (double)(me + mi);
    return PYIPM_OK;
} PYIPM_CATCH_H(h)

// out[0] = ms of the last block_products call ("profile" = 1), out[1] = the bytes of the blocks it passed over,
// out[2], out[3] = the same for block_products_t
int pyipm_newton_provider_stats(pyipm_newton_ctx* h, double out[4]) try {
    PYIPM_ENTER("provider_stats", G_DEVICE)
    if (!out) return PYIPM_E_BADARG;
    PYIPM_HIP(hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < 2; ++k) {
        float ms = 0.f;
        if (ctx->prov_valid[k]) PYIPM_HIP(hipEventElapsedTime(&ms, ctx->ev_prov[2 * k], ctx->ev_prov[2 * k + 1]));
        out[2 * k] = ms; out[2 * k + 1] = ctx->prov_bytes[k];
    }
    return PYIPM_OK;
} PYIPM_CATCH_H(h)

// The fused step.  While the staged blocks, delta and delta_c stay what they were it keeps the factor of the x-block groups
// (prefix_mode: full, recording or reusing).
static int step_fused(Ctx* ctx, double delta, double delta_c, int refine, double* dz, pyipm_factor_stats* stats, int memkind) {
    int rc = residual_dev(ctx); if (rc) return rc;
    rc = assemble_planned(ctx, delta, delta_c); if (rc) return rc;
    const bool fuse = ctx->fuse_forward != 0;
    if (fuse) { rc = solve_prepare(ctx, nullptr, memkind, true); if (rc) return rc; }     // v0 = v1 = g before factoring
    rc = factor_planned(ctx, stats, fuse);
    ctx->held.factor_returned(rc, false);                    // (the solve below consumes the fused pass at once)
    if (rc) return rc;
    PYIPM_HIP(hipEventRecord(ctx->ev[4], ctx->stream));
    if (!fuse) { rc = solve_prepare(ctx, nullptr, memkind); if (rc) return rc; }
    return solve_finish(ctx, kLocalOps, dz, 1, refine, memkind, fuse && ctx->held.forward_fused);
}

int pyipm_newton_step(pyipm_newton_ctx* h, double delta, double delta_c, int refine, double* dz,
                      pyipm_factor_stats* stats, int memkind) try {
    PYIPM_ENTER("step", G_SINGLE | G_DEVICE)
    if (!dz) { ctx->err = "step: null output"; return PYIPM_E_BADARG; }
    const int rc = step_fused(ctx, delta, delta_c, refine, dz, stats, memkind);
    if (rc) ctx->held.prefix_dropped();                      // a failed step: the next one runs in full
    return rc;
} PYIPM_CATCH_H(h)

int pyipm_newton_reuse_info(pyipm_newton_ctx* h, int64_t out[4]) try {
    PYIPM_ENTER("reuse_info", 0)
    if (!out) return PYIPM_E_BADARG;
    out[0] = ctx->n_reused; out[1] = ctx->n_recorded; out[2] = (int64_t)((ctx->snap.capacity() + ctx->snap_e.capacity()) * sizeof(double)); out[3] = ctx->last_step_kind;
    return PYIPM_OK;
} PYIPM_CATCH_H(h)

int pyipm_newton_step_lengths(pyipm_newton_ctx* h, double tau, const double* dz_in, double* alpha_s, double* alpha_l) try {
    PYIPM_ENTER("step_lengths", G_SINGLE | G_DEVICE) const Geo& g = ctx->g;
    if (!alpha_s || !alpha_l) return PYIPM_E_BADARG;
    *alpha_s = 1.0; *alpha_l = 1.0;
    if (g.mi == 0) return PYIPM_OK;
    if (!ctx->held.have_vectors || (!dz_in && !ctx->held.have_direction)) { ctx->err = "step_lengths: stage vectors and solve first (or pass dz)"; return PYIPM_E_BADARG; }
    // v2 holds the last direction in the reference's order with the multiplier block already sign-flipped
    const double* dz = dz_in ? dz_in : ctx->v2;
    hipLaunchKernelGGL(k_step_lengths, dim3(1), dim3(256), 0, ctx->stream, ctx->partial, ctx->s, ctx->lda + g.me,
                       dz + g.n, dz + g.n + g.mi + g.me, g.mi, tau);
    PYIPM_KCHECK();
    double out[2];
    PYIPM_HIP(hipMemcpyAsync(out, ctx->partial, 2 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    PYIPM_HIP(hipStreamSynchronize(ctx->stream));
    *alpha_s = out[0]; *alpha_l = out[1];
    return PYIPM_OK;
} PYIPM_CATCH_H(h)

// ---- merit-function pieces of the line search (kernels_merit.hpp) -----------------------------
static int merit_scratch(Ctx* ctx) {
    if (ctx->merit_buf) return 0;
    // [partials | info out (MERIT_NQ) | gq (2) | dots (8) | alphas (MERIT_MAXK) | ray out (MERIT_MAXK)]
    PYIPM_HIP(ctx->merit_buf.reserve((size_t)(MERIT_NB * MERIT_NQ + MERIT_NQ + 2 + 8 + 2 * 1024)));
    return 0;
}
static const double* merit_direction(Ctx* ctx, const double* dz, const char* who) {
    if (dz) return dz;
    if (!ctx->held.have_direction) { ctx->err = std::string(who) + ": no direction (solve with flip first, or pass dz)"; return nullptr; }
    return ctx->v2;
}

// out[16] for the STAGED point (stage_vectors) and the direction dz (device, reference order, multipliers flipped; NULL = the
// last solve's; a handle without one: the direction entries come back as NaN):
//   [0] ||ce||_1  [1] ||ci - s||_1  [2] df.dx  [3] sum ds/(s+eps)  [4] sum log s
//   [5..8] the KKT report |dL/dx|, |s (lda_i - mu/(s+eps))|, |ce|, |ci - s| (2-norms; from g = -grad: NaN before residual())
//   [9] sum s lda_i  [10] min s lda_i  [11] |dx|_2  [12] |ds|_2
int pyipm_newton_merit_info(pyipm_newton_ctx* h, const double* dz, double* out) try {
    PYIPM_ENTER("merit_info", G_SINGLE | G_DEVICE) const Geo& g = ctx->g;
    if (!out) return PYIPM_E_BADARG;
    if (g.world != 1) { ctx->err = "merit_info: single-rank handles"; return PYIPM_E_BADARG; }
    if (!ctx->held.have_vectors) { ctx->err = "merit_info: stage vectors first"; return PYIPM_E_BADARG; }
    int rc = merit_scratch(ctx); if (rc) return rc;
    const double* d = dz ? dz : (ctx->held.have_direction ? ctx->v2 : nullptr);
    const double* gres = ctx->held.have_rhs ? ctx->rhs : nullptr;
    double* part = ctx->merit_buf; double* res = part + MERIT_NB * MERIT_NQ;
    hipLaunchKernelGGL(k_merit_info, dim3(MERIT_NB), dim3(256), 0, ctx->stream, part, g, ctx->df, ctx->ce, ctx->ci, ctx->s,
                       ctx->lda, d, gres, ctx->eps);
    PYIPM_KCHECK();
    hipLaunchKernelGGL(k_merit_info_final, dim3(1), dim3(64), 0, ctx->stream, res, part, MERIT_NB);
    PYIPM_KCHECK();
    double q[MERIT_NQ];
    PYIPM_HIP(hipMemcpyAsync(q, res, sizeof(q), hipMemcpyDeviceToHost, ctx->stream));
    PYIPM_HIP(hipStreamSynchronize(ctx->stream));
    const double nan = __builtin_nan("");
    for (int k = 0; k < MERIT_NQ; ++k) out[k] = q[k];
    for (int k = 5; k <= 8; ++k) out[k] = sqrt(q[k]);
    out[11] = sqrt(q[11]); out[12] = sqrt(q[12]);
    if (!d) { out[2] = out[3] = out[11] = out[12] = nan; }
    if (!gres) { out[5] = out[6] = nan; }
    if (g.mi == 0) out[10] = nan;
    return PYIPM_OK;
} PYIPM_CATCH_H(h)

// out[p] = a_p . b_p, count <= 8 pairs of device vectors (host array of device pointers); fixed summation order.
int pyipm_newton_dots(pyipm_newton_ctx* h, int count, const double* const* a, const double* const* b, const int64_t* len,
                      double* out) try {
    PYIPM_ENTER("dots", G_DEVICE)
    if (!a || !b || !len || !out || count < 1 || count > 8) return PYIPM_E_BADARG;
    int rc = merit_scratch(ctx); if (rc) return rc;
    DotPairs dp; memset(&dp, 0, sizeof(dp));
    for (int p = 0; p < count; ++p) { dp.a[p] = a[p]; dp.b[p] = b[p]; dp.len[p] = len[p]; if ((!a[p] || !b[p]) && len[p] > 0) return PYIPM_E_BADARG; }
    double* dev = ctx->merit_buf + MERIT_NB * MERIT_NQ + MERIT_NQ + 2;
    hipLaunchKernelGGL(k_dots, dim3((unsigned)count), dim3(1024), 0, ctx->stream, dev, dp);
    PYIPM_KCHECK();
    PYIPM_HIP(hipMemcpyAsync(out, dev, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    PYIPM_HIP(hipStreamSynchronize(ctx->stream));
    return PYIPM_OK;
} PYIPM_CATCH_H(h)

// QP family (the staged blocks are the constant Q, A', G'): phi(x + a dx, s + a ds) - phi(x, s) for K candidates a at once
// (k_merit_ray).  The products Q dx, Je' dx, Ji' dx and the two dot products are formed once per direction and kept until the
// next solve / stage_vectors.  quad: NULL = dx' d2L dx from the staged block, else *quad (a caller whose Q is not staged).
int pyipm_newton_merit_ray(pyipm_newton_ctx* h, const double* dz, double nu, double mu, const double* quad,
                           const double* alphas, int K, double* out) try {
    PYIPM_ENTER("merit_ray", G_SINGLE | G_DEVICE) const Geo& g = ctx->g;
    if (!alphas || !out || K < 1 || K > 1024) return PYIPM_E_BADARG;
    if (g.world != 1 || ctx->sharded) { ctx->err = "merit_ray: single-rank handles with fully staged blocks"; return PYIPM_E_BADARG; }
    if (!ctx->held.have_vectors || !ctx->held.have_blocks) { ctx->err = "merit_ray: stage blocks and vectors first"; return PYIPM_E_BADARG; }
    const double* d = merit_direction(ctx, dz, "merit_ray"); if (!d) return PYIPM_E_BADARG;
    if (!quad && !ctx->d2L) { ctx->err = "merit_ray: no d2L block staged (pass quad = dx' Q dx)"; return PYIPM_E_BADARG; }
    int rc = merit_scratch(ctx); if (rc) return rc;
    const size_t need = (size_t)(g.n + g.me + g.mi + 8);
    if (ctx->ray_buf.capacity() < need) { ctx->ray_for = nullptr; PYIPM_HIP(ctx->ray_buf.reserve(need)); }
    double* qd = ctx->ray_buf; double* dce = qd + g.n; double* dci = dce + g.me;
    double* gq = ctx->merit_buf + MERIT_NB * MERIT_NQ + MERIT_NQ;
    double* dal = gq + 2 + 8; double* dout = dal + 1024;
    if (ctx->ray_for != d || !ctx->held.ray_valid) {
        rc = block_products_dev(ctx, d, quad ? nullptr : qd, g.me ? dce : nullptr, g.mi ? dci : nullptr); if (rc) return rc;
        DotPairs dp; memset(&dp, 0, sizeof(dp));
        dp.a[0] = ctx->df; dp.b[0] = d; dp.len[0] = g.n;
        dp.a[1] = d; dp.b[1] = qd; dp.len[1] = quad ? 0 : g.n;
        hipLaunchKernelGGL(k_dots, dim3(2), dim3(1024), 0, ctx->stream, gq, dp);
        PYIPM_KCHECK();
        ctx->ray_for = d; ctx->held.ray_formed(); ctx->ray_quad_given = quad != nullptr;
    }
    if (quad) PYIPM_HIP(hipMemcpyAsync(gq + 1, quad, sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    else if (ctx->ray_quad_given) { ctx->held.ray_dropped(); ctx->err = "merit_ray: quad given for this direction before, missing now"; return PYIPM_E_BADARG; }
    PYIPM_HIP(hipMemcpyAsync(dal, alphas, (size_t)K * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_merit_ray, dim3((unsigned)K), dim3(256), 0, ctx->stream, dout, dal, g, gq, ctx->ce, dce, ctx->ci, dci,
                       ctx->s, d + g.n, nu, mu);
    PYIPM_KCHECK();
    PYIPM_HIP(hipMemcpyAsync(out, dout, (size_t)K * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    PYIPM_HIP(hipStreamSynchronize(ctx->stream));
    return PYIPM_OK;
} PYIPM_CATCH_H(h)

// ---- per-panel phases -----------------------------------------------------------------------------
int pyipm_newton_factor_begin(pyipm_newton_ctx* h) try {
    PYIPM_ENTER("factor_begin", G_SINGLE | G_DEVICE | G_STORAGE)
    if (!ctx->held.assembled) { ctx->err = "factor_begin: assemble first"; return PYIPM_E_BADARG; }
    if (ctx->held.cond_active) { ctx->err = "per-panel phases do not apply to the condensed system; use factor()"; return PYIPM_E_BADARG; }
    ctx->sched.clear();                                 // per-panel phases: uniform group map, dense panels
    ctx->held.panel_phases_begun();
    return factor_begin(ctx);
} PYIPM_CATCH_H(h)
int pyipm_newton_factor_end(pyipm_newton_ctx* h, pyipm_factor_stats* stats) try {
    PYIPM_ENTER("factor_end", G_SINGLE | G_DEVICE)
    ctx->held.factor_enqueued();
    return factor_end(ctx, stats);
} PYIPM_CATCH_H(h)
int pyipm_newton_factor_panel(pyipm_newton_ctx* h, int64_t p) try {
    PYIPM_ENTER("factor_panel", G_SINGLE | G_DEVICE | G_STORAGE)
    return factor_panel(ctx, p, ctx->stream, false);
} PYIPM_CATCH_H(h)
int pyipm_newton_trailing_update(pyipm_newton_ctx* h, int64_t p) try {
    PYIPM_ENTER("trailing_update", G_SINGLE | G_DEVICE | G_STORAGE)
    if (p < 0 || p >= ctx->g.npanels) return PYIPM_E_BADARG;
    return trailing_update(ctx, p);
} PYIPM_CATCH_H(h)

int pyipm_newton_trailing_update_range(pyipm_newton_ctx* h, int64_t p, int64_t first, int64_t count) try {
    PYIPM_ENTER("trailing_update_range", G_SINGLE | G_DEVICE | G_STORAGE)
    const Geo& g = ctx->g;
    if (p < 0 || p >= g.npanels || first <= p || count < 0) return PYIPM_E_BADARG;
    if (g.panel_c0(p) + g.panel_w(p) >= g.Npad) return PYIPM_OK;
    // locally owned panels inside [first, first+count)
    int64_t q = first;
    while (q < g.npanels && g.owner(q) != g.rank) ++q;
    int64_t last = first + count; if (last > g.npanels) last = g.npanels;
    if (q >= last) return PYIPM_OK;
    int64_t n_lp = 0;
    for (int64_t qq = q; qq < last; qq += g.world) ++n_lp;
    return timed_update(ctx, p, 1, q / g.world, n_lp);
} PYIPM_CATCH_H(h)

// message = [ W rows below the panel (m x nbw, column-major, ld = m) | nbw/64 tile inverses | nbw/64 tiles | nbw/64 flags ]
size_t pyipm_newton_panel_msg_bytes(pyipm_newton_ctx* h, int64_t p) try {
    Ctx* ctx; if (enter(h, "panel_msg_bytes", 0, &ctx)) return 0;
    const Geo& g = ctx->g;
    if (p < 0 || p >= g.npanels) return 0;
    if (panel_in_s(ctx, p)) return 0;                    // slack-block panel: every rank derives what it needs locally
    int64_t h0, h1;
    panel_hole(ctx, p, &h0, &h1);
    const int64_t nbw = g.panel_w(p), m = g.Npad - (g.panel_c0(p) + nbw) - (h1 - h0);    // slack rows of an x panel stay home
    return (size_t)(m * nbw + 2 * (nbw / TB) * TB * TB + nbw / TB) * sizeof(double);
} PYIPM_CATCH_SIZE

int pyipm_newton_panel_pack(pyipm_newton_ctx* h, int64_t p, double* buf) try {
    PYIPM_ENTER("panel_pack", G_SINGLE | G_DEVICE | G_STORAGE) const Geo& g = ctx->g;
    if (!buf) return PYIPM_E_BADARG;
    if (p < 0 || p >= g.npanels || g.owner(p) != g.rank) { ctx->err = "panel_pack: not the owner"; return PYIPM_E_BADARG; }
    int64_t h0, h1;
    panel_hole(ctx, p, &h0, &h1);
    const int64_t nbw = g.panel_w(p), c1 = g.panel_c0(p) + nbw, m = g.Npad - c1 - (h1 - h0);
    // rows [c1, Npad) without [h0, h1): one or two strided copies into a message of leading dimension m
    const int64_t seg0 = (h1 > h0) ? h0 - c1 : g.Npad - c1, seg1 = (h1 > h0) ? g.Npad - h1 : 0;
    if (seg0 > 0)
        PYIPM_HIP(hipMemcpy2DAsync(buf, (size_t)m * sizeof(double), wbuf(ctx, p) + c1, (size_t)g.Npad * sizeof(double),
                                   (size_t)seg0 * sizeof(double), (size_t)nbw, hipMemcpyDeviceToDevice, ctx->stream));
    if (seg1 > 0)
        PYIPM_HIP(hipMemcpy2DAsync(buf + seg0, (size_t)m * sizeof(double), wbuf(ctx, p) + h1, (size_t)g.Npad * sizeof(double),
                                   (size_t)seg1 * sizeof(double), (size_t)nbw, hipMemcpyDeviceToDevice, ctx->stream));
    const size_t tbytes = (size_t)(nbw / TB) * TB * TB * sizeof(double);
    PYIPM_HIP(hipMemcpyAsync(buf + m * nbw, ctx->Dinv + (g.panel_c0(p) / TB) * (int64_t)(TB * TB), tbytes,
                             hipMemcpyDeviceToDevice, ctx->stream));
    PYIPM_HIP(hipMemcpyAsync(buf + m * nbw + (nbw / TB) * TB * TB, ctx->Tsv + (g.panel_c0(p) / TB) * (int64_t)(TB * TB),
                             tbytes, hipMemcpyDeviceToDevice, ctx->stream));
    PYIPM_HIP(hipMemcpyAsync(buf + m * nbw + 2 * (nbw / TB) * TB * TB, ctx->Tflag + g.panel_c0(p) / TB,
                             (size_t)(nbw / TB) * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    return PYIPM_OK;
} PYIPM_CATCH_H(h)

int pyipm_newton_panel_unpack(pyipm_newton_ctx* h, int64_t p, const double* buf) try {
    PYIPM_ENTER("panel_unpack", G_SINGLE | G_DEVICE | G_STORAGE) const Geo& g = ctx->g;
    if (!buf) return PYIPM_E_BADARG;
    if (p < 0 || p >= g.npanels || g.owner(p) == g.rank) { ctx->err = "panel_unpack: owner does not unpack"; return PYIPM_E_BADARG; }
    { int rc = unpack_panel_from(ctx, p, buf, 0, /*with_tiles=*/true, ctx->stream); if (rc) return rc; }
    return PYIPM_OK;
} PYIPM_CATCH_H(h)

int pyipm_newton_fwd_panel(pyipm_newton_ctx* h, int64_t p, double* v) try {
    PYIPM_ENTER("fwd_panel", G_SINGLE | G_DEVICE)
    if (!v) return PYIPM_E_BADARG;
    if (p < 0 || p >= ctx->g.npanels || ctx->g.owner(p) != ctx->g.rank) return PYIPM_E_BADARG;
    return fwd_panel(ctx, p, v);
} PYIPM_CATCH_H(h)
int pyipm_newton_diag_panel(pyipm_newton_ctx* h, int64_t p, double* v) try {
    PYIPM_ENTER("diag_panel", G_SINGLE | G_DEVICE)
    if (!v) return PYIPM_E_BADARG;
    if (p < 0 || p >= ctx->g.npanels) return PYIPM_E_BADARG;
    return diag_panel(ctx, p, v);
} PYIPM_CATCH_H(h)
int pyipm_newton_bwd_panel(pyipm_newton_ctx* h, int64_t p, double* v) try {
    PYIPM_ENTER("bwd_panel", G_SINGLE | G_DEVICE)
    if (!v) return PYIPM_E_BADARG;
    if (p < 0 || p >= ctx->g.npanels || ctx->g.owner(p) != ctx->g.rank) return PYIPM_E_BADARG;
    return bwd_panel(ctx, p, v);
} PYIPM_CATCH_H(h)

// ---- introspection --------------------------------------------------------------------------------
int pyipm_newton_kkt_storage(pyipm_newton_ctx* h, double** ptr, int64_t* ld, int64_t* ncols) try {
    PYIPM_ENTER("kkt_storage", G_DEVICE | G_STORAGE)
    if (ptr) { *ptr = ctx->A; ctx->held.storage_handed_out(); }
    if (ld) *ld = ctx->held.cond_active ? ctx->gc.Npad : ctx->g.Npad;
    if (ncols) *ncols = ctx->held.cond_active ? ctx->gc.ncols_local : ctx->g.ncols_local;
    return PYIPM_OK;
} PYIPM_CATCH_H(h)

int pyipm_newton_last_timings(pyipm_newton_ctx* h, double out[8]) try {
    PYIPM_ENTER("last_timings", G_DEVICE)
    if (!out) return PYIPM_E_BADARG;
    PYIPM_HIP(hipStreamSynchronize(ctx->stream));          // timers are resolved lazily, never inside a step
    if (ctx->batched) {                                    // step_batched: [0] residual + assembly, [6] factorisation, [3] substitutions, [1] whole step
        for (int k = 0; k < 8; ++k) out[k] = 0.0;
        if (ctx->held.ev_assemble_valid) {
            float a = 0.f, f = 0.f, sv = 0.f, all = 0.f;
            PYIPM_HIP(hipEventElapsedTime(&a, ctx->ev[0], ctx->ev[2])); PYIPM_HIP(hipEventElapsedTime(&f, ctx->ev[2], ctx->ev[3]));
            PYIPM_HIP(hipEventElapsedTime(&sv, ctx->ev[3], ctx->ev[1])); PYIPM_HIP(hipEventElapsedTime(&all, ctx->ev[0], ctx->ev[1]));
            out[0] = a; out[6] = f; out[3] = sv; out[1] = all;
        }
        return PYIPM_OK;
    }
    if (ctx->held.ev_assemble_valid) { float ms = 0.f; PYIPM_HIP(hipEventElapsedTime(&ms, ctx->ev[2], ctx->ev[3])); ctx->t_assemble = ms; }
    if (ctx->held.ev_solve_valid) { float ms = 0.f; PYIPM_HIP(hipEventElapsedTime(&ms, ctx->ev[4], ctx->ev[5])); ctx->t_solve = ms; }
    out[0] = ctx->t_assemble; out[1] = ctx->t_panel; out[2] = ctx->t_trailing; out[3] = ctx->t_solve;
    out[4] = (double)(ctx->n_trailing_real > 0 ? ctx->n_trailing_real : ctx->n_trailing); out[5] = ctx->trailing_flops; out[6] = ctx->t_factor;
    out[7] = ctx->held.cond_active ? ctx->t_gram : ctx->trailing_area;   // full system: entries updated by the trailing launches
    return PYIPM_OK;
} PYIPM_CATCH_H(h)

int pyipm_newton_trailing_instances(pyipm_newton_ctx* h, double out[8]) try {
    PYIPM_ENTER("trailing_instances", 0)
    if (!out) return PYIPM_E_BADARG;
    for (int k = 0; k < 2; ++k) {
        out[4 * k + 0] = (double)ctx->inst_n[k]; out[4 * k + 1] = ctx->inst_ms[k];
        out[4 * k + 2] = ctx->inst_flops[k]; out[4 * k + 3] = ctx->inst_area[k];
    }
    return PYIPM_OK;
} PYIPM_CATCH_H(h)

// The bulk launches' algorithmic bytes in both definitions (rounds must stay comparable):
// out[k] = C tiles only (16 B per updated entry: read once, written once), out[2 + k] = C tiles + the two operand panels read once
// (what trailing_instances reports); k = 0: 128 x 128 tiles, k = 1: 128 x 256.  Sums over the launches of the last factorisation.
int pyipm_newton_trailing_bytes(pyipm_newton_ctx* h, double out[4]) try {
    PYIPM_ENTER("trailing_bytes", 0)
    if (!out) return PYIPM_E_BADARG;
    for (int k = 0; k < 2; ++k) { out[k] = ctx->inst_cbytes[k]; out[2 + k] = ctx->inst_area[k]; }
    return PYIPM_OK;
} PYIPM_CATCH_H(h)

int pyipm_newton_set_option(pyipm_newton_ctx* h, const char* name, double value) try {
    PYIPM_ENTER("set_option", G_DEVICE | G_STORAGE)          // (any option may change the schedule or the numbers)
    if (!name) return PYIPM_E_BADARG;
    if (!strcmp(name, "expert")) { ctx->expert = (int)value != 0; return PYIPM_OK; }
    {   // expert switches (include/pyipm_newton.h): measurement knobs, test hooks, parked experiments
        static const char* const kExpert[] = {
            "tail_group", "group_chain", "tile_step", "tile_waves", "bc_per_problem", "chain_cpy", "chain_whole", "chain_lds_kb",
            "sweep_max_blocks", "debug_fault", "debug_timeline_ptr", "debug_chain_ptr"};
        bool is_expert = false;
        for (const char* e : kExpert) if (!strcmp(name, e)) { is_expert = true; break; }
        if (is_expert && !ctx->expert) {
            const char* env = getenv("PYIPM_EXPERT");
            if (!(env && env[0] && env[0] != '0')) {
                ctx->err = std::string("option ") + name + " is an expert switch: set PYIPM_EXPERT=1 or set_option(\"expert\", 1) first";
                return PYIPM_E_BADARG;
            }
        }
    }
    if (!strcmp(name, "pivtol_rel")) { ctx->pivtol_rel = value; return PYIPM_OK; }
    if (!strcmp(name, "reserve_cus")) { ctx->reserve_cus = (int)value; return PYIPM_OK; }
    if (!strcmp(name, "persist_rows")) { ctx->persist_rows = (int64_t)value; return PYIPM_OK; }
    if (!strcmp(name, "bulk_bn")) { ctx->bulk_bn = (int)value == 256 ? 256 : 128; return PYIPM_OK; }
    if (!strcmp(name, "tile_blocked")) { ctx->tile_blocked = (int)value != 0; ctx->tile_blocked_user = true; return PYIPM_OK; }
    if (!strcmp(name, "tile_waves")) {              // 4 | 8 (eight waves where a whole CU is to be had: first group, last 12288 rows) | 9 (eight waves everywhere: tests)
        const int v = (int)value; ctx->tile_waves = v >= 8 ? 8 : 4; ctx->tile8_rows = v == 9 ? ((int64_t)1 << 40) : 12288; return PYIPM_OK; }
    if (!strcmp(name, "bc_per_problem")) { ctx->bc_per_problem = (int)value != 0; return PYIPM_OK; }
    if (!strcmp(name, "tile_chain")) { int v = (int)value; ctx->tile_chain = v < 0 ? 0 : (v > 2 ? 2 : v); return PYIPM_OK; }
    if (!strcmp(name, "debug_chain_ptr")) {         // diagnostics (tools/chain_clock.py): device buffer of 64 x CHAIN_DBG_WORDS u64, one region per chain launch from now on
        ctx->chain_dbg = (unsigned long long*)(uintptr_t)(unsigned long long)value; ctx->chain_dbg_launch = 0; return PYIPM_OK; }
    if (!strcmp(name, "chain_lds_kb")) { int v = (int)value; ctx->chain_lds_kb = v < 0 ? 0 : (v > 110 ? 110 : v); return PYIPM_OK; }
    if (!strcmp(name, "chain_whole")) { ctx->chain_whole = (int)value != 0; return PYIPM_OK; }
    if (!strcmp(name, "chain_cpy")) { int v = (int)value; ctx->chain_cpy = v < 1 ? 1 : (v > 32 ? 32 : v); return PYIPM_OK; }
    if (!strcmp(name, "profile")) { ctx->profile = (int)value; return PYIPM_OK; }
    if (!strcmp(name, "debug_fault")) { ctx->debug_fault = (int)value; return PYIPM_OK; }
    if (!strcmp(name, "refine_target")) { ctx->refine_target = value; return PYIPM_OK; }
    if (!strcmp(name, "refine_max")) { ctx->refine_max = (int)value < 0 ? 0 : (int)value; return PYIPM_OK; }
    if (!strcmp(name, "refine_cond")) { ctx->refine_cond = value; return PYIPM_OK; }
    if (!strcmp(name, "block_refine")) { int v = (int)value; ctx->block_refine = v < 0 ? 0 : (v > 3 ? 3 : v); return PYIPM_OK; }
    if (!strcmp(name, "condensed")) {
        ctx->condensed = (int)value;                          // (several ranks: full blocks on every rank, see assemble)
        // (until round 6 this also rewrote a batched handle's tile_blocked -- 1 with the condensed form, 0 with the full one -- and so
        //  discarded an explicit choice; the blocked inversion is the default of both forms now)
        return PYIPM_OK; }
    if (!strcmp(name, "condensed_sigma_max")) { ctx->cond_sigma_max = value; return PYIPM_OK; }
    if (!strcmp(name, "condensed_refine")) { ctx->cond_min_refine = (int)value < 0 ? 0 : (int)value; return PYIPM_OK; }
    if (!strcmp(name, "lookahead")) { ctx->lookahead = (int)value < 0 ? 0 : ((int)value > 2 ? 2 : (int)value); return PYIPM_OK; }
    if (!strcmp(name, "group")) {           // may only shrink below the create-time value (workspace is sized for it)
        int v = (int)value; if (v < 1 || v > default_group(ctx->g.world, ctx->g.nb)) { ctx->err = "group out of range"; return PYIPM_E_BADARG; }
        ctx->group = v; return PYIPM_OK; }
    if (!strcmp(name, "skip_zeros")) { ctx->skip_zeros = (int)value != 0; return PYIPM_OK; }
    if (!strcmp(name, "tail_group")) { ctx->tail_group = (int)value; ctx->tail_group_user = true; return PYIPM_OK; }
    { bool handled = false; int rc = dist_set_option(ctx, name, value, &handled); if (handled) return rc; }
    if (!strcmp(name, "tile_step")) { ctx->tile_step = (int)value != 0; return PYIPM_OK; }
    if (!strcmp(name, "group_chain")) { ctx->group_chain = (int)value != 0; return PYIPM_OK; }
    if (!strcmp(name, "keep_zeros")) { ctx->keep_zeros = (int)value != 0; ctx->held.keep_zeros_set(); return PYIPM_OK; }
    if (!strcmp(name, "wide_sub")) { ctx->wide_sub = (int)value; return PYIPM_OK; }
    if (!strcmp(name, "sweep_persist")) { ctx->sweep_persist = (int)value; return PYIPM_OK; }
    if (!strcmp(name, "sweep_max_blocks")) { ctx->sweep_max_blocks = (int)value; return PYIPM_OK; }
    if (!strcmp(name, "fuse_forward")) { ctx->fuse_forward = (int)value; return PYIPM_OK; }
    if (!strcmp(name, "debug_timeline_ptr")) {      // diagnostics: device buffer of 8 x u64 per block (pointer passed as double-encoded integer halves is lossy; use set via low 52 bits)
        ctx->dbg_buf = (unsigned long long*)(uintptr_t)(unsigned long long)value; return PYIPM_OK; }
    ctx->err = std::string("unknown option ") + name;
    return PYIPM_E_BADARG;
} PYIPM_CATCH_H(h)

int pyipm_newton_abi_version(void) { return PYIPM_NEWTON_ABI_VERSION; }

int pyipm_mfma_f64_peak(int device, int iters, double* tflops) try {
    if (!tflops || iters <= 0) return PYIPM_E_BADARG;
    if (hipSetDevice(device) != hipSuccess) return PYIPM_E_NODEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return PYIPM_E_HIP;
    DevBuf<double> d;
    if (d.reserve(8) != hipSuccess) return PYIPM_E_NOMEM;
    const int blocks = prop.multiProcessorCount * 2;        // 8 waves per CU = 2 per SIMD
    Event e0, e1;
    if (e0.ensure(hipEventDefault) != hipSuccess || e1.ensure(hipEventDefault) != hipSuccess) return PYIPM_E_HIP;
    hipLaunchKernelGGL(k_mfma_peak, dim3(blocks), dim3(256), 0, 0, d, 16);   // warm-up
    hipEventRecord(e0, 0);
    hipLaunchKernelGGL(k_mfma_peak, dim3(blocks), dim3(256), 0, 0, d, iters);
    hipEventRecord(e1, 0);
    hipEventSynchronize(e1);
    float ms = 0.f; hipEventElapsedTime(&ms, e0, e1);
    const double flops = (double)blocks * 4.0 /*waves*/ * (double)iters * 32.0 * 2.0 * 16 * 16 * 4;
    *tflops = flops / (ms * 1e-3) / 1e12;
    return hipGetLastError() == hipSuccess ? PYIPM_OK : PYIPM_E_HIP;
} PYIPM_CATCH_NOH

}  // extern "C"

#pragma GCC visibility pop

// (The distributed driver -- pyipm_dist.hip / dist_impl.hpp -- and the L-BFGS direction -- pyipm_lbfgs.hip / lbfgs_impl.hpp -- are
//  translation units of their own since round 6: what they share with this file is declared in driver.hpp.)
