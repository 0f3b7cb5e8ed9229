// driver.hpp -- what the translation units of the library share (round 6: pyipm_newton.hip = the single-rank driver and the
// C-ABI of include/pyipm_newton.h, pyipm_dist.hip = the distributed driver, pyipm_lbfgs.hip = include/pyipm_lbfgs.h).  Host
// functions only: a kernel is launched from the unit that defines it (the two launch_* wrappers below).
#pragma once
#include "ctx.hpp"
#include <algorithm>
#include <functional>
#include <chrono>

namespace pyipm { namespace drv {

// An exception unwinds out of the middle of a schedule: kernels may still be running on the helper streams against
// storage the next call will overwrite.  Drain them and drop the half-done state before reporting.
inline void quiesce_noexcept(Ctx* c) noexcept {
    if (!c) return;
    try {
        if (c->side) hipStreamSynchronize(c->side);
        if (c->fwd) hipStreamSynchronize(c->fwd);
        if (c->rest) hipStreamSynchronize(c->rest);
        if (c->dist) hipDeviceSynchronize();            // the distributed driver's own streams
        if (c->stream) hipStreamSynchronize(c->stream); else hipDeviceSynchronize();
        c->held.quiesced();
    } catch (...) {}
}
#define PYIPM_SETERR_NEWTON(msg_) (quiesce_noexcept(reinterpret_cast<Ctx*>(h)), set_err_noexcept(reinterpret_cast<Ctx*>(h), (msg_)))
#define PYIPM_CATCH_H(h_)  PYIPM_CATCH_CORE(PYIPM_SETERR_NEWTON, PYIPM_E_NOMEM, PYIPM_E_HIP)


// The entry guard: every extern "C" entry that takes a handle starts with it.  `need` says what the entry requires of the handle;
// the checks run in the order of the bits, the entry's own argument checks follow, and the texts of the refusals live here.
enum : unsigned {
    G_SINGLE = 1,        // refuses a batched handle
    G_BATCHED = 2,       // requires one
    G_FACTOR_ABLE = 4,   // not a provider-only handle
    G_ONE_RANK = 8,      // world == 1
    G_FACTORED = 16,     // a factor is in the storage
    G_DEVICE = 32,       // makes the handle's device current (a refusal costs no HIP call)
    G_STORAGE = 64,      // the entry looks at the KKT storage as a matrix, writes into it or changes what a pending factorisation was
                         // planned with: an assembly that kept the x-block prefix is completed first, the prefix dropped (with G_DEVICE)
};
int storage_whole(Ctx* ctx);        // pyipm_newton.hip
inline int need_factor(Ctx* ctx, const char* name) {
    if (ctx->held.factored) return 0;
    ctx->err = std::string(name) + ": factor first"; return PYIPM_E_BADARG;
}
inline int enter(pyipm_newton_ctx* h, const char* name, unsigned need, Ctx** out) {
    Ctx* ctx = *out = reinterpret_cast<Ctx*>(h);
    if (!ctx) return PYIPM_E_BADARG;
    if ((need & G_SINGLE) && ctx->batched) { ctx->err = "batched handle: only stage_*_batched / stage_vectors / step_batched apply"; return PYIPM_E_BADARG; }
    if ((need & G_BATCHED) && !ctx->batched) { ctx->err = std::string(name) + ": not a batched handle"; return PYIPM_E_BADARG; }
    if ((need & G_FACTOR_ABLE) && ctx->provider_only) { ctx->err = std::string(name) + ": a provider-only handle has no factor"; return PYIPM_E_BADARG; }
    if ((need & G_ONE_RANK) && ctx->g.world != 1) { ctx->err = std::string(name) + "(): single-rank entry point"; return PYIPM_E_BADARG; }
    if (need & G_FACTORED) { int rc = need_factor(ctx, name); if (rc) return rc; }
    if (need & G_DEVICE) PYIPM_HIP(hipSetDevice(ctx->device));
    if (need & G_STORAGE) return storage_whole(ctx);
    return 0;
}
#define PYIPM_ENTER(name_, need_)  Ctx* ctx; { const int rc_ = enter(h, name_, need_, &ctx); if (rc_) return rc_; }
inline dim3 grid1(int64_t n, int b = 256) { return dim3((unsigned)((n + b - 1) / b)); }
// -W columns of panel p: the buffer of its group (parity-alternating) + its offset inside the group
inline double* wbuf(Ctx* ctx, int64_t p) {
    const int64_t G = ctx->group;
    return ctx->Wbuf + ((ctx->sched.group_of(p, G) % 3) * G + ctx->sched.offset_of(p, G)) * ctx->g.Npad * (int64_t)ctx->g.nb;
}

int put_vec(Ctx* ctx, double* dst, const double* src, size_t count, int memkind);
int copy_out(Ctx* ctx, double* dst, const double* src_dev, size_t count, int memkind);
int stage_block(Ctx* ctx, const double* src, int64_t rows, int64_t cols, int64_t ld, int memkind,
                DevBuf<double>& stg, const double** out_ptr, int64_t* out_ld);
void active_ranges(const Ctx* ctx, int64_t cA, int64_t cB, int64_t* a0, int64_t* a1, int64_t* b0, int64_t* b1);
bool panel_in_s(const Ctx* ctx, int64_t p);
void panel_hole(const Ctx* ctx, int64_t p, int64_t* h0, int64_t* h1);
// What a call of launch_update128 may set beside its operands (designated initialisers, in this order).
struct UpdLaunch {
    bool bulk = true;            // tile-list order, bulk instances; false: a panel-chain launch (plain grid, raised wave priority)
    int64_t ldw = 0;             // leading dimension of Wop;   0: the KKT storage's (Npad)
    int64_t row_end = 0;         // rows [row_begin, row_end);  0: Npad
    int64_t col_end = 0;         // columns below col_end;      0: Npad (the Gram launch of the condensed option narrows it)
    int64_t src_c0 = -1;         // >= 0: global column of the first source column (tiles its active ranges leave at zero are skipped)
    int ksplit = 1;              // split-K: grid.y splits of K columns each, split y accumulating into C + y * ks_cstride
    int64_t ks_cstride = 0;
    int waves = 0;               // waves per block; 0: BULK_WAVES
    int sub0 = 0, nct_sub = 0;   // nct_sub > 0: only column tiles [sub0, sub0 + nct_sub) of local panel first_lp
                                 // (128 wide; the sub-panels of a wide panel, factor_block)
    int* used_bn = nullptr;      // out: the tile width of the instance that ran (64 / 128 / 256)
    int prio = -1;               // >= 0: wave priority flag of the launch whatever `bulk` says
    const unsigned* tiles = nullptr;   // the caller's own tile list on the device (row tile | column tile << 16, 0xffffffff = none,
    unsigned ntiles = 0;               // ntiles a multiple of 8): only these 128 x 128 tiles, whole column range (first_lp = sub0 = 0)
};
int launch_update128(Ctx* ctx, hipStream_t stream, const double* Lop, int64_t ldl, const double* Wop, int K,
                     int64_t row_begin, int64_t first_lp, int64_t n_lp, const UpdLaunch& o = {});
struct UpdTimed {
    hipStream_t stream = nullptr;   // nullptr: the handle's
    bool as_bulk = false;           // a bulk launch (instance, trailing figures) although it runs on another stream
};
int timed_update(Ctx* ctx, int64_t p0, int64_t np, int64_t first_lp, int64_t n_lp, const UpdTimed& o = {});
int factor_panel(Ctx* ctx, int64_t p, hipStream_t stream, bool apply_pending = false);
int fwd_panel(Ctx* ctx, int64_t p, double* v, hipStream_t stream = nullptr, int nrhs = 1, int64_t vstride = 0);
int diag_panel(Ctx* ctx, int64_t p, double* v, hipStream_t stream = nullptr, int nrhs = 1, int64_t vstride = 0);
int bwd_panel(Ctx* ctx, int64_t p, double* v, int nrhs = 1, int64_t vstride = 0, double* part = nullptr, int64_t pstride = 0);
int factor_begin(Ctx* ctx, hipStream_t st = nullptr);
int solve_inplace(Ctx* ctx, double* v, bool forward_done = false);
int solve_plain(Ctx* ctx, double* v, bool forward_done, int nrhs = 1, int64_t vstride = 0, double* part = nullptr,
                int64_t pstride = 0);
// V := M^{-1} V for kpad columns at stride ldv (kernels_msolve.hpp); kpad and the doubles of `part` from solve_many_sizes
int solve_many_plain(Ctx* ctx, double* V, int64_t ldv, int64_t kpad, double* part);
void solve_many_sizes(int64_t Npad, int64_t k, int64_t* kpad, size_t* part_doubles);
int ensure_rest_stream(Ctx* ctx);
bool panel_is_wide(const Ctx* ctx, int64_t p);
bool panel_piecewise_ok(const Ctx* ctx, int64_t p);
int panel_chain(Ctx* ctx, int64_t p, hipStream_t stream, int64_t xrows = 0, const unsigned* xword = nullptr, unsigned xwant = 0);
bool chain_extra_ok(const Ctx* ctx, int64_t p, int64_t xrows);
int panel_rows(Ctx* ctx, int64_t p, int64_t r0, int64_t r1, hipStream_t stream);
size_t slice_numel(const Geo& g, int64_t p, int j);
int pack_slice(Ctx* ctx, int64_t p, int j, double* buf, hipStream_t st);
int unpack_slice(Ctx* ctx, int64_t p, int j, const double* buf, const double* tiles, double* EL, hipStream_t st);
int unpack_slice_tiles(Ctx* ctx, int64_t p, const double* tiles, hipStream_t st);
int unpack_panel_from(Ctx* ctx, int64_t p, const double* buf, int64_t row_from, bool with_tiles, hipStream_t st);
int factor_end(Ctx* ctx, pyipm_factor_stats* stats);
int factor_dispatch(Ctx* ctx, pyipm_factor_stats* stats, bool fuse_forward, int px = 0);   // px: factor_all (pyipm_newton_step alone passes one)
int cond_reduce(Ctx* ctx, const double* b, double* vc);
int cond_expand(Ctx* ctx, const double* vc, double* v);
int kkt_matvec_dev(Ctx* ctx, const double* v, double* y);
int residual_dev(Ctx* ctx);
int solve_prepare(Ctx* ctx, const double* rhs, int memkind, bool for_fused_forward = false);
// pyipm_dist.hip
void dist_abort_broken(Ctx* ctx);      // teardown (pyipm_newton_destroy), in this order: the communicators of a handle whose step
void dist_sync(Ctx* ctx);              // timed out aborted, or the synchronisations never return;  the driver's streams drained;
void dist_comm_destroy(Ctx* ctx);      // the communicators destroyed.  The state itself goes with the handle (Ctx::dist).
int dist_set_option(Ctx* ctx, const char* name, double value, bool* handled);
// kernels of pyipm_newton.hip on behalf of the other units
int launch_mask_owned(Ctx* ctx, hipStream_t st, double* v, const double* b);
int launch_inpanel_update(Ctx* ctx, hipStream_t st, dim3 grid, double* Cm, int64_t ldc, int64_t ccol, const double* Lop, int64_t ldl,
                          const double* Wop, int64_t ldw, int64_t cglob, int K, int64_t row_begin, int64_t row_end,
                          int64_t a0, int64_t a1, int64_t b0, int64_t b1, int prio);

// The two operations a solve is written in; the single-rank and the distributed driver each bring theirs (pyipm_newton.hip).
struct SolveOps {
    int (*solve)(Ctx*, const double* b, double* x, bool forward_done);   // x := Hc^{-1} b.  x holds a copy of b on entry (b may BE x) -- or, with
                                                                         // forward_done, the driver's own vector holds b's forward pass already
    int (*matvec)(Ctx*, const double* v, double* y);                     // y := Hc v, from the blocks
    bool ray_survives;                                                   // Held::solved
};
int assemble_timed(Ctx* ctx, double delta, double delta_c);
int solve_finish(Ctx* ctx, const SolveOps& ops, double* dz, int flip, int refine, int memkind, bool forward_done);
int kkt_matvec_io(Ctx* ctx, const SolveOps& ops, const double* v, double* y, int memkind);

// Iterative refinement of a solve: the host-side state machine of solve_finish and solve_many.
// refine >= 0: that many steps of   r = b - Hc x ;  x += Hc^{-1} r   (Hc applied from the blocks, not from the factor).
// refine <  0: adaptive -- measure |r|/|b| before every step and stop at refine_target, after refine_max steps or
//              when a step gains less than 4x; a step that made it worse (or NaN) is taken back.  This is what turns the
//              factor of a statically pivoted (perturbed) matrix into the solution of the UNperturbed system; the host
//              reads the outcome with solve_info (the info_* fields).
// The caller's kernels, buffers and streams (each callback returns a PYIPM code):  residual() enqueues r = b - Hc x;
// berr(&e) gives |r|/|b| as a host double (several columns: the worst, NaN if any is);  save() / restore() copy x to / from
// the spare iterate;  correct() enqueues x += Hc^{-1} r.
inline int refine_steps(const Ctx* ctx, int refine) {      // a condensed solve gets at least cond_min_refine steps against the FULL blocks
    return (ctx->held.cond_active && refine >= 0 && refine < ctx->cond_min_refine) ? ctx->cond_min_refine : refine;
}
template <class Residual, class Berr, class Save, class Restore, class Correct>
int refine_loop(Ctx* ctx, int refine, Residual residual, Berr berr_of, Save save, Restore restore, Correct correct) {
    refine = refine_steps(ctx, refine);
    ctx->info_steps = 0; ctx->info_converged = 0; ctx->info_berr0 = -1.0; ctx->info_berr = -1.0;
    const bool adaptive = refine < 0;
    const int maxit = adaptive ? ctx->refine_max : refine;
    double prev = -1.0;
    for (int it = 0; it <= maxit; ++it) {
        if (!adaptive && it == maxit) break;
        int rc = residual(); if (rc) return rc;
        if (adaptive) {
            double berr = 0.0;
            rc = berr_of(&berr); if (rc) return rc;
            if (it == 0) ctx->info_berr0 = berr;
            ctx->info_berr = berr;
            if (prev >= 0.0 && !(berr <= prev)) {                             // the last step made it worse (or NaN): take it back
                rc = restore(); if (rc) return rc;
                ctx->info_berr = prev; ctx->info_steps = it - 1;
                break;
            }
            if (!(berr <= 1.0e300)) break;                                    // NaN / Inf: nothing to refine
            if (berr <= ctx->refine_target) { ctx->info_converged = 1; break; }
            if (it == maxit || (prev >= 0.0 && berr > 0.25 * prev)) break;    // out of budget / stagnating
            prev = berr;
            rc = save(); if (rc) return rc;                                   // the iterate this error belongs to
        }
        rc = correct(); if (rc) return rc;
        ctx->info_steps = it + 1;
    }
    return 0;
}

} }  // namespace pyipm::drv
