// qn_impl.hpp — the quasi-Newton KKT operator of the last L-BFGS direction: product, kept-state solve, backward error and
// refinement (include/pyipm_newton.h, pyipm_qn_*).  Included behind lbfgs_impl.hpp: everything works from what
// pyipm_lbfgs_direction left in the handle (LbCtx::qn_valid) and on vectors of its own, so that a direction after these
// calls returns the bits it would without them.  Column 0 of V, P and R is the right-hand side being solved: a solve
// overwrites it, the operator needs columns 1.. only.
#pragma once
#include "lbfgs_impl.hpp"

namespace {

int qn_enter(LbCtx* lb, const char* name) {
    if (lb->mb > 0) { lb->err = std::string(name) + ": not supported on a bounded handle (K would need the bound block)"; return PYIPM_E_BADARG; }
    if (lb->p == 0) { lb->err = std::string(name) + ": no constraints -- the unconstrained direction is an explicit formula, there is no system"; return PYIPM_E_BADARG; }
    if (lb->allreduce) { lb->err = std::string(name) + ": a row-sharded handle (all-reduce callback installed) is not supported"; return PYIPM_E_BADARG; }
    if (!lb->qn_valid) { lb->err = std::string(name) + ": no direction since the handle was created or the Jacobians were staged"; return PYIPM_E_BADARG; }
    LB_HIP(hipSetDevice(lb->device));
    return 0;
}

// a caller's vector of the SOLUTION space (multiplier rows negated when flip) into / out of a work vector
int qn_get(LbCtx* lb, double* dst, const double* src, int flip, int memkind) {
    int rc = lb_put(lb, dst, src, (size_t)lb->N, memkind); if (rc) return rc;
    if (flip) {
        hipLaunchKernelGGL(k_qn_copy_flip, grid1(lb->N), dim3(256), 0, lb->stream, dst, dst, lb->N, lb->n + lb->mi, -1.0);
        LB_KCHECK();
    }
    return 0;
}
int qn_give(LbCtx* lb, double* dst, double* src, int flip, int memkind) {
    if (flip) {                                  // (src is a work vector nobody reads again)
        hipLaunchKernelGGL(k_qn_copy_flip, grid1(lb->N), dim3(256), 0, lb->stream, src, src, lb->N, lb->n + lb->mi, -1.0);
        LB_KCHECK();
    }
    LB_HIP(hipMemcpyAsync(dst, src, (size_t)lb->N * sizeof(double),
                          memkind == PYIPM_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, lb->stream));
    LB_HIP(hipStreamSynchronize(lb->stream));
    return 0;
}

// out = K x, or b - K x where b != NULL (device vectors of N; x raw, its multiplier rows not flipped)
int qn_apply(LbCtx* lb, const double* x, const double* b, double* out) {
    const int64_t n = lb->n, me = lb->me, mi = lb->mi, p = lb->p, ldp = lb->p_pad;
    const int m = lb->qn_m, r = 2 * m, rr = r + 1;
    hipStream_t st = lb->stream;
    const int64_t kper = (n + lb->nsplit - 1) / lb->nsplit;
    const dim3 gcol((unsigned)((ldp + 255) / 256), (unsigned)lb->nsplit, 1);
    if (!lb->qn_two_pass) {
        hipLaunchKernelGGL(k_qn_jpass, gcol, dim3(256), 0, st, lb->part, lb->qrow, ldp, lb->JT, ldp, x, x + n + mi, p, n, kper);
        LB_KCHECK();
        hipLaunchKernelGGL(k_qn_rowsum, grid1(n), dim3(256), 0, st, lb->qJv, lb->qrow, n, (int)(ldp / 64));
        LB_KCHECK();
    } else {                                     // the two kernels the pass replaces: J is read twice
        hipLaunchKernelGGL(k_tall_tn, gcol, dim3(256), 0, st, lb->part, ldp, lb->JT, ldp, x, 1, n, kper);
        LB_KCHECK();
        int64_t nblk = (n + 15) / 16; if (nblk > 16384) nblk = 16384;
        hipLaunchKernelGGL(k_jvec, dim3((unsigned)nblk), dim3(256), 0, st, lb->qJv, lb->JT, ldp, x + n + mi, p, n);
        LB_KCHECK();
    }
    hipLaunchKernelGGL(k_tall_tn_reduce, dim3((unsigned)((ldp + 255) / 256), 1), dim3(256), 0, st, lb->qJtv, lb->part, ldp, 1, lb->nsplit);
    LB_KCHECK();
    if (m > 0) {                                 // t = inv(M) W'x_x, M = [[zeta SS, L], [L', -D]] = +1 * M2
        hipLaunchKernelGGL(k_small_gram, dim3(LB_GBLK), dim3(256), (size_t)LB_GCH * (r + 1) * sizeof(double), st,
                           lb->gpart, lb->V, (int64_t)rr, (int64_t)1, 1, x, (int64_t)1, (int64_t)1, 1, r, n);
        LB_KCHECK();
        hipLaunchKernelGGL(k_small_gram_reduce, grid1(r), dim3(256), 0, st, lb->qHa, lb->gpart, r, LB_GBLK);
        LB_KCHECK();
        hipLaunchKernelGGL(k_small_solve, dim3(1), dim3(64), 0, st, lb->qt, lb->qinfo, (const double*)nullptr, 0, 0,
                           lb->M2, 1.0, lb->qHa, 1, r);
        LB_KCHECK();
    }
    hipLaunchKernelGGL(k_qn_res_x, grid1(n), dim3(256), 0, st, out, b, x, lb->V, rr, lb->qt, r, lb->qJv, lb->qn_zeta, n);
    LB_KCHECK();
    if (mi > 0) {
        hipLaunchKernelGGL(k_qn_res_s, grid1(mi), dim3(256), 0, st, out, b, x, lb->sig, n, me, mi);
        LB_KCHECK();
    }
    hipLaunchKernelGGL(k_qn_res_l, grid1(p), dim3(256), 0, st, out, b, x, lb->qJtv, n, me, mi);
    LB_KCHECK();
    return 0;
}

// x = inv(K~) b from the kept state alone (K~: with the regularised factor where the direction regularised): the tail of
// pyipm_lbfgs_direction for ONE new column -- no Gram launch, no factorisation, the 2m columns X00 and P_w = J'W as kept.
// b, x: device vectors of N, x raw.  b = the direction's g gives that direction's bits: every kernel sums in the order the
// direction's did, and the substitution takes the direction's path (the one-launch sweeps serve a single right-hand side only,
// so a direction with m > 0, which substituted 2m + 1 columns panel by panel, is followed panel by panel).
int qn_solve_dev(LbCtx* lb, const double* b, double* x) {
    const int64_t n = lb->n, me = lb->me, mi = lb->mi, p = lb->p, ldp = lb->p_pad;
    const int m = lb->qn_m, r = 2 * m, rr = r + 1;
    const double zeta = lb->qn_zeta;
    hipStream_t st = lb->stream;
    Ctx* gc = lb->gcx.get();
    gc->stream = st;
    const int64_t kper = (n + lb->nsplit - 1) / lb->nsplit;
    hipLaunchKernelGGL(k_qn_setcol0, grid1(n), dim3(256), 0, st, lb->V, rr, b, n);
    LB_KCHECK();
    // P_0 = J'b_x, R_0 = its right-hand side, y = inv(zeta G) R_0
    hipLaunchKernelGGL(k_tall_tn, dim3((unsigned)((ldp + 255) / 256), (unsigned)lb->nsplit, 1), dim3(256), 0, st,
                       lb->part, ldp, lb->JT, ldp, b, 1, n, kper);
    LB_KCHECK();
    hipLaunchKernelGGL(k_tall_tn_reduce, dim3((unsigned)((ldp + 255) / 256), 1), dim3(256), 0, st, lb->P, lb->part, ldp, 1, lb->nsplit);
    LB_KCHECK();
    hipLaunchKernelGGL(k_lb_rhs, dim3((unsigned)((ldp + 255) / 256), 1), dim3(256), 0, st, lb->R, lb->P, ldp, 1, p, me, b, n, mi,
                       lb->sig, zeta);
    LB_KCHECK();
    const int keep_persist = gc->sweep_persist;
    if (m > 0) gc->sweep_persist = 0;
    int rc = solve_plain(gc, lb->R, false, 1, ldp, lb->spart, lb->spstride);
    gc->sweep_persist = keep_persist;
    if (rc) { lb->err = gc->err; return rc; }
    if (m > 0) {
        // (W'X01 - Minv) v11 = W'Zg_x: the matrix is the direction's (columns 1.. of Hs), the right-hand side this column's
        hipLaunchKernelGGL(k_small_gram, dim3(LB_GBLK), dim3(256), (size_t)LB_GCH * (r + 1) * sizeof(double), st,
                           lb->gpart, lb->V, (int64_t)rr, (int64_t)1, 1, b, (int64_t)1, (int64_t)1, 1, r, n);
        LB_KCHECK();
        hipLaunchKernelGGL(k_small_gram_reduce, grid1(r), dim3(256), 0, st, lb->qHa, lb->gpart, r, LB_GBLK);
        LB_KCHECK();
        hipLaunchKernelGGL(k_small_gram, dim3(LB_GBLK), dim3(256), (size_t)LB_GCH * (r + 1) * sizeof(double), st,
                           lb->gpart, lb->P, (int64_t)1, ldp, 1, lb->R, (int64_t)1, ldp, 1, r, p);
        LB_KCHECK();
        hipLaunchKernelGGL(k_small_gram_reduce, grid1(r), dim3(256), 0, st, lb->qHb, lb->gpart, r, LB_GBLK);
        LB_KCHECK();
        hipLaunchKernelGGL(k_lb_hs, grid1(r), dim3(256), 0, st, lb->qHs, lb->qHa, lb->qHb, r, 1, zeta);
        LB_KCHECK();
        hipLaunchKernelGGL(k_small_solve, dim3(1), dim3(64), 0, st, lb->v11, lb->qinfo, lb->Hs, rr, 1, lb->M2, -1.0,
                           lb->qHs, 1, r);
        LB_KCHECK();
    }
    hipLaunchKernelGGL(k_lb_comb_ls, grid1(p), dim3(256), 0, st, x, lb->u, lb->R, ldp, p, me, n, mi, b, lb->sig, lb->v11, r, 1.0);
    LB_KCHECK();
    int64_t nblk = (n + 15) / 16; if (nblk > 16384) nblk = 16384;
    hipLaunchKernelGGL(k_jvec, dim3((unsigned)nblk), dim3(256), 0, st, lb->Ju, lb->JT, ldp, lb->u, p, n);
    LB_KCHECK();
    hipLaunchKernelGGL(k_lb_comb_x, grid1(n), dim3(256), 0, st, x, lb->V, rr, n, lb->v11, r, 1.0 / zeta, (const double*)lb->Ju);
    LB_KCHECK();
    return 0;
}

// |a|_2^2 and |b|_2^2 to the host: the one synchronisation of a measured backward error
int qn_sumsq2(LbCtx* lb, const double* a, const double* b, double out[2]) {
    hipLaunchKernelGGL(k_qn_sumsq, dim3(QN_NBLK, 2), dim3(256), 0, lb->stream, lb->qnrm + 2, a, b, lb->N);
    LB_KCHECK();
    hipLaunchKernelGGL(k_qn_sumsq_fin, dim3(1), dim3(64), 0, lb->stream, lb->qnrm, lb->qnrm + 2, 2);
    LB_KCHECK();
    LB_HIP(hipMemcpyAsync(out, lb->qnrm, 2 * sizeof(double), hipMemcpyDeviceToHost, lb->stream));
    LB_HIP(hipStreamSynchronize(lb->stream));
    return 0;
}

int qn_copy(LbCtx* lb, double* dst, const double* src) {
    LB_HIP(hipMemcpyAsync(dst, src, (size_t)lb->N * sizeof(double), hipMemcpyDeviceToDevice, lb->stream));
    return 0;
}

}  // namespace

extern "C" {

int pyipm_qn_matvec(pyipm_lbfgs_ctx* h, const double* v, int flip, int memkind, double* out) try {
    if (!h) return PYIPM_E_BADARG;
    LbCtx* lb = LB(h);
    int rc = qn_enter(lb, "qn_matvec"); if (rc) return rc;
    if (!v || !out) { lb->err = "qn_matvec: null v / out"; return PYIPM_E_BADARG; }
    rc = qn_get(lb, lb->qx, v, flip, memkind); if (rc) return rc;
    rc = qn_apply(lb, lb->qx, nullptr, lb->qr); if (rc) return rc;
    return qn_give(lb, out, lb->qr, 0, memkind);
} PYIPM_CATCH_H(h)

int pyipm_qn_solve(pyipm_lbfgs_ctx* h, const double* rhs, double* dz, int flip, int memkind) try {
    if (!h) return PYIPM_E_BADARG;
    LbCtx* lb = LB(h);
    int rc = qn_enter(lb, "qn_solve"); if (rc) return rc;
    if (!rhs || !dz) { lb->err = "qn_solve: null rhs / dz"; return PYIPM_E_BADARG; }
    rc = lb_put(lb, lb->qb, rhs, (size_t)lb->N, memkind); if (rc) return rc;
    rc = qn_solve_dev(lb, lb->qb, lb->qx); if (rc) return rc;
    return qn_give(lb, dz, lb->qx, flip, memkind);
} PYIPM_CATCH_H(h)

int pyipm_qn_refine(pyipm_lbfgs_ctx* h, const double* rhs, double* dz, int flip, int refine, int memkind) try {
    if (!h) return PYIPM_E_BADARG;
    LbCtx* lb = LB(h);
    int rc = qn_enter(lb, "qn_refine"); if (rc) return rc;
    if (!dz) { lb->err = "qn_refine: null dz"; return PYIPM_E_BADARG; }
    const double* b = lb->g;                     // rhs == NULL: the g of the last direction
    if (rhs) { rc = lb_put(lb, lb->qb, rhs, (size_t)lb->N, memkind); if (rc) return rc; b = lb->qb; }
    rc = qn_get(lb, lb->qx, dz, flip, memkind); if (rc) return rc;
    Ctx* gc = lb->gcx.get();                     // (refine_target / refine_max live where pyipm_lbfgs_set_option puts them)
    auto residual = [&]() -> int { return qn_apply(lb, lb->qx, b, lb->qr); };
    auto berr_of = [&](double* e) -> int {
        double ss[2];
        const int rc2 = qn_sumsq2(lb, lb->qr, b, ss); if (rc2) return rc2;
        *e = ss[1] > 0.0 ? sqrt(ss[0] / ss[1]) : (ss[0] > 0.0 ? 1.0e308 : 0.0);
        return 0;
    };
    if (refine == 0) {                           // measure only
        double e = 0.0;
        rc = residual(); if (rc) return rc;
        rc = berr_of(&e); if (rc) return rc;
        lb->qn_info[0] = 0.0; lb->qn_info[1] = lb->qn_info[2] = e; lb->qn_info[3] = e <= gc->refine_target ? 1.0 : 0.0;
        return PYIPM_OK;                         // dz is left as it is, bit for bit
    }
    rc = refine_loop(gc, refine, residual, berr_of,
                     [&]() -> int { return qn_copy(lb, lb->qsave, lb->qx); },
                     [&]() -> int { return qn_copy(lb, lb->qx, lb->qsave); },
                     [&]() -> int {
                         const int rc2 = qn_solve_dev(lb, lb->qr, lb->qd); if (rc2) return rc2;
                         hipLaunchKernelGGL(k_qn_add, grid1(lb->N), dim3(256), 0, lb->stream, lb->qx, lb->qd, lb->N);
                         LB_KCHECK();
                         return 0;
                     });
    if (rc) return rc;
    lb->qn_info[0] = (double)gc->info_steps; lb->qn_info[1] = gc->info_berr0; lb->qn_info[2] = gc->info_berr;
    lb->qn_info[3] = (double)gc->info_converged;
    return qn_give(lb, dz, lb->qx, flip, memkind);
} PYIPM_CATCH_H(h)

int pyipm_qn_info(pyipm_lbfgs_ctx* h, double out[4]) try {
    if (!h || !out) return PYIPM_E_BADARG;
    for (int i = 0; i < 4; ++i) out[i] = LB(h)->qn_info[i];
    return PYIPM_OK;
} PYIPM_CATCH_H(h)

}  // extern "C"
