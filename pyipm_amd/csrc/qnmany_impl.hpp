// qnmany_impl.hpp — the quasi-Newton KKT operator of the last L-BFGS direction for k columns per call (include/pyipm_newton.h,
// pyipm_lbfgs_kkt_matvec_many / pyipm_lbfgs_kkt_solve_many; kernels_qnmany.hpp).  Included behind qn_impl.hpp: the same kept
// state (LbCtx::qn_valid, qn_enter), the arithmetic of qn_apply and qn_solve_dev column by column, the two products with J on
// the matrix pipe and the substitution through solve_many_plain.  Everything written lives in LbCtx::qm_buf: column 0 of V, P
// and R, the work vectors of pyipm_qn_* and whatever the direction left are not touched.
#pragma once
#include "qn_impl.hpp"
#include "kernels_qnmany.hpp"

namespace {

// The partition of n in k_qm_jt, from (n, p_pad) alone: about 1024 workgroups per block of 64 columns, at least 256 rows per
// split, kper a multiple of the K step.
void qm_nsplit(int64_t n, int64_t p_pad, int* nsplit, int64_t* kper) {
    const int64_t tiles = p_pad / QM_TR;
    int64_t s = (1024 + tiles - 1) / tiles;
    const int64_t by_rows = (n + 255) / 256;
    if (s > by_rows) s = by_rows;
    if (s < 1) s = 1;
    const int64_t per = ((n + s - 1) / s + QM_KC - 1) / QM_KC * QM_KC;
    *kper = per;
    *nsplit = (int)((n + per - 1) / per);
}

inline unsigned qm_cols(int64_t k) { return (unsigned)(k < QM_YMAX ? k : QM_YMAX); }
inline dim3 qm_grid(int64_t rows, int64_t k) { return dim3((unsigned)((rows + 255) / 256), qm_cols(k)); }

// The work buffers of one call, carved from qm_buf (doubles).  What a call does not need has count 0.
struct QmBufs {
    double *Y, *Jb, *jtpart, *gpa, *gpb, *Hq, *Tq, *info, *X, *mpart, *R, *D, *Xs, *ss, *Hin, *Hout;
    int64_t kpad;
};
int qm_reserve(LbCtx* lb, int64_t k, bool solve, int refine, bool host, QmBufs* b) {
    const int64_t n = lb->n, N = lb->N, ldp = lb->p_pad;
    const size_t r = (size_t)(2 * lb->qn_m), K = (size_t)k;
    int nsplit; int64_t kper; qm_nsplit(n, ldp, &nsplit, &kper);
    size_t n_mpart; solve_many_sizes(ldp, k, &b->kpad, &n_mpart);
    size_t off = 0;
    auto take = [&](size_t count) { const size_t o = off; off += (count + 31) / 32 * 32; return o; };
    const size_t col = (size_t)N * K;
    const size_t oY = take((size_t)ldp * (size_t)b->kpad), oJb = take((size_t)n * K);
    const size_t ojt = take((size_t)nsplit * (size_t)(k < QM_GROUP ? k : QM_GROUP) * (size_t)ldp);
    const size_t ogpa = take((size_t)QM_GBLK * K * r), ogpb = take(solve ? (size_t)QM_GBLK * K * r : 0);
    const size_t oHq = take(K * r), oTq = take(K * r), oinfo = take(K);
    const size_t oX = take(solve ? col : 0), omp = take(solve ? n_mpart : 0);
    const size_t oR = take(refine != 0 ? col : 0), oD = take(refine != 0 ? col : 0);
    const size_t oXs = take(refine < 0 ? col : 0), oss = take(refine < 0 ? 2 * K : 0);
    const size_t oHin = take(host ? col : 0), oHout = take(host && !solve ? col : 0);
    if (lb->qm_buf.capacity() < off) {
        LB_HIP(lb->qm_buf.reserve(off));
        if (getenv("PYIPM_POISON_WORKSPACE")) LB_HIP(hipMemsetAsync(lb->qm_buf, 0xFF, off * sizeof(double), lb->stream));   // as the workspace
    }
    double* base = lb->qm_buf;
    b->Y = base + oY; b->Jb = base + oJb; b->jtpart = base + ojt; b->gpa = base + ogpa; b->gpb = base + ogpb;
    b->Hq = base + oHq; b->Tq = base + oTq; b->info = base + oinfo; b->X = base + oX; b->mpart = base + omp;
    b->R = base + oR; b->D = base + oD; b->Xs = base + oXs; b->ss = base + oss; b->Hin = base + oHin; b->Hout = base + oHout;
    return 0;
}

// P (ld ldo) = J'B_x for k columns: B_x = rows 0 .. n-1 of the columns at B + j * ldb
int qm_jt(LbCtx* lb, const QmBufs& q, int64_t k, const double* B, int64_t ldb, double* P, int64_t ldo) {
    const int64_t ldp = lb->p_pad;
    int nsplit; int64_t kper; qm_nsplit(lb->n, ldp, &nsplit, &kper);
    for (int64_t j0 = 0; j0 < k; j0 += QM_GROUP) {
        const int64_t kc = k - j0 < QM_GROUP ? k - j0 : QM_GROUP;
        const int ncb = (int)((kc + QM_KB - 1) / QM_KB);
        hipLaunchKernelGGL(k_qm_jt, dim3((unsigned)(ncb * (ldp / QM_TR)), (unsigned)nsplit), dim3(256), 0, lb->stream,
                           q.jtpart, ldp, lb->JT, ldp, B + j0 * ldb, ldb, kc, ncb, lb->n, kper);
        LB_KCHECK();
        hipLaunchKernelGGL(k_qm_jt_reduce, qm_grid(ldp, kc), dim3(256), 0, lb->stream, P + j0 * ldo, ldo, q.jtpart, ldp, kc, nsplit);
        LB_KCHECK();
    }
    return 0;
}
// out (n x k, ld ldo) = J (usgn U), U: p rows of the columns at U + j * ldu
int qm_ju(LbCtx* lb, int64_t k, const double* U, int64_t ldu, double usgn, double* out, int64_t ldo) {
    const int ncb = (int)((k + QM_KB - 1) / QM_KB);
    const int64_t tiles = (lb->n + QM_TR - 1) / QM_TR;
    hipLaunchKernelGGL(k_qm_ju, dim3((unsigned)(ncb * tiles)), dim3(256), 0, lb->stream, out, ldo, lb->JT, lb->p_pad, U, ldu, usgn,
                       k, ncb, lb->n, lb->p);
    LB_KCHECK();
    return 0;
}
// x_j = inv(M) Hq_j for the k columns of q.Hq into `x` (k x r)
int qm_small(LbCtx* lb, const QmBufs& q, int64_t k, double* x, const double* M1, int ld1, int off1, double s2) {
    hipLaunchKernelGGL(k_qm_small_solve, dim3((unsigned)k), dim3(64), 0, lb->stream, x, q.info, M1, ld1, off1, lb->M2, s2, q.Hq,
                       2 * lb->qn_m);
    LB_KCHECK();
    return 0;
}

// out = K x, or b - K x where b != NULL, for k columns (device blocks; x read with its multiplier rows times sgn_l)
int qm_apply(LbCtx* lb, const QmBufs& q, int64_t k, const double* x, int64_t ldx, double sgn_l, const double* b, int64_t ldb,
             double* out, int64_t ldo) {
    const int64_t n = lb->n, me = lb->me, mi = lb->mi, ldp = lb->p_pad;
    const int m = lb->qn_m, r = 2 * m, rr = r + 1;
    hipStream_t st = lb->stream;
    int rc = qm_jt(lb, q, k, x, ldx, q.Y, ldp); if (rc) return rc;                       // J'x_x
    rc = qm_ju(lb, k, x + n + mi, ldx, sgn_l, q.Jb, n); if (rc) return rc;               // J x_l
    if (m > 0) {                                 // t = inv(M) W'x_x
        hipLaunchKernelGGL(k_qm_gram, dim3(QM_GBLK, qm_cols(k)), dim3(256), 0, st, q.gpa, lb->V + 1, (int64_t)rr, (int64_t)1,
                           x, ldx, r, n, k);
        LB_KCHECK();
        hipLaunchKernelGGL(k_qm_hs, grid1(k * r), dim3(256), 0, st, q.Hq, q.gpa, (const double*)nullptr, r, k, QM_GBLK, 1.0);
        LB_KCHECK();
        rc = qm_small(lb, q, k, q.Tq, nullptr, 0, 0, 1.0); if (rc) return rc;
    }
    hipLaunchKernelGGL(k_qm_res_x, qm_grid(n, k), dim3(256), 0, st, out, ldo, b, ldb, x, ldx, lb->V, rr, q.Tq, r, q.Jb, n,
                       lb->qn_zeta, n, k);
    LB_KCHECK();
    hipLaunchKernelGGL(k_qm_res_sl, qm_grid(2 * mi + me, k), dim3(256), 0, st, out, ldo, b, ldb, x, ldx, sgn_l, lb->sig, q.Y, ldp,
                       n, me, mi, k);
    LB_KCHECK();
    return 0;
}

// X (ld N, raw) = inv(K~) B for k columns from the kept state: qn_solve_dev's steps, the substitution through solve_many_plain
int qm_solve_dev(LbCtx* lb, const QmBufs& q, int64_t k, const double* B, int64_t ldb, double* X) {
    const int64_t n = lb->n, me = lb->me, mi = lb->mi, p = lb->p, N = lb->N, ldp = lb->p_pad;
    const int m = lb->qn_m, r = 2 * m, rr = r + 1;
    const double zeta = lb->qn_zeta;
    hipStream_t st = lb->stream;
    Ctx* gc = lb->gcx.get();
    gc->stream = st;
    int rc = qm_jt(lb, q, k, B, ldb, q.Y, ldp); if (rc) return rc;
    hipLaunchKernelGGL(k_qm_rhs, qm_grid(ldp, k), dim3(256), 0, st, q.Y, ldp, B, ldb, lb->sig, zeta, p, me, n, mi, k);
    LB_KCHECK();
    if (q.kpad > k) LB_HIP(hipMemsetAsync(q.Y + k * ldp, 0, (size_t)((q.kpad - k) * ldp) * sizeof(double), st));
    rc = solve_many_plain(gc, q.Y, ldp, q.kpad, q.mpart);
    if (rc) { lb->err = gc->err; return rc; }
    if (m > 0) {                                 // (W'X01 - Minv) v11 = (W'b_x - P_w'y) / zeta, the direction's matrix
        hipLaunchKernelGGL(k_qm_gram, dim3(QM_GBLK, qm_cols(k)), dim3(256), 0, st, q.gpa, lb->V + 1, (int64_t)rr, (int64_t)1,
                           B, ldb, r, n, k);
        LB_KCHECK();
        hipLaunchKernelGGL(k_qm_gram, dim3(QM_GBLK, qm_cols(k)), dim3(256), 0, st, q.gpb, lb->P + ldp, (int64_t)1, ldp,
                           q.Y, ldp, r, p, k);
        LB_KCHECK();
        hipLaunchKernelGGL(k_qm_hs, grid1(k * r), dim3(256), 0, st, q.Hq, q.gpa, (const double*)q.gpb, r, k, QM_GBLK, zeta);
        LB_KCHECK();
        rc = qm_small(lb, q, k, q.Tq, lb->Hs, rr, 1, -1.0); if (rc) return rc;
    }
    hipLaunchKernelGGL(k_qm_comb_ls, qm_grid(p, k), dim3(256), 0, st, X, N, q.Y, ldp, lb->R, ldp, p, me, n, mi, B, ldb, lb->sig,
                       q.Tq, r, k);
    LB_KCHECK();
    rc = qm_ju(lb, k, q.Y, ldp, 1.0, q.Jb, n); if (rc) return rc;
    hipLaunchKernelGGL(k_qm_comb_x, qm_grid(n, k), dim3(256), 0, st, X, N, B, ldb, lb->V, rr, n, q.Tq, r, 1.0 / zeta, q.Jb, n, k);
    LB_KCHECK();
    return 0;
}

// the argument checks the two entries share; *done: k == 0, nothing to do
int qm_check(LbCtx* lb, const char* name, int64_t k, const double* in, int64_t ld_in, const double* out, int64_t ld_out,
             int memkind, bool no_overlap, bool* done) {
    *done = false;
    const std::string nm(name);
    if (k < 0) { lb->err = nm + ": k < 0"; return PYIPM_E_BADARG; }
    if (memkind != PYIPM_MEM_HOST && memkind != PYIPM_MEM_DEVICE) { lb->err = nm + ": bad memkind"; return PYIPM_E_BADARG; }
    if (k == 0) { *done = true; return 0; }
    if (!in || !out) { lb->err = nm + ": null block"; return PYIPM_E_BADARG; }
    if (ld_in < lb->N || ld_out < lb->N) { lb->err = nm + ": leading dimension below N = n + 2 mi + me"; return PYIPM_E_BADARG; }
    if (no_overlap) {
        const double *ie = in + (k - 1) * ld_in + lb->N, *oe = out + (k - 1) * ld_out + lb->N;
        if (in < oe && out < ie) { lb->err = nm + ": out overlaps v"; return PYIPM_E_BADARG; }
    }
    return 0;
}

}  // namespace

extern "C" {

int pyipm_lbfgs_kkt_matvec_many(pyipm_lbfgs_ctx* h, int64_t k, const double* v, int64_t ld_v, double* out, int64_t ld_out,
                                int flip, int memkind) try {
    if (!h) return PYIPM_E_BADARG;
    LbCtx* lb = LB(h);
    int rc = qn_enter(lb, "kkt_matvec_many"); if (rc) return rc;
    bool done;
    rc = qm_check(lb, "kkt_matvec_many", k, v, ld_v, out, ld_out, memkind, true, &done); if (rc || done) return rc;
    const bool host = memkind == PYIPM_MEM_HOST;
    const int64_t N = lb->N;
    hipStream_t st = lb->stream;
    QmBufs q;
    rc = qm_reserve(lb, k, false, 0, host, &q); if (rc) return rc;
    const double sgn = flip ? -1.0 : 1.0;
    if (!host) return qm_apply(lb, q, k, v, ld_v, sgn, nullptr, 0, out, ld_out);
    LB_HIP(hipMemcpy2DAsync(q.Hin, (size_t)N * sizeof(double), v, (size_t)ld_v * sizeof(double), (size_t)N * sizeof(double),
                            (size_t)k, hipMemcpyHostToDevice, st));
    LB_HIP(hipStreamSynchronize(st));                                        // host memory is not retained
    rc = qm_apply(lb, q, k, q.Hin, N, sgn, nullptr, 0, q.Hout, N); if (rc) return rc;
    LB_HIP(hipMemcpy2DAsync(out, (size_t)ld_out * sizeof(double), q.Hout, (size_t)N * sizeof(double), (size_t)N * sizeof(double),
                            (size_t)k, hipMemcpyDeviceToHost, st));
    LB_HIP(hipStreamSynchronize(st));
    return PYIPM_OK;
} PYIPM_CATCH_H(h)

int pyipm_lbfgs_kkt_solve_many(pyipm_lbfgs_ctx* h, int64_t k, const double* rhs, int64_t ld_rhs, double* dz, int64_t ld_dz,
                               int flip, int refine, int memkind) try {
    if (!h) return PYIPM_E_BADARG;
    LbCtx* lb = LB(h);
    int rc = qn_enter(lb, "kkt_solve_many"); if (rc) return rc;
    bool done;
    rc = qm_check(lb, "kkt_solve_many", k, rhs, ld_rhs, dz, ld_dz, memkind, false, &done); if (rc || done) return rc;
    const bool host = memkind == PYIPM_MEM_HOST;
    const int64_t N = lb->N;
    hipStream_t st = lb->stream;
    Ctx* gc = lb->gcx.get();                     // (refine_target / refine_max live where pyipm_lbfgs_set_option puts them)
    refine = refine_steps(gc, refine);
    QmBufs q;
    rc = qm_reserve(lb, k, true, refine, host, &q); if (rc) return rc;
    const double* B = rhs; int64_t ldb = ld_rhs;
    if (host) {
        LB_HIP(hipMemcpy2DAsync(q.Hin, (size_t)N * sizeof(double), rhs, (size_t)ld_rhs * sizeof(double), (size_t)N * sizeof(double),
                                (size_t)k, hipMemcpyHostToDevice, st));
        LB_HIP(hipStreamSynchronize(st));                                    // host memory is not retained
        B = q.Hin; ldb = N;
    }
    rc = qm_solve_dev(lb, q, k, B, ldb, q.X); if (rc) return rc;
    if (refine != 0) {
        const size_t col = (size_t)N * (size_t)k;
        std::vector<double> ss(refine < 0 ? 2 * (size_t)k : 0);
        rc = refine_loop(gc, refine,
            [&]() -> int { return qm_apply(lb, q, k, q.X, N, 1.0, B, ldb, q.R, N); },
            [&](double* worst) -> int {                  // the worst column's |r|/|b| (NaN if any is): one synchronisation
                hipLaunchKernelGGL(k_qm_sumsq2, dim3((unsigned)k), dim3(256), 0, st, q.ss, q.R, N, B, ldb, N);
                LB_KCHECK();
                LB_HIP(hipMemcpyAsync(ss.data(), q.ss, 2 * (size_t)k * sizeof(double), hipMemcpyDeviceToHost, st));
                LB_HIP(hipStreamSynchronize(st));
                double berr = 0.0;
                for (int64_t j = 0; j < k; ++j) {
                    const double s0 = ss[2 * j], s1 = ss[2 * j + 1];
                    const double e = (s0 != s0 || s1 != s1) ? s0 + s1 : s1 > 0.0 ? sqrt(s0 / s1) : (s0 > 0.0 ? 1.0e308 : 0.0);
                    if (!(e <= berr) && berr == berr) berr = e;
                }
                *worst = berr;
                return 0;
            },
            [&]() -> int { LB_HIP(hipMemcpyAsync(q.Xs, q.X, col * sizeof(double), hipMemcpyDeviceToDevice, st)); return 0; },
            [&]() -> int { LB_HIP(hipMemcpyAsync(q.X, q.Xs, col * sizeof(double), hipMemcpyDeviceToDevice, st)); return 0; },
            [&]() -> int {                               // X += solve_many(R)
                const int rc2 = qm_solve_dev(lb, q, k, q.R, N, q.D); if (rc2) return rc2;
                hipLaunchKernelGGL(k_qn_add, grid1((int64_t)col), dim3(256), 0, st, q.X, q.D, (int64_t)col);
                LB_KCHECK();
                return 0;
            });
        if (rc) return rc;
        lb->qn_info[0] = (double)gc->info_steps; lb->qn_info[1] = gc->info_berr0; lb->qn_info[2] = gc->info_berr;
        lb->qn_info[3] = (double)gc->info_converged;
    }
    const double sgn = flip ? -1.0 : 1.0;
    if (!host) {
        hipLaunchKernelGGL(k_qm_copy_flip, qm_grid(N, k), dim3(256), 0, st, dz, ld_dz, q.X, N, N, lb->n + lb->mi, sgn, k);
        LB_KCHECK();
        return PYIPM_OK;
    }
    if (flip) {                                  // (X is a work block nobody reads again)
        hipLaunchKernelGGL(k_qm_copy_flip, qm_grid(N, k), dim3(256), 0, st, q.X, N, q.X, N, N, lb->n + lb->mi, sgn, k);
        LB_KCHECK();
    }
    LB_HIP(hipMemcpy2DAsync(dz, (size_t)ld_dz * sizeof(double), q.X, (size_t)N * sizeof(double), (size_t)N * sizeof(double),
                            (size_t)k, hipMemcpyDeviceToHost, st));
    LB_HIP(hipStreamSynchronize(st));
    return PYIPM_OK;
} PYIPM_CATCH_H(h)

}  // extern "C"
