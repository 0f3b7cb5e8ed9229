// kernels_qnmany.hpp — the quasi-Newton KKT operator of an L-BFGS direction for MANY columns (include/pyipm_newton.h,
// pyipm_lbfgs_kkt_matvec_many / pyipm_lbfgs_kkt_solve_many): the two products with the staged Jacobian on
// v_mfma_f64_16x16x4f64 and the column-wise glue around the kept 2m x 2m system.  K, W, M as in kernels_qn.hpp.
//
//   k_qm_jt   J'B   (p_pad x k, the sum over n): tall.  A FIXED partition of n chosen from (n, p_pad) alone (qm_nsplit), a
//             workgroup per 64 columns of J x 64 columns of B x split; partials in a buffer, k_qm_jt_reduce sums them in
//             ascending order.  Rows n .. n_pad-1 of JT are never read (selected out by address).
//   k_qm_ju   J U   (n x k, the sum over p): owner-computes, a workgroup per 64 rows of J x 64 columns of U walks p in
//             ascending order: no partials, no second launch.  Columns p .. p_pad-1 of JT and those rows of U are never read.
// JT is read once by each per block of QM_KB = 64 columns.  Tiles of QM_KC x 64 staged through shared memory and the
// operand maps of kernels_kmany.hpp / kernels_msolve.hpp: A[i = lane & 15][k = lane >> 4] takes the caller's columns,
// B[k][j = lane & 15] the rows of the tile of J, D[i = (lane >> 4) + 4 r][j = lane & 15].  The caller's column is an operand
// dimension and never a summation dimension, every walk and every partition is fixed by the geometry: column j gets the
// same operations in the same order whatever k is, wherever j stands and whatever the other columns hold (a NaN column stays
// in its column), and no sum uses atomics.
//
// Column blocks: column j of a block at base + j * ld.  The element-wise kernels put the rows on grid.x and walk the columns
// from blockIdx.y in steps of gridDim.y.  A vector of the solution space read with sgn_l = -1 has its multiplier rows negated
// (flip): the product with -1 is exact.
#pragma once
#include "kernels_qn.hpp"

namespace pyipm {

typedef double double4_qm __attribute__((ext_vector_type(4)));      // the accumulator of one v_mfma_f64_16x16x4f64

constexpr int QM_KB = 64;          // the caller's columns per workgroup of the products (JT is read twice per QM_KB columns)
constexpr int QM_TR = 64;          // rows of the result per workgroup
constexpr int QM_KC = 64;          // K per step staged in shared memory (80 KB per workgroup: two per CU)
constexpr int QM_LSTR = 64 + 16;   // padded shared-memory row stride (doubles), as KM_LSTR
constexpr int QM_GBLK = 64;        // blocks (= partial sums) of the skinny products over n and over p
constexpr int QM_GROUP = 256;      // columns per launch of k_qm_jt (bounds its partial buffer)
constexpr int QM_YMAX = 4096;      // grid.y of the column-walking kernels

// acc += M[rows of this tile, 0 .. Kn) * Vb[0 .. Kn, columns of this block] (Vb entries times vsgn), K ascending in steps of
// 4.  elem(row, c): entry (tile row, K index c) of the operand, 0 outside it.  LANE_K: the operand is contiguous along K (the
// lane takes the K index of the load), else along the tile's rows (the lane takes the row).  Block-uniform control flow; the
// next chunk's operands are requested into registers before the MFMAs of the current one.  A wave all of whose 16 columns
// lie past ncol loads and stores with the others and skips the MFMAs (nobody reads its accumulators).
template <bool LANE_K, class Elem>
__device__ __forceinline__ void qm_product(double4_qm (&acc)[4], double (&Ms)[QM_KC][QM_LSTR], double (&Vs)[QM_KC][QM_LSTR],
                                           int64_t Kn, const double* __restrict__ Vb, int64_t ldv, int ncol, double vsgn, Elem elem)
{
    if (Kn <= 0) return;
    const int tid = threadIdx.x, L = tid & 63, q0 = tid >> 6, l15 = L & 15, l4 = L >> 4;
    constexpr int PT = QM_KC / 4;                        // operand elements per thread and step
    const bool live = q0 * 16 < ncol;
    double mr[PT], vr[PT];
    auto fetch = [&](int64_t kc) {
        #pragma unroll
        for (int m = 0; m < PT; ++m) {
            const int q = q0 + 4 * m;
            mr[m] = LANE_K ? elem(q, kc + L) : elem(L, kc + q);
            vr[m] = (kc + L < Kn && q < ncol) ? vsgn * Vb[(kc + L) + (int64_t)q * ldv] : 0.0;
        }
    };
    fetch(0);
    for (int64_t kc = 0; kc < Kn; kc += QM_KC) {
        if (LANE_K) {
            #pragma unroll
            for (int m = 0; m < PT; ++m) Ms[L][q0 + 4 * m] = mr[m];
        } else {
            #pragma unroll
            for (int m = 0; m < PT; ++m) Ms[q0 + 4 * m][L] = mr[m];
        }
        #pragma unroll
        for (int m = 0; m < PT; ++m) Vs[L][q0 + 4 * m] = vr[m];
        __syncthreads();
        if (kc + QM_KC < Kn) fetch(kc + QM_KC);
        if (live) {
            #pragma unroll
            for (int kk = 0; kk < QM_KC; kk += 4) {
                const double a = Vs[kk + l4][q0 * 16 + l15];
                #pragma unroll
                for (int ti = 0; ti < 4; ++ti)
                    acc[ti] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Ms[kk + l4][ti * 16 + l15], acc[ti], 0, 0, 0);
            }
        }
        __syncthreads();
    }
}

// part[(split * kcols + j) * ldp + c] = sum_{i in split} JT[c + i*ldj] * B[i + j*ldb]          (J'B)
// grid (ncb * ldp / 64, nsplit), block 256; ncb = ceil(kcols / QM_KB), the column block is the fastest index: the workgroups
// that share a tile of JT run side by side.  Wave w computes 64 columns of J x the caller's columns [16 w, 16 w + 16).
__global__ __launch_bounds__(256) void k_qm_jt(double* __restrict__ part, int64_t ldp, const double* __restrict__ JT, int64_t ldj,
                                               const double* __restrict__ B, int64_t ldb, int64_t kcols, int ncb, int64_t n,
                                               int64_t kper)
{
    __shared__ double Ms[QM_KC][QM_LSTR];                // Ms[k][column of J in the tile]
    __shared__ double Vs[QM_KC][QM_LSTR];                // Vs[k][the caller's column in the block]
    const int tid = threadIdx.x, L = tid & 63, wave = tid >> 6, l15 = L & 15, l4 = L >> 4;
    const int64_t j0 = (int64_t)(blockIdx.x % ncb) * QM_KB, c0 = (int64_t)(blockIdx.x / ncb) * QM_TR;
    const int ncol = (int)(kcols - j0 < QM_KB ? kcols - j0 : QM_KB);
    const int64_t k0 = (int64_t)blockIdx.y * kper;
    int64_t k1 = k0 + kper; if (k1 > n) k1 = n;
    const int64_t Kn = k1 - k0;
    double4_qm acc[4];
    #pragma unroll
    for (int ti = 0; ti < 4; ++ti) acc[ti] = double4_qm{0.0, 0.0, 0.0, 0.0};
    const double* Jt = JT + c0 + k0 * ldj;               // (ldp is a multiple of 128: the 64 columns of the tile exist)
    qm_product<false>(acc, Ms, Vs, Kn, B + j0 * ldb + k0, ldb, ncol, 1.0,
                      [=](int row, int64_t c) { return c < Kn ? Jt[row + c * ldj] : 0.0; });
    double* out = part + ((int64_t)blockIdx.y * kcols + j0) * ldp + c0;
    #pragma unroll
    for (int ti = 0; ti < 4; ++ti)
        #pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = ti * 16 + l15, c = wave * 16 + l4 + 4 * r;
            if (c < ncol) out[row + (int64_t)c * ldp] = acc[ti][r];
        }
}

// P[j*ldo + c] = sum_split part[(split * kcols + j) * ldp + c], split ascending        grid (ceil(ldp / 256), columns)
__global__ __launch_bounds__(256) void k_qm_jt_reduce(double* __restrict__ P, int64_t ldo, const double* __restrict__ part,
                                                      int64_t ldp, int64_t kcols, int nsplit)
{
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= ldp) return;
    for (int64_t j = blockIdx.y; j < kcols; j += gridDim.y) {
        double t = 0.0;
        for (int sp = 0; sp < nsplit; ++sp) t += part[((int64_t)sp * kcols + j) * ldp + c];
        P[j * ldo + c] = t;
    }
}

// out[i + j*ldo] = sum_{c < p} JT[c + i*ldj] * usgn * U[c + j*ldu], c ascending          (J U)
// grid (ncb * ceil(n / 64)), block 256: the only writer of its 64 rows x QM_KB columns.
__global__ __launch_bounds__(256) void k_qm_ju(double* __restrict__ out, int64_t ldo, const double* __restrict__ JT, int64_t ldj,
                                               const double* __restrict__ U, int64_t ldu, double usgn, int64_t kcols, int ncb,
                                               int64_t n, int64_t p)
{
    __shared__ double Ms[QM_KC][QM_LSTR];                // Ms[k][row of J in the tile]
    __shared__ double Vs[QM_KC][QM_LSTR];
    const int tid = threadIdx.x, L = tid & 63, wave = tid >> 6, l15 = L & 15, l4 = L >> 4;
    const int64_t j0 = (int64_t)(blockIdx.x % ncb) * QM_KB, r0 = (int64_t)(blockIdx.x / ncb) * QM_TR;
    const int ncol = (int)(kcols - j0 < QM_KB ? kcols - j0 : QM_KB);
    const int rows = (int)(n - r0 < QM_TR ? n - r0 : QM_TR);
    double4_qm acc[4];
    #pragma unroll
    for (int ti = 0; ti < 4; ++ti) acc[ti] = double4_qm{0.0, 0.0, 0.0, 0.0};
    const double* Jr = JT + r0 * ldj;
    qm_product<true>(acc, Ms, Vs, p, U + j0 * ldu, ldu, ncol, usgn,
                     [=](int row, int64_t c) { return (row < rows && c < p) ? Jr[c + (int64_t)row * ldj] : 0.0; });
    double* o = out + r0 + j0 * ldo;
    #pragma unroll
    for (int ti = 0; ti < 4; ++ti)
        #pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = ti * 16 + l15, c = wave * 16 + l4 + 4 * r;
            if (row < rows && c < ncol) o[row + (int64_t)c * ldo] = acc[ti][r];
        }
}

// part[(b * kcols + j) * r + a] = sum_{i in block b} A[i*ars + a*acs] * E[i + j*lde],  a < r <= 64:  W'B_x over n (A = columns
// 1.. of V, row-major) and P_w'Y over p (A = columns 1.. of P, column-major).  grid (QM_GBLK, columns): block b takes the rows
// [b per, (b + 1) per), per = ceil(n / QM_GBLK); thread t every 256th of them, ascending; the 64 lanes of a wave meet in a
// butterfly, the four waves in a fixed order.  k_qm_hs sums the blocks, b ascending.
__global__ __launch_bounds__(256) void k_qm_gram(double* __restrict__ part, const double* __restrict__ A, int64_t ars, int64_t acs,
                                                 const double* __restrict__ E, int64_t lde, int r, int64_t n, int64_t kcols)
{
    __shared__ double sm[4][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t per = (n + gridDim.x - 1) / gridDim.x, i0 = (int64_t)blockIdx.x * per;
    const int64_t i1 = i0 + per < n ? i0 + per : n;
    for (int64_t j = blockIdx.y; j < kcols; j += gridDim.y) {
        double acc[64];
        #pragma unroll
        for (int a = 0; a < 64; ++a) acc[a] = 0.0;
        for (int64_t i = i0 + tid; i < i1; i += 256) {
            const double e = E[i + j * lde];
            const double* row = A + i * ars;
            #pragma unroll
            for (int a = 0; a < 64; ++a) if (a < r) acc[a] = fma(row[a * acs], e, acc[a]);
        }
        #pragma unroll
        for (int a = 0; a < 64; ++a)
            if (a < r) {
                double t = acc[a];
                #pragma unroll
                for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off, 64);
                if (lane == 0) sm[wave][a] = t;
            }
        __syncthreads();
        if (tid < r) part[((int64_t)blockIdx.x * kcols + j) * r + tid] = (sm[0][tid] + sm[1][tid]) + (sm[2][tid] + sm[3][tid]);
        __syncthreads();
    }
}

// Right-hand sides of the k small systems, Hq[j*r + a]:  pb == NULL: W'v_x (the operator's t = inv(M) W'v_x);  else column 0 of
// k_lb_hs, (W'b_x - P_w'y) / zeta.
__global__ __launch_bounds__(256) void k_qm_hs(double* __restrict__ Hq, const double* __restrict__ pa, const double* __restrict__ pb,
                                               int r, int64_t kcols, int nblk, double zeta)
{
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= kcols * r) return;
    double ta = 0.0, tb = 0.0;
    for (int b = 0; b < nblk; ++b) ta += pa[(int64_t)b * kcols * r + o];
    if (!pb) { Hq[o] = ta; return; }
    for (int b = 0; b < nblk; ++b) tb += pb[(int64_t)b * kcols * r + o];
    Hq[o] = (ta - tb) / zeta;
}

// x_j = inv(M) b_j for k right-hand sides against ONE matrix (small_solve_body's M): a workgroup of one wave per column.
__global__ __launch_bounds__(64) void k_qm_small_solve(double* __restrict__ x, double* __restrict__ info,
                                                       const double* __restrict__ M1, int ld1, int off1,
                                                       const double* __restrict__ M2, double s2,
                                                       const double* __restrict__ B, int r)
{
    const int64_t j = blockIdx.x;
    small_solve_body(x + j * r, info + j, M1, ld1, off1, M2, s2, B + j * r, 1, r);
}

// ---- the operator, block by block (k_qn_res_x / _s / _l for a column block):  out = K v, or rhs - K v where rhs != NULL
//   x :  zeta v_x - W t + J v_l            T[j*r ..] = inv(M) W'v_x,  Jv = J v_l (ld ldjv)
__global__ __launch_bounds__(256) void k_qm_res_x(double* __restrict__ out, int64_t ldo, const double* __restrict__ rhs, int64_t ldr,
                                                  const double* __restrict__ v, int64_t ldv, const double* __restrict__ V, int rr,
                                                  const double* __restrict__ T, int r, const double* __restrict__ Jv, int64_t ldjv,
                                                  double zeta, int64_t n, int64_t kcols)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const double* row = V + k * rr;
    for (int64_t j = blockIdx.y; j < kcols; j += gridDim.y) {
        const double* t = T + j * r;
        double a = fma(zeta, v[k + j * ldv], Jv[k + j * ldjv]);
        for (int c = 0; c < r; ++c) a = fma(-row[1 + c], t[c], a);
        out[k + j * ldo] = rhs ? rhs[k + j * ldr] - a : a;
    }
}
//   s :  Sigma v_s - v_li  (rows n .. n+mi-1);   l :  J'v_x - [0 ; v_s]  (rows n+mi .. N-1),  Jtv = J'v_x (ld ldp)
__global__ __launch_bounds__(256) void k_qm_res_sl(double* __restrict__ out, int64_t ldo, const double* __restrict__ rhs, int64_t ldr,
                                                   const double* __restrict__ v, int64_t ldv, double sgn_l,
                                                   const double* __restrict__ sig, const double* __restrict__ Jtv, int64_t ldp,
                                                   int64_t n, int64_t me, int64_t mi, int64_t kcols)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= 2 * mi + me) return;
    for (int64_t j = blockIdx.y; j < kcols; j += gridDim.y) {
        const double* vj = v + j * ldv;
        double a;
        if (i < mi) a = fma(sig[i], vj[n + i], -(sgn_l * vj[n + mi + me + i]));
        else {
            const int64_t c = i - mi;
            a = Jtv[c + j * ldp];
            if (c >= me) a -= vj[n + (c - me)];
        }
        out[n + i + j * ldo] = rhs ? rhs[n + i + j * ldr] - a : a;
    }
}

// ---- the kept-state solve, column by column the arithmetic of qn_solve_dev
// Y (p_pad x kcols, holding J'b_x) -> the right-hand side of the block solve, k_lb_rhs's column 0; zero on the padding rows
__global__ __launch_bounds__(256) void k_qm_rhs(double* __restrict__ Y, int64_t ldp, const double* __restrict__ B, int64_t ldb,
                                                const double* __restrict__ sig, double zeta, int64_t p, int64_t me, int64_t n,
                                                int64_t mi, int64_t kcols)
{
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= ldp) return;
    for (int64_t j = blockIdx.y; j < kcols; j += gridDim.y) {
        const double* b = B + j * ldb;
        double v = 0.0;
        if (c < p) {
            v = Y[c + j * ldp];
            v -= zeta * b[n + mi + c];
            if (c >= me) v -= zeta * b[n + (c - me)] / sig[c - me];
        }
        Y[c + j * ldp] = v;
    }
}
// u = y + X00 v11 in place on Y (R: the direction's solved columns, 1.. = X00);  x_lambda = u;  x_s = (b_s + u_i) / Sigma
__global__ __launch_bounds__(256) void k_qm_comb_ls(double* __restrict__ X, int64_t ldx, double* __restrict__ Y, int64_t ldp,
                                                    const double* __restrict__ R, int64_t ldr, int64_t p, int64_t me, int64_t n,
                                                    int64_t mi, const double* __restrict__ B, int64_t ldb,
                                                    const double* __restrict__ sig, const double* __restrict__ V11, int r,
                                                    int64_t kcols)
{
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= p) return;
    for (int64_t j = blockIdx.y; j < kcols; j += gridDim.y) {
        const double* v = V11 + j * r;
        double u = Y[c + j * ldp];
        for (int a = 0; a < r; ++a) u = fma(R[c + (int64_t)(1 + a) * ldr], v[a], u);
        Y[c + j * ldp] = u;
        X[n + mi + c + j * ldx] = u;
        if (c >= me) X[n + (c - me) + j * ldx] = (B[n + (c - me) + j * ldb] + u) / sig[c - me];
    }
}
// x_x = (b_x - W v11 - J u) / zeta        (k_lb_comb_x with Ju; column 0 of V is not read: b_x comes from the caller's block)
__global__ __launch_bounds__(256) void k_qm_comb_x(double* __restrict__ X, int64_t ldx, const double* __restrict__ B, int64_t ldb,
                                                   const double* __restrict__ V, int rr, int64_t n, const double* __restrict__ V11,
                                                   int r, double a0, const double* __restrict__ Ju, int64_t ldju, int64_t kcols)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const double* row = V + k * rr;
    for (int64_t j = blockIdx.y; j < kcols; j += gridDim.y) {
        const double* v = V11 + j * r;
        double t = B[k + j * ldb] - Ju[k + j * ldju];
        for (int c = 0; c < r; ++c) t = fma(-row[1 + c], v[c], t);
        X[k + j * ldx] = t * a0;
    }
}

// ss[2 j] = |R_j|_2^2, ss[2 j + 1] = |B_j|_2^2: one workgroup per column, thread t adds the entries t + 256 i in ascending i,
// the block sums its 256 values in a tree through shared memory.
__global__ __launch_bounds__(256) void k_qm_sumsq2(double* __restrict__ ss, const double* __restrict__ R, int64_t ldr,
                                                   const double* __restrict__ B, int64_t ldb, int64_t N)
{
    __shared__ double sm[2][256];
    const int64_t j = blockIdx.x;
    double t0 = 0.0, t1 = 0.0;
    for (int64_t i = threadIdx.x; i < N; i += 256) {
        const double a = R[i + j * ldr], b = B[i + j * ldb];
        t0 = fma(a, a, t0); t1 = fma(b, b, t1);
    }
    sm[0][threadIdx.x] = t0; sm[1][threadIdx.x] = t1;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) { sm[0][threadIdx.x] += sm[0][threadIdx.x + off]; sm[1][threadIdx.x] += sm[1][threadIdx.x + off]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { ss[2 * j] = sm[0][0]; ss[2 * j + 1] = sm[1][0]; }
}

// dst[i + j*ldd] = (i >= first_l ? sgn_l : 1) * src[i + j*lds]: a column block out of the library, rows 0 .. N-1 of each column
// (dst may be src)
__global__ __launch_bounds__(256) void k_qm_copy_flip(double* dst, int64_t ldd, const double* src,
                                                      int64_t lds, int64_t N, int64_t first_l, double sgn_l, int64_t kcols)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    for (int64_t j = blockIdx.y; j < kcols; j += gridDim.y) {
        const double v = src[i + j * lds];
        dst[i + j * ldd] = i >= first_l ? sgn_l * v : v;
    }
}

}  // namespace pyipm
