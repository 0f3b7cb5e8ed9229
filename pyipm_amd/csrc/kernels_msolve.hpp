// kernels_msolve.hpp — block substitutions for MANY right-hand sides against one block-LDL' factor
// (pyipm_newton_solve_many: sym_solve_cmp with a matrix b, /root/reference/pyipm.py:18-20, 911-914).
//
// The per-panel structure of kernels_solve.hpp (fwd_panel / diag_panel / bwd_panel), with every GEMV replaced by a
// product over a block of columns, so that a tile of L is read once for MS_KB right-hand sides instead of once each:
//   forward : k_ms_fwd_diag  in-panel block substitution   Y_u -= sum_{t<u} L[u,t] Y_t         (one workgroup per MS_CW columns)
//             k_ms_fwd_gemm  rows below the panel          Y[rows] -= L[rows, panel] Y_panel   (fp64 MFMA, 64 x MS_KB tiles)
//   diagonal: k_ms_diag      Z_t = inv(T_t) Y_t, refined against T_t on flagged tiles exactly as k_diag_apply
//   backward: k_ms_bwd_part  partials over fixed MS_RCH-row chunks  P[c] = L[chunk c, panel]' X[chunk c]   (fp64 MFMA)
//             k_ms_bwd_reduce  S = sum_c P[c] in a fixed order, 64 entries x 4 chunk groups per workgroup
//             k_ms_bwd_diag  X_panel -= S, then the in-panel backward block substitution
// The column block is an operand dimension of every product and never a summation dimension: column j of the result
// takes the same operations in the same order whatever the other columns are and however many there are (bitwise
// independent of k), and no sum uses atomics.  Vectors: column j at V + j * ldv, ldv = the geometry's Npad, the column
// count padded to a multiple of MS_KB with zero columns (the driver's buffer), so no launch needs a bounds check on j.
// v_mfma_f64_16x16x4f64 operand maps: A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][j = lane & 15],
// D[i = (lane >> 4) + 4 r][j = lane & 15] -- the same as k_update's (kernels_factor.hpp).
#pragma once
#include "ctx.hpp"

namespace pyipm {

constexpr int MS_KB = 64;      // right-hand sides per column block of the MFMA products (the driver pads k to a multiple)
constexpr int MS_CW = 8;       // right-hand sides per workgroup of the one-workgroup-per-block kernels (in-panel, diagonal)
constexpr int MS_KC = 64;      // rows of K staged in shared memory per step of the products (80 KB per block: two per CU)
constexpr int MS_RCH = 128;    // rows per partial of the backward products (fixed: the partition does not depend on k; two
                               // K steps per block, so even the short launches near the end fill the GPU)
constexpr int MS_SUBW = 256;   // widest (sub-)panel the in-panel kernels take: wider panels are swept in sub-panels of this width
constexpr int MS_LSTR = 64 + 16;   // padded shared-memory row strides (doubles): rows k and k + 1 on disjoint bank halves

// can rows [r0, r1) of L in the current panel's columns be non-zero?  (active_ranges: exact zeros are not read)
__device__ __forceinline__ bool ms_rows_active(int64_t r0, int64_t r1, int64_t a0, int64_t a1, int64_t b0, int64_t b1) {
    return (r1 > a0 && r0 < a1) || (r1 > b0 && r0 < b1);
}

// In-panel forward substitution on the nbw x nbw diagonal block (nbw <= MS_SUBW) for MS_CW columns.  grid = kpad / MS_CW,
// block 512.  Step u: wave w sums the panel columns [w u 8, (w + 1) u 8) of row `lane` of tile u for all MS_CW columns (its
// at most 24 loads of L issued at once: the recursion has nt - 1 dependent steps, each one memory latency), the eight
// partial sums meet in shared memory and are added in a fixed order.
__global__ __launch_bounds__(512) void k_ms_fwd_diag(const double* __restrict__ A, int64_t ld, int64_t lc0, int64_t c0,
                                                     int nbw, double* __restrict__ V, int64_t ldv)
{
    __shared__ double ys[MS_SUBW * MS_CW];               // ys[i * MS_CW + c]
    __shared__ double ps[8][TB][MS_CW + 1];
    const int tid = threadIdx.x, row = tid & 63, w = tid >> 6;
    double* Vb = V + (int64_t)blockIdx.x * MS_CW * ldv;
    for (int e = tid; e < nbw * MS_CW; e += 512) {
        const int i = e % nbw, c = e / nbw;
        ys[i * MS_CW + c] = Vb[c0 + i + (int64_t)c * ldv];
    }
    const int nt = nbw / TB;
    for (int u = 1; u < nt; ++u) {
        __syncthreads();
        const int kq = u * 8, k0 = w * kq;               // this wave's columns of the panel: [k0, k0 + kq)
        const double* Lr = A + (c0 + (int64_t)u * TB + row) + (lc0 + k0) * ld;
        double la[3 * 8];
        #pragma unroll
        for (int k = 0; k < 3 * 8; ++k) la[k] = (k < kq) ? Lr[(int64_t)k * ld] : 0.0;
        double acc[MS_CW];
        #pragma unroll
        for (int c = 0; c < MS_CW; ++c) acc[c] = 0.0;
        #pragma unroll
        for (int k = 0; k < 3 * 8; ++k)
            if (k < kq) {
                #pragma unroll
                for (int c = 0; c < MS_CW; ++c) acc[c] = fma(la[k], ys[(k0 + k) * MS_CW + c], acc[c]);
            }
        #pragma unroll
        for (int c = 0; c < MS_CW; ++c) ps[w][row][c] = acc[c];
        __syncthreads();
        {
            const int r = tid & 63, c = tid >> 6;
            const double t = ((ps[0][r][c] + ps[1][r][c]) + (ps[2][r][c] + ps[3][r][c])) +
                             ((ps[4][r][c] + ps[5][r][c]) + (ps[6][r][c] + ps[7][r][c]));
            ys[(u * TB + r) * MS_CW + c] -= t;
        }
    }
    __syncthreads();
    for (int e = tid; e < nbw * MS_CW; e += 512) {
        const int i = e % nbw, c = e / nbw;
        Vb[c0 + i + (int64_t)c * ldv] = ys[i * MS_CW + c];
    }
}

// Rows below the panel:  Y[r, j] -= sum_{k < nbw} L[r, lc0 + k] Y[c0 + k, j].  grid = (kpad / MS_KB, row tiles of 64),
// block 256: wave w computes the 64 rows x columns [16 w, 16 w + 16) of the block's MS_KB, four 16 x 16 MFMA tiles, k
// ascending in steps of 4.  The column block is the fastest grid dimension: the blocks that share a row tile of L run
// side by side and read it from L2.
__global__ __launch_bounds__(256) void k_ms_fwd_gemm(const double* __restrict__ A, int64_t ld, int64_t lc0, int64_t c0,
                                                     int nbw, int64_t row_begin, double* __restrict__ V, int64_t ldv,
                                                     int64_t a0, int64_t a1, int64_t b0, int64_t b1)
{
    __shared__ double Ls[MS_KC][MS_LSTR];                // Ls[k][row]
    __shared__ double Ys[MS_KC][MS_LSTR];                // Ys[k][column]
    const int64_t r0 = row_begin + (int64_t)blockIdx.y * TB;
    if (!ms_rows_active(r0, r0 + TB, a0, a1, b0, b1)) return;          // structural zeros: nothing to subtract
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
    double* Vb = V + (int64_t)blockIdx.x * MS_KB * ldv;
    double4_t acc[4];
    #pragma unroll
    for (int ti = 0; ti < 4; ++ti) acc[ti] = double4_t{0.0, 0.0, 0.0, 0.0};
    // the next K step's operands are requested into registers before the MFMAs of the current one (one barrier pair per step)
    constexpr int PT = MS_KC / 4;                        // operand elements per thread and step
    double lr[PT], yr[PT];
    auto fetch = [&](int kc) {
        #pragma unroll
        for (int m = 0; m < PT; ++m) {                   // lane = row of L / of Y_panel (coalesced), PT columns per thread
            lr[m] = A[(r0 + (tid & 63)) + (lc0 + kc + (tid >> 6) + 4 * m) * ld];
            yr[m] = Vb[(c0 + kc + (tid & 63)) + (int64_t)((tid >> 6) + 4 * m) * ldv];
        }
    };
    fetch(0);
    for (int kc = 0; kc < nbw; kc += MS_KC) {
        #pragma unroll
        for (int m = 0; m < PT; ++m) { Ls[(tid >> 6) + 4 * m][tid & 63] = lr[m]; Ys[tid & 63][(tid >> 6) + 4 * m] = yr[m]; }
        __syncthreads();
        if (kc + MS_KC < nbw) fetch(kc + MS_KC);
        #pragma unroll
        for (int kk = 0; kk < MS_KC; kk += 4) {
            const double a = Ys[kk + l4][wave * 16 + l15];
            #pragma unroll
            for (int ti = 0; ti < 4; ++ti)
                acc[ti] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Ls[kk + l4][ti * 16 + l15], acc[ti], 0, 0, 0);
        }
        __syncthreads();
    }
    #pragma unroll
    for (int ti = 0; ti < 4; ++ti)
        #pragma unroll
        for (int r = 0; r < 4; ++r)
            Vb[(r0 + ti * 16 + l15) + (int64_t)(wave * 16 + l4 + 4 * r) * ldv] -= acc[ti][r];
}

// z_t = inv(T_t) y_t for every tile t, MS_CW columns per workgroup, refined nref times against T_t on flagged tiles --
// per column the operations of k_diag_apply in its order.  grid = (kpad / MS_CW, tiles), block 256 (row, q): columns
// q and q + 4.
__global__ __launch_bounds__(256) void k_ms_diag(const double* __restrict__ Dinv, const double* __restrict__ Tsave,
                                                 const double* __restrict__ Tflag, int nref, double* __restrict__ V, int64_t ldv)
{
    __shared__ double y[MS_CW][TB];
    __shared__ double w[MS_CW][TB];
    const int tid = threadIdx.x, row = tid & 63, q = tid >> 6;
    const int64_t tile = blockIdx.y;
    double* va = V + (int64_t)blockIdx.x * MS_CW * ldv + (int64_t)q * ldv + tile * TB;
    double* vb = va + 4 * ldv;
    const double ya = va[row], yb = vb[row];
    y[q][row] = ya; y[q + 4][row] = yb;
    __syncthreads();
    const double* X = Dinv + tile * (int64_t)(TB * TB);
    const double* T = Tsave + tile * (int64_t)(TB * TB);
    double za = 0.0, zb = 0.0;
    #pragma unroll 8
    for (int j = 0; j < TB; ++j) { const double x = X[j * TB + row]; za = fma(x, y[q][j], za); zb = fma(x, y[q + 4][j], zb); }
    if (Tflag[tile] == 0.0) nref = 0;                    // well-conditioned tile
    for (int it = 0; it < nref; ++it) {
        w[q][row] = za; w[q + 4][row] = zb;
        __syncthreads();
        double ra = ya, rb = yb;
        #pragma unroll 8
        for (int j = 0; j < TB; ++j) { const double t = T[j * TB + row]; ra = fma(-t, w[q][j], ra); rb = fma(-t, w[q + 4][j], rb); }
        __syncthreads();
        w[q][row] = ra; w[q + 4][row] = rb;
        __syncthreads();
        #pragma unroll 8
        for (int j = 0; j < TB; ++j) { const double x = X[j * TB + row]; za = fma(x, w[q][j], za); zb = fma(x, w[q + 4][j], zb); }
        __syncthreads();
    }
    va[row] = za; vb[row] = zb;
}

// Backward, rows below the panel: part[(c * kpad + j) * nbw + i] = sum_{r in chunk c} L[r, lc0 + i] X[r, j], chunk c =
// rows [row_begin + c MS_RCH, + MS_RCH) (clipped at Npad).  grid = (kpad / MS_KB, nbw / 64, chunks), block 256: wave w
// computes columns [16 w, 16 w + 16) x the 64 panel columns of the block, rows ascending in steps of 4.  A chunk of
// structural zeros stores zeros; 64-row pieces of exact zeros inside a chunk are skipped.
__global__ __launch_bounds__(256) void k_ms_bwd_part(const double* __restrict__ A, int64_t ld, int64_t lc0, int nbw,
                                                     int64_t row_begin, int64_t Npad, const double* __restrict__ V, int64_t ldv,
                                                     double* __restrict__ part, int64_t kpad,
                                                     int64_t a0, int64_t a1, int64_t b0, int64_t b1)
{
    __shared__ double Ls[MS_KC][MS_LSTR];                // Ls[k][panel column]
    __shared__ double Xs[MS_KC][MS_LSTR];                // Xs[k][right-hand side]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
    const int64_t j0 = (int64_t)blockIdx.x * MS_KB;
    const int i0 = blockIdx.y * 64;
    const int64_t r0 = row_begin + (int64_t)blockIdx.z * MS_RCH;
    int64_t r1 = r0 + MS_RCH; if (r1 > Npad) r1 = Npad;
    const double* Vb = V + j0 * ldv;
    double4_t acc[4];
    #pragma unroll
    for (int ti = 0; ti < 4; ++ti) acc[ti] = double4_t{0.0, 0.0, 0.0, 0.0};
    // K steps of MS_KC rows, 64-row pieces of exact zeros skipped (row_begin and Npad are multiples of 64); the next step's
    // operands are requested into registers before the MFMAs of the current one
    auto next_active = [&](int64_t rk) {
        while (rk < r1 && !ms_rows_active(rk & ~(int64_t)(TB - 1), (rk & ~(int64_t)(TB - 1)) + TB, a0, a1, b0, b1))
            rk = (rk & ~(int64_t)(TB - 1)) + TB;
        return rk;
    };
    constexpr int PT = MS_KC / 4;                        // operand elements per thread and step
    double lr[PT], xr[PT];
    auto fetch = [&](int64_t rk) {
        #pragma unroll
        for (int m = 0; m < PT; ++m) {                   // lane = row (coalesced), PT columns per thread
            const int c = (tid >> 6) + 4 * m;
            lr[m] = A[(rk + (tid & 63)) + (lc0 + i0 + c) * ld];
            xr[m] = Vb[(rk + (tid & 63)) + (int64_t)c * ldv];
        }
    };
    int64_t rk = next_active(r0);
    if (rk < r1) fetch(rk);
    while (rk < r1) {
        #pragma unroll
        for (int m = 0; m < PT; ++m) { Ls[tid & 63][(tid >> 6) + 4 * m] = lr[m]; Xs[tid & 63][(tid >> 6) + 4 * m] = xr[m]; }
        __syncthreads();
        const int64_t rn = next_active(rk + MS_KC);
        if (rn < r1) fetch(rn);
        #pragma unroll
        for (int kk = 0; kk < MS_KC; kk += 4) {
            const double a = Xs[kk + l4][wave * 16 + l15];
            #pragma unroll
            for (int ti = 0; ti < 4; ++ti)
                acc[ti] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Ls[kk + l4][ti * 16 + l15], acc[ti], 0, 0, 0);
        }
        __syncthreads();
        rk = rn;
    }
    double* P = part + ((int64_t)blockIdx.z * kpad + j0) * nbw + i0;
    #pragma unroll
    for (int ti = 0; ti < 4; ++ti)
        #pragma unroll
        for (int r = 0; r < 4; ++r)
            P[(int64_t)(wave * 16 + l4 + 4 * r) * nbw + ti * 16 + l15] = acc[ti][r];
}

// Sum of the partials of k_ms_bwd_part: out[e] = sum_c part[c * nelem + e], e = j * nbw + i.  Block 256 = 64 entries x 4 chunk
// groups: group g adds chunks g, g + 4, ... in ascending order, the four group sums are added in a fixed order.  grid =
// nelem / 64.
__global__ __launch_bounds__(256) void k_ms_bwd_reduce(const double* __restrict__ part, int nchunk, int64_t nelem,
                                                       double* __restrict__ out)
{
    __shared__ double ps[4][64];
    const int tid = threadIdx.x, g = tid >> 6;
    const int64_t e = (int64_t)blockIdx.x * 64 + (tid & 63);
    double t = 0.0;
    #pragma unroll 8
    for (int c = g; c < nchunk; c += 4) t += part[(int64_t)c * nelem + e];
    ps[g][tid & 63] = t;
    __syncthreads();
    if (g == 0) out[e] = (ps[0][tid] + ps[1][tid]) + (ps[2][tid] + ps[3][tid]);
}

// In-panel backward substitution for MS_CW columns (nbw <= MS_SUBW): x = v[panel] - sums (k_ms_bwd_reduce; NULL when no
// rows lie below), then for u = nt-1 .. 1: x_t -= L[u, t]' x_u for all t < u.  grid = kpad / MS_CW, block 512: at step u
// thread (i, h) sums rows [32 h, 32 h + 32) of tile u against panel column i (its 32 loads issued at once), the two halves
// meet in shared memory and are added in a fixed order.
__global__ __launch_bounds__(512) void k_ms_bwd_diag(const double* __restrict__ A, int64_t ld, int64_t lc0, int64_t c0,
                                                     int nbw, const double* __restrict__ sums,
                                                     double* __restrict__ V, int64_t ldv)
{
    __shared__ double xs[MS_SUBW * MS_CW];               // xs[i * MS_CW + c]
    __shared__ double ps[2][3 * TB][MS_CW + 1];
    const int tid = threadIdx.x;
    const int64_t j0 = (int64_t)blockIdx.x * MS_CW;
    double* Vb = V + j0 * ldv;
    for (int e = tid; e < nbw * MS_CW; e += 512) {
        const int i = e % nbw, c = e / nbw;
        const double t = sums ? sums[(j0 + c) * nbw + i] : 0.0;
        xs[i * MS_CW + c] = Vb[c0 + i + (int64_t)c * ldv] - t;
    }
    const int nt = nbw / TB;
    const int i = tid & 255, h = tid >> 8;
    for (int u = nt - 1; u >= 1; --u) {
        __syncthreads();
        if (i < u * TB) {
            const double* Lc = A + (c0 + (int64_t)u * TB + 32 * h) + (lc0 + i) * ld;
            double la[32];
            #pragma unroll
            for (int k = 0; k < 32; ++k) la[k] = Lc[k];
            double acc[MS_CW];
            #pragma unroll
            for (int c = 0; c < MS_CW; ++c) acc[c] = 0.0;
            #pragma unroll
            for (int k = 0; k < 32; ++k)
                #pragma unroll
                for (int c = 0; c < MS_CW; ++c) acc[c] = fma(la[k], xs[(u * TB + 32 * h + k) * MS_CW + c], acc[c]);
            #pragma unroll
            for (int c = 0; c < MS_CW; ++c) ps[h][i][c] = acc[c];
        }
        __syncthreads();
        for (int e = tid; e < u * TB * MS_CW; e += 512) {
            const int r = e / MS_CW, c = e % MS_CW;
            xs[r * MS_CW + c] -= ps[0][r][c] + ps[1][r][c];
        }
    }
    __syncthreads();
    for (int e = tid; e < nbw * MS_CW; e += 512) {
        const int r = e % nbw, c = e / nbw;
        Vb[c0 + r + (int64_t)c * ldv] = xs[r * MS_CW + c];
    }
}

// the sign flip of solve (pyipm.py:1723-1725) on rows [from, N) of k columns, in place.  1-D grid over (N - from) * k
__global__ __launch_bounds__(256) void k_ms_flip(double* __restrict__ V, int64_t ldv, int64_t from, int64_t N, int64_t k)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x, rows = N - from;
    if (e >= rows * k) return;
    double* p = V + (e / rows) * ldv + from + e % rows;
    *p = -*p;
}

// out[2 j] = |a_j|^2, out[2 j + 1] = |b_j|^2 over the first n rows of column j (columns at stride ld).  grid = k, block 1024;
// a fixed reduction tree per column.
__global__ __launch_bounds__(1024) void k_ms_sumsq2(double* __restrict__ out, const double* __restrict__ a,
                                                    const double* __restrict__ b, int64_t ld, int64_t n)
{
    __shared__ double ra[16], rb[16];
    const int tid = threadIdx.x;
    a += (int64_t)blockIdx.x * ld; b += (int64_t)blockIdx.x * ld;
    double sa = 0.0, sb = 0.0;
    for (int64_t i = tid; i < n; i += 1024) { sa = fma(a[i], a[i], sa); sb = fma(b[i], b[i], sb); }
    #pragma unroll
    for (int off = 32; off > 0; off >>= 1) { sa += __shfl_xor(sa, off, 64); sb += __shfl_xor(sb, off, 64); }
    if ((tid & 63) == 0) { ra[tid >> 6] = sa; rb[tid >> 6] = sb; }
    __syncthreads();
    if (tid == 0) {
        double ta = 0.0, tb = 0.0;
        for (int w = 0; w < 16; ++w) { ta += ra[w]; tb += rb[w]; }
        out[2 * blockIdx.x] = ta; out[2 * blockIdx.x + 1] = tb;
    }
}

}  // namespace pyipm
