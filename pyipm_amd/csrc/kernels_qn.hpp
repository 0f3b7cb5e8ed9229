// kernels_qn.hpp — the quasi-Newton KKT operator behind the L-BFGS direction (include/pyipm_newton.h, "quasi-Newton KKT
// operator"): out = K v, the residual rhs - K v and its 2-norm, from what a direction left in the handle.
//
//   K = [ B_k   0    J        ]      B_k = zeta I - W inv(M) W',  W = [zeta S, Y] (columns 1.. of V),  M = M2
//       [ 0   Sigma  [0 | -I] ]      v = [v_x (n) | v_s (mi) | v_l (me + mi)]
//       [ J'  [0;-I]   0      ]
//
// J is read ONCE per product: k_qn_jpass forms J'v_x (a column accumulator per thread) and J v_l (a wave reduction per
// row) in the same pass over JT.  Every sum has an order the sizes alone decide (no floating-point atomics): two calls
// give the same bits.  Layouts are those of kernels_lbfgs.hpp.
#pragma once
#include "kernels_lbfgs.hpp"

namespace pyipm {

constexpr int QN_NBLK = 256;      // blocks (= partial sums) of the norm reduction

// Four row terms of one wave -> four row sums with 7 exchanges instead of 24: the halves of the wave swap what the other
// half keeps (rows 0|1 and 2|3 at distance 32, then the pairs at distance 16), the last four steps are a plain butterfly.
// Afterwards every lane holds the whole sum of row  2 * bit4(lane) + bit5(lane).
__device__ __forceinline__ double qn_reduce4(double t0, double t1, double t2, double t3, int lane)
{
    const bool h5 = lane & 32, h4 = lane & 16;
    const double r01 = (h5 ? t1 : t0) + __shfl_xor(h5 ? t0 : t1, 32, 64);
    const double r23 = (h5 ? t3 : t2) + __shfl_xor(h5 ? t2 : t3, 32, 64);
    double q = (h4 ? r23 : r01) + __shfl_xor(h4 ? r01 : r23, 16, 64);
    #pragma unroll
    for (int off = 8; off > 0; off >>= 1) q += __shfl_xor(q, off, 64);
    return q;
}

// One pass over JT (p_pad x n_pad, column-major: JT[j + k*ldj] = J[k][j]) for both products with J:
//   colpart[split*ldp + j] = sum_{k in split} JT[j + k*ldj] * vx[k]                  (J'v_x; k_tall_tn_reduce sums the splits)
//   rowpart[w*n + k]       = sum_{j in wave w} JT[j + k*ldj] * vl[j]                 (J v_l; k_qn_rowsum sums the waves)
// grid (ceil(ldp / 256), nsplit), one thread per column j, wave w = j / 64 (ldp is a multiple of 64: a wave is inside
// or outside as a whole).  vl is read as 0 on the padding columns p .. ldp-1 (JT is zero there as well).  Rows n .. n_pad-1
// are never read.  Four rows in flight, the next four loaded while these are consumed (as k_tall_tn).
__global__ __launch_bounds__(256) void k_qn_jpass(double* __restrict__ colpart, double* __restrict__ rowpart, int64_t ldp,
                                                  const double* __restrict__ JT, int64_t ldj,
                                                  const double* __restrict__ vx, const double* __restrict__ vl,
                                                  int64_t p, int64_t n, int64_t kper)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= ldp) return;
    const int lane = threadIdx.x & 63;
    const int64_t w = j >> 6;
    const int64_t k0 = (int64_t)blockIdx.y * kper;
    int64_t k1 = k0 + kper; if (k1 > n) k1 = n;
    const double vj = j < p ? vl[j] : 0.0;
    double* rp = rowpart + w * n;
    const int myrow = ((lane >> 4) & 1) * 2 + ((lane >> 5) & 1);
    double acc = 0.0;
    int64_t k = k0;
    if (k + 4 <= k1) {
        const double* col = JT + j + k * ldj;
        double a0 = col[0], a1 = col[ldj], a2 = col[2 * ldj], a3 = col[3 * ldj];
        for (; k + 4 <= k1; k += 4) {
            const int64_t kn = (k + 8 <= k1) ? k + 4 : k;                // past the end: re-read the current four (harmless)
            const double* cn = JT + j + kn * ldj;
            const double b0 = cn[0], b1 = cn[ldj], b2 = cn[2 * ldj], b3 = cn[3 * ldj];
            acc = fma(a3, vx[k + 3], fma(a2, vx[k + 2], fma(a1, vx[k + 1], fma(a0, vx[k], acc))));
            const double q = qn_reduce4(a0 * vj, a1 * vj, a2 * vj, a3 * vj, lane);
            if ((lane & 15) == 0) rp[k + myrow] = q;
            a0 = b0; a1 = b1; a2 = b2; a3 = b3;
        }
    }
    for (; k < k1; ++k) {
        const double a = JT[j + k * ldj];
        acc = fma(a, vx[k], acc);
        double t = a * vj;
        #pragma unroll
        for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off, 64);
        if (lane == 0) rp[k] = t;
    }
    colpart[(int64_t)blockIdx.y * ldp + j] = acc;
}

// out[k] = sum_w rowpart[w*n + k], w ascending
__global__ __launch_bounds__(256) void k_qn_rowsum(double* __restrict__ out, const double* __restrict__ rowpart, int64_t n, int nw)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    double t = 0.0;
    for (int w = 0; w < nw; ++w) t += rowpart[(int64_t)w * n + k];
    out[k] = t;
}

// The three blocks of K v, or of rhs - K v where rhs != NULL (rhs, v, out: full vectors of N = n + 2 mi + me).
//   x :  zeta v_x - W t + J v_l            t = inv(M) W'v_x (r entries; r = 0: B_k = zeta I),  Jv = J v_l
__global__ __launch_bounds__(256) void k_qn_res_x(double* __restrict__ out, const double* __restrict__ rhs,
                                                  const double* __restrict__ v, const double* __restrict__ V, int rr,
                                                  const double* __restrict__ t, int r, const double* __restrict__ Jv,
                                                  double zeta, int64_t n)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const double* row = V + k * rr;
    double a = fma(zeta, v[k], Jv[k]);
    for (int c = 0; c < r; ++c) a = fma(-row[1 + c], t[c], a);
    out[k] = rhs ? rhs[k] - a : a;
}
//   s :  Sigma v_s - v_li
__global__ __launch_bounds__(256) void k_qn_res_s(double* __restrict__ out, const double* __restrict__ rhs,
                                                  const double* __restrict__ v, const double* __restrict__ sig,
                                                  int64_t n, int64_t me, int64_t mi)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= mi) return;
    const double a = fma(sig[i], v[n + i], -v[n + mi + me + i]);
    out[n + i] = rhs ? rhs[n + i] - a : a;
}
//   l :  J'v_x - [0 ; v_s]                 Jtv = J'v_x (ld p_pad)
__global__ __launch_bounds__(256) void k_qn_res_l(double* __restrict__ out, const double* __restrict__ rhs,
                                                  const double* __restrict__ v, const double* __restrict__ Jtv,
                                                  int64_t n, int64_t me, int64_t mi)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= me + mi) return;
    double a = Jtv[j];
    if (j >= me) a -= v[n + (j - me)];
    out[n + mi + j] = rhs ? rhs[n + mi + j] - a : a;
}

// Sums of squares of up to two vectors of length N in one launch, two stages, fixed order: grid (QN_NBLK, nvec); thread t of
// block b adds the entries b*256 + t + i * 256 * QN_NBLK in ascending i, the block sums its 256 values in a tree through
// shared memory; k_qn_sumsq_fin adds the QN_NBLK partials of each vector, b ascending:  out[y] = |vec_y|_2^2.
__global__ __launch_bounds__(256) void k_qn_sumsq(double* __restrict__ part, const double* __restrict__ a,
                                                  const double* __restrict__ b, int64_t N)
{
    __shared__ double sm[256];
    const double* x = blockIdx.y == 0 ? a : b;
    double t = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (int64_t)256 * QN_NBLK) t = fma(x[i], x[i], t);
    sm[threadIdx.x] = t;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) sm[threadIdx.x] += sm[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[(int64_t)blockIdx.y * QN_NBLK + blockIdx.x] = sm[0];
}
__global__ __launch_bounds__(64) void k_qn_sumsq_fin(double* __restrict__ out, const double* __restrict__ part, int nvec)
{
    if ((int)threadIdx.x >= nvec) return;
    double t = 0.0;
    for (int b = 0; b < QN_NBLK; ++b) t += part[(int64_t)threadIdx.x * QN_NBLK + b];
    out[threadIdx.x] = t;
}

// dst[i] = (i >= first_l ? sgn_l : 1) * src[i]: a vector in or out of the library with its multiplier rows flipped or not
// (dst may be src)
__global__ __launch_bounds__(256) void k_qn_copy_flip(double* dst, const double* src, int64_t N,
                                                      int64_t first_l, double sgn_l)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < N) dst[i] = i >= first_l ? sgn_l * src[i] : src[i];
}
// x += d
__global__ __launch_bounds__(256) void k_qn_add(double* __restrict__ x, const double* __restrict__ d, int64_t N)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < N) x[i] += d[i];
}
// V[k*rr] = src[k]: column 0 of V belongs to the right-hand side being solved (k_lb_comb_x reads it there)
__global__ __launch_bounds__(256) void k_qn_setcol0(double* __restrict__ V, int rr, const double* __restrict__ src, int64_t n)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k < n) V[k * rr] = src[k];
}

}  // namespace pyipm
