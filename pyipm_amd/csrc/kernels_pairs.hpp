// kernels_pairs.hpp -- device half of the L-BFGS pair store (include/pyipm_newton.h, "pair store"; the reference's
// lbfgs_update, pyipm.py:1282-1371).  gfx950.
//
// Layout.  ONE buffer St of n rows with pitch P = 2*cap doubles (cap = memory + 1 <= 32): row k holds S[k][0..cap) and then
// Y[k][0..cap), oldest pair first, so S = St, Y = St + cap and ld = P for both.  A row is one contiguous read of at most
// 512 B: LPR = the power of two >= P (at least 4) consecutive lanes take one row, lane c of them column c of [S | Y], and a
// wavefront covers 64 / LPR rows per load.  Every product of an offer multiplies the storage by ONE vector v (dx when the
// problem is constrained: S'dx and dx'Y; dg when it is not: Y'dg and S'dg), so a lane keeps one accumulator.
//
// Determinism.  The grid (PAIRS_GBLK workgroups), the map of rows to workgroups (chunk q of PAIRS_ROWCHUNK rows belongs to
// workgroup q mod PAIRS_GBLK), the order of a lane's rows, the shuffle tree and the order in which k_pairs_reduce adds the
// workgroups' partial sums are all fixed by (n, cap): no floating-point atomics, the same bits on every run.
#pragma once
#include "ctx.hpp"

namespace pyipm {

constexpr int PAIRS_GBLK = 1024;        // workgroups of the products kernel (= partial sums per product)
constexpr int PAIRS_ROWCHUNK = 64;      // rows a workgroup takes per round; one grid round = PAIRS_GBLK * PAIRS_ROWCHUNK rows
constexpr int PAIRS_PSTRIDE = 72;       // doubles per workgroup in the partial-sum buffer: 64 columns, curv, den, padding
constexpr int PAIRS_NPROD = 66;         // 2*32 + 2: what view / reduce buffers are sized for

// log2 of the lanes per row
inline int pairs_lanes_log2(int cap) { int lg = 2; while ((1 << lg) < 2 * cap) ++lg; return lg; }

// One pass over the stored pairs.  dx = x_new - x_old, dg = g_old - g_new (first n entries) -> dxo, dgo;
// part[b][c] = sum over the rows of workgroup b of St[k][c] * v[k] for the kept columns c (column j of either half is kept
// when drop <= j < m), 0 for the others; part[b][64] = dg.dx, part[b][65] = v.v over the same rows.
__global__ __launch_bounds__(256) void k_pairs_products(double* __restrict__ part, double* __restrict__ dxo,
                                                        double* __restrict__ dgo, const double* __restrict__ St, int cap,
                                                        int m, int drop, int lg, const double* __restrict__ x_old,
                                                        const double* __restrict__ x_new, const double* __restrict__ g_old,
                                                        const double* __restrict__ g_new, int64_t n, int con)
{
    __shared__ double sv[2][PAIRS_ROWCHUNK];
    __shared__ double red[4][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lpr = 1 << lg, c = lane & (lpr - 1), sub = lane >> lg, rpw = 64 >> lg, rstep = 4 * rpw;
    const int P = 2 * cap, j = c >= cap ? c - cap : c;
    const bool act = c < P && j < m && j >= drop;
    double acc = 0.0, curv = 0.0, den = 0.0;
    const int64_t nchunk = (n + PAIRS_ROWCHUNK - 1) / PAIRS_ROWCHUNK;
    int buf = 0;
    for (int64_t q = blockIdx.x; q < nchunk; q += PAIRS_GBLK, buf ^= 1) {
        const int64_t r0 = q * PAIRS_ROWCHUNK;
        const int rows = (int)(n - r0 < PAIRS_ROWCHUNK ? n - r0 : PAIRS_ROWCHUNK);
        if (tid < rows) {                                  // (wave 0) the chunk's dx, dg: coalesced, written once
            const int64_t r = r0 + tid;
            const double dx = x_new[r] - x_old[r], dg = g_old[r] - g_new[r];
            dxo[r] = dx; dgo[r] = dg;
            const double v = con ? dx : dg;
            sv[buf][tid] = v;
            curv = fma(dg, dx, curv);
            den = fma(v, v, den);
        }
        __syncthreads();                                   // one barrier per round: sv is double-buffered
        if (act) {
            const double* base = St + r0 * P + c;
            const double* v = sv[buf];
            int lr = wave * rpw + sub;
            for (; lr + 3 * rstep < rows; lr += 4 * rstep) {     // four rows in flight per lane
                const double a0 = base[(int64_t)lr * P], a1 = base[(int64_t)(lr + rstep) * P];
                const double a2 = base[(int64_t)(lr + 2 * rstep) * P], a3 = base[(int64_t)(lr + 3 * rstep) * P];
                acc = fma(a0, v[lr], acc);
                acc = fma(a1, v[lr + rstep], acc);
                acc = fma(a2, v[lr + 2 * rstep], acc);
                acc = fma(a3, v[lr + 3 * rstep], acc);
            }
            for (; lr < rows; lr += rstep) acc = fma(base[(int64_t)lr * P], v[lr], acc);
        }
    }
    for (int o = lpr; o < 64; o <<= 1) acc += __shfl_xor(acc, o);          // the lanes of a wave that hold column c
    for (int o = 32; o >= 1; o >>= 1) { curv += __shfl_xor(curv, o); den += __shfl_xor(den, o); }
    red[wave][lane] = acc;
    __syncthreads();
    double* out = part + (int64_t)blockIdx.x * PAIRS_PSTRIDE;
    if (tid < 64) out[tid] = tid < lpr ? ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid] : 0.0;
    if (tid == 0) { out[64] = curv; out[65] = den; }       // (wave 0 alone formed dx, dg)
}

// prods = [inner (k) | cross (k) | curv | den], k = m - drop + 1, from the PAIRS_GBLK partial sums, added in workgroup order
// inside four fixed segments and the segments left to right.  One workgroup of 512 threads.
__global__ __launch_bounds__(512) void k_pairs_reduce(double* __restrict__ prods, const double* __restrict__ part, int cap,
                                                      int m, int drop, int con)
{
    __shared__ double seg[4][128];
    __shared__ double tot[128];
    const int t = threadIdx.x & 127, s = threadIdx.x >> 7;
    double a = 0.0;
    if (t < PAIRS_NPROD) {
        constexpr int per = PAIRS_GBLK / 4;
        const double* p = part + (int64_t)s * per * PAIRS_PSTRIDE + t;
        for (int b = 0; b < per; ++b) a += p[(int64_t)b * PAIRS_PSTRIDE];
    }
    seg[s][t] = a;
    __syncthreads();
    if (threadIdx.x < 128) tot[t] = ((seg[0][t] + seg[1][t]) + seg[2][t]) + seg[3][t];
    __syncthreads();
    const int kept = m - drop, k = kept + 1;
    const int oi = con ? 0 : cap, oc = con ? cap : 0;      // which half feeds `inner`, which `cross`
    const double curv = tot[64], den = tot[65];
    for (int i = threadIdx.x; i < 2 * k + 2; i += 512) {
        double v;
        if (i < kept) v = tot[oi + drop + i];
        else if (i == kept) v = den;
        else if (i < k + kept) v = tot[oc + drop + (i - k)];
        else if (i == k + kept || i == 2 * k) v = curv;
        else v = den;
        prods[i] = v;
    }
}

// An accepted pair becomes the newest column.  drop = 0: column m of both halves is written, one thread per row (grid over
// n / 256).  drop = 1 (the store is full, m = cap): every row moves one column to the left inside the lanes that hold it
// -- lane c reads column c + 1 (the last lane of a half takes dx or dg), then writes column c; a row never leaves its
// wavefront, whose loads have all returned before its first store is issued -- grid over n / (4 * rows per wave).
__global__ __launch_bounds__(256) void k_pairs_commit(double* St, int cap, int m, int drop, int lg,
                                                      const double* __restrict__ dx, const double* __restrict__ dg, int64_t n)
{
    const int P = 2 * cap;
    if (!drop) {
        const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
        if (r < n) { St[r * P + m] = dx[r]; St[r * P + cap + m] = dg[r]; }
        return;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lpr = 1 << lg, c = lane & (lpr - 1), sub = lane >> lg, rpw = 64 >> lg;
    const int64_t r = ((int64_t)blockIdx.x * 4 + wave) * rpw + sub;
    const int j = c >= cap ? c - cap : c;
    if (r >= n || c >= P || j >= m) return;
    double* row = St + r * P;
    const bool last = j + 1 == m;
    const double a = row[last ? c : c + 1];                // (no branch between the loads and the store: selects only)
    const double b = (c < cap ? dx : dg)[r];
    __builtin_amdgcn_wave_barrier();                       // the compiler keeps the loads above the store as well
    row[c] = last ? b : a;
}

}  // namespace pyipm
