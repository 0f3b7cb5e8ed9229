// kernels_kmany.hpp — Y = Hc V for MANY columns from the staged blocks in one launch (pyipm_newton_kkt_matvec_many: the
// four-block matrix of /root/reference/pyipm.py:824-842 applied to a matrix, as kkt_matvec_dev applies it to a vector).
//
// Owner-computes: a workgroup owns KM_TR rows x KM_KB columns of Y and walks, in ascending order, everything of Hc that
// lies in its rows; it is the only writer of its entries, so there are no partial buffers and no second launch:
//   x rows          : the tiles of its column of triu(d2L) above the diagonal (mirrored), the diagonal tile, the tiles of its
//                     row to the right; then its rows of Je times V_e and of Ji times V_i;  + delta v
//   lambda_e rows   : its columns of Je over all n rows (Je' V_x);  - delta_c v
//   lambda_i rows   : its columns of Ji over all n rows (Ji' V_x);  - v_s
//   s rows, pad rows: element-wise, k_matvec_tail's arithmetic
// Every block is therefore read twice per column block of KM_KB columns (the triangle once as rows and once as mirrored
// columns, a Jacobian once by the x rows and once by its multiplier rows).  Products on v_mfma_f64_16x16x4f64, tiles of
// KM_KC x 64 staged through shared memory as in kernels_msolve.hpp (same operand maps: A[i = lane & 15][k = lane >> 4] takes
// the columns of V, B[k][j = lane & 15] the rows of Hc, D[i = (lane >> 4) + 4 r][j = lane & 15]).  The column of V is an
// operand dimension and never a summation dimension, the K walk is fixed by the geometry alone: column j gets the same
// operations in the same order whatever k is, wherever j stands and whatever the other columns hold (a NaN column stays in
// its column), and no sum uses atomics.  Staged-block contract: any ld >= width, 8-byte alignment, entries below the
// diagonal of d2L and row pads are never loaded (selected out by address, not multiplied by zero).
#pragma once
#include "ctx.hpp"

namespace pyipm {

constexpr int KM_KB = 64;      // columns of V per workgroup (the column block: each staged block is read twice per KM_KB columns)
constexpr int KM_TR = 64;      // rows of Y per workgroup
constexpr int KM_KC = 64;      // K per step staged in shared memory (80 KB per workgroup: two per CU)
constexpr int KM_LSTR = 64 + 16;   // padded shared-memory row stride (doubles), as MS_LSTR

struct KmArgs {
    const double* U; int64_t ldu;          // triu(d2L), row-major
    const double* Je; int64_t lde;
    const double* Ji; int64_t ldi;
    const double* s; const double* lda;
    double eps, delta, delta_c;
    int64_t n, me, mi, N, rows_out;        // rows_out: N, or Npad (the pad rows pass through, k_matvec_tail's last case)
    const double* V; int64_t ldv;
    double* Y; int64_t ldy;
    int64_t k;
    int tx, te, ti, ts;                    // row tiles of the x, lambda_e, lambda_i and s rows (blockIdx.y in that order, the pad tile last)
};

// acc += M[rows of this tile, 0 .. Kn) * Vb[0 .. Kn, columns of this block], K ascending in steps of 4.  elem(row, c): entry
// (tile row, K index c) of the operand, 0 outside it;  lane_k(kc): the chunk at kc is contiguous along K (the lane takes the K
// index of the load) or along the tile's rows (the lane takes the row).  Block-uniform control flow; the next chunk's operands
// are requested into registers before the MFMAs of the current one.
template <class Elem, class LaneK>
__device__ __forceinline__ void km_product(double4_t (&acc)[4], double (&Ms)[KM_KC][KM_LSTR], double (&Vs)[KM_KC][KM_LSTR],
                                           int64_t Kn, const double* __restrict__ Vb, int64_t ldv, int ncol, Elem elem, LaneK lane_k)
{
    if (Kn <= 0) return;
    const int tid = threadIdx.x, L = tid & 63, q0 = tid >> 6, l15 = L & 15, l4 = L >> 4;
    constexpr int PT = KM_KC / 4;                        // operand elements per thread and step
    double mr[PT], vr[PT];
    auto fetch = [&](int64_t kc) {
        const bool lk = lane_k(kc);
        #pragma unroll
        for (int m = 0; m < PT; ++m) {
            const int q = q0 + 4 * m;
            mr[m] = lk ? elem(q, kc + L) : elem(L, kc + q);
            vr[m] = (kc + L < Kn && q < ncol) ? Vb[(kc + L) + (int64_t)q * ldv] : 0.0;
        }
    };
    fetch(0);
    for (int64_t kc = 0; kc < Kn; kc += KM_KC) {
        if (lane_k(kc)) {
            #pragma unroll
            for (int m = 0; m < PT; ++m) Ms[L][q0 + 4 * m] = mr[m];
        } else {
            #pragma unroll
            for (int m = 0; m < PT; ++m) Ms[q0 + 4 * m][L] = mr[m];
        }
        #pragma unroll
        for (int m = 0; m < PT; ++m) Vs[L][q0 + 4 * m] = vr[m];
        __syncthreads();
        if (kc + KM_KC < Kn) fetch(kc + KM_KC);
        #pragma unroll
        for (int kk = 0; kk < KM_KC; kk += 4) {
            const double a = Vs[kk + l4][q0 * 16 + l15];
            #pragma unroll
            for (int ti = 0; ti < 4; ++ti)
                acc[ti] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Ms[kk + l4][ti * 16 + l15], acc[ti], 0, 0, 0);
        }
        __syncthreads();
    }
}

// grid = (ceil(k / KM_KB), tx + te + ti + ts + (rows_out > N)), block 256: wave w computes the 64 rows x columns [16 w, 16 w + 16)
// of the block's KM_KB.  The column block is the fastest grid dimension: the workgroups that share a tile of Hc run side by side.
__global__ __launch_bounds__(256) void k_kmany(KmArgs a)
{
    __shared__ double Ms[KM_KC][KM_LSTR];                // Ms[k][row of the tile]
    __shared__ double Vs[KM_KC][KM_LSTR];                // Vs[k][column of the block]
    const int tid = threadIdx.x, L = tid & 63, wave = tid >> 6, l15 = L & 15, l4 = L >> 4;
    const int64_t n = a.n, me = a.me, mi = a.mi;
    const int64_t j0 = (int64_t)blockIdx.x * KM_KB;
    const int ncol = (int)(a.k - j0 < KM_KB ? a.k - j0 : KM_KB);
    const double* Vb = a.V + j0 * a.ldv;
    double* Yb = a.Y + j0 * a.ldy;
    int t = blockIdx.y;
    if (t >= a.tx + a.te + a.ti) {                       // element-wise tiles: the s rows, then the pad rows
        t -= a.tx + a.te + a.ti;
        int64_t i0, i1;
        if (t < a.ts) { i0 = n + (int64_t)t * KM_TR; i1 = i0 + KM_TR < n + mi ? i0 + KM_TR : n + mi; }
        else          { i0 = a.N; i1 = a.rows_out; }
        const int64_t rows = i1 - i0;
        for (int64_t e = tid; e < rows * ncol; e += 256) {
            const int64_t i = i0 + e % rows, c = e / rows;
            const double* v = Vb + c * a.ldv;
            double r;
            if (i < a.N) { const int64_t b = i - n; r = a.lda[me + b] / (a.s[b] + a.eps) * v[i] - v[n + mi + me + b]; }
            else         { r = v[i]; }
            Yb[i + c * a.ldy] = r;
        }
        return;
    }
    double4_t acc[4];
    #pragma unroll
    for (int ti = 0; ti < 4; ++ti) acc[ti] = double4_t{0.0, 0.0, 0.0, 0.0};
    int64_t y0;                                          // first row of Y of this tile
    int64_t rows;                                        // ... and how many
    if (t < a.tx) {
        const int64_t r0 = (int64_t)t * KM_TR;
        y0 = r0; rows = n - r0 < KM_TR ? n - r0 : KM_TR;
        {   // sym(triu(d2L)) V_x: entry (r, c) is U[min(r, c)][max(r, c)] -- below the diagonal nothing is loaded
            const double* U = a.U; const int64_t ld = a.ldu;
            km_product(acc, Ms, Vs, n, Vb, a.ldv, ncol,
                [=](int row, int64_t c) {
                    const int64_t r = r0 + row;
                    if (r >= n || c >= n) return 0.0;
                    return r <= c ? U[r * ld + c] : U[c * ld + r];
                },
                [=](int64_t kc) { return kc >= r0; });  // left of the diagonal tile the mirrored rows are contiguous along the tile's rows
        }
        {   // + Je V_e
            const double* M = a.Je; const int64_t ld = a.lde;
            km_product(acc, Ms, Vs, me, Vb + (n + mi), a.ldv, ncol,
                [=](int row, int64_t c) { const int64_t r = r0 + row; return (r < n && c < me) ? M[r * ld + c] : 0.0; },
                [](int64_t) { return true; });
        }
        {   // + Ji V_i
            const double* M = a.Ji; const int64_t ld = a.ldi;
            km_product(acc, Ms, Vs, mi, Vb + (n + mi + me), a.ldv, ncol,
                [=](int row, int64_t c) { const int64_t r = r0 + row; return (r < n && c < mi) ? M[r * ld + c] : 0.0; },
                [](int64_t) { return true; });
        }
    } else {
        const bool eq = t < a.tx + a.te;
        const int64_t c0 = (int64_t)(eq ? t - a.tx : t - a.tx - a.te) * KM_TR;       // first column of the Jacobian block
        const int64_t m = eq ? me : mi;
        const double* M = eq ? a.Je : a.Ji; const int64_t ld = eq ? a.lde : a.ldi;
        y0 = n + mi + (eq ? 0 : me) + c0; rows = m - c0 < KM_TR ? m - c0 : KM_TR;
        km_product(acc, Ms, Vs, n, Vb, a.ldv, ncol,                                   // J' V_x
            [=](int row, int64_t c) { const int64_t e = c0 + row; return (e < m && c < n) ? M[c * ld + e] : 0.0; },
            [](int64_t) { return false; });
    }
    // the element-wise term of the row (k_matvec_tail's, k_symv_finish's), then the one store of the entry
    const int64_t vrow = t < a.tx + a.te ? y0 : y0 - me - mi;          // x: v_x, lambda_e: v_e (the row itself); lambda_i: v_s
    #pragma unroll
    for (int ti = 0; ti < 4; ++ti)
        #pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = ti * 16 + l15, c = wave * 16 + l4 + 4 * r;
            if (row < rows && c < ncol) {
                const double v = Vb[(vrow + row) + (int64_t)c * a.ldv];
                double e;
                if (t < a.tx)             e = a.delta * v;
                else if (t < a.tx + a.te) e = -a.delta_c * v;
                else                      e = -v;
                Yb[(y0 + row) + (int64_t)c * a.ldy] = e + acc[ti][r];
            }
        }
}

}  // namespace pyipm
