// kernels_bsolve.hpp -- the kept factors of a batched handle as a solver (included from kernels_batched.hpp):
// k right-hand sides per problem against the factor its last step left (k_b_solve_many), the KKT product of every problem
// from the staged blocks for k columns (k_b_kkt_matvec; its arithmetic is b_kkt_rows of kernels_batched.hpp, k_b_berr's), and
// the two small kernels of the per-problem condition estimate (start vectors, norm + normalisation).
// Plain launches: no atomics, no waits between workgroups; every sum runs over a partition and in an order the problem's sizes
// alone decide, and a column's arithmetic never reads another column -- its bits depend neither on k, nor on its place among
// the columns, nor on the batch size or the problem's place in the batch.
#pragma once

namespace pyipm {

constexpr int BS_W = 16;            // right-hand-side columns of a chunk (the N of the 16 x 16 x 4 product)
constexpr int BS_S = BS_W + 1;      // doubles between two rows of the chunk in shared memory: the loads / stores that walk along a
                                    // column (one lane per row) fall into 32 different bank pairs instead of one, the operand reads
                                    // of the products (four rows of 16 consecutive doubles per wave) stay within one conflict
constexpr int BS_NW = 8;            // waves of a workgroup

struct BSolveIO {
    const double* rhs; int64_t ld_rhs, stride_rhs;     // column j of problem b: rhs + b stride_rhs + j ld_rhs
    double* x; int64_t ld_x, stride_x;                 // may BE rhs (same ld and stride); must not overlap it otherwise
    int64_t k;
    const int* act;                                    // NULL: every problem
    const int* form;                                   // [B]: 0 full / 1 condensed factor of the problem's last step, < 0: none yet
    int flip;
};

// acc -- a 16 x 16 strip, lane (l15, l4) holds D[l4 + 4 r][l15] -- += sum over k in [0, 64) of a(l15, k) * Yb[k][l15], k
// ascending in the matrix pipe's groups of four.  a(k): this lane's entry A[l15][k] (all 16 requested before the first
// product); rows k >= kvalid of Yb are not read (they count as zero, and so must a(k) there).
template <class LoadA>
__device__ __forceinline__ void bs_strip_mac(double4_t& acc, const double* Yb, int kvalid, LoadA a_of)
{
    const int lane = threadIdx.x & 63, l15 = lane & 15, l4 = lane >> 4;
    double a[16];
    #pragma unroll
    for (int ks = 0; ks < 16; ++ks) a[ks] = a_of(ks * 4 + l4);
    #pragma unroll
    for (int ks = 0; ks < 16; ++ks) {
        const int k = ks * 4 + l4;
        const double bop = k < kvalid ? Yb[k * BS_S + l15] : 0.0;
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ks], bop, acc, 0, 0, 0);
    }
}
__device__ __forceinline__ double4_t bs_strip_load(const double* Y, int64_t row0)
{
    const int lane = threadIdx.x & 63, l15 = lane & 15, l4 = lane >> 4;
    double4_t v;
    #pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = Y[(row0 + l4 + 4 * r) * BS_S + l15];
    return v;
}
__device__ __forceinline__ void bs_strip_store(double* Y, int64_t row0, int64_t row_end, const double4_t& v)
{
    const int lane = threadIdx.x & 63, l15 = lane & 15, l4 = lane >> 4;
    #pragma unroll
    for (int r = 0; r < 4; ++r) if (row0 + l4 + 4 * r < row_end) Y[(row0 + l4 + 4 * r) * BS_S + l15] = v[r];
}

// X_b = inv(factor_b) RHS_b for a chunk of BS_W columns: grid (B, ceil(k / BS_W)), 512 threads.  The chunk -- the rows of the
// sweep by BS_W columns, the columns behind k zero -- stays in shared memory from the load to the store (ROWS: the rows the
// instance has room for: Npad, + 64 for the condensed form's Ji-sided vector).  Forward: for every tile column u the strips of
// 16 rows below it take Y(t) -= L(t,u) Y(u) on the matrix pipe (a wave per strip, the tiles the block pattern leaves at zero
// skipped as k_b_factor skips them); block diagonal: a wave per tile, Z = inv(T) Y with k_b_solve's `nref` correction steps
// against the saved tile where the tile is flagged (the strip layout of a product IS the operand layout of the next one: no
// trip through memory); backward: Y(t) -= L(u,t)' Y(u) likewise.
// Condensed factor (form 1): each column is reduced as k_bc_prep reduces the residual (pos / cnt of the problem's step; the
// x rows' Ji (Sigma g_i + g_s) on the matrix pipe), the sweeps run over n + me + |A| rows, and the full [dx|ds|dle|dli] is
// recovered with k_b_solve's formulas (Ji' dx on the matrix pipe; g_s, g_i read again from rhs by the thread that then
// writes those two rows of x -- which is what lets x be rhs).
// A problem with act[b] == 0 or without a factor returns at once: its rows of x are not written.  flip: rows n + mi .. N - 1 negated.
template <int ROWS>
__global__ __launch_bounds__(64 * BS_NW) void k_b_solve_many(BatchPtrs bp, Geo g, int nref, BSolveIO io, BatchCond bc, double eps)
{
    __shared__ double Y[ROWS * BS_S];
    const int64_t b = blockIdx.x;
    if (io.act && !io.act[b]) return;                    // (block-uniform: no barrier is left waiting)
    const int form = io.form[b];
    if (form < 0) return;
    const bool cond = form != 0;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, l4 = lane >> 4;
    constexpr int NT = 64 * BS_NW;
    const int64_t n = g.n, me = g.me, mi = g.mi, ld = g.Npad;
    const int64_t c0 = (int64_t)blockIdx.y * BS_W;
    const int nc = (int)((io.k - c0) < BS_W ? (io.k - c0) : BS_W);
    const double* A = bp.A + b * bp.sA;
    const double* rhs = io.rhs + b * io.stride_rhs + c0 * io.ld_rhs;
    double* x = io.x + b * io.stride_x + c0 * io.ld_x;
    const int na = cond ? bc.cnt[b] : 0;
    const int64_t nrows = cond ? (n + me + na + TB - 1) / TB * TB : g.Npad;       // rows that take part in the sweeps
    const int nt = (int)(nrows / TB);
    Geo gs = g;                                          // the block pattern of the factored matrix (k_b_factor's)
    if (cond) { gs.me = me + na; gs.mi = 0; gs.N = n + gs.me; gs.Npad = nrows; }
    const double* Ji = mi ? bp.Ji + b * bp.sJi : nullptr;
    const double* sv = bp.s + b * mi;
    const double* lv = bp.lda + b * (me + mi) + me;
    const int* pos = bc.pos + b * bc.sP;
    double* T = Y + nrows * BS_S;                        // condensed: mi rows behind the sweep's (nrows + mi <= N + 63 < ROWS)

    // ---- load (and reduce) ----
    if (!cond) {
        for (int c = 0; c < BS_W; ++c)
            for (int64_t r = tid; r < nrows; r += NT) Y[r * BS_S + c] = (r < g.N && c < nc) ? rhs[c * io.ld_rhs + r] : 0.0;
    } else {
        for (int c = 0; c < BS_W; ++c) {
            const bool in = c < nc;
            const double* col = rhs + c * io.ld_rhs;
            for (int64_t r = tid; r < nrows; r += NT) {
                if (r >= n + me && r < n + me + na) continue;          // (the rows of the active set: below)
                Y[r * BS_S + c] = !in ? 0.0 : r < n ? col[r] : r < n + me ? col[n + mi + (r - n)] : 0.0;
            }
            for (int64_t k = tid; k < mi; k += NT) {
                const double gsk = in ? col[n + k] : 0.0, gik = in ? col[n + mi + me + k] : 0.0;
                if (pos[k] < 0) T[k * BS_S + c] = lv[k] / (sv[k] + eps) * gik + gsk;
                else { T[k * BS_S + c] = 0.0; Y[(n + me + pos[k]) * BS_S + c] = gik + gsk * (sv[k] + eps) / lv[k]; }
            }
        }
        __syncthreads();
        // x rows += Ji T, a strip of 16 rows per wave and trip
        for (int64_t r0 = (int64_t)wave * 16; r0 < n; r0 += 16 * BS_NW) {
            double4_t acc = bs_strip_load(Y, r0);
            const int64_t row = r0 + l15;
            for (int64_t a0 = 0; a0 < mi; a0 += 64) {
                const int kv = (int)((mi - a0) < 64 ? (mi - a0) : 64);
                bs_strip_mac(acc, T + a0 * BS_S, kv, [&](int k) { return (row < n && k < kv) ? Ji[row * bp.ldji + a0 + k] : 0.0; });
            }
            bs_strip_store(Y, r0, n, acc);
        }
    }
    // ---- forward: unit block lower triangular ----
    for (int u = 0; u + 1 < nt; ++u) {
        __syncthreads();
        const double* Yu = Y + (int64_t)u * TB * BS_S;
        for (int q = (u + 1) * 4 + wave; q < nt * 4; q += BS_NW) {
            const int t = q >> 2;
            if (!rows_active(gs, (int64_t)u * TB, (int64_t)(u + 1) * TB, (int64_t)t * TB, (int64_t)(t + 1) * TB)) continue;   // L(t,u) = 0
            const int64_t r0 = (int64_t)q * 16;
            double4_t acc = bs_strip_load(Y, r0);
            const double* Lp = A + (r0 + l15) + ((int64_t)u * TB) * ld;
            bs_strip_mac(acc, Yu, TB, [&](int k) { return -Lp[(int64_t)k * ld]; });
            bs_strip_store(Y, r0, nrows, acc);
        }
    }
    __syncthreads();
    // ---- block diagonal: z = inv(T) y, refined against the saved tile where it is flagged; a wave per tile ----
    for (int t = wave; t < nt; t += BS_NW) {
        const double* Xi = bp.Tinv + b * bp.sT + (int64_t)t * TB * TB;
        const double* Tt = bp.Tsave + b * bp.sT + (int64_t)t * TB * TB;
        const bool flagged = bp.Tflag[b * bp.sF + t] != 0.0;
        const double* Yt = Y + (int64_t)t * TB * BS_S;
        double yb[16];
        #pragma unroll
        for (int ks = 0; ks < 16; ++ks) yb[ks] = Yt[(ks * 4 + l4) * BS_S + l15];
        double4_t z[4];
        #pragma unroll
        for (int s = 0; s < 4; ++s) {
            z[s] = (double4_t){0.0, 0.0, 0.0, 0.0};
            double a[16];
            #pragma unroll
            for (int ks = 0; ks < 16; ++ks) a[ks] = Xi[(ks * 4 + l4) * TB + s * 16 + l15];
            #pragma unroll
            for (int ks = 0; ks < 16; ++ks) z[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ks], yb[ks], z[s], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);           // (one strip's operand loads in flight at a time)
        }
        if (flagged) {
            for (int it = 0; it < nref; ++it) {                           // rare: ill-conditioned tile
                // (the tiles are loaded again in every step: kept in registers across the steps -- 128 doubles per lane, which
                // is what the compiler makes of loop-invariant loads -- they spilled)
                const double* Xi_it = Xi; const double* Tt_it = Tt;
                asm volatile("" : "+v"(Xi_it), "+v"(Tt_it));
                double4_t res[4];
                #pragma unroll
                for (int s = 0; s < 4; ++s) {
                    #pragma unroll
                    for (int r = 0; r < 4; ++r) res[s][r] = yb[4 * s + r];
                    double a[16];
                    #pragma unroll
                    for (int ks = 0; ks < 16; ++ks) a[ks] = -Tt_it[(ks * 4 + l4) * TB + s * 16 + l15];
                    #pragma unroll
                    for (int ks = 0; ks < 16; ++ks) res[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ks], z[ks >> 2][ks & 3], res[s], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                }
                #pragma unroll
                for (int s = 0; s < 4; ++s) {
                    double a[16];
                    #pragma unroll
                    for (int ks = 0; ks < 16; ++ks) a[ks] = Xi_it[(ks * 4 + l4) * TB + s * 16 + l15];
                    #pragma unroll
                    for (int ks = 0; ks < 16; ++ks) z[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ks], res[ks >> 2][ks & 3], z[s], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
        #pragma unroll
        for (int s = 0; s < 4; ++s) bs_strip_store(Y, (int64_t)t * TB + s * 16, nrows, z[s]);
    }
    // ---- backward ----
    for (int u = nt - 1; u >= 1; --u) {
        __syncthreads();
        const double* Yu = Y + (int64_t)u * TB * BS_S;
        for (int q = wave; q < u * 4; q += BS_NW) {
            const int t = q >> 2;
            if (!rows_active(gs, (int64_t)t * TB, (int64_t)(t + 1) * TB, (int64_t)u * TB, (int64_t)(u + 1) * TB)) continue;   // L(u,t) = 0
            const int64_t r0 = (int64_t)q * 16;
            double4_t acc = bs_strip_load(Y, r0);
            const double* Lp = A + ((int64_t)u * TB) + (r0 + l15) * ld;
            bs_strip_mac(acc, Yu, TB, [&](int k) { return -Lp[k]; });
            bs_strip_store(Y, r0, nrows, acc);
        }
    }
    __syncthreads();
    // ---- store (and expand) ----
    if (!cond) {
        for (int c = 0; c < nc; ++c)
            for (int64_t r = tid; r < g.N; r += NT) {
                const double v = Y[r * BS_S + c];
                x[c * io.ld_x + r] = (io.flip && r >= n + mi) ? -v : v;
            }
        return;
    }
    // T <- Ji' dx, a strip of 16 inequalities per wave and trip
    for (int64_t k0 = (int64_t)wave * 16; k0 < mi; k0 += 16 * BS_NW) {
        double4_t acc = (double4_t){0.0, 0.0, 0.0, 0.0};
        const int64_t kk = k0 + l15;
        for (int64_t j0 = 0; j0 < n; j0 += 64) {
            const int kv = (int)((n - j0) < 64 ? (n - j0) : 64);
            bs_strip_mac(acc, Y + j0 * BS_S, kv, [&](int k) { return (kk < mi && k < kv) ? Ji[(j0 + k) * bp.ldji + kk] : 0.0; });
        }
        bs_strip_store(T, k0, mi, acc);
    }
    __syncthreads();
    for (int c = 0; c < nc; ++c) {
        const double* col = rhs + c * io.ld_rhs;
        double* out = x + c * io.ld_x;
        for (int64_t k = tid; k < mi; k += NT) {
            const double bs = col[n + k], b_i = col[n + mi + me + k];      // (read before this thread writes the same two rows)
            const double sg = lv[k] / (sv[k] + eps), u = T[k * BS_S + c];
            double ds, dl;
            if (pos[k] < 0) { ds = u - b_i; dl = sg * ds - bs; }
            else            { dl = Y[(n + me + pos[k]) * BS_S + c]; ds = (dl + bs) / sg; }
            out[n + k] = ds; out[n + mi + me + k] = io.flip ? -dl : dl;
        }
        for (int64_t r = tid; r < n; r += NT) out[r] = Y[r * BS_S + c];
        for (int64_t a = tid; a < me; a += NT) { const double v = Y[(n + a) * BS_S + c]; out[n + mi + a] = io.flip ? -v : v; }
    }
}

// Y_b = Hc_b V_b (or SUB_b - Hc_b V_b) for a chunk of BMV_NC columns: grid (B, ceil(k / BMV_NC)), 256 threads.  Hc from the
// staged blocks with the problem's own pdelta / pdelta_c and Sigma = lda / (s + eps), never from the factor: b_kkt_rows, one
// pass over the blocks for the chunk's columns.  v, y, sub: raw sign (no multiplier flip); y must not overlap v.
constexpr int BMV_NC = 8;
struct BMatvecIO {
    const double* v; int64_t ld_v, stride_v;
    double* y; int64_t ld_y, stride_y;
    const double* sub; int64_t ld_s, stride_s;         // != NULL: y = sub - Hc v
    int64_t k;
    const int* act;                                    // NULL: every problem
};
__global__ __launch_bounds__(256) void k_b_kkt_matvec(BatchPtrs bp, Geo g, double eps, BMatvecIO io)
{
    const int64_t b = blockIdx.x;
    if (io.act && !io.act[b]) return;
    const int64_t c0 = (int64_t)blockIdx.y * BMV_NC, n = g.n, me = g.me, mi = g.mi;
    const int nc = (int)((io.k - c0) < BMV_NC ? (io.k - c0) : BMV_NC);
    const double* cols[BMV_NC];
    #pragma unroll
    for (int c = 0; c < BMV_NC; ++c) cols[c] = io.v + b * io.stride_v + (c0 + (c < nc ? c : nc - 1)) * io.ld_v;   // (behind k: a valid column, not stored)
    double* y = io.y + b * io.stride_y + c0 * io.ld_y;
    const double* sub = io.sub ? io.sub + b * io.stride_s + c0 * io.ld_s : nullptr;
    auto put = [&](int64_t row, int c, double v) {
        if (c < nc) y[c * io.ld_y + row] = sub ? sub[c * io.ld_s + row] - v : v;
    };
    b_kkt_rows<BMV_NC, false>(bp, g, b, eps, cols,
        [&](int64_t j, int c, double v) { put(j, c, v); },
        [&](int64_t k, int c, double vs, double vi) { put(n + k, c, vs); put(n + mi + me + k, c, vi); },
        [&](int64_t a, int c, double v) { put(n + mi + a, c, v); });
}

// x += d for the problems that take part (the correction of a refinement step); flip: the rows from neg_from on are negated
// afterwards (the last step's: refinement works on the raw solution).  grid (B, k, ceil(N / 256)).
__global__ __launch_bounds__(256) void k_b_add_cols(double* __restrict__ x, int64_t ld_x, int64_t stride_x, const double* __restrict__ d,
                                                    int64_t ld_d, int64_t stride_d, int64_t N, const int* __restrict__ act, int flip,
                                                    int64_t neg_from)
{
    const int64_t b = blockIdx.x, j = blockIdx.y, i = (int64_t)blockIdx.z * 256 + threadIdx.x;
    if (i >= N || (act && !act[b])) return;
    const double v = x[b * stride_x + j * ld_x + i] + d[b * stride_d + j * ld_d + i];
    x[b * stride_x + j * ld_x + i] = (flip && i >= neg_from) ? -v : v;
}

// dst ([B][k][N], packed) = the k columns of every problem of src: the right-hand sides kept aside when a refined solve
// runs in place (x == rhs: the first sweep overwrites them, the residuals still need them).  grid (B, k, ceil(N / 256)).
__global__ __launch_bounds__(256) void k_b_copy_cols(double* __restrict__ dst, const double* __restrict__ src, int64_t ld, int64_t stride,
                                                     int64_t N)
{
    const int64_t b = blockIdx.x, j = blockIdx.y, i = (int64_t)blockIdx.z * 256 + threadIdx.x;
    if (i < N) dst[(b * gridDim.y + j) * N + i] = src[b * stride + j * ld + i];
}

// ---- the condition estimate of every problem (pyipm_newton_rcond_batched) ----
// Start vector of an iteration, the rule of k_hash_vector (the same vector for every problem: N is the batch's), and the
// reset of the problem's running state: grid (B, ceil(N / 256)).
__global__ __launch_bounds__(256) void k_b_rc_start(double* __restrict__ w, double* __restrict__ est, double* __restrict__ alive, int64_t N,
                                                    unsigned long long seed)
{
    const int64_t b = blockIdx.x, i = (int64_t)blockIdx.y * 256 + threadIdx.x;
    if (i == 0) { est[b] = 0.0; alive[b] = 1.0; }
    if (i < N) w[b * N + i] = hash_entry(i, seed);
}

// |v_b| of every problem and the normalised vector: ONE WAVE per problem (four per block, grid ceil(B / 4)), the lanes stride
// over the N entries and the sum crosses the wave by shuffles -- a fixed order.  record: est[b] = |v_b| (an iteration's
// estimate); out != NULL: out_b = v_b / |v_b|.  A problem whose norm is zero or not finite stops there, as pyipm_newton_rcond
// leaves its loop: its estimate stays, its vector is zero from then on.
__global__ __launch_bounds__(256) void k_b_rc_norm(const double* __restrict__ v, double* __restrict__ out, double* __restrict__ est,
                                                   double* __restrict__ alive, const int* __restrict__ act, int64_t N, int B, int record)
{
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;                                      // (wave-uniform)
    if (act && !act[b]) return;
    const double* vb = v + b * N;
    double ss = 0.0;
    for (int64_t i = lane; i < N; i += 64) ss = fma(vb[i], vb[i], ss);
    ss = wave_sum(ss);
    const double nrm = sqrt(ss);
    bool live = alive[b] != 0.0;
    if (record && live && lane == 0) est[b] = nrm;
    if (!(nrm > 0.0) || !(nrm <= 1.0e300)) live = false;
    const double inv = live ? 1.0 / nrm : 0.0;
    if (out) for (int64_t i = lane; i < N; i += 64) out[b * N + i] = live ? inv * vb[i] : 0.0;
    if (lane == 0 && !live) alive[b] = 0.0;
}

// Where a factor holds static pivots it is the factor of Hc + E, E of rank n_zero at the level sqrt(eps) max|Hc|, and inverse
// iteration with it finds the smallest eigenvalue of THAT matrix -- at the level of E exactly when Hc itself is singular, which
// is the case the estimate is asked about.  For those problems the iterate x is therefore taken back to the unperturbed
// matrix with the blocks:  x' = x - inv(Hc + E) (Hc x) = inv(Hc + E) E x  lies in the n_zero-dimensional space that holds the
// null vector of a singular Hc (rank one: x' IS that vector), and |Hc x'| / |x'| -- formed from the blocks, an upper bound of
// min|w| of Hc for ANY x' -- replaces the factor's estimate where it is smaller.  k_b_rc_fix_begin selects those problems
// (mask2: takes part, full factor, n_zero > 0; the statistics record is only read) and resets their running state;
// k_b_rc_sub forms x' = xa - xb.  Problems without static pivots return at once from every launch of the correction.
__global__ __launch_bounds__(256) void k_b_rc_fix_begin(int* __restrict__ mask2, double* __restrict__ fix, double* __restrict__ alive,
                                                        const int* __restrict__ act, const int* __restrict__ form,
                                                        const DevStats* __restrict__ st, int B)
{
    const int b = (int)(blockIdx.x * 256 + threadIdx.x);
    if (b >= B) return;
    const int on = (!act || act[b]) && form[b] == 0 && st[b].n_zero > 0;
    mask2[b] = on;
    fix[b] = 1.0e308;
    if (on) alive[b] = 1.0;
}
__global__ __launch_bounds__(256) void k_b_rc_sub(double* __restrict__ xb, const double* __restrict__ xa, const int* __restrict__ mask, int64_t N)
{
    const int64_t b = blockIdx.x, i = (int64_t)blockIdx.y * 256 + threadIdx.x;      // grid (B, ceil(N / 256))
    if (i >= N || !mask[b]) return;
    xb[b * N + i] = xa[b * N + i] - xb[b * N + i];
}

// out[b] = (min|w| estimate, max|w| estimate, their ratio, sqrt(eps) max|Hc_b| from the problem's anorm word) as
// pyipm_newton_rcond forms them (min|w|: the smaller of the factor's estimate and the corrected one, fix[b]); NaN for a problem
// whose factor is a condensed one.  grid ceil(B / 256).
__global__ __launch_bounds__(256) void k_b_rc_finish(double* __restrict__ out, const double* __restrict__ est_pow, const double* __restrict__ est_inv,
                                                     const double* __restrict__ fix, const unsigned long long* __restrict__ anorm,
                                                     const int* __restrict__ act, const int* __restrict__ form, int B)
{
    const int b = (int)(blockIdx.x * 256 + threadIdx.x);
    if (b >= B || (act && !act[b])) return;
    double* o = out + 4 * (int64_t)b;
    if (form[b] != 0) { o[0] = o[1] = o[2] = o[3] = __builtin_nan(""); return; }
    const double lmax = est_pow[b], linv = est_inv[b];
    const double lmin = fmin(linv > 0.0 ? 1.0 / linv : 0.0, fix[b]);
    const double an = __longlong_as_double((long long)anorm[2 * b]);
    o[0] = lmin; o[1] = lmax; o[2] = lmax > 0.0 ? lmin / lmax : 0.0;
    o[3] = 1.4901161193847656e-08 * ((an > 0.0 && an <= 1.0e300) ? an : 1.0);
}

}  // namespace pyipm
