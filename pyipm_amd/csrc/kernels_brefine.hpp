// kernels_brefine.hpp -- adaptive refinement of the directions of a batch, every problem by its own rule (included from
// kernels_batched.hpp behind kernels_bsolve.hpp; pyipm_newton_refine_batched).  The host enqueues
// max_steps + 1 rounds of  k_b_ref_round -> k_b_solve_many (the correction, kernels_bsolve.hpp) -> k_b_ref_add  and nothing
// comes back to it in between: whether a problem is still going is a word of its own in device memory (`go`), written by the
// one workgroup that measures that problem and read by the launches behind it, whose workgroups return at once for a problem
// that has stopped -- as the step kernels do on bp.act.  Plain launches: no atomics, no waits between workgroups.  Every sum
// runs over a partition and in an order the problem's sizes alone decide, so the bits of a problem depend neither on the batch
// size, nor on its place, nor on which other problems take part or how many steps they take.
#pragma once
#include "refine_each_plan.hpp"

namespace pyipm {

struct BRefine {
    double* dz; int64_t stride;        // the iterate of problem b: dz + b stride, N doubles, multiplier rows negated when the round is FLIPPED
    double* r;                         // [B][N]: r = g - Hc x of the round, solved in place by the correction
    double* saved;                     // [B][N]: the iterate the last measured error belongs to
    int* go;                           // [B]: 1 = going, 0 = stopped or sitting out
    int* it;                           // [B]: steps taken
    double* prev;                      // [B]: the error before the last step, < 0: none yet
    double* info;                      // [B][4]: steps, error before the first step, error of the kept iterate, converged (solve_info's layout)
    int max_steps; double target;
};

// First launch of a call (grid ceil(B / 256)): which problems take part -- the caller's flags, and a factor to correct with.
__global__ __launch_bounds__(256) void k_b_ref_begin(BRefine rf, const int* __restrict__ act, const int* __restrict__ form, int B)
{
    const int b = (int)(blockIdx.x * 256 + threadIdx.x);
    if (b >= B) return;
    rf.go[b] = ((!act || act[b]) && form[b] >= 0) ? 1 : 0;
    rf.it[b] = 0;
    rf.prev[b] = -1.0;
}

// One visit of every problem that is still going: grid B, 256 threads.  r = g - Hc x from the staged blocks with the problem's
// own shifts and Sigma (b_kkt_rows: never the factor, always the full 4-block matrix whatever form the factor has), g the
// residual the last step kept (bp.rhs);  berr = |r|_2 / |g|_2 (k_b_berr's sums: per thread in the order the rows are formed,
// across the wave by shuffles, the four waves in order);  thread 0 asks refine_each_verdict and moves the problem's state;
// then the whole workgroup saves the iterate (GO ON) or takes the last step back (TAKE BACK).
template <bool FLIPPED>
__global__ __launch_bounds__(256) void k_b_ref_round(BatchPtrs bp, Geo g, double eps, BRefine rf)
{
    __shared__ double red[2][4];
    __shared__ int verdict_s;
    const int64_t b = blockIdx.x;
    if (!rf.go[b]) return;                               // (block-uniform; the word is written behind the barrier below only)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t n = g.n, me = g.me, mi = g.mi, N = g.N;
    const double* gr = bp.rhs + b * bp.sV;
    double* x = rf.dz + b * rf.stride;
    double* r = rf.r + b * N;
    double* keep = rf.saved + b * N;
    const double* const cols[1] = {x};
    double rr = 0.0, gg = 0.0;
    auto put = [&](int64_t row, double hv) {
        const double gv = gr[row], d = gv - hv;
        r[row] = d; rr += d * d; gg += gv * gv;
    };
    b_kkt_rows<1, FLIPPED>(bp, g, b, eps, cols,
        [&](int64_t j, int, double v) { put(j, v); },
        [&](int64_t k, int, double vs, double vi) { put(n + k, vs); put(n + mi + me + k, vi); },
        [&](int64_t a, int, double v) { put(n + mi + a, v); });
    rr = wave_sum(rr); gg = wave_sum(gg);
    if (lane == 0) { red[0][wave] = rr; red[1][wave] = gg; }
    __syncthreads();
    if (tid == 0) {
        const double R = red[0][0] + red[0][1] + red[0][2] + red[0][3], G = red[1][0] + red[1][1] + red[1][2] + red[1][3];
        const double berr = G > 0.0 ? sqrt(R / G) : sqrt(R);
        const int it = rf.it[b];
        const double prev = rf.prev[b];
        double* info = rf.info + 4 * b;
        if (it == 0) info[1] = berr;
        const RefineEachVerdict v = refine_each_verdict(it, prev, berr, rf.max_steps, rf.target);
        if (v == REFINE_EACH_GO_ON) { rf.prev[b] = berr; rf.it[b] = it + 1; }       // (the correction and the sum follow in this round)
        else {
            const RefineEachInfo o = refine_each_close(v, it, prev, berr, info[1]);
            info[0] = o.steps; info[2] = o.berr; info[3] = o.converged;
            rf.go[b] = 0;
        }
        verdict_s = (int)v;
    }
    __syncthreads();
    const int v = verdict_s;
    if (v == REFINE_EACH_GO_ON) for (int64_t i = tid; i < N; i += 256) keep[i] = x[i];
    else if (v == REFINE_EACH_TAKE_BACK) for (int64_t i = tid; i < N; i += 256) x[i] = keep[i];
}

// x += d for the problems still going, d = inv(factor) r in raw sign: where the iterate carries the multiplier flip, the rows
// from neg_from on take -d.  grid (B, ceil(N / 256)).
__global__ __launch_bounds__(256) void k_b_ref_add(BRefine rf, int64_t N, int flip, int64_t neg_from)
{
    const int64_t b = blockIdx.x, i = (int64_t)blockIdx.y * 256 + threadIdx.x;
    if (i >= N || !rf.go[b]) return;
    const double d = rf.r[b * N + i];
    rf.dz[b * rf.stride + i] += (flip && i >= neg_from) ? -d : d;
}

}  // namespace pyipm
