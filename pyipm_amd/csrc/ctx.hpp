// ctx.hpp — handle, geometry and small helpers of the Newton-step core (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <new>
#include <stdexcept>
#include <map>
#include <memory>
#include <vector>
#include "../../include/pyipm_newton.h"
#include "owned.hpp"
#include "step_plan.hpp"

namespace pyipm {

constexpr int TB = PYIPM_TILE;      // 64: block-pivot tile
static_assert(TB == PLAN_TB, "step_plan.hpp states the tile on its own");
constexpr int PADG = PYIPM_PAD;     // 128: Npad granularity = row tile of the MFMA update
constexpr int BM = 128;             // MFMA update tile rows (i)
constexpr int BKU = 16;             // MFMA update k-stage
constexpr int ROWCHUNK = 2048;      // rows per block in the backward column dots

// Tuning numbers of the schedules (measured on MI355X; constants, not per-handle state)
constexpr int BULK_WAVES = 8;                 // waves per block of the BULK update tiles (8: 128 VGPRs each, 4 waves per SIMD;
                                              // 4: 241 VGPRs, 2 per SIMD: 1.5 % slower); the short side-stream launches keep 4
constexpr int HEAD_WAVES = 4;                 // waves per block of a lookahead head launched on the chain's stream (4: k_update<128,true,4>,
                                              // its own line in a kernel trace; 8: the bulk instance)
constexpr int SIDE_PRIO = 1;                  // panel-chain update launches raise their wave priority
constexpr int64_t PENDING_LEFT_ROWS = 12288;  // group chain: left-looking in-group updates of the rows below the diagonal block while more
                                              // rows than this remain below it
constexpr int64_t PENDING32_ROWS = 24576;     // a panel's pending in-group update in 32 x 64 blocks (k_inpanel_update) while at most this many
                                              // rows remain (128x128 tiles keep one CU busy for 27 us per 256 columns of K, on the chain)
constexpr int64_t HEAD32_ROWS = 6144;         // ... and the lookahead HEAD update (next group's columns, on the critical path between two
                                              // groups' chains: one 128x128 tile at K = 512 takes 132 us however few tiles there are)
constexpr int64_t HEAD32_ROWS_DIST = 16384;   // per-panel (multi-GPU) schedule: single-panel launches (the owner's head update of the
                                              // next panel, always on the critical path there) while at most this many rows remain
constexpr int64_t BULK_BN_ROWS = 20480;       // 128 x 256 tiles only for launches over more rows than this (and than persist_rows): below it the
                                              // next group's chain is no longer hidden behind the bulk launch, and beside the wide tiles (one
                                              // block per CU, every register) its kernels wait twice as long for a slot -- exposed panel 6.0
                                              // instead of 5.3 ms with the threshold at persist_rows, the step 0.8 % slower
constexpr int BULK_BN_MIN_K = 512;            // ... and with at least this K (shorter ones keep 128 x 128: twice the blocks)
constexpr int TILE_FREE_CUS = 64;             // k_tile_step8: CUs assumed free beside a persistent bulk launch (units per block: 1 while the launch fits)

// Block-cyclic 1D column distribution by panels of width nb.
struct Geo {
    int64_t n, me, mi, N, Npad;
    int nb, world, rank;
    int64_t npanels;        // global panels
    int64_t ncols_local;    // columns stored on this rank
    __host__ __device__ int64_t panel_c0(int64_t p) const { return p * (int64_t)nb; }
    __host__ __device__ int64_t panel_w(int64_t p) const {
        int64_t w = Npad - p * (int64_t)nb;
        return w < nb ? w : nb;
    }
    __host__ __device__ int owner(int64_t p) const { return (int)(p % world); }
    __host__ __device__ int64_t local_c0(int64_t p) const { return (p / world) * (int64_t)nb; }
    operator PlanGeo() const { return PlanGeo{n, me, mi, Npad, nb, npanels}; }
};

// Panels aggregated per bulk trailing update (K = group * nb).  Grouping needs the group's panels on
// one rank, so it applies to single-rank handles; PYIPM_NEWTON_GROUP overrides (read at create time).
inline int default_group(int world, int nb = 256) {
    if (world > 1) return 1;
    const char* e = getenv("PYIPM_NEWTON_GROUP");
    // 8 panels of 256 since the end of round 3 (K = 2048 per bulk launch while more than TAIL_COLS columns remain, then
    // tail_group = 4): with the 128 x 256 bulk tiles -1.2 % at N = 32768, -2.7 % at N = 131072 (4 before: no difference with
    // 128 x 128 tiles).  A group's diagonal block is one chain of at most 32 tile steps: 8 x nb / 64 <= 32.
    int g = e ? atoi(e) : (nb <= 256 ? 8 : 4);
    if (g < 1) g = 1;
    if (g > 8) g = 8;
    return g;
}

inline Geo make_geo(int64_t n, int64_t me, int64_t mi, int nb, int world, int rank) {
    Geo g;
    g.n = n; g.me = me; g.mi = mi;
    g.N = n + 2 * mi + me;
    g.Npad = ((g.N + PADG - 1) / PADG) * PADG;
    if (g.Npad == 0) g.Npad = PADG;
    g.nb = nb > 0 ? nb : 256;
    g.world = world; g.rank = rank;
    g.npanels = (g.Npad + g.nb - 1) / g.nb;
    int64_t c = 0;
    for (int64_t p = rank; p < g.npanels; p += world) c += g.panel_w(p);
    g.ncols_local = c;
    return g;
}

struct DevStats {          // lives in device memory; tile kernels of one rank run serially
    long long n_neg, n_zero, n_2x2, n_pos, nonfinite;
    double d_min, d_max;
    unsigned long long growth_bits;   // bit pattern of max |L| (monotone for non-negative doubles)
};

// One launch of k_tile_chain (kernels_chain.hpp)
struct ChainGeo {
    int ta, tb, nT;          // steps [ta, tb) of a diagonal block of nT tiles
    int cpy;                 // column tiles per unit and stage a row tile is split for (5: k_tile_step's rule)
    int nR;                  // row tiles of the launch: nT, or more -- EXTRA rows right below the diagonal block whose every stage the
                             // launch applies too (per-panel schedule: the rows the next panel's owner waits for)
    const unsigned* xword; unsigned xwant;   // the extra rows may be touched once *xword has reached xwant (NULL: at once)
    unsigned base;           // epoch of the progress words: word - base = progress of THIS launch (wrap-safe compare)
    unsigned* sync;          // [0]: tiles inverted by the chain (base + t + 1 after tile t);  [1 + 4 r + y]: stages unit (r, y) completed
    unsigned* err;           // sticky: a poll timed out
    unsigned long long timeout;   // 100 MHz ticks
    unsigned long long* dbg;      // diagnostics (NULL normally; tools/chain_clock.py): 100 MHz stamps, [8 t + k] of the chain's step t,
                                  // [256 + 64 (4 r + y) + 2 tp + k] of unit (r, y)'s stage tp (CHAIN_DBG_WORDS per launch)
};
constexpr int CHAIN_DBG_WORDS = 256 + 64 * 4 * 32;

// What a handle currently holds, as one record: which staged data, matrix, factor and work vectors are valid.  Fields are read
// anywhere and written only by the transitions below, one per event; each carries the one statement of why it invalidates
// what it invalidates (DESIGN.md section 1 has the table, with the work vector every entry borrows).
struct Held {
    bool have_blocks = false, have_vectors = false;
    bool have_rhs = false;                // rhs holds g = -grad of the staged vectors
    bool assembled = false, factored = false;
    bool cond_active = false;             // the current assembled / factored matrix is the condensed one
    bool batch_stepped = false;           // batched handle: a step has been enqueued -- the problems that took part hold a factor, their
                                          // shifts and (condensed) their active sets; nothing of the solve_batched family writes any of it
    bool forward_fused = false;           // the last factor_all ran a forward substitution under itself
    bool forward_pending = false;         // v1 = the staged right-hand side, v0 (vc: condensed) = its forward pass: solve(rhs = NULL) starts at the diagonal
    bool fwd_done = false;                // the same for the distributed driver: its vloc holds the forward pass.  A field of its own: it
                                          // outlives a step_dist whose factorisation came back nonfinite, and only what writes vloc clears it
    bool have_direction = false;          // v2 holds the last sign-flipped direction (for step_lengths)
    bool ray_valid = false;               // ray_buf holds the block products of the direction ray_for (merit_ray)
    bool zeros_clean = false;             // the last writer of the places K1 need not store again (keep_zeros) was a full assembly
    bool storage_exported = false;        // kkt_storage() handed the pointer out: a holder may write into those zeros at any time,
                                          // so every assembly is a full one until set_option("keep_zeros") is called again
    bool rc_warm_valid[2] = {false, false};   // rc_warm[k] holds the vector the last adaptive condition estimate ended with
    bool ev_assemble_valid = false, ev_solve_valid = false;   // events 2-3 / 4-5 have been recorded (last_timings)
    // The reusable x-block prefix: columns [0, cB) of the storage hold L of the groups inside the x block, and
    // the snapshot holds the columns behind them as those groups left them -- a function of the staged blocks, delta and delta_c.
    bool px_valid = false;
    double px_delta = 0.0, px_delta_c = 0.0;   // ... the shifts it was recorded with
    // ... and the plan of the step that recorded it: gB, cB and, the second level (e.ok), the lambda_e groups kept as well (their
    // L in place, their W rows and everything behind them in the second snapshot).  Only ever consulted together with px_valid.
    StepPlan px_rec;
    // The recording policy: whoever restages the blocks before any step reused them is an NLP loop and stops paying for
    // snapshots; a second step on the same blocks starts them again.
    bool px_record = true;
    int px_steps = 0;                          // fused steps since the blocks were staged
    bool px_reused = false;                    // ... one of them reused the prefix
    double px_last_delta = 0.0, px_last_delta_c = 0.0;   // shifts of the last factorisation (a shift loop changes them every time: no snapshot)
    // What the last assembly decided for the factorisation that follows it (step_plan.hpp).  Reusing with `assembled`: the storage
    // holds L of the prefix in columns [0, cB) -- whoever looks at the storage as a matrix first has it completed (storage_whole).
    StepPlan plan;
    bool partial() const { return assembled && plan.kind == PX_REUSE; }

    enum : unsigned { V0 = 1, V1 = 2, V2 = 4, VLOC = 8 };
    // Somebody writes work vectors of the handle.  v0 / v1 carry a pending fused forward pass and its right-hand side, vloc the
    // distributed one; v2 is the last direction, which step_lengths, merit_info and the kept products of merit_ray refer to.
    // (v3, vc, vt, partial carry nothing between calls -- except vc with the condensed factor, which goes with v0.)
    void borrowed(unsigned v) {
        if (v & (V0 | V1)) forward_pending = false;
        if (v & VLOC) fwd_done = false;
        if (v & V2) { have_direction = false; ray_valid = false; }
    }
    // Another matrix: the kept products of merit_ray belong to the old blocks and the condition estimate starts cold.
    // stage_blocks_owned has never said so (forget = false): on a single-rank handle merit_ray / rcond after it see the old ones.
    void blocks_staged(bool forget = true) {
        have_blocks = true;
        if (px_steps > 0 && !px_reused) px_record = false;
        px_valid = false; px_steps = 0; px_reused = false;
        if (forget) { ray_valid = false; rc_warm_cold(); }
        batch_stepped = false;            // (the kept factors, shifts and active sets belong to the blocks and vectors of their step)
    }
    // g = -grad belongs to the vectors staged before, and so does the merit function along the kept ray.
    void vectors_staged() { have_vectors = true; have_rhs = false; ray_valid = false; batch_stepped = false; }
    // rhs is rewritten: a forward pass that ran on the old one is worthless.
    void residual_formed() { have_rhs = true; forward_pending = false; }
    // Assembly, in two halves around its launches.  The condensed system lives in the same storage with another layout, so the
    // zeros are gone as soon as it starts.
    // A whole assembly overwrites the x columns: the prefix is gone.
    void assemble_begun(bool condensed) { if (condensed) zeros_clean = false; else cond_active = false; px_valid = false; plan = StepPlan(); }
    void assembly_planned(const StepPlan& p) { plan = p; }
    // The slack columns re-assembled and the snapshot restored behind a valid prefix: a matrix again, its zeros as they were.
    void prefix_reassembled() { assembled = true; factored = false; forward_pending = false; }
    // Anything that may change the schedule or the order on the stream (set_option, set_stream), and a step that failed.
    void prefix_dropped() { px_valid = false; px_rec = StepPlan(); if (plan.kind == PX_RECORD) plan = StepPlan(); }
    // An assembly of a step starts / its factorisation is done.  A second one on the same blocks: the caller is no NLP loop.
    void step_begun() { if (px_steps >= 1) px_record = true; }
    void step_factored(const StepPlan& done, double delta, double delta_c) {
        ++px_steps; px_last_delta = delta; px_last_delta_c = delta_c; plan = StepPlan();
        if (done.kind == PX_REUSE) px_reused = true;
        if (done.kind == PX_RECORD) { px_valid = true; px_delta = delta; px_delta_c = delta_c; px_rec = done; }
    }

    // The zeros of a full single-rank assembly survive a factorisation of finite numbers (every update that reaches them adds an
    // exact zero); whatever else may write into the storage clears the flag.  The storage holds a matrix, no factor.
    void assemble_done(bool condensed, bool single_rank) {
        if (condensed) cond_active = true; else zeros_clean = single_rank;
        assembled = true; factored = false; forward_pending = false;
    }
    void assemble_timed() { ev_assemble_valid = true; }
    // The owner of the storage wrote a matrix into it (the L-BFGS Gram system): full layout, no residual of this handle's.
    void matrix_written() { px_valid = false; plan = StepPlan(); assembled = true; factored = false; have_rhs = false; forward_pending = false; cond_active = false; }
    void step_batched_begun(bool condensed) { cond_active = condensed; }
    // rhs = g of every problem (backward_error_batched reads it).  v2 is the staging copy of a HOST output: the directions of the
    // problems that took part (step_lengths_batched with dz = NULL reads it); a device output is the caller's tensor alone.
    void step_batched_enqueued(bool host_out) { have_rhs = true; ev_assemble_valid = true; have_direction = host_out; batch_stepped = true; }
    // Factorisation.  Per-panel phases (the caller or the distributed driver drives the panels): no promise about what gets written.
    void panel_phases_begun() { zeros_clean = false; px_valid = false; }
    void factor_begun() { forward_fused = false; }
    void forward_fused_under_factor() { forward_fused = true; }
    void forward_done_dist() { fwd_done = true; }
    void factor_enqueued() { assembled = false; }                  // the storage now holds the factor
    void factor_invalid() { zeros_clean = false; px_valid = false; }               // a chain poll timed out: anything may be in the storage
    void factor_read_back(bool nonfinite) { factored = true; if (nonfinite) zeros_clean = false; }
    void factor_timed_out() { factored = false; }                  // distributed step: the device never completed it
    // The factorisation call returns rc.  Failed: the zeros are no longer clean.  keep_forward: a fused forward pass stays
    // pending for solve(rhs = NULL) -- factor() keeps it, after a nonfinite factorisation too; step() consumes it at once.
    void factor_returned(int rc, bool keep_forward) {
        if (rc) zeros_clean = false;
        forward_pending = (rc == 0 || rc == PYIPM_E_NONFINITE) && keep_forward && forward_fused;
    }
    // v2 = dz with the reference's sign convention (or not: flip = 0 with multipliers).  The kept products of merit_ray are the OLD
    // direction's -- solve_dist has never said so (ray_survives): on a single-rank handle merit_ray(dz = NULL) after it reuses them.
    void solved(bool direction, bool ray_survives) {
        ev_solve_valid = true; have_direction = direction;
        if (!ray_survives) ray_valid = false;
    }
    void ray_formed() { ray_valid = true; }
    void ray_dropped() { ray_valid = false; }
    void rc_warm_cold() { rc_warm_valid[0] = rc_warm_valid[1] = false; }      // another or a shifted matrix, or a new buffer
    void rc_warm_kept(int phase, bool good) { rc_warm_valid[phase] = good; }
    // A holder of the pointer may write through it, now or later.
    void storage_handed_out() { zeros_clean = false; storage_exported = true; px_valid = false; }   // (... into the x columns too: no reuse either)
    void keep_zeros_set() { zeros_clean = false; storage_exported = false; }
    // An exception unwound out of the middle of a schedule: the half-done state is dropped.
    void quiesced() { factored = false; forward_pending = false; forward_fused = false; zeros_clean = false; px_valid = false; }
};

// The words of a device-driven launch (k_tile_chain, k_fwd_sweep / k_bwd_sweep, k_fwd_prefix): `words` flags and progress words
// in the layout its kernel indexes, and behind them, as the last word of the allocation, the sticky error word a poll that
// timed out sets.  factor_end reads the error word of every owner that launched since it last did, and reports `message`.
constexpr unsigned long long POLL_TIMEOUT = 200000000ull;   // a poll gives up after 2 s (100 MHz clock)
struct PollWords {
    DevBuf<unsigned> buf;
    size_t words; const char* message;
    bool used = false;                    // a launch ran since the error word was last read
    PollWords(size_t words_, const char* message_) : words(words_), message(message_) {}
    unsigned* err() const { return buf + words; }
    hipError_t allocate() { return buf.reserve(words + 1); }
    hipError_t ensure(hipStream_t st) {   // first use: allocated, the error word zeroed on `st`
        if (buf) return hipSuccess;
        const hipError_t e = allocate();
        return e != hipSuccess ? e : clear_err(st);
    }
    hipError_t arm(size_t n, hipStream_t st) { return hipMemsetAsync(buf, 0, n * sizeof(unsigned), st); }   // the first n words := 0 in front of a launch on `st`
    // The first n words := 0 for launches on ANY stream.  The fill is ordered on the NULL stream and the kernels poll from
    // non-blocking streams, which are not ordered behind it: k_chain_wait met the words of an earlier handle's life in this memory
    // -- larger epochs: "done" -- and let the rows kernels run ahead of the chain (tools/chain_stress.py).  So: wait for the fill.
    hipError_t zero_and_wait(size_t n) {
        const hipError_t e = hipMemset(buf, 0, n * sizeof(unsigned));
        return e != hipSuccess ? e : hipDeviceSynchronize();
    }
    hipError_t fetch_err(int* host, hipStream_t st) const { return hipMemcpyAsync(host, err(), sizeof(int), hipMemcpyDeviceToHost, st); }
    hipError_t clear_err(hipStream_t st) { return hipMemsetAsync(err(), 0, sizeof(unsigned), st); }
};

struct DistState;                                       // dist_impl.hpp
struct DistDelete { void operator()(DistState*) const; };   // (pyipm_dist.hip: the type is complete there)

struct Ctx {
    Geo g;
    int batch = 1;                        // problems of a batched small-system handle (kernels_batched.hpp)
    bool batched = false;                 // batched handle: single-system entry points refuse it
    int64_t b_sH = 0, b_sJe = 0, b_sJi = 0;   // batch strides (doubles) of the caller's blocks
    // per-problem parameters of a batched handle, [batch] each, carved from the workspace (ws owns it): mu, delta, delta_c and
    // the activity flag of the last step each problem took part in (k_b_begin writes them); b_in / b_in_act: where host arrays
    // of step_batched_each land before that launch ([3][batch] doubles, [batch] flags); b_alpha: staging of host step lengths
    double *b_mu = nullptr, *b_delta = nullptr, *b_delta_c = nullptr, *b_in = nullptr, *b_alpha = nullptr;
    int *b_act = nullptr, *b_in_act = nullptr;
    DevBuf<double> b_merit_buf;           // merit pieces of a batched handle (outside the workspace, allocated on first use, grown on demand):
                                          // [info B x 16 | gq B x 2 | dce B x me | dci B x mi | nu, mu, quad B each | alphas B x K | ray out B x K]
    DevBuf<double> b_solve_buf;           // scratch of solve_batched / kkt_matvec_batched / rcond_batched (outside the workspace, grown on demand):
                                          // the staged mask, staged host columns, the residual / correction of a refinement step, the
                                          // iteration vectors and running estimates of the condition estimate
    DevBuf<int> b_form;                   // [batch]: which factor each problem holds -- 0 full, 1 condensed (k_b_begin writes it), -1 none yet
    bool b_any_cond = false;              // some step of this handle ran condensed: a problem may hold a condensed factor
    int device = 0;
    hipStream_t stream = nullptr;         // the caller's: not owned
    Stream side;                          // panel lookahead stream (created on first factor)
    Event ev_head, ev_panel, ev_fwd;      // (no event of the handle is a timing event but ev, ev_prov and ev_trailing)
    Stream fwd;                           // fused forward-substitution stream
    std::vector<Event> ev_done;           // panel q factored
    int fuse_forward = 1;
    int lookahead = 2;                    // 0 none, 1 one group (two groups on a dedicated stream measured no faster: removed), 2 = 1 + the
                                          // first group's update panel by panel under its own chain where the slack block follows it (factor_all)
    Event ev_early;
    struct TileList { unsigned* dev = nullptr; unsigned count = 0;
                      Event ready; hipStream_t on = nullptr; bool seen_done = false; };   // the async upload: its event, its stream
    struct TlArena { DevBuf<unsigned> dev; PinnedBuf<unsigned> host{hipHostMallocDefault}; size_t used = 0; };   // device + pinned host memory of the lists
    std::vector<TlArena> tl_arenas;
    std::map<std::vector<int64_t>, TileList> tile_lists;   // compact tile orders of the bulk launches (geometry repeats every step)
    int skip_zeros = 1;                   // trailing updates skip tiles that the KKT block structure makes exact zeros
    int group = 1;                        // panels per bulk trailing update
    bool tail_group_user = false;         // set_option("tail_group") was called (else: 8 for systems of at most 8192 rows)
    int tail_group = 4;                   // group size once at most TAIL_COLS columns remain
    GroupSched sched;                     // group schedule (plan_groups); not active: the per-panel phases or the distributed driver drive this factorisation
    double* Wnext = nullptr;              // 64 x 64: -S of the next diagonal tile's rows, handed from the tile kernel to the scaling launch
                                          // that carries the next tile's in-panel update (k_panel_scale + NextUpd, factor_panel)
    int group_chain = 1;                  // single rank: the panels of a group are chained tile to tile (factor_group), the rows
                                          // below the group's diagonal block follow on their own stream; same bits
    Stream rest;                          // ... that stream (high priority, created on first use: ensure_rest_stream)
    std::vector<Event> ev_band;           // panel (by offset in its group): its tiles are inverted and applied inside the diagonal block
    Event ev_join, ev_main, ev_split, ev_sfast;
    int tail_split = 1;                   // reusing step: a chain group hands over to the next chain behind its own launch and the diagonal block's
                                          // share of the head (StepPlan::tail_split); PYIPM_TAIL_SPLIT=0 at create time keeps the old order
    Event ev_rows, ev_head2, ev_chain_end;   // ... the source's rows kernels are through; the rest of the head is; the source's chain launch is
    DevBuf<unsigned> tail_flag;           // ... one word: the token of the last head whose rest is through (releases the next chain's extra rows)
    unsigned tail_token = 0;
    int keep_zeros = 1;                   // K1 does not store again the zeros nothing can fill in (k_assemble, zeros_in_place)
    int tile_step = 1;                    // stepped panel schedule (kernels_panel.hpp): one launch per diagonal tile (the rows inside the
                                          // diagonal block), one for the rows below it; panels of at most 4 tiles; same bits
    int sweep_max_blocks = 0;             // test hook: cap on the workgroups of the one-launch sweeps (0 = as many as the GPU holds)
    int occ_fwd_sweep = 0, occ_bwd_sweep = 0, occ_fwd_prefix = 0, occ_fwd_range = 0;   // resident workgroups per CU of the one-launch sweeps (occupancy query, cached)
    int sweep_persist = 1;                // single rank, one right-hand side: the backward sweep as ONE device-driven launch (k_bwd_sweep)
    int bwd_slack = 1;                    // ... its chain leaves the closed-form slack panels out (bwd_chain_plan.hpp); PYIPM_BWD_SLACK=0 at create
                                          // time keeps every panel on the chain
    DevBuf<double> sweep_buf;             // ... the near sums as the column owners hand them to workgroup 0 (Npad doubles, NaN = not there yet)
    DevBuf<double> ms_buf;                // solve_many: its column blocks, partials and refinement vectors (allocated on first use, grown on demand)
    DevBuf<double> km_buf;                // kkt_matvec_many: host operands and results pass through it (allocated on first use, grown on demand)
    int ms_matvec_many = 0;               // solve_many's refinement forms Hc X through kkt_matvec_many (one launch for all columns);
                                          // PYIPM_MS_MATVEC_MANY=1 at create time
    PollWords sweep_words{3 * 4096,       // ... its flags and counters (at most 3 npanels words, zeroed before every sweep)
                          "backward sweep (k_bwd_sweep): a poll timed out in an earlier solve; its result was NaN"};
    int dist_slices = 2;                  // distributed schedule: the two-message protocol (slices ahead of the panel message: the next owner's tile
                                          // chain starts on an nb x nb message); 0 = one message per panel (rounds 1-4); collective
    double dist_timeout_s = 300.0;        // distributed step: bound on the host's wait for the device (dist_impl.hpp:bounded_wait); <= 0: none
    int dist_comm2 = 0;                   // RCCL transport: the slice messages on a second communicator of their own (set before comm_init; dist_impl.hpp:comm2_setup)
    int wide_sub = 256;                   // per-panel schedule: a panel wider than this is factored as a block of sub-panels this wide
                                          // (factor_wide_panel: the single-rank group chain inside one panel); 0 = all stages in one launch
    int reserve_cus = 16;                 // chain-bound phases: bulk updates run as persistent launches that leave this many CUs
    int64_t persist_rows = 12288;         // free for the panel chain -- while at most this many rows remain (on one rank the per-panel schedule with it
    int num_cus = 256;                    // everywhere took 140 instead of 120 ms); 0 = ordinary launches everywhere.  num_cus: of this device
    int bulk_bn = 256;                    // column width of a bulk update tile: 256 = 128 x 256 per block (8 waves x 64 x 64, one block per
                                          // CU): 22 % less L2-miss traffic than 128 x 128; the same step time on a fast box, 1.3 % less on
                                          // the slow ones (boxes differ in memory speed, not in MFMA rate); a chain kernel waits twice as
                                          // long for a slot beside it (tools/contention_probe.py), so the chain-bound phase keeps the
                                          // persistent 128 x 128 launches (bulk_bn_all = 0).  128: 128 x 128 everywhere (rounds 1-2)
    unsigned long long* dbg_buf = nullptr;   // diagnostics only
    // condensed KKT option: factor the (n+me)-dimensional system
    //   [[H + delta I + Ji Sigma Ji', Je], [Je', -delta_c I]]  instead of the full (n+2mi+me) one
    int condensed = 0;                    // requested by set_option("condensed", 1); single-rank, mi > 0
    int cond_min_refine = 0;              // refinement steps against the FULL blocks every condensed solve gets at least
                                          // (dli = Sigma ds - b_s amplifies the rounding of ds by Sigma <= cond_sigma_max)
    Geo gc;                               // geometry of the condensed system: (n, me + cond_na, 0), set by assemble
    double cond_sigma_max = 1.0e4;        // inequalities with Sigma above this stay explicit rows (-1/Sigma diagonal)
    int64_t cond_na = 0;                  // |A| of the current condensed system
    int *cond_pos = nullptr, *cond_idx = nullptr, *cond_cnt = nullptr;   // device: position in A / members / count: views, into the
    DevBuf<int> cond_store;               // workspace of a batched handle, into this (allocated on first use) of a single-system one
    DevBuf<double> Jx;                    // [Je | Ji[:, A]] (allocated on first use)
    DevBuf<double> JT; double* WT = nullptr;   // Ji' and, behind it, Sigma Ji': operands of the rank-mi update (allocated on first use)
    double *vc = nullptr, *vt = nullptr;  // condensed vector / mi-sized temporary (carved)
    double* fwd_vec = nullptr;            // vector the fused forward substitution runs on
    double t_gram = 0;                    // ms of the Ji Sigma Ji' launch (profile)
    bool provider_only = false;           // pyipm_newton_create_provider: staged blocks + vectors, products and residuals; no factorisation
    // reuse of the x-block factorisation while the staged blocks stay (Held::px_*)
    int reuse_x = 1;                      // PYIPM_REUSE_X=0 at create time switches it off; so does a snapshot that could not be allocated
    DevBuf<double> snap;                  // the snapshot, outside the workspace (allocated by the first recording step): PX_HDR doubles
                                          // (DevStats and the assembly's maximum as they stood at the boundary), then the column ranges
    int reuse_lam_e = 1;                  // the second level (the lambda_e groups kept too); PYIPM_REUSE_LAM_E=0 at create time switches it
                                          // off, a second snapshot that could not be allocated does so for the handle
    DevBuf<double> snap_e;                // the second snapshot: PX_HDR doubles (the record in front of the lambda_e groups, then their own),
                                          // W of the lambda_e groups in the rows below cE, the square [cE, Npad) as it stood behind them
    DevBuf<unsigned> diag_tiles;          // tile list of k_update<64>: the 128-row diagonal blocks of the columns [cE, Npad)
    std::vector<unsigned> diag_tiles_host; int64_t diag_tiles_n = -1;   // ... its host copy and the (Npad - cE) / 128 it was built for
    int64_t n_reused = 0, n_recorded = 0; // fused steps of this handle that reused the prefix / recorded one
    int fwd_prefix = 1;                   // a reusing step's forward substitution through the kept panels in one launch (k_fwd_prefix);
    int fwd_prefix_wgs = 96;              // PYIPM_FWD_PREFIX=0 at create time keeps the per-panel launches, =W (>= 2) sets its workgroups
    PollWords fwdp_words{4096 + 8192,     // ... its own flags and progress words (at most 4096 panels and 8192 chunks: sweeps_in_one_launch)
                         "forward sweep over the kept panels (k_fwd_prefix): a poll timed out; the direction was NaN "
                         "(PYIPM_FWD_PREFIX=0 runs it panel by panel)"};
    int fwd_range = 1;                    // ... and through the other kept panels (slack, lambda_e groups) in a second launch (k_fwd_range);
    int fwd_range_wgs = 32;               // PYIPM_FWD_RANGE=0 at create time keeps their per-panel launches, =W (>= 2) sets its workgroups
                                          // (32: a guest beside the first lambda_i chain and its head -- 16 .. 48 measure alike, 96 costs
                                          //  0.1 ms of the step: profiles/fwd_range_ab.json)
    int64_t fwd_range_key[8] = {-1, -1, -1, -1, -1, -1, -1, -1}, fwd_range_owned = 0;   // ... the chunks its owners share, and what they were counted for
    PollWords fwdr_words{4096 + 8192,     // ... its own flags and progress words
                         "forward sweep over the kept slack and lambda_e panels (k_fwd_range): a poll timed out; the direction was NaN "
                         "(PYIPM_FWD_RANGE=0 runs it panel by panel)"};
    int slack_one = 1;                    // the closed-form slack panels of a group schedule in one launch per contiguous run (k_s_panels);
                                          // PYIPM_SLACK_ONE=0 at create time keeps a launch and an event per panel
    int last_step_kind = 0;               // 0 full, 1 recording, 2 reusing
    DevBuf<char> ws;                      // the workspace: the caller's (adopted) or the library's; capacity = the bytes the geometry needs
    // carved from workspace
    double *A = nullptr, *Wbuf = nullptr, *Lbuf = nullptr, *Dinv = nullptr;
    double *Tsv = nullptr;                // the diagonal tiles T_k themselves (refinement of the block solves)
    double *Tflag = nullptr;              // per tile: 1.0 = refine block solves with it (pivot spread beyond refine_cond)
    double *rhs = nullptr, *v0 = nullptr, *v1 = nullptr, *v2 = nullptr, *partial = nullptr;
    double *v3 = nullptr;                 // adaptive refinement: the iterate before the last correction (a step that made it worse is taken back)
    double *df = nullptr, *ce = nullptr, *ci = nullptr, *s = nullptr, *lda = nullptr;
    DevStats* dstats = nullptr;
    unsigned long long* anorm = nullptr;  // device: bits of max |assembled KKT entry| (per problem for a batched handle): scale of a static pivot
    // staged blocks (device pointers; either caller-owned or library staging)
    const double *d2L = nullptr, *Je = nullptr, *Ji = nullptr;
    int64_t ld_d2L = 0, ld_Je = 0, ld_Ji = 0;
    int sharded = 0;                      // the staged blocks hold only the rows of the x-columns this rank owns (local column order)
    std::unique_ptr<DistState, DistDelete> dist;   // distributed driver (dist_impl.hpp): exchange, streams, message buffers
    DevBuf<double> stg_d2L, stg_Je, stg_Ji;        // staging of host blocks (allocated on first use)
    double mu = 0.2, eps = 2.220446049250313e-16;
    double delta = 0.0, delta_c = 0.0;
    Held held;                            // what of all this is valid right now
    // merit-function pieces (kernels_merit.hpp): scratch, the products of the current direction with the blocks (Q dx | Je' dx | Ji' dx)
    DevBuf<double> merit_buf, ray_buf;
    const double* ray_for = nullptr; bool ray_quad_given = false;
    // last solve (pyipm_newton_solve_info): refinement steps taken, |b - Hc x|/|b| before the first and after the last
    // one (-1 = not measured: a fixed-count solve), 1 = the adaptive loop met its target
    int info_steps = 0, info_converged = 0;
    double info_berr0 = -1.0, info_berr = -1.0;
    int rcond_its[2] = {0, 0};            // power / inverse iterations the last pyipm_newton_rcond took (solve_info reports them)
    DevBuf<double> rc_warm_buf;           // warm start of the adaptive condition estimate: the vectors its power / inverse
    double* rc_warm[2] = {nullptr, nullptr};   // iterations ended with last time (the next estimate starts from them): the halves of rc_warm_buf
    double refine_target = 1.0e-14;       // adaptive refinement stops at this backward error ...
    int refine_max = 8;                   // ... or after this many steps, or when a step gains less than 4x
    // options
    double pivtol_rel = 1e-14;
    bool tile_blocked_user = false;       // set_option("tile_blocked") was called: a batched handle's set_option("condensed") leaves it alone
    int tile_blocked = 1;                 // tile inversion 16 pivots at a time while Bunch-Kaufman would accept them in natural order
                                          // (tile_blocked.hpp); 0: the single sweeps of rounds 1-2 only
    int tile_waves = 8;                   // k_tile_step on 512 threads (round 5): the critical block = four chain waves + four helper waves
                                          // (diagonal tile prefetched beside the scaling product; the blocked inversion's updates and commits
                                          // beside the next elimination, tile_blocked8.hpp); 4: the 256-thread kernel of rounds 2-4.  Same bits.
    int tile_chain = 1;                   // the tile steps of a diagonal block as ONE launch of persistent workgroups per piece (k_tile_chain,
                                          // kernels_chain.hpp; round 6): 1 where the chain is exposed (first group, at most tile8_rows rows left,
                                          // the per-panel / multi-GPU schedule), 2 everywhere, 0 one launch per tile.  Same bits.
    int chain_whole = 1;                  // ... a group's (wide panel's) whole diagonal block as ONE launch: the rows below wait for the chain's
                                          // progress words on their own stream (k_chain_wait); 0: one launch per sub-panel piece, events between
    int chain_lds_kb = 100;               // ... KB of untouched dynamic shared memory per workgroup (keeps other workgroups off its CU)
    bool chain_lds_set = false;
    int chain_cpy = 5;                    // ... column tiles per unit and stage a row tile is split for
    static constexpr int CHAIN_SLOTS = 8, CHAIN_WORDS = 160;
    PollWords chain_words{CHAIN_SLOTS * CHAIN_WORDS,   // ... progress words: CHAIN_SLOTS regions used round robin, epoch-stamped
                          "tile chain (k_tile_chain): a poll timed out -- a workgroup of the chain did not become resident; this factorisation "
                          "is invalid (set_option(\"tile_chain\", 0) runs one launch per tile)"};
    unsigned chain_epoch = 0;
    ChainGeo chain_last = {};             // ... the last chain launch (factor_block hands it to k_chain_wait)
    unsigned long long* chain_dbg = nullptr; int chain_dbg_launch = 0;   // diagnostics only (option debug_chain_ptr)
    int64_t tile8_rows = 12288;           // ... used by the single-rank schedule for the first group and where at most this many rows are left
    int bc_per_problem = 1;               // batched condensed form: the Gram part by one workgroup per problem where n = 64 .. 256 allows it
    int block_refine = 2;                 // refinement steps of L T = S in the panel scaling and of T z = y in the solves
    double refine_cond = 1.0e2;           // ... applied to tiles whose pivot spread dmax/dmin exceeds this.  A heuristic: the spread is a cheap
                                          // stand-in for cond(T), not a bound on it, and a dense tile below it can still want refining.  (1e3 until the factor was checked
                                          // entrywise, tests/test_gpu_factor_entrywise.py: the spread underestimates cond(T) of a dense tile, and an
                                          // unrefined block solve at a spread between 1e2 and 1e3 left Lb 37 eps |Lb| |T| from S -- 4.4 once refined)
    int profile = 0;
    int expert = 0;                       // set_option("expert", 1): the expert switches are accepted on this handle (else PYIPM_EXPERT=1)
    // timings of last calls (ms)
    double t_assemble = 0, t_panel = 0, t_trailing = 0, t_solve = 0, t_factor = 0;
    double t_trailing_union = 0; int64_t n_trailing_real = 0;   // time with some update launch running (launches may overlap); launches that did work
    double trailing_flops = 0, trailing_area = 0; int64_t n_trailing = 0;   // area: matrix entries updated, summed over launches
    std::vector<std::pair<Event, Event>> ev_trailing;   // reused pool of timing-event pairs
    struct TrailTag { int bn; double flops, area, cbytes; };   // (area: the launch's algorithmic bytes -- C tiles once in, once out, operand panels once)
    std::vector<TrailTag> trailing_tag;   // per bulk launch of the last factorisation: which k_update instance ran, its flops / bytes
    double inst_ms[2] = {0, 0}, inst_flops[2] = {0, 0}, inst_area[2] = {0, 0}, inst_cbytes[2] = {0, 0}; int64_t inst_n[2] = {0, 0};   // [0]: 128 x 128 tiles, [1]: 128 x 256
    Event ev[8];                          // timing events
    Event ev_prov[4]; bool prov_valid[2] = {false, false}; double prov_bytes[2] = {0.0, 0.0};   // provider products
    double setup_lists_ms = 0.0; int setup_lists_n = 0;     // host time spent building tile lists (one-time per geometry; PYIPM_SETUP_TRACE)
    int debug_fault = 0;                  // test hook: 1 / 2 = the next tile-list build throws std::bad_alloc / std::runtime_error;
                                          // 3 = the message of the middle panel of the next distributed factorisation stalls (dist_impl.hpp)
    std::string err;
};

#define PYIPM_HIP(call)                                                                   \
    do {                                                                                  \
        hipError_t e__ = (call);                                                          \
        if (e__ != hipSuccess) {                                                          \
            ctx->err = std::string(#call) + ": " + hipGetErrorString(e__);                \
            return PYIPM_E_HIP;                                                           \
        }                                                                                 \
    } while (0)

#define PYIPM_KCHECK()  PYIPM_HIP(hipGetLastError())

// No C++ exception crosses the C-ABI (include/pyipm_newton.h): every extern "C" entry is a function-try-block that
// ends in one of these.  std::bad_alloc (host containers: tile lists, schedules, event pools) -> PYIPM_E_NOMEM,
// anything else -> PYIPM_E_HIP; the message goes to last_error when that itself does not throw.
template <class H>
inline void set_err_noexcept(H* h, const char* what) noexcept {
    if (!h) return;
    try { h->err = what; } catch (...) {}
}
#define PYIPM_CATCH_CORE(seterr_, ret_nomem_, ret_other_)                                              \
    catch (const std::bad_alloc&) { seterr_("out of host memory (std::bad_alloc)"); return ret_nomem_; } \
    catch (const std::exception& e__) { seterr_(e__.what()); return ret_other_; }                        \
    catch (...) { seterr_("unknown C++ exception"); return ret_other_; }
#define PYIPM_SETERR_NONE(msg_) (void)(msg_)
#define PYIPM_CATCH_NOH   PYIPM_CATCH_CORE(PYIPM_SETERR_NONE, PYIPM_E_NOMEM, PYIPM_E_HIP)
#define PYIPM_CATCH_SIZE  PYIPM_CATCH_CORE(PYIPM_SETERR_NONE, 0, 0)

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
struct Carve { size_t off = 0; size_t take(size_t bytes) { size_t o = off; off = align_up(off + bytes, 256); return o; } };

// Rows of the staged blocks a rank works on (the columns it owns: column j of the lower triangle is row j of
// triu(d2L) | Je | Ji), in local column order; kernels_assemble.hpp.
struct RowMap {
    int64_t nloc;                 // rows this rank works on
    int nb, world, rank, sharded;
    __host__ __device__ int64_t glob(int64_t r) const {
        return world == 1 ? r : ((r / nb) * world + rank) * (int64_t)nb + r % nb;
    }
    __host__ __device__ int64_t brow(int64_t r) const { return sharded ? r : glob(r); }
};
inline RowMap make_rowmap(const Geo& g, int sharded) {
    RowMap m; m.nb = g.nb; m.world = g.world; m.rank = g.rank; m.sharded = sharded;
    int64_t c = 0;
    for (int64_t p = g.rank; p < g.npanels; p += g.world) {
        const int64_t c0 = p * (int64_t)g.nb;
        if (c0 >= g.n) break;
        c += (c0 + g.nb <= g.n) ? g.nb : g.n - c0;
    }
    m.nloc = g.world == 1 ? g.n : c;
    return m;
}


// Run a section of the single-rank machinery on another geometry (the condensed system).
struct GeoSwap {
    Ctx* c; Geo saved;
    GeoSwap(Ctx* c_, const Geo& g) : c(c_), saved(c_->g) { c->g = g; }
    ~GeoSwap() { c->g = saved; }
};

}  // namespace pyipm
