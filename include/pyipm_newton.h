/*
 * pyipm_newton.h — C-ABI of the MI355X-native Newton-step core.
 *
 * The reference (jkaardal/pyipm) has no FFI: the seam this library replaces is the
 * Python method boundary inside IPM.solve(), /root/reference/pyipm.py:1717-1725:
 *
 *     g  = -self.grad(x, s, lda)                                   # :1717
 *     Hc = self.reghess(self.hess(x, s, lda))                      # :1718
 *     dz = self.sym_solve_cmp(Hc, g.reshape((g.size,1))).reshape() # :1720-1721
 *     dz[nvar+nineq:] = -dz[nvar+nineq:]                           # :1723-1725
 *
 * Each entry point below names the reference function it replaces.  Plain C types
 * only; no torch / C++ types cross this boundary; no exceptions cross it (every entry
 * point catches: std::bad_alloc -> PYIPM_E_NOMEM, anything else -> PYIPM_E_HIP).  Every
 * function returns 0 on success or a negative PYIPM_E_* code;
 * pyipm_newton_last_error() gives the message.  A handle is not thread-safe.
 *
 * Conventions
 *   n = nvar, me = neq, mi = nineq, N = n + 2*mi + me   (pyipm.py:824-825)
 *   block order [x | s | lambda_e | lambda_i]            (pyipm.py:824-842)
 *   all data fp64.  d2L is n x n ROW-major, only its UPPER triangle is read
 *   (pyipm.py:826-827); Je is n x me row-major (= dce), Ji is n x mi row-major
 *   (= dci) (pyipm.py:486-487, 500-501).
 *   Device KKT storage: column-major, lower triangle referenced, leading dimension
 *   Npad = roundup(N,128); rows/cols N..Npad-1 are an identity pad.  Read as a
 *   row-major array this is exactly triu(H) of the reference.
 *
 * Streams and synchronisation
 *   Work is enqueued on the handle's stream (create / set_stream; NULL = the default stream; the
 *   caller passes torch's current stream).  The library also runs panel work and the fused forward
 *   substitution on internal streams, always joined back into the handle's stream before an entry
 *   point's results are visible on it.  A call whose results go to DEVICE memory (PYIPM_MEM_DEVICE)
 *   returns after enqueue: it is asynchronous with respect to the host and ordered on the stream.  A
 *   call that returns data to the HOST — a PYIPM_MEM_HOST output, pyipm_factor_stats, step lengths,
 *   timings — synchronises the stream before returning, and host INPUT buffers are never read after
 *   the call returns (the library stages them).  Device input blocks passed to stage_blocks are NOT
 *   copied: their pointers are retained until the next stage_blocks / destroy.  Their CONTENTS must
 *   not change between two stage_blocks calls: the handle keeps what it factored of them (below).
 *   Restaging the same pointers is how a caller announces new contents.
 */
#ifndef PYIPM_NEWTON_H
#define PYIPM_NEWTON_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PYIPM_OK              0
#define PYIPM_E_BADARG       -1   /* invalid argument / call order            */
#define PYIPM_E_HIP          -2   /* a HIP runtime call failed                 */
#define PYIPM_E_NOMEM        -3   /* workspace missing or too small, or host memory exhausted */
#define PYIPM_E_NONFINITE    -4   /* NaN/Inf met during factorisation          */
#define PYIPM_E_NODEVICE     -5   /* no usable HIP device                      */
#define PYIPM_E_COMM         -6   /* the exchange failed (RCCL / a caller-supplied callback) or a distributed step timed out */

#define PYIPM_MEM_DEVICE      0   /* pointer is device memory (e.g. torch.Tensor.data_ptr()) */
#define PYIPM_MEM_HOST        1   /* pointer is host memory; the library stages it           */

#define PYIPM_TILE           64   /* block-pivot (diagonal tile) size          */
#define PYIPM_PAD           128   /* Npad granularity                          */

typedef struct pyipm_newton_ctx pyipm_newton_ctx;   /* opaque handle */

/* What the factorisation reports instead of the reference's eigen-inertia test
 * (reghess, pyipm.py:1378-1381, 1399): inertia from the signs of the block pivots. */
typedef struct pyipm_factor_stats {
    int64_t n_neg;     /* negative pivots  (must equal me+mi for correct inertia, pyipm.py:1381) */
    int64_t n_zero;    /* STATIC pivots: |d| <= pivtol_rel * max|its tile column|, i.e. a pivot Bunch-Kaufman could not
                          avoid INSIDE its 64x64 tile had cancelled to nothing.  It was replaced by sqrt(eps)*max|Hc| with
                          the sign its KKT block calls for (+ for x and s rows, - for multiplier rows) and is ALSO
                          counted in n_neg / n_pos by that sign.  The factor is then that of a slightly perturbed
                          matrix: solve with refine < 0 and read pyipm_newton_solve_info (see there)          */
    int64_t n_2x2;     /* 2x2 Bunch-Kaufman pivots taken inside tiles                              */
    int64_t n_pos;     /* positive pivots among the N real rows (n_neg + n_pos == N)                 */
    double  d_min;     /* min |pivot| over accepted real pivots                                     */
    double  d_max;     /* max |pivot|                                                               */
    double  growth;    /* max |entry| of the block factor L (growth monitor)                        */
    int64_t nonfinite; /* != 0 if a NaN/Inf was met                                                  */
} pyipm_factor_stats;

/* ---- lifetime ----------------------------------------------------------------------- */

/* Bytes of device workspace the handle needs for (n,me,mi) when the KKT columns are
 * distributed block-cyclically (panel width nb) over `world` ranks and this is `rank`.
 * nb must be a multiple of 128, at most 1024 (0 = default 256). */
size_t pyipm_newton_workspace_bytes(int64_t n, int64_t me, int64_t mi, int nb, int world, int rank);

/* Create a handle on HIP device `device`.  `workspace` is caller-owned device memory
 * (a torch tensor) of at least pyipm_newton_workspace_bytes(); pass NULL to let the
 * library hipMalloc it.  `stream` is a hipStream_t (NULL = default stream). */
int pyipm_newton_create(pyipm_newton_ctx** out, int64_t n, int64_t me, int64_t mi, int nb,
                        int device, int world, int rank, void* workspace, size_t workspace_bytes,
                        void* stream);
int pyipm_newton_destroy(pyipm_newton_ctx* ctx);
int pyipm_newton_set_stream(pyipm_newton_ctx* ctx, void* stream);
const char* pyipm_newton_last_error(pyipm_newton_ctx* ctx);
/* Geometry: out[0]=N, [1]=Npad, [2]=nb, [3]=npanels, [4]=local columns, [5]=world, [6]=rank. */
int pyipm_newton_geometry(pyipm_newton_ctx* ctx, int64_t out[8]);

/* ---- staging (host evaluates derivatives; pyipm.py:474-509 stays host-side) ---------- */

/* Constant-per-iteration blocks: Hessian of the Lagrangian and the constraint Jacobians.
 * Device pointers are retained (caller keeps them alive until re-staged); host pointers are
 * copied into library-owned staging and not retained.  Je/Ji may be NULL when me/mi == 0.
 * Layout of a retained device block (tests/test_gpu_strided_blocks.py): row-major, row r at ptr + r * ld doubles,
 * any ld >= the block's width, each block with its own.  The base needs the alignment of a double (8 bytes) and no
 * more, and ld may be odd.  Of d2L only the upper triangle (column >= row) is used; the entries below the diagonal
 * and the ld - width doubles that pad every row may hold anything, NaN included: no result depends on them, and no
 * result depends on ld or on the base address -- every one is bit for bit that of the packed block.  The extent that
 * must be readable is (rows - 1) * ld + width doubles.  pyipm_newton_stage_blocks_batched: the same for every problem,
 * whose block b starts at ptr + b * stride doubles (stride >= rows * ld; the members may lie in any order in memory
 * as long as that holds).  ld < width is PYIPM_E_BADARG. */
int pyipm_newton_stage_blocks(pyipm_newton_ctx* ctx, const double* d2L, int64_t ld_d2L,
                              const double* Je, int64_t ld_Je, const double* Ji, int64_t ld_Ji,
                              int memkind);
/* Per-step vectors: df(n), ce(me), ci(mi), s(mi), lda(me+mi) and the scalars mu, eps. */
int pyipm_newton_stage_vectors(pyipm_newton_ctx* ctx, const double* df, const double* ce,
                               const double* ci, const double* s, const double* lda,
                               double mu, double eps, int memkind);

/* ---- the hot path ---------------------------------------------------------------------- */

/* replaces self.grad (pyipm.py:655-668) negated as at :1717:
 *   g = -[ df - Je.lda_e - Ji.lda_i ; lda_i - mu/(s+eps) ; ce ; ci - s ]
 * g is kept on the device as the right-hand side; g_out (N doubles, may be NULL) receives it. */
int pyipm_newton_residual(pyipm_newton_ctx* ctx, double* g_out, int memkind);

/* replaces self.hess (pyipm.py:816-844) plus the diagonal shifts reghess applies
 * (pyipm.py:1383-1397): +delta on the x block, -delta_c on the lambda_e block. */
int pyipm_newton_assemble(pyipm_newton_ctx* ctx, double delta, double delta_c);

/* replaces the factorisation inside scipy.linalg.solve (pyipm.py:18-20, 1720) and the
 * eigen-inertia test of reghess (pyipm.py:1378-1381): block LDL' with 64x64 Bunch-Kaufman
 * block pivots; stats carries the inertia.  Inertia mismatch is NOT an error. */
int pyipm_newton_factor(pyipm_newton_ctx* ctx, pyipm_factor_stats* stats);

/* replaces the substitution inside sym_solve_cmp (pyipm.py:911-914, 1720-1721) and, when
 * flip != 0, the multiplier sign flip (pyipm.py:1723-1725).  rhs == NULL uses the residual
 * kept by pyipm_newton_residual.  refine > 0 adds that many steps of fp64 iterative
 * refinement against the KKT blocks.  refine < 0 = ADAPTIVE refinement: |rhs - Hc dz| / |rhs| (Hc from the
 * blocks) is measured before every step; it stops at "refine_target" (option, default 1e-14), after
 * "refine_max" steps (default 8) or when a step gains less than 4x.  This is how the solution of the
 * UNPERTURBED system is recovered from a factor with static pivots (stats.n_zero > 0): the reference's LU
 * pivots across the whole matrix (pyipm.py:18-20), the tile-local pivot search here cannot, static pivots +
 * refinement (GESP) give the same dz with the same "no shift" decision of reghess whenever Hc is
 * non-singular -- and no convergence (solve_info) when it is not, which the host treats like the
 * reference's rcond test (pyipm.py:1379-1381). */
int pyipm_newton_solve(pyipm_newton_ctx* ctx, const double* rhs, double* dz, int flip,
                       int refine, int memkind);
/* Outcome of the last solve()/step(): out[0] = refinement steps taken, out[1] = |rhs - Hc dz|/|rhs| before the
 * first step, out[2] = after the last, out[3] = 1 when the adaptive loop met its target (out[1..2] = -1 for a
 * fixed-count solve, which does not measure). */
int pyipm_newton_solve_info(pyipm_newton_ctx* ctx, double out[4]);
/* sym_solve_cmp with a matrix right-hand side (pyipm.py:18-20, 911-914): k systems against the factor of the last
 * factor().  rhs: k vectors of N doubles, vector j at rhs + j*ld_rhs (ld_rhs >= N); dz likewise at ld_dz (entries N ..
 * ld_dz-1 of each column are not written).  flip / refine / memkind as in pyipm_newton_solve, column by column.
 *   Valid: a single-rank handle with a factor (full or condensed) -- after factor() and before the next assemble().
 *   PYIPM_E_BADARG: world > 1, provider-only and batched handles, ld_rhs or ld_dz < N, no factor yet, k < 0.
 *   k == 0 returns 0 and does nothing.
 *   Column j of dz solves Hc x = rhs_j, flip applied to rows n+mi .. N-1 as in solve.  With refine >= 0 it is bit for bit
 *   independent of k and of the other columns (rhs_j alone or at any position of any batch gives the same bits; no
 *   atomics, fixed partitions) and equal to rounding -- not to the bit -- to pyipm_newton_solve of that column.  With
 *   refine < 0 the step count follows the worst column of the batch, so a column's bits depend on the others (a NaN
 *   column ends the refinement of all); two identical calls still give identical bits.
 *   refine > 0: that many steps R = B - Hc X; X += solve_many(R), Hc from the staged blocks.  refine < 0: adaptive, stops
 *   when EVERY column meets "refine_target", after "refine_max" steps or when the worst column gains less than 4x;
 *   pyipm_newton_solve_info then reports the step count and the worst column's backward errors.  A condensed factor
 *   takes at least "condensed_refine" steps, as solve does.
 *   The call leaves the factor, the kept residual, the direction of the last solve()/step() (step_lengths / merit_info /
 *   merit_ray with dz = NULL) and a pending fused forward pass alone: solve() after it returns the bits it would without it.
 *   Asynchronous on the handle's stream for device outputs; synchronises for PYIPM_MEM_HOST, host inputs are staged.
 *   Working memory for the column blocks is allocated by the library on first use and grown on demand (not part of
 *   pyipm_newton_workspace_bytes). */
int pyipm_newton_solve_many(pyipm_newton_ctx* ctx, int64_t k, const double* rhs, int64_t ld_rhs,
                            double* dz, int64_t ld_dz, int flip, int refine, int memkind);
/* Restates the quantity reghess tests (pyipm.py:1379-1381: rcond = min|w| / max|w| over the eigenvalues w of Hc, "singular"
 * when rcond <= eps) without the eigendecomposition: it_pow power iterations on Hc applied from the blocks give max|w|,
 * it_inv inverse iterations through the factor (one substitution sweep each) give min|w| (0 = defaults 6 / 3; negative =
 * ADAPTIVE, for the threshold test only: either iteration stops once two successive estimates agree to 10 %, and the
 * inverse iteration also as soon as even a pessimistic correction of its running estimate -- x 64 sqrt(N): a random start
 * vector's component along the extreme eigenvector -- leaves rcond a factor 100 above eps; the estimate returned is then
 * the running one, an over-estimate of rcond that decides "not singular" correctly).
 * out[0] = min|w| estimate (of the FACTORED matrix: with static pivots that is the perturbed one, whose smallest
 * eigenvalue sits at the perturbation level out[3] exactly when Hc itself is singular), out[1] = max|w| estimate,
 * out[2] = their ratio, out[3] = magnitude of a static pivot (sqrt(eps) max|Hc|).  Call between factor() and solve();
 * a forward substitution fused into factor() is redone by the next solve(). */
int pyipm_newton_rcond(pyipm_newton_ctx* ctx, int it_inv, int it_pow, double out[4]);
/* Device address of max |assembled entry| (one double, valid after assemble): the scale of a static pivot.  Ranks of
 * a distributed factorisation reduce it (MAX) so that every rank perturbs alike. */
int pyipm_newton_anorm(pyipm_newton_ctx* ctx, double** dev_ptr);

/* y = Hc * v with Hc applied from the staged blocks (never from the factor): used by the
 * refinement step and by the parity tests (backward error). */
int pyipm_newton_kkt_matvec(pyipm_newton_ctx* ctx, const double* v, double* y, int memkind);
/* Y = Hc * V for k columns in one pass over the staged blocks: column j computes y_j = Hc v_j, v_j at v + j*ld_v, y_j at
 * y + j*ld_y (ld_v, ld_y >= N; entries N .. ld_y-1 of each output column are not written).  Hc is exactly what
 * pyipm_newton_kkt_matvec applies: the full four-block matrix of pyipm.py:824-842 from the staged blocks and the staged s,
 * lda, eps with the handle's current delta / delta_c, raw sign (no flip), never the factor -- the full matrix on a
 * condensed handle too.  Replaces k calls of pyipm_newton_kkt_matvec (residuals and backward errors of k solutions, the
 * check of a solve_many): triu(d2L), Je and Ji are each read twice per 64 columns instead of once per column, and the
 * products run on the fp64 matrix pipe.
 *   Valid: a single-rank single-system handle (a provider-only one included) with blocks and vectors staged.
 *   PYIPM_E_BADARG, each with a last_error text: a batched handle, world > 1, blocks or vectors not staged, NULL v or y,
 *   ld_v or ld_y < N, k < 0, y overlapping v, a bad memkind.  k == 0 returns 0 and does nothing.
 *   Column j is bit for bit independent of k, of its place among the columns and of what the other columns hold (a NaN
 *   column stays in its column; no atomics, a summation order the geometry alone decides); two identical calls give
 *   identical bits.  It equals pyipm_newton_kkt_matvec of that column to rounding, not to the bit.
 *   The call writes no work vector and changes nothing the handle holds: the factor, the kept residual, the direction of the
 *   last solve()/step() and a pending fused forward pass are left alone; solve() after it returns the bits it would without it.
 *   Device pointers: asynchronous on the handle's stream, v and y used where they are.  PYIPM_MEM_HOST: staged through a
 *   buffer the library allocates on first use and grows on demand (not part of pyipm_newton_workspace_bytes); the call
 *   synchronises.
 *   PYIPM_MS_MATVEC_MANY=1 in the environment at create time sends the residual product of pyipm_newton_solve_many's
 *   refinement through this routine (one launch instead of k products); unset, solve_many is unchanged bit for bit. */
int pyipm_newton_kkt_matvec_many(pyipm_newton_ctx* ctx, int64_t k, const double* v, int64_t ld_v,
                                 double* y, int64_t ld_y, int memkind);

/* Fused convenience: residual + assemble + factor + solve + flip = pyipm.py:1717-1725
 * without regularisation retries (the host loop re-issues assemble/factor with new shifts). */
int pyipm_newton_step(pyipm_newton_ctx* ctx, double delta, double delta_c, int refine,
                      double* dz, pyipm_factor_stats* stats, int memkind);
/* Reuse of the x-block factorisation.  In the order x | s | lambda_e | lambda_i the panels of the x block hold d2L + delta I,
 * Je' and Ji': the staged blocks and delta, nothing of s, lda or mu.  On a single-rank handle in the full form, step() and
 * the pair assemble() / factor() therefore factor the groups of panels inside the x block once per stage_blocks: the first
 * factorisation after it RECORDS (a full factorisation that also copies the columns behind those groups, as they stand once
 * the last of them has been applied, into a snapshot the handle allocates outside its workspace: (N - n)^2 doubles at the
 * most, none for the panels inside the slack block); every later one with the same delta and delta_c REUSES: its assembly
 * writes the slack columns and restores the snapshot, its factorisation runs the forward substitution over the kept panels
 * and factors the multiplier block alone.  Bit for bit the result of a full factorisation.  Between a reusing assemble() and
 * its factor() the x columns of the storage hold the kept factor, not the matrix; every entry point that looks at the storage
 * as a matrix or writes into it (kkt_storage, the per-panel phases, set_option, stage_vectors, set_stream with another stream)
 * completes the assembly first and drops what was kept.  stage_blocks, a failed factorisation and one with other shifts
 * drop it too; other shifts are recorded only when they come twice in a row (a shift loop never pays for a snapshot).  A
 * caller that restages before every step (an NLP loop) pays for one snapshot per handle: recording stops when blocks are
 * restaged before anything reused them and resumes with the second factorisation of the same blocks.  Once kkt_storage has
 * handed the pointer out every factorisation is a full one until set_option("keep_zeros") is called again (the holder may
 * write anywhere).  PYIPM_REUSE_X=0 in the environment at create time switches all of it off; so does a snapshot that cannot
 * be allocated, silently.  Condensed, batched, provider and multi-rank handles, lookahead = 0 and systems whose first
 * group reaches beyond the x block never reuse.
 * A reusing step sends its right-hand side through the kept panels in one launch (k_fwd_prefix) where the one-launch sweeps apply
 * (sweep_persist, one rank, panels of at most 256 columns); PYIPM_FWD_PREFIX=0 at create time keeps the launches per panel,
 * PYIPM_FWD_PREFIX=W (W >= 2) sets the workgroups of that launch (default 96).  The same bits either way.  The kept panels behind
 * the prefix (the closed-form slack panels, the kept lambda_e groups below) follow in a second launch of the same kind
 * (k_fwd_range) under the same conditions; PYIPM_FWD_RANGE=0 at create time keeps their launches per panel, =W (W >= 2) sets its
 * workgroups (default 32).  The same bits either way.
 * With me > 0 and mi > 0 a reusing step also keeps the groups of the schedule that lie wholly inside the lambda_e columns (at
 * least one such group, at least one group behind them; a group that straddles a border of lambda_e is factored): the slack
 * columns couple to lambda_i only, so those groups depend on the blocks and the shifts alone.  A second snapshot holds their W and
 * what lies behind them; the diagonal blocks of the lambda_i columns are recomputed every step (the slack term changes them).
 * The same bits.  Whatever drops the prefix drops them too; PYIPM_REUSE_LAM_E=0 at create time, or a second snapshot that cannot
 * be allocated (silently), leaves the x prefix alone.
 * out[0] = factorisations of this handle that reused, [1] = that recorded, [2] = bytes of the snapshots (both), [3] = the last
 * one: 0 full, 1 recording, 2 reusing (whichever groups it kept).  With PYIPM_GROUP_TRACE set every factorisation says which kind
 * it is and how many groups it recorded or kept. */
int pyipm_newton_reuse_info(pyipm_newton_ctx* ctx, int64_t out[4]);

/* SURVEY.md section 8(f) rank 3 -- the derivative provider of the QP family on the device.  For
 *   min 1/2 x'Qx + c'x  s.t.  Ax = b,  Gx - h >= 0
 * the reference's compiled provider functions (pyipm.py:855-954: df, ce, ci; the J lambda terms of self.grad,
 * :655-668) are products with the constant blocks stage_blocks already holds: d2L = Q (UPPER triangle read, as
 * everywhere), Je = A', Ji = G'.  All pointers DEVICE memory; any output may be NULL.
 *   block_products   : Qv = sym(triu(d2L)) v (n),  JeTv = Je' v (me),  JiTv = Ji' v (mi)     -- df, ce, ci, merit ray
 *   block_products_t : out = Je le + Ji li (n; le / li may be NULL)                           -- dL/dx
 *   provider_stats   : ms ("profile" = 1) and block bytes of the last call of each */
int pyipm_newton_block_products(pyipm_newton_ctx* ctx, const double* v, double* Qv, double* JeTv, double* JiTv);
int pyipm_newton_block_products_t(pyipm_newton_ctx* ctx, const double* le, const double* li, double* out);
int pyipm_newton_provider_stats(pyipm_newton_ctx* ctx, double out[4]);
/* A provider-only handle (round 3): the same staging calls, block products, residual and kkt_matvec, but no KKT storage,
 * no W buffers and no tile inverses -- O(N) workspace instead of O(N^2) -- for callers that never factor the KKT matrix
 * (the limited-memory mode, pyipm.py:1007-1246: QPDeviceIPM(lbfgs=m) forms df, ce, ci and the J lambda terms through it).
 * stage_blocks may pass d2L = NULL (a factored Hessian model: Jacobian products only; block_products then needs
 * Qv = NULL).  assemble / factor / solve / step return PYIPM_E_BADARG. */
size_t pyipm_newton_workspace_bytes_provider(int64_t n, int64_t me, int64_t mi);
int pyipm_newton_create_provider(pyipm_newton_ctx** ctx, int64_t n, int64_t me, int64_t mi, int device,
                                 void* workspace, size_t workspace_bytes, void* stream);

/* SURVEY.md section 8(f) rank 1 — replaces the two IPM.step calls of the inner loop (pyipm.py:1408-1436,
 * 1737-1742): the largest alpha in [0,1] with v + alpha*dv >= (1-tau)*v, for v = s (dv = ds) and
 * v = lda_i (dv = dlda_i), from the staged s / lda and the direction of the last solve()/step() kept on
 * the device.  Closed form min(1, min_{dv_i<0} -tau*v_i/dv_i); the reference's golden-section search
 * converges to the same value from below (to Xtol = eps).  With mi == 0 both are 1.
 * dz: NULL = the direction of the last solve()/step(); else a DEVICE pointer to N doubles in the reference's order with the
 * multiplier block already sign-flipped (as merit_info / merit_ray take it) -- a host loop that steps along another direction
 * than the handle's last solve (an earlier, less shifted one kept by its regularisation loop) passes that one. */
int pyipm_newton_step_lengths(pyipm_newton_ctx* ctx, double tau, const double* dz, double* alpha_s, double* alpha_l);

/* SURVEY.md section 8(f) rank 1, second half — the merit-function pieces of the line search as device reductions over the
 * STAGED point (stage_vectors: df, ce, ci, s, lda) and a direction dz (device pointer, N doubles, reference order with the
 * multiplier block already sign-flipped; NULL = the direction of the last solve()/step(), kept on the device).  Replaces
 * the host passes of phi / dphi (pyipm.py:670-721, used by search :1438-1565), the merit-parameter update (:1727-1735),
 * the KKT report (:958-991) and the barrier update (:1804-1814).  One small D2H per call; sums are taken over a fixed
 * partition in a fixed order (bit-reproducible, independent of the launch).
 * merit_info: out[16] =
 *   [0] ||ce||_1   [1] ||ci - s||_1   [2] df . dx   [3] sum ds_i / (s_i + eps)   [4] sum log s_i
 *   [5] |dL/dx|_2  [6] |s * (lda_i - mu/(s + eps))|_2   [7] |ce|_2   [8] |ci - s|_2      (5, 6: from g = -grad, i.e. after residual(); else NaN)
 *   [9] sum s_i lda_i   [10] min s_i lda_i   [11] |dx|_2   [12] |ds|_2   [13..15] 0
 *   so that  phi = f + nu ([0] + [1]) - mu [4],  dphi = [2] - nu ([0] + [1]) - mu [3],  nu threshold = ([2] - mu [3]) / ((1 - rho)([0] + [1])).
 *   Entries that need a direction are NaN when there is none. */
int pyipm_newton_merit_info(pyipm_newton_ctx* ctx, const double* dz, double* out16);
/* out[p] = a_p . b_p for count <= 8 pairs of DEVICE vectors (a, b, len: host arrays) -- e.g. f(x) = x'(Qx)/2 + c'x from the
 * provider's product; fixed summation order; works on any handle. */
int pyipm_newton_dots(pyipm_newton_ctx* ctx, int count, const double* const* a, const double* const* b, const int64_t* len,
                      double* out);
/* QP family (the staged blocks are the constant Q, A', G' of min x'Qx/2 + c'x, Ax = b, Gx - h >= 0): the merit function
 * ALONG THE RAY as a difference,  out[k] = phi(x + a_k dx, s + a_k ds) - phi(x, s)  for K <= 1024 candidates a_k at once
 * (host arrays alphas / out) -- one launch evaluates every backtracking candidate alpha * tau^k of a search
 * (pyipm.py:1534-1548 shrinks alpha by tau = 0.995 per trial).  f is quadratic and the constraints affine, so with
 * g1 = df . dx, g2 = dx' Q dx, dce = Je' dx, dci = Ji' dx (formed once per direction from the staged blocks and kept):
 *   a g1 + a^2 g2 / 2 + nu sum(|ce + a dce| - |ce|) + nu sum(|ci - s + a (dci - ds)| - |ci - s|) - mu sum log1p(a ds / s),
 * every term a difference formed element by element (error relative to the CHANGE of phi).  quad: NULL = g2 from the staged
 * d2L block, else *quad is taken for g2 (handles whose Q is not a staged dense block). */
int pyipm_newton_merit_ray(pyipm_newton_ctx* ctx, const double* dz, double nu, double mu, const double* quad,
                           const double* alphas, int K, double* out);

/* ---- per-panel phases (multi-GPU host orchestration; single-rank factor() loops these) --- */

/* Factor panel p on its owner: left-looking in-panel updates, tile inversions, scaling. */
int pyipm_newton_factor_panel(pyipm_newton_ctx* ctx, int64_t p);
/* Owner: pack rows below panel p of W plus its tile inverses into `buf` for broadcast.
 * Non-owner: unpack a received buffer and rebuild the block column L = W * inv(T).
 * pyipm_newton_panel_msg_bytes gives the buffer size. */
size_t pyipm_newton_panel_msg_bytes(pyipm_newton_ctx* ctx, int64_t p);
int pyipm_newton_panel_pack(pyipm_newton_ctx* ctx, int64_t p, double* buf);
int pyipm_newton_panel_unpack(pyipm_newton_ctx* ctx, int64_t p, const double* buf);
/* Rank-nb trailing update of every locally owned column to the right of panel p. */
int pyipm_newton_trailing_update(pyipm_newton_ctx* ctx, int64_t p);
/* Same, restricted to the locally owned panels q with first <= q < first+count (lookahead:
 * the next owner updates and factors its panel before the bulk of the update). */
int pyipm_newton_trailing_update_range(pyipm_newton_ctx* ctx, int64_t p, int64_t first, int64_t count);
/* Finish: fetch statistics accumulated by this rank's tile kernels. */
int pyipm_newton_factor_begin(pyipm_newton_ctx* ctx);
int pyipm_newton_factor_end(pyipm_newton_ctx* ctx, pyipm_factor_stats* stats);
/* Panel-wise substitution phases (vector `v` is Npad doubles on the device). */
int pyipm_newton_fwd_panel(pyipm_newton_ctx* ctx, int64_t p, double* v);
int pyipm_newton_diag_panel(pyipm_newton_ctx* ctx, int64_t p, double* v);
int pyipm_newton_bwd_panel(pyipm_newton_ctx* ctx, int64_t p, double* v);

/* ---- distributed driver: one call per phase, the per-panel schedule runs inside the library -------------------
 * (SURVEY.md section 8e / 8b "Multi-GPU").  One process per GPU, handle created with (world, rank).  The per-panel
 * phases above remain for callers that orchestrate themselves; these entry points run the whole one-panel-lookahead
 * schedule (owner: head update -> factor -> pack -> broadcast on helper streams; everyone: unpack -> bulk update on
 * the handle's stream) and the sweeps in C, so no interpreter sits between two panels.
 *
 * Exchange, variant 1 -- caller-supplied collectives (like pyipm_lbfgs_set_allreduce).  A callback must leave its
 * result ordered on `stream` (a hipStream_t): enqueue on it, or complete before returning.  bcast: `bytes` bytes at
 * dev_buf from rank `root` to every rank, in place.  allreduce: `count` doubles in place, op 0 = sum, 1 = max.
 * Non-zero return = failure (PYIPM_E_COMM).
 * STREAMS: the callbacks are invoked with DIFFERENT streams -- the collective stream for panel broadcasts, the stream of
 * the trailing forward substitution for its segment sums, the handle's stream for statistics and the static-pivot scale --
 * and operations on those streams may be in flight at the same time.  A transport whose communicator must not run two
 * operations concurrently (NCCL / RCCL: one communicator, one stream at a time) has to serialise them itself, e.g. by
 * hopping every call through one stream of its own with a pair of events (what the library does for the communicator it
 * owns, variant 2), or by completing each call before it returns. */
typedef int (*pyipm_bcast_fn)(void* user, void* dev_buf, size_t bytes, int root, void* stream);
typedef int (*pyipm_allreduce_fn)(void* user, double* dev_buf, size_t count, int op, void* stream);
int pyipm_newton_set_exchange(pyipm_newton_ctx* ctx, pyipm_bcast_fn bcast, pyipm_allreduce_fn allreduce, void* user);
/* The optional point-to-point half of variant 1 (round 5).  send / recv: `bytes` bytes at dev_buf to / from rank `peer`;
 * allgather: every rank contributes bytes_per_rank bytes at send_buf, recv_buf receives the W pieces in rank order (send_buf
 * may point into recv_buf at this rank's place: in place).  Same stream rule as above; `user` is set_exchange's.  With all
 * three installed the library runs over the callbacks everything it runs over its own communicator: the scatter + all-gather
 * form of the panel messages (after pyipm_newton_exchange_selftest has reproduced the plain broadcast with it) and the slice
 * messages of the two-message protocol as point-to-point sends (without them a slice travels as a broadcast).  serialize != 0:
 * the transport must not run two operations at once -- the library then issues every operation on its collective stream, one
 * after the other, hopping from the stream that asked with a pair of events (what it does for RCCL). */
typedef int (*pyipm_send_fn)(void* user, const void* dev_buf, size_t bytes, int peer, void* stream);
typedef int (*pyipm_recv_fn)(void* user, void* dev_buf, size_t bytes, int peer, void* stream);
typedef int (*pyipm_allgather_fn)(void* user, const void* send_buf, void* recv_buf, size_t bytes_per_rank, void* stream);
int pyipm_newton_set_exchange_p2p(pyipm_newton_ctx* ctx, pyipm_send_fn send, pyipm_recv_fn recv, pyipm_allgather_fn allgather,
                                  int serialize);
/* COLLECTIVE (every rank or none): the self-test comm_init runs on a fresh communicator, on whichever exchange is installed.
 * The ranks agree on whether every one of them wants and can run the scatter + all-gather form (three ranks or more, all
 * primitives present, PYIPM_DIST_SAG != 0), reproduce the plain broadcast with it (two roots, a count that does not divide by
 * the number of ranks), agree on the outcome, and switch the form on for all or for none (pyipm_newton_comm_bcast_mode). */
int pyipm_newton_exchange_selftest(pyipm_newton_ctx* ctx);
/* Wire accounting of the last factor_dist / step_dist on this rank: out[0] panel messages that travelled as a plain broadcast,
 * [1] their bytes, [2] panel messages in the scatter + all-gather form, [3] their bytes, [4] point-to-point pieces sent or
 * received, [5] all-gathers, [6] hops through the collective stream, [7] slice messages sent or received (two-message
 * protocol), [8] their bytes, [9] slices that travelled as a broadcast, [10] ms of the owner's rows work behind the chain path,
 * [11] tile chains of this rank's panels that took the second slice's rows along in their own launch (dist_slices = 2). */
int pyipm_newton_dist_wire(pyipm_newton_ctx* ctx, double out[12]);
/* Exchange, variant 2 -- the handle owns an RCCL communicator over the `world` ranks it was created for.  Rank 0
 * obtains an id (128 bytes), it reaches the other ranks out of band (torch.distributed, MPI, a file), every rank calls
 * comm_init.  RCCL is dlopen'ed at that point (pyipm_newton_rccl_library names the library to bind: a process that has
 * torch loaded should name torch's own librccl; default: one already loaded, then librccl.so.1). */
int pyipm_newton_rccl_library(const char* path);
int pyipm_newton_comm_unique_id(void* id128);
int pyipm_newton_comm_init(pyipm_newton_ctx* ctx, const void* id128);
/* Number of ranks of the handle's RCCL communicator as RCCL itself reports it (ncclCommCount); 0 = no communicator
 * (callback exchange or single rank), negative = error.  bench.py prints it so that a multi-GPU line proves RCCL saw N ranks. */
int pyipm_newton_comm_ranks(pyipm_newton_ctx* ctx);
/* How the panel messages of factor_dist travel over the handle's communicator: 1 = scatter + all-gather (the owner sends
 * piece r to rank r, then an in-place all-gather: W - 1 links of the xGMI mesh at once instead of the one link's bandwidth of
 * ncclBroadcast's ring), 0 = ncclBroadcast.  comm_init switches the first form on for three ranks or more after it has
 * reproduced ncclBroadcast on that communicator (two roots, a count that does not divide by the number of ranks; all ranks
 * agree -- first on whether every rank wants the form at all, so PYIPM_DIST_SAG=0 on ONE rank switches it off for all); the
 * environment variable PYIPM_DIST_SAG=0 or set_option("dist_sag", 0) keep ncclBroadcast.  set_option("dist_sag", 0) is
 * COLLECTIVE: call it on every rank or on none (a subset would mix the two forms inside one exchange).  Messages below
 * 4 MiB and the nb-long exchanges of the sweeps always use ncclBroadcast. */
int pyipm_newton_comm_bcast_mode(pyipm_newton_ctx* ctx);
/* Row-sharded staging: a rank assembles only the KKT columns it owns, and column j (j < n) of the lower triangle is
 * row j of triu(d2L) | Je | Ji -- so it needs only those rows.  owned_rows returns their number and (rows != NULL)
 * their global indices in the order the arrays must hold them (= the rank's local column order).  After
 * stage_blocks_owned, residual / assemble / kkt_matvec address the blocks by local row. */
int64_t pyipm_newton_owned_rows(pyipm_newton_ctx* ctx, int64_t* rows);
int pyipm_newton_stage_blocks_owned(pyipm_newton_ctx* ctx, const double* d2L_rows, int64_t ld_d2L, const double* Je_rows,
                                    int64_t ld_Je, const double* Ji_rows, int64_t ld_Ji, int memkind);
/* The phases of pyipm.py:1717-1725 over the ranks (vectors replicated: every rank passes the same s / lda / rhs and
 * receives the same g / dz; statistics reduced over the ranks).  refine as in pyipm_newton_solve (Hc applied from the
 * ranks' blocks, one N-long sum per product).  With world == 1 they run the same per-panel schedule on one GPU. */
int pyipm_newton_residual_dist(pyipm_newton_ctx* ctx, double* g_out, int memkind);
int pyipm_newton_factor_dist(pyipm_newton_ctx* ctx, pyipm_factor_stats* stats);
int pyipm_newton_solve_dist(pyipm_newton_ctx* ctx, const double* rhs, double* dz, int flip, int refine, int memkind);
int pyipm_newton_kkt_matvec_dist(pyipm_newton_ctx* ctx, const double* v, double* y, int memkind);
int pyipm_newton_step_dist(pyipm_newton_ctx* ctx, double delta, double delta_c, int refine, double* dz,
                           pyipm_factor_stats* stats, int memkind);
/* ms of the last factor_dist / solve_dist ("profile" = 1): out[0] factorisation wall, [1] this rank's panel
 * factorisations, [2] packing, [3] broadcasts as seen on the collective stream, [4] unpacking (rebuild of L),
 * [5] solve wall, [6] bytes this rank put on / took off the wire, [7] messages. */
int pyipm_newton_dist_timings(pyipm_newton_ctx* ctx, double out[8]);

/* ---- batched small systems (BASELINE.json configs[4]: 512 independent n=256 QPs) ------------------------
 * Independent problems of one shape, Npad = roundup(n+2mi+me,128) <= 1024.  One workgroup per problem: a
 * single launch factors the whole batch.  Blocks are caller-owned DEVICE arrays with a batch stride (in
 * doubles); pyipm_newton_stage_vectors on such a handle takes [batch][len] contiguous arrays.  Replaces a
 * loop of pyipm.py:1717-1725 over independent problems (multi-start); nothing in the reference batches. */
size_t pyipm_newton_workspace_bytes_batched(int64_t n, int64_t me, int64_t mi, int batch);
int pyipm_newton_create_batched(pyipm_newton_ctx** ctx, int64_t n, int64_t me, int64_t mi, int batch, int device,
                                void* workspace, size_t workspace_bytes, void* stream);
int pyipm_newton_stage_blocks_batched(pyipm_newton_ctx* ctx, const double* d2L, int64_t ld_d2L, int64_t stride_d2L,
                                      const double* Je, int64_t ld_Je, int64_t stride_Je,
                                      const double* Ji, int64_t ld_Ji, int64_t stride_Ji);
/* residual + assemble + factor + solve + flip for every problem; dz is [batch][N], stats (may be NULL) [batch].
 * set_option("condensed", 1) (round 5): per problem the (s_k, lambda_i_k) pairs with Sigma_k <= "condensed_sigma_max" are
 * eliminated analytically (pyipm.py:824-842's block structure), the rest stay as rows -1/Sigma_k: n + me + |A| columns are
 * factored instead of n + 2 mi + me (BASELINE config 5: 256 instead of 768).  Same inputs, same outputs: the full
 * [dx|ds|dle|dli] and the inertia of the FULL matrix.  pyipm_newton_last_timings on a batched handle: out[0] residual +
 * assembly, [6] factorisation, [3] substitutions, [1] the whole step (ms). */
int pyipm_newton_step_batched(pyipm_newton_ctx* ctx, double delta, double delta_c, double* dz,
                              pyipm_factor_stats* stats, int memkind);
/* The per-problem statistics of the last pyipm_newton_step_batched (B records), for a step that was called with
 * stats = NULL -- such a step returns once its launches are enqueued; this call synchronises the handle's stream.  Returns
 * PYIPM_E_NONFINITE when a problem met NaN/Inf (the records are filled in all the same).  (The reference reads the inertia of
 * every system eagerly, pyipm.py:1378-1381: one eigendecomposition per problem.) */
int pyipm_newton_stats_batched(pyipm_newton_ctx* ctx, pyipm_factor_stats* stats);

/* out[b] = |g - Hc raw_b| / |g| for every problem of the last step_batched: Hc applied from the staged blocks with that
 * step's shifts (never from the factor), raw = dz ([batch][N], DEVICE) with the multiplier flip undone.  The guard of the
 * condensed form (the host falls back to the full system when a problem misses its bar) and the batched counterpart of the
 * kkt_matvec check of a single system.  out: batch doubles, host or device per memkind. */
int pyipm_newton_backward_error_batched(pyipm_newton_ctx* ctx, const double* dz, double* out, int memkind);

/* A batched step with every problem's OWN barrier parameter and shifts: after the first barrier update (pyipm.py:1804-1814)
 * and the first reghess (pyipm.py:1373-1406, which persists one delta per system) no two problems of a multi-start batch share
 * them.  mu, delta, delta_c: batch doubles; active: batch flags or NULL = every problem; host or device per memkind, copied on
 * the handle's stream.  The handle keeps, per problem, the values of the last step the problem took part in (step_batched
 * fills them with its scalars and stage_vectors' mu, every problem active; backward_error_batched reads each problem's own).
 * A problem with active[b] == 0 sits the step out: every kernel of the step returns at once for it, its row of dz is NOT
 * written, its statistics record, its mu / delta / delta_c and the scale of its static pivots stay those of its last step --
 * a retry of the one problem of 512 whose inertia came out wrong leaves the directions of the other 511 alone.
 * Both forms (full, condensed).  Returns once the launches are enqueued, like step_batched(stats = NULL) (host output: once
 * the rows of the active problems have arrived); statistics through pyipm_newton_stats_batched.
 * PYIPM_E_BADARG: not a batched handle, blocks / vectors not staged, NULL mu / delta / delta_c / dz. */
int pyipm_newton_step_batched_each(pyipm_newton_ctx* ctx, const double* mu, const double* delta, const double* delta_c,
                                   const int32_t* active, double* dz, int memkind);

/* The fraction-to-the-boundary rule (pyipm.py:1408-1436, the two IPM.step calls at 1737-1742) for every problem of a batch in
 * one launch, one wave per problem: alpha[b] = (alpha_s, alpha_l), the closed form of pyipm_newton_step_lengths with its
 * arithmetic entry by entry -- bit for bit what a single-system handle returns for that problem; (1, 1) when mi == 0.
 * dz: DEVICE [batch][N], multiplier block sign-flipped as the steps return it; NULL = the directions of the last step, which
 * the handle keeps only where that step's output was host memory (PYIPM_E_BADARG otherwise: pass the tensor the step wrote).
 * alpha: [batch][2], host or device per memkind (host: synchronises).  Needs stage_vectors. */
int pyipm_newton_step_lengths_batched(pyipm_newton_ctx* ctx, double tau, const double* dz, double* alpha, int memkind);

/* The batch as a solver: what a line search and a barrier loop over the whole batch need between two steps, per problem and
 * without leaving the device -- the batched counterparts of block_products / _t, merit_info and merit_ray above.  Plain
 * launches, one workgroup or one wave per problem; every sum runs over a fixed partition in a fixed order given by the
 * problem's sizes alone, so the bits of problem b depend neither on the batch size nor on b's place in the batch, and those of
 * one ray value neither on K nor on the value's place in the call.
 * PYIPM_E_BADARG for all four: not a batched handle, what the entry reads (blocks; vectors) not staged, a required pointer NULL.
 *
 * block_products_batched -- the provider of the QP family (pyipm.py:855-954: df = Qx + c, ce = Ax - b, ci = Gx - h) for every
 *   problem: Qv[b] = sym(triu(d2L_b)) v_b (n), JeTv[b] = Je_b' v_b (me), JiTv[b] = Ji_b' v_b (mi) from the staged blocks, ONE
 *   pass over each block (only the UPPER triangle of d2L is read).  v: [batch][n]; any output may be NULL.  DEVICE pointers.
 * block_products_t_batched -- the J lambda terms of self.grad (pyipm.py:655-668): out[b] = Je_b le_b + Ji_b li_b (n);
 *   le [batch][me] / li [batch][mi], either may be NULL.  DEVICE pointers.
 * Both return once their launch is enqueued on the handle's stream. */
int pyipm_newton_block_products_batched(pyipm_newton_ctx* ctx, const double* v, double* Qv, double* JeTv, double* JiTv);
int pyipm_newton_block_products_t_batched(pyipm_newton_ctx* ctx, const double* le, const double* li, double* out);
/* merit_info_batched -- out[b][16] = the quantities of pyipm_newton_merit_info for problem b over the staged vectors
 *   ([batch][len]) and the directions dz: the host passes of phi / dphi (pyipm.py:670-721), the merit-parameter update
 *   (:1727-1735), the KKT report (:958-991) and the barrier update (:1804-1814), for the whole batch in one launch.
 *   dz: DEVICE [batch][N], multiplier block sign-flipped as the steps return it; NULL = the directions of the last step where
 *   the handle keeps them (a step with host output), else none: entries 2, 3, 11, 12 are NaN.  Entries 5 and 6 come from the
 *   residual g = -grad the last step left (each problem's with its own mu of that step): NaN before any step since
 *   stage_vectors.  Entry 10 is NaN when mi == 0.  out: host (synchronises) or device (asynchronous) per memkind.
 * merit_ray_batched -- out[b][k] = phi_b(x + a dx, s + a ds) - phi_b(x, s) for a = alphas[b][k], K <= 1024 candidates per problem
 *   in one launch (pyipm.py:1534-1548: every backtracking candidate alpha tau^k of every problem's search), term by term as
 *   pyipm_newton_merit_ray, with each problem's own nu[b], mu[b].  g1 = df . dx, g2 = dx' Q dx, Je' dx, Ji' dx are formed from the
 *   staged blocks for every call (nothing of a direction is kept); quad != NULL: quad[b] is taken for g2 and d2L is not read.
 *   dz as above, but required (NULL without kept directions: PYIPM_E_BADARG).  nu, mu, quad: [batch]; alphas, out:
 *   [batch][K]; all five host or device per memkind (host: staged, synchronises).  PYIPM_E_BADARG also for K < 1 or K > 1024. */
int pyipm_newton_merit_info_batched(pyipm_newton_ctx* ctx, const double* dz, double* out, int memkind);
int pyipm_newton_merit_ray_batched(pyipm_newton_ctx* ctx, const double* dz, const double* nu, const double* mu, const double* quad,
                                   const double* alphas, int K, double* out, int memkind);

/* The kept factors of a batch as a solver: after a step every problem holds its factor, its own shifts and (condensed form) its
 * active set; these three entries work against them as solve / solve_many, kkt_matvec and rcond do on a single-system handle
 * -- refinement against the blocks, the rcond <= eps test of reghess (pyipm.py:1379-1381), extra right-hand sides
 * (pyipm.py:18-20, 911-914).  Plain launches, no atomics or waits between workgroups, every sum over a partition and in an
 * order the problem's sizes alone decide: the bits of a column depend neither on k, nor on its place among the columns, nor on
 * the batch size or the problem's place in the batch.  None of them writes the factor, the kept residual, the statistics or a
 * kept host-output direction: a following backward_error_batched, step_lengths_batched(dz = NULL) or step returns the bits
 * it would have returned without the call.  The factors, shifts and active sets are those of a step's blocks AND vectors
 * (a condensed solve rebuilds Sigma from the staged s, lda): staging blocks or vectors again drops them -- all three entries
 * then return PYIPM_E_BADARG until the next step.  Scratch is the library's own buffer outside the workspace, grown on demand
 * (pyipm_newton_workspace_bytes_batched is unchanged).
 *
 * solve_batched -- x = inv(Hc_b) rhs for k columns per problem (pyipm.py:1718-1725 for any right-hand side) against the factor
 *   of the last step each problem took part in: the matrix with THAT problem's shifts, full or condensed as that step was (a
 *   condensed factor: each column is reduced as the step reduces its residual, the sweeps run over n + me + |A| rows, the full
 *   [dx|ds|dle|dli] is recovered).  Column j of problem b: rhs + b stride_rhs + j ld_rhs (doubles), likewise x; ld >= N, entries
 *   N .. ld - 1 are not written; x may BE rhs (same pointer, ld and stride: solved in place -- with refine > 0 the library keeps
 *   a copy of the right-hand sides for the residuals); any other overlap of the two device blocks is PYIPM_E_BADARG.  active: batch flags or
 *   NULL = every problem; a problem with active[b] == 0 (or one no step has factored yet) costs workgroups that return at
 *   once, its columns of x are NOT written.  flip != 0: rows n + mi .. N - 1 negated (the reference's multiplier sign).
 *   refine > 0: that many steps R = B - Hc X; X += solve(R) with Hc from the blocks (kkt_matvec_batched's kernel);
 *   refine < 0 (adaptive on a single system): PYIPM_E_BADARG -- a column's bits never depend on its neighbours.
 *   k == 0 returns 0.  Device pointers: asynchronous on the handle's stream; host pointers are staged and the call synchronises.
 *   PYIPM_E_BADARG: not a batched handle, no step yet, a NULL pointer, ld < N, k < 0 or k > 65535, refine < 0.
 * kkt_matvec_batched -- y = Hc_b v for k columns per problem from the staged blocks (never the factor), with the problem's own
 *   delta / delta_c of its last step and Sigma = lda / (s + eps) of the staged vectors (pyipm.py:824-842); raw sign, no flip.
 *   The blocks are read once per chunk of 8 columns.  y must not overlap v.  Needs staged blocks and vectors and one step.
 * rcond_batched -- out[b][4] = the quantities of pyipm_newton_rcond for problem b (pyipm.py:1379-1381): the min|w| estimate from
 *   it_inv inverse iterations (solve_batched's kernel), the max|w| estimate from it_pow power iterations (kkt_matvec_batched's
 *   kernel), their ratio, and the static-pivot magnitude sqrt(eps) max|Hc_b|.  0 = the defaults 3 / 6; negative (adaptive)
 *   counts: PYIPM_E_BADARG.  Start vectors as pyipm_newton_rcond's; norms and normalisation by one wave per problem in a
 *   fixed order.  Where a problem's factor holds static pivots (n_zero > 0) it is the factor of a matrix perturbed at the
 *   level of the fourth quantity, and inverse iteration alone finds THAT matrix' smallest eigenvalue; there the iterate x is
 *   taken back to the unperturbed blocks, x' = x - inv(factored)(Hc x), and |Hc x'| / |x'| (an upper bound of min|w| of Hc
 *   for any x') replaces the estimate where it is smaller: a singular Hc_b reads as singular (rcond at rounding level)
 *   although its factor is not.  active as above (rows of out of the others are not written).  Full form only: PYIPM_E_BADARG when the
 *   handle's last step was condensed; NaN for a problem that still holds a condensed factor from an earlier step.
 *   out: host (synchronises) or device per memkind, and active with it. */
int pyipm_newton_solve_batched(pyipm_newton_ctx* ctx, int64_t k, const double* rhs, int64_t ld_rhs, int64_t stride_rhs,
                               double* x, int64_t ld_x, int64_t stride_x, const int32_t* active, int flip, int refine, int memkind);
int pyipm_newton_kkt_matvec_batched(pyipm_newton_ctx* ctx, int64_t k, const double* v, int64_t ld_v, int64_t stride_v,
                                    double* y, int64_t ld_y, int64_t stride_y, int memkind);
int pyipm_newton_rcond_batched(pyipm_newton_ctx* ctx, int it_inv, int it_pow, const int32_t* active, double* out, int memkind);

/* Adaptive refinement of a batch of directions, EVERY PROBLEM BY ITSELF: pyipm_newton_solve's refine < 0 for the batched handle
 * (which solve_batched refuses: there a fixed count makes every problem pay for the worst one and cannot say who converged).
 * dz_b -- N doubles at dz + b stride, device memory, ld >= N and stride >= N -- is a solution of problem b's kept system: the
 * right-hand side is the residual g the last step kept, the matrix the staged blocks with that problem's own delta, delta_c
 * and Sigma (kkt_matvec_batched's arithmetic: never the factor, always the full 4-block matrix).  flip != 0: rows n + mi ..
 * are negated, as the step wrote them.  It is refined in place by the rule of solve(refine < 0), per visit of a problem:
 * berr = |g - Hc x|_2 / |g|_2 is measured from the blocks before every step; the problem stops converged at berr <= target,
 * after max_steps steps, or when a step gained less than 4x (berr > 0.25 prev); a step that made it worse, or not finite, is
 * TAKEN BACK (the saved iterate restored, the step not counted); NaN / Inf at the first measurement: nothing is done.  The
 * decision is refine_each_verdict of pyipm_amd/csrc/refine_each_plan.hpp, the one statement the kernel and the CPU replay
 * compile.  A step is x += inv(factor_b) r through solve_batched's kernel: a problem whose last step was condensed is
 * corrected through its condensed factor, its residual formed against the full blocks all the same.
 * target <= 0 / max_steps < 0: the handle's "refine_target" / "refine_max" (1e-14 / 8).
 * info[b][4] = {steps taken, berr before the first step, berr of the kept iterate, converged 0|1} -- the layout of
 * pyipm_newton_solve_info -- in host (the call synchronises) or device memory per memkind, and active with it.  active: batch
 * flags or NULL = every problem; for a problem with active[b] == 0 (or one no step has factored yet) neither its row of dz
 * nor its row of info is written.
 * Nothing returns to the host between the steps: max_steps + 1 rounds of plain launches are enqueued, a problem's state
 * (going / stopped, the last error, its step count) lives in the library's own scratch outside the workspace (grown on
 * demand; pyipm_newton_workspace_bytes_batched is unchanged), and the workgroups of a stopped problem return at once.  No
 * atomics or waits between workgroups, every sum in an order the sizes alone decide: the bits of problem b, in dz and in
 * info, depend neither on the batch size, nor on b's place, nor on which other problems take part or how many steps they
 * take.  The factors, the statistics, the kept residual and solution, a kept host-output direction and the handle's
 * record of its last step are left alone, as by solve_batched.
 * PYIPM_E_BADARG: not a batched handle, no step since the blocks or vectors were staged, a NULL dz or info, ld or stride < N. */
int pyipm_newton_refine_batched(pyipm_newton_ctx* ctx, double* dz, int64_t ld, int64_t stride, const int32_t* active, int flip,
                                double target, int max_steps, double* info, int memkind);

/* ---- introspection for tests / bench ------------------------------------------------------ */

/* Device pointer + leading dimension of the local KKT storage (column-major lower).  The caller may write through the
 * pointer: handing it out makes EVERY following assemble() store every entry again (otherwise the zeros that no elimination
 * step can fill in are left in place from one assembly to the next, option "keep_zeros") -- the holder of the pointer may
 * write at any later time, so the shortcut stays off for this handle until set_option("keep_zeros", 1) is called again
 * (a promise that nothing writes through the pointer any more). */
int pyipm_newton_kkt_storage(pyipm_newton_ctx* ctx, double** ptr, int64_t* ld, int64_t* ncols);
/* Time (ms, HIP events on the handle's stream) of the phases of the last factor/solve call:
 * out[0]=assemble, [1]=panel work (factor time during which no update launch ran), [2]=trailing updates (sum of the launches'
 * durations -- a lookahead head on the side stream may overlap the bulk launch behind it, so [1]+[2] can exceed [6]),
 * [3]=solve, [4]=#trailing launches,
 * [5]=algorithmic flops of those launches, [6]=factor, [7]=Ji Sigma Ji' launch (condensed option) or, for the
 * full system, the number of matrix entries those launches update (their C-tile traffic is 16 B each). */
int pyipm_newton_last_timings(pyipm_newton_ctx* ctx, double out[8]);

/* The bulk trailing-update launches of the last factorisation by kernel instance (profile option on): out[0..3] = launches,
 * summed HIP-event duration (ms), flops, algorithmic bytes (C tiles read and written once + the two operand panels read
 * once) of the 128 x 128-tile launches (k_update<128,true,8>),
 * out[4..7] = the same for the 128 x 256-tile launches (k_update<256,true,8>) -- what a kernel trace lists under the two
 * names.  Measurement only; nothing in the reference. */
int pyipm_newton_trailing_instances(pyipm_newton_ctx* h, double out[8]);
/* The same launches' algorithmic bytes in both definitions: out[k] = C tiles only (16 B per updated entry), out[2 + k] = C tiles +
 * the two operand panels read once; k = 0: 128 x 128 tiles, k = 1: 128 x 256. */
int pyipm_newton_trailing_bytes(pyipm_newton_ctx* ctx, double out[4]);
/* Options.  Every one defaults to the measured-best setting; the public ones (28 names) choose numerics, forms of the
 * system and the few schedule parameters a deployment may have to adapt; the 12 EXPERT switches (test hooks, diagnostics
 * and the reference forms the bit-identity tests compare against) are refused unless the process has PYIPM_EXPERT=1 in
 * its environment or the handle was given set_option("expert", 1) -- so that nothing outside the tests and tools/ runs a
 * path nobody else runs.  Round 6 removed the 35 switches whose measurements HISTORY.md records as lost or neutral (with
 * the code paths behind the ones that lost): 40 names in all.  tests/test_gpu_symmetric.py checks both lists against the
 * library and runs the bitwise-neutrality sweep over every schedule option in them.
 *
 * PUBLIC OPTIONS: expert, condensed, condensed_sigma_max, condensed_refine, block_refine, refine_cond, refine_target,
 *   refine_max, pivtol_rel, tile_blocked, profile, skip_zeros, keep_zeros, fuse_forward, sweep_persist, lookahead, group,
 *   bulk_bn, reserve_cus, persist_rows, tile_chain, wide_sub, dist_sag, dist_sag_min_bytes, dist_slices, dist_comm2,
 *   dist_timeout_s, dist_selfmsg
 *
 *   "expert" 0|1        unlock the expert switches on this handle.
 *   "condensed" 0|1     handles with mi > 0: assemble / factor / solve work on the condensed system
 *                       [[d2L + delta I + Ji Sigma Ji', Je], [Je', -delta_c I]] of dimension n + me (+ active rows): s and
 *                       lambda_i eliminated analytically.  Same inputs, same outputs (full [dx|ds|dle|dli], inertia of the
 *                       full matrix); kkt_storage then exposes the condensed matrix.  Several ranks: with the FULL blocks
 *                       staged on every rank (stage_blocks, not stage_blocks_owned).  Batched handles: per problem.
 *   "condensed_sigma_max" (1e4): inequalities whose Sigma_k = lda_i/(s+eps) exceeds it are not folded into the x-x block but
 *                       kept as rows with -1/Sigma_k on the diagonal; "condensed_refine" (0): refinement steps against the
 *                       full blocks every condensed solve gets at least.
 *   "block_refine" 0..3 (2), "refine_cond" (1e2): refinement steps of the block solves L T = S / T z = y for diagonal tiles
 *                       whose pivot spread exceeds refine_cond (the tile inverses are explicit).
 *   "refine_target" (1e-14) / "refine_max" (8): adaptive refinement of solve(refine < 0): stop at this backward error or
 *                       after this many steps.
 *   "pivtol_rel" (1e-14): a pivot below this fraction of its tile column's magnitude has cancelled: static pivot.
 *   "tile_blocked" 0|1  (1): the 64 x 64
 *                       tile inversion 16 pivots at a time (in-register LDL' of the micro-block + fp64 MFMA block sweeps,
 *                       Bunch-Kaufman verified afterwards, fallback to the single sweeps) -- same pivots and inertia, another
 *                       order of rounding than the single sweeps (not bit-identical).
 *   "profile" 0|1       HIP-event timings (last_timings, trailing_instances, dist_timings, provider_stats).
 *   "skip_zeros" 0|1    (1) products with blocks that pyipm.py:824-842 makes identically zero are not formed; bitwise-neutral.
 *   "keep_zeros" 0|1    (1) K1 leaves in place the zeros nothing can fill in; single rank; bitwise-neutral.
 *   "fuse_forward" 0|1  (1) the forward substitution of a pending residual trails the factorisation; bitwise-neutral
 *                       against the per-panel sweeps.
 *   "sweep_persist" 0|1 (1; single rank, one right-hand side, nb <= 256): each substitution sweep as ONE device-driven
 *                       launch (k_fwd_sweep / k_bwd_sweep; flags and values cross workgroups through agent-scope atomics,
 *                       every poll has a 2 s timeout that poisons the result with NaN and is reported by the next
 *                       factorisation) -- equal to rounding, not to the bit (another summation order), deterministic.
 *                       Their workgroups wait for each other, so all of them must become resident: under a CU mask, or
 *                       beside a kernel that holds CUs for seconds, use 0.
 *   "lookahead" 0|1|2   (2) 1 = one-group lookahead of the single-rank schedule; 2 = that, and where the x block is one group
 *                       its update is applied panel by panel under its own chain; "group" 1..create-time
 *                       value: panels per bulk trailing update (K = group * nb).  Bitwise-neutral.
 *   "bulk_bn" 256|128   (256) column width of a bulk update tile; "reserve_cus" (16) / "persist_rows" (12288): in the
 *                       chain-bound phase (at most persist_rows rows left) the bulk update runs as a persistent launch
 *                       that leaves reserve_cus CUs to the panel chain; 0 = ordinary launches.  Bitwise-neutral.
 *   "tile_chain" 0|1|2  (1; round 6) the 64 x 64 tile steps of a diagonal block as ONE launch of persistent workgroups
 *                       (k_tile_chain: the chain workgroup + units that own row tiles; hand-overs through written-through
 *                       stores and progress words, every poll with a 2 s timeout that factor() reports as PYIPM_E_HIP)
 *                       instead of one launch per tile: 1 where the chain is what the step waits for (first group, last
 *                       12288 rows, the per-panel / multi-GPU schedule), 2 everywhere, 0 never.  Same condition on residency
 *                       as sweep_persist.  Bit-identical to the launches.
 *   "wide_sub" (256)    per-panel / multi-GPU schedule: a panel wider than this is factored by its owner as a block of
 *                       sub-panels this wide (the launches, and the bits, of the single-rank schedule at nb = 256).
 *   "dist_sag" 0|1      COLLECTIVE: 0 keeps the plain broadcast for the panel messages, 1 goes back to what the exchange
 *                       self-test decided (see pyipm_newton_comm_bcast_mode); "dist_sag_min_bytes" (4 MiB): smaller messages
 *                       always take the plain broadcast.
 *   "dist_slices" 0|1|2 (2) COLLECTIVE: the two-message protocol of the distributed factorisation -- the rows of panel p
 *                       that meet the diagonal block of panel p + 1 (and the rows of panel p + 2) go from owner(p) to
 *                       owner(p + 1) point to point AHEAD of the panel message, so the next owner's tile chain starts on an
 *                       nb x nb message; 2: the rows of the second slice take their stages inside the chain's own launch
 *                       (no launch of their own behind it); 0: one message per panel (rounds 1-4).  Bit-identical.
 *   "dist_comm2" 0|1    (0) COLLECTIVE, RCCL transport: the slice messages on a SECOND communicator over the same ranks, on
 *                       the owner's stream, so that they do not queue behind a panel broadcast in flight.  Setting it (before
 *                       or after comm_init) creates the communicator -- every rank must make the call; the ranks agree before
 *                       anyone enters ncclCommInitRank.  Off by default: two communicators in flight on one device have not
 *                       run on more than one GPU yet; bench.py's ladder tries it last.  Bit-identical.
 *   "dist_timeout_s"    (300) bound on the host's wait for the device at the end of a distributed factorisation; on expiry
 *                       PYIPM_E_COMM names the panel whose message / update / chain did not complete and the handle refuses
 *                       further distributed steps (destroy aborts its communicators).  <= 0: wait for ever.
 *   "dist_selfmsg" 0|1  world == 1 only: the distributed driver packs and "sends" every panel anyway (measures the
 *                       message path on one GPU).
 *
 * EXPERT OPTIONS: tail_group, group_chain, tile_step, tile_waves, bc_per_problem, chain_cpy, chain_whole, chain_lds_kb,
 *   sweep_max_blocks, debug_fault, debug_timeline_ptr, debug_chain_ptr
 *   (which stream runs what, in how many launches: tail_group = panels per group once at most 24576 columns remain (4; 8 for systems of at most 8192 rows);
 *   group_chain 0 = a group's panels one after the other instead of one tile chain; tile_step 0 = the two-launches-per-tile
 *   schedule of round 1; tile_waves 4|8|9 = the launch-per-tile kernel on four waves, on eight where a whole CU is to be had,
 *   on eight everywhere; bc_per_problem 0 = the batched condensed form's Gram part by one workgroup per tile; chain_cpy / chain_whole /
 *   chain_lds_kb = units per row tile, one launch per group or per sub-panel, and the shared-memory pad that gives a workgroup
 *   of k_tile_chain its compute unit to itself; sweep_max_blocks, debug_* = test hooks and diagnostics buffers.  All of them
 *   choose between implementations that accumulate the same products in the same order: bit-identical results,
 *   tests/test_gpu_symmetric.py, tests/test_gpu_tile_blocked.py.) */
int pyipm_newton_set_option(pyipm_newton_ctx* ctx, const char* name, double value);

/* Version of this interface: bumped whenever an entry point changes its argument list (round 5 added `dz` to
 * pyipm_newton_step_lengths in place: a caller built against the older header would have passed a host pointer where the
 * device direction goes).  A binding checks pyipm_newton_abi_version() == PYIPM_NEWTON_ABI_VERSION of the header it was
 * written against before any other call (pyipm_amd/newton.py does).  7: step_batched_each, step_lengths_batched; the
 * workspace of a batched handle grew by the per-problem parameters.  8: block_products_batched, block_products_t_batched,
 * merit_info_batched, merit_ray_batched.  (Still 8: solve_batched, kkt_matvec_batched, rcond_batched, then refine_batched, pyipm_pairs_*, pyipm_qn_* -- entries
 * added, no argument list, layout or workspace size changed.) */
#define PYIPM_NEWTON_ABI_VERSION 8
int pyipm_newton_abi_version(void);

/* fp64 MFMA peak micro-benchmark: register-resident v_mfma_f64_16x16x4_f64 only.
 * Returns achieved TFLOP/s in *tflops. */
int pyipm_mfma_f64_peak(int device, int iters, double* tflops);

/* ===================================================================================================================
 * L-BFGS pair store: lbfgs_init / lbfgs_update of the reference (pyipm.py:993-1005, 1282-1371) where the pairs live.
 *
 * A store owns S and Y (n x (memory + 1), DEVICE), the small arrays SS, L, D (HOST, O(memory^2)), zeta and the counter of
 * skipped pairs.  An offer forms dx = x_new - x_old and dg = g_old - g_new on the device, takes their products against the
 * stored pairs in ONE read pass (2 n m + 4 n doubles), brings the 2 (m + 1) + 2 products to the host in one copy, decides
 * there -- accept iff dg.dx > sqrt(eps) and zeta_new = dg.dx / (den + eps) > sqrt(eps), den = dx.dx for a constrained
 * problem and dg.dg otherwise; more than `memory` skips in a row empty a non-empty store -- and appends an accepted pair,
 * dropping the oldest once the store holds memory + 1 (the reference lets the storage reach that, :1300).  Constrained:
 * SS = S'S, L = strictly lower S'Y; unconstrained: SS = Y'Y, L = upper S'Y; D = diag(S'Y).  The view is the argument list
 * of pyipm_lbfgs_direction(..., PYIPM_MEM_DEVICE) (include/pyipm_lbfgs.h) on a handle with max_pairs >= memory + 1.
 *
 * Streams: the kernels of an offer run on the store's stream; an offer synchronises it ONCE (the products).  The append of
 * an accepted pair is left in flight on that stream: read S / Y on the same stream or synchronise it first.  The products
 * are deterministic (fixed grid, fixed order of the partial sums, no floating-point atomics): the same offers give the
 * same bits.  One store per problem; row-sharded use is not offered yet -- the products of an offer are kept in ONE device
 * buffer so that an all-reduce callback like pyipm_lbfgs_set_allreduce can be added without a change of layout.
 * Entries return PYIPM_E_BADARG for a NULL handle or pointer (pyipm_pairs_last_error says which) and leave the store as it was. */
typedef struct pyipm_pairs pyipm_pairs;
typedef struct pyipm_pairs_view {          /* valid until the next offer / reset / destroy */
    int64_t m, ld;                         /* stored pairs; pitch of S and Y in doubles      */
    const double *S, *Y;                   /* DEVICE, n x m row-major, oldest pair first      */
    const double *SS, *L, *D;              /* HOST, m x m row-major, contiguous               */
    double zeta; int64_t fail;
} pyipm_pairs_view;

size_t pyipm_pairs_workspace_bytes(int64_t n, int memory);                 /* 0: bad geometry; 1 <= memory <= 31 */
int pyipm_pairs_create(pyipm_pairs** out, int64_t n, int memory, int constrained, double zeta0, int device, void* stream);
int pyipm_pairs_destroy(pyipm_pairs* p);
const char* pyipm_pairs_last_error(pyipm_pairs* p);
int pyipm_pairs_set_stream(pyipm_pairs* p, void* stream);
int pyipm_pairs_reset(pyipm_pairs* p);                                     /* lbfgs_init */
/* lbfgs_update.  x_*: n; g_*: at least n (only the first n are read).  outcome: 1 accepted, 0 skipped, 2 reset. */
int pyipm_pairs_offer(pyipm_pairs* p, const double* x_old, const double* x_new, const double* g_old,
                      const double* g_new, double eps, int memkind, int* outcome);
int pyipm_pairs_view_get(pyipm_pairs* p, pyipm_pairs_view* v);

/* ===================================================================================================================
 * Quasi-Newton KKT operator of the last L-BFGS direction: product, kept-state solve, backward error, refinement.
 *
 * pyipm_lbfgs_direction (include/pyipm_lbfgs.h) solves, through the normal equations G = J'J/zeta + diag(0, 1/Sigma),
 *
 *   K dz = g ,   K = [ B_k   0      J        ]     B_k = zeta I - W inv(M) W',  W = [zeta S, Y],  M = [[zeta SS, L], [L', -D]]
 *                    [ 0     Sigma  [0 | -I] ]     (no pairs: B_k = zeta I),   Sigma = lda_i / (s + eps),   J = [Je | Ji]
 *                    [ J'    [0;-I]  0       ]     dz = [dz_x (n) | dz_s (mi) | dz_lambda (me + mi)]  -- the RAW direction
 *
 * (the system of the reference's general branch, pyipm.py:1099-1148), and so pays the squared conditioning of J and the
 * whole spread of Sigma.  These four entries take the handle of a direction and work from what that call left in it: K is
 * applied from the staged Jacobians, Sigma and the pairs -- never from a factor, and WITHOUT the regularisation the
 * direction may have added to the equality block (stats.regularised): a regularised factor is the preconditioner of the
 * refinement and nothing more.  One step of refinement against K recovers the digits the normal equations lost.
 *
 * Vectors are N = n + 2 mi + me doubles, host or device by memkind.  flip != 0: a vector of the SOLUTION space (v of
 * matvec, dz of solve and refine) has its multiplier rows n + mi .. N-1 negated, as the direction writes them with flip;
 * the entries undo that on read and apply it on write.  Right-hand sides (rhs, out of matvec) are never flipped.
 * Every entry synchronises the handle's stream before it returns.  Sums run in an order the sizes alone decide (no
 * floating-point atomics): equal calls give equal bits.
 *
 * PYIPM_E_BADARG, with a message in pyipm_lbfgs_last_error: a NULL handle or vector; no direction since the handle was
 * created or since pyipm_lbfgs_stage_jacobian / _stage_jacobian_columns / pyipm_lbfgs_set_allreduce; me + mi = 0 (the unconstrained direction is an
 * explicit formula: there is no system); a handle with an all-reduce callback installed -- a row-sharded handle is not
 * supported here.  A direction after any of these calls returns the bits it would have returned without them. */
typedef struct pyipm_lbfgs_ctx pyipm_lbfgs_ctx;
/* out = K v: one pass over J for both J'v_x and J v_lambda. */
int pyipm_qn_matvec(pyipm_lbfgs_ctx* h, const double* v, int flip, int memkind, double* out);
/* K~ dz = rhs from the kept state alone (K~ = K, with the direction's regularisation where it regularised): the direction's
 * arithmetic for one new column against the kept factor of zeta G, the kept 2m solved columns and the kept 2m x 2m system --
 * no Gram launch, no factorisation.  rhs = the g of the last direction reproduces that direction bit for bit. */
int pyipm_qn_solve(pyipm_lbfgs_ctx* h, const double* rhs, double* dz, int flip, int memkind);
/* Refines dz in place as a solution of K dz = rhs (rhs == NULL: the g of the last direction).
 *   refine > 0: that many steps  r = rhs - K dz ;  dz += qn_solve(r).
 *   refine < 0: adaptive, the rule of pyipm_newton_solve: berr = |rhs - K dz|_2 / |rhs|_2 is measured before every step; stop
 *               converged at berr <= "refine_target", after "refine_max" steps, or when a step gained less than 4x; a step that
 *               made berr worse or not finite is taken back and the kept iterate returned.  Both options are set through
 *               pyipm_lbfgs_set_option (1e-14 / 8).  The host sees one synchronisation per measured berr.
 *   refine == 0: measures berr only; dz is not written. */
int pyipm_qn_refine(pyipm_lbfgs_ctx* h, const double* rhs, double* dz, int flip, int refine, int memkind);
/* Outcome of the last qn_refine, the layout of pyipm_newton_solve_info: out[0] = steps taken, out[1] = berr before the first
 * step, out[2] = berr of the kept iterate, out[3] = 1 when berr met the target (out[1..2] = -1 after refine > 0, which does
 * not measure). */
int pyipm_qn_info(pyipm_lbfgs_ctx* h, double out[4]);

/* ---- L-BFGS direction: partial restaging of the Jacobians (the handle and its conventions: pyipm_lbfgs.h).
 * Restage columns c0 .. c0 + count - 1 of J = [Je | Ji] alone (global column indices: 0 .. me - 1 is Je, me .. me + mi - 1
 * is Ji) from Jc, n x count row-major with ld >= count: for problems where only some constraints are nonlinear.  A strided
 * 2-D copy on the handle's stream like pyipm_lbfgs_stage_jacobian's; the padding columns stay zero.  The handle keeps the set of touched
 * tile indices c / 128 (calls accumulate until the next direction), and that direction computes again only the 128 x 128
 * lower-triangle tiles (i, j) of J'J with i or j in the set -- with the K partition, the tile arithmetic and the summation
 * order of the full launch, so the direction is bit for bit the one a full pyipm_lbfgs_stage_jacobian of the same J gives.
 * Tiles outside the set are neither read nor written; when every tile index is in it the full launch runs.
 * A full pyipm_lbfgs_stage_jacobian must have come first.  PYIPM_E_BADARG, with the staged J and the cached J'J untouched
 * and the handle usable, for: no full staging yet, c0 < 0, count < 0, c0 + count > me + mi, ld < count, Jc == NULL with
 * count > 0, a bad memkind.  count == 0 returns PYIPM_OK and changes nothing (the only accepted form when me = mi = 0).
 * Like a full staging the call ends the validity of the state pyipm_qn_* work from, until the next direction.
 * Row-sharded handles (pyipm_lbfgs_set_allreduce) accept the call and copy the columns, but the next direction then
 * computes and exchanges the whole of J'J: correct, nothing saved. */
int pyipm_lbfgs_stage_jacobian_columns(pyipm_lbfgs_ctx* h, int64_t c0, int64_t count, const double* Jc, int64_t ld,
                                       int memkind);

/* ---- L-BFGS direction: simple bounds as structure, not as Jacobian columns.
 * The mi inequalities of a direction split as mi = mg + mb: mg general ones, columns of Ji, then mb simple bounds.  Bound j
 * acts on variable var[j] with sign[j]: +1 is a lower bound x_k - l >= 0 (the column +e_k), -1 an upper bound u - x_k >= 0
 * (the column -e_k).  A bounded handle never sees those columns.  With k = var[j] the slack and the multiplier of bound j
 * eliminate in closed form,
 *     ds_j = sign_j dx_k - g_li,j ,   dlambda_j = Sigma_j ds_j - g_s,j ,
 *     theta_k = zeta + sum_{var[j]=k} Sigma_j ,   ghat_x[k] = g_x[k] + sum_{var[j]=k} sign_j (Sigma_j g_li,j + g_s,j) ,
 * and with omega_k = sqrt(zeta / theta_k) the system in (dx / omega, ds_g, dlambda_g) is the one pyipm_lbfgs_direction solves,
 * with the same zeta and M, on diag(omega) [Je | Ji], diag(omega) W and omega ghat_x: order me + mg, whatever mb is.
 *   The handle is a pyipm_lbfgs_ctx: destroy, last_error, set_stream, set_option, last_timings, stage_jacobian (Ji is n x mg),
 * stage_jacobian_columns and direction work on it.  EVERY vector of a direction keeps the layout it would have with explicit
 * columns: s has mg + mb entries, lda me + mg + mb, g and dz n + 2 (mg + mb) + me, the bounds in the last mb places of each
 * inequality block.  stats describe the factorisation of the reduced G of order me + mg (me + mg = 0: bounds only -- the general
 * branch with an empty J, no Gram matrix and no factorisation; all zero apart from m and small_pivot_min); the regularisation
 * rule is pyipm_lbfgs_direction's on the equality block of the reduced G.
 *   mb == 0 gives a plain handle: every call on it is the call on a handle from pyipm_lbfgs_create, to the bit.
 *   mb > 0: the Gram matrix of the scaled operand depends on Sigma of the bounds, so the Gram launch runs in every direction
 * (last_timings out[7] counts them; stage_jacobian_columns copies and saves nothing); pyipm_qn_matvec / _solve / _refine,
 * pyipm_lbfgs_kkt_*_many and pyipm_lbfgs_set_allreduce return PYIPM_E_BADARG with a text that names the bounded handle.  Sums
 * over a variable's bounds run in the order the bounds were given: equal calls give equal bits.
 *   bounded_workspace_bytes answers without a GPU (0: bad geometry); against pyipm_lbfgs_workspace_bytes(n, me, mg, ...) it
 * grows by O(n + mb) doubles and, where me + mg > 0, one more padded operand for the scaled copy -- never by mb^2.
 *   bounded_create: geometry as pyipm_lbfgs_create with n >= 1, me, mg, mb >= 0, checked before any device is looked for.
 *   bounded_stage: var and sign are HOST arrays of mb entries; the handle keeps a CSR by variable (a stable grouping: a
 * variable may carry none, one, two or repeated bounds).  Stage again to change the bounds; a direction before the first staging
 * on a handle with mb > 0 is PYIPM_E_BADARG.  PYIPM_E_BADARG with a last_error text and the bounds staged before untouched: a
 * NULL pointer with mb > 0, an index outside 0 .. n-1, a sign that is not +-1, more than 64 bounds on one variable (the tail of a
 * direction walks a variable's bounds once per bound of that variable). */
size_t pyipm_lbfgs_bounded_workspace_bytes(int64_t n, int64_t me, int64_t mg, int64_t mb, int max_pairs, int nb);
int pyipm_lbfgs_bounded_create(pyipm_lbfgs_ctx** out, int64_t n, int64_t me, int64_t mg, int64_t mb,
                               int max_pairs, int nb, int device, void* stream);
int pyipm_lbfgs_bounded_stage(pyipm_lbfgs_ctx* h, const int64_t* var, const double* sign);

/* ---- The quasi-Newton KKT operator for k columns per call: what pyipm_newton_kkt_matvec_many and pyipm_newton_solve_many
 * are to the exact-Hessian handle.  Column j of a block sits at base + j*ld, every ld >= N = n + 2 mi + me; entries
 * N .. ld-1 of an output column are not written.  flip as in pyipm_qn_*: the solution-space blocks (v, dz) have their
 * multiplier rows n + mi .. N-1 negated on read and on write; right-hand sides and products are never flipped.
 *   Valid exactly where pyipm_qn_* are.  PYIPM_E_BADARG, each but the first with a pyipm_lbfgs_last_error text: a NULL handle,
 *   no direction since the handle was created or the Jacobians were (re)staged, me + mi = 0, an all-reduce callback installed,
 *   a NULL block, an ld below N, k < 0, out overlapping v, a bad memkind.  k == 0 returns PYIPM_OK and does nothing.
 *   kkt_matvec_many: column j of out = K v_j with the K pyipm_qn_matvec applies -- from the staged Jacobians, the kept Sigma
 *   and the kept pairs, never from the factor, without regularisation.
 *   kkt_solve_many: column j of dz solves K~ dz_j = rhs_j from the kept state alone (the kept factor of zeta G, the kept 2m
 *   solved columns, the kept J'W and the kept 2m x 2m system): no Gram launch, no factorisation; the arithmetic of
 *   pyipm_qn_solve per column, the k substitutions as ONE block substitution (pyipm_newton_solve_many's, on the handle of
 *   order me + mi).  refine as in pyipm_newton_solve_many: > 0 that many steps R = B - K X; X += solve_many(R) with the residual
 *   formed by the many-column product; < 0 adaptive, stops when EVERY column meets "refine_target", after "refine_max" steps or
 *   when the worst column gains less than 4x, and takes back a step that made the worst column worse or not finite
 *   (pyipm_lbfgs_set_option reaches both options).  After refine != 0, pyipm_qn_info reports the step count and the worst
 *   column's backward errors.
 *   The two products with J run on the fp64 matrix pipe and read the staged J twice per 64 columns, where k calls of the
 *   single-column entries read it k (matvec) and 2k (solve) times.
 *   Column j of matvec_many, and of solve_many with refine >= 0, is bit for bit independent of k, of its place among the
 *   columns and of what the other columns hold (a NaN column stays in its column; no floating-point atomics; every split of a
 *   sum over n or me + mi is decided by the geometry alone); two identical calls give identical bits.  With refine < 0 the step
 *   count follows the worst column.  A column equals pyipm_qn_matvec / pyipm_qn_solve of that column to rounding, not to the bit.
 *   The calls write only buffers of their own and leave everything a direction left in the handle alone: a following
 *   pyipm_lbfgs_direction and pyipm_qn_solve(rhs = g) return the bits they return without them.
 *   Working memory for the column blocks is allocated by the library on first use and grown on demand (not part of
 *   pyipm_lbfgs_workspace_bytes).  Device blocks are used where they are, asynchronously on the handle's stream apart from the
 *   one synchronisation per measured backward error; PYIPM_MEM_HOST blocks are staged, and the call synchronises. */
int pyipm_lbfgs_kkt_matvec_many(pyipm_lbfgs_ctx* h, int64_t k, const double* v, int64_t ld_v,
                                double* out, int64_t ld_out, int flip, int memkind);
int pyipm_lbfgs_kkt_solve_many(pyipm_lbfgs_ctx* h, int64_t k, const double* rhs, int64_t ld_rhs,
                               double* dz, int64_t ld_dz, int flip, int refine, int memkind);

#ifdef __cplusplus
}
#endif
#endif /* PYIPM_NEWTON_H */
