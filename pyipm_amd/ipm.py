"""Host-side ``IPM`` — the reference's user surface over the MI355X Newton-step core.

Mirrors ``/root/reference/pyipm.py``: constructor keywords (``:311-314``),
``solve(x0, s0, lda0, force_recompile) -> (x, s, lda, fval, kkt)`` (``:1567, 1863``),
``signal`` codes (``:1656, 1665, 1680, 1761, 1781, 1796, 1502, 1548``) and the
verbosity transcript (``README.md:101-122``).  The outer/inner barrier loop and the
line search stay host Python (restated here from the algorithm the reference
documents: ``:1597-1628`` init, ``:1408-1436`` fraction-to-boundary, ``:1438-1565``
backtracking search, ``:1727-1735`` merit parameter, ``:1804-1814`` barrier update,
``:958-991`` KKT report); the per-iteration Newton step ``:1717-1725`` is delegated
to a *Newton backend* — the HIP core (``pyipm_amd.newton``).  There is no CPU
implementation of that backend in the product: without the HIP library and a GPU
the constructor of the default backend raises.

Inputs.  Aesara is not required: ``f, df, d2f, ce, dce, d2ce, ci, dci, d2ci`` are
plain callables over NumPy arrays with the signatures of the reference's
"precompiled" functions (``:85-146, 512-562``):
``f(x)``, ``df(x)``, ``d2f(x)``, ``ce(x)``, ``dce(x)->(n,me)``, ``d2ce(x,lda)``,
``ci(x)``, ``dci(x)->(n,mi)``, ``d2ci(x,lda)``.  All derivatives must be supplied
(no autodiff).

``lbfgs=m`` (pyipm.py:195-203) switches the direction to the limited-memory quasi-Newton form
(``:1007-1371``): no second derivatives are needed, the host keeps the displacement storage
(``lbfgs_init`` / ``lbfgs_update``, O(n m)) and the direction itself — a Gram matrix over the n
variables, an (me+mi)-order symmetric factorisation and the Woodbury correction — runs on the device
behind ``pyipm_lbfgs_direction`` (``HipLbfgsBackend``).
"""
from __future__ import annotations

import numpy as np

from . import reghess
from .loop import BarrierLoop, lbfgs_pair_update


class BoundBlock(object):
    """Simple bounds lb <= x <= ub as the LAST mb inequalities of ci: lower bounds first in ascending k (x_k - lb_k >= 0, the
    column +e_k), then upper bounds (ub_k - x_k >= 0, the column -e_k).  -inf / +inf or None: no bound.  The columns are never
    formed: every product with them is an index operation, O(n + mb)."""

    def __init__(self, lb, ub, n):
        lo = np.full(n, -np.inf) if lb is None else np.asarray(lb, dtype=np.float64).reshape(-1)
        hi = np.full(n, np.inf) if ub is None else np.asarray(ub, dtype=np.float64).reshape(-1)
        if lo.size != n or hi.size != n:
            raise ValueError("bounds: lb and ub need n = %d entries" % n)
        kl, ku = np.flatnonzero(np.isfinite(lo)), np.flatnonzero(np.isfinite(hi))
        self.n, self.mb = n, int(kl.size + ku.size)
        self.var = np.concatenate([kl, ku]).astype(np.int64)
        self.sign = np.concatenate([np.ones(kl.size), -np.ones(ku.size)])
        self.off = np.concatenate([-lo[kl], hi[ku]])
        self.count = np.bincount(self.var, minlength=n).astype(np.float64)

    def residual(self, x):
        """The bounds' rows of ci(x)."""
        return self.sign * x[self.var] + self.off

    def dot(self, v):
        """E v: the bound columns times mb multipliers (n)."""
        return np.bincount(self.var, weights=self.sign * v, minlength=self.n)

    def tdot(self, r):
        """E' r (mb)."""
        return self.sign * r[self.var]


class BoundedJacobian(object):
    """[Jd | E]: the dense columns [Je | Ji_general] and the bound block E of a BoundBlock, as the operator the host-side
    least-squares problems need (first multiplier estimate, feasibility restoration)."""

    def __init__(self, Jd, bb):
        self.Jd, self.bb = Jd, bb
        self.shape = (Jd.shape[0], Jd.shape[1] + bb.mb)

    def dot(self, v):
        pd = self.Jd.shape[1]
        return self.Jd @ v[:pd] + self.bb.dot(v[pd:])

    def tdot(self, r):
        return np.concatenate([self.Jd.T @ r, self.bb.tdot(r)])

    def gram(self, wide):
        """J J' (n x n: E E' is the diagonal of the bounds per variable) or J'J (p x p, by index)."""
        Jd, bb = self.Jd, self.bb
        if wide:
            G = Jd @ Jd.T
            G[np.diag_indices_from(G)] += bb.count
            return G
        cross = Jd[bb.var, :].T * bb.sign                                  # Jd'E
        same = (bb.var[:, None] == bb.var[None, :]) * np.outer(bb.sign, bb.sign)      # E'E (tall: mb < n)
        return np.block([[Jd.T @ Jd, cross], [cross.T, same]])

    def fro(self):
        return float(np.sqrt(np.linalg.norm(self.Jd) ** 2 + self.bb.mb))

    def dense(self):
        """Only where a rank-deficient Jacobian sends the first multiplier estimate to the SVD."""
        E = np.zeros((self.bb.n, self.bb.mb))
        E[self.bb.var, np.arange(self.bb.mb)] = self.bb.sign
        return np.concatenate([self.Jd, E], axis=1)


def pinv_apply(J, g):
    """pinv(J) @ g -- the reference's first multiplier estimate (pyipm.py:726-730) -- without the SVD where J allows it: for a
    Jacobian of full rank and moderate condition the normal equations (Cholesky + one refinement step) give the same vector at
    a fraction of the cost (an SVD of a 1500 x 3600 Jacobian was half of a whole LP solve); rank-deficient or badly conditioned
    Jacobians (Cholesky fails or its diagonal spans more than three decades) take numpy.linalg.pinv as before."""
    import scipy.linalg
    if isinstance(J, BoundedJacobian):             # the same steps with the bound block applied by index
        return _pinv_apply_bounded(J, g)
    J = np.asarray(J, dtype=np.float64)
    n, m = J.shape
    wide = m >= n
    G = J @ J.T if wide else J.T @ J
    try:
        cf = scipy.linalg.cho_factor(G, lower=True, check_finite=False)
        d = np.abs(np.diag(cf[0]))
        if d.size and np.isfinite(d).all() and d.min() > 1.0e-3 * d.max():
            def apply(r):
                if wide:
                    return J.T @ scipy.linalg.cho_solve(cf, r, check_finite=False)
                return scipy.linalg.cho_solve(cf, J.T @ r, check_finite=False)
            lam = apply(g)
            lam = lam + apply(g - J @ lam)
            # the spread of an unpivoted Cholesky diagonal does not bound cond(J J'): accept the vector only if it satisfies
            # the normal equations -- J lam = g for a wide J, J'(g - J lam) = 0 for a tall one -- to working precision
            # (ADVICE r4); anything else takes the SVD, whose rcond cutoff is what the reference's pinv applies
            r = g - J @ lam
            if not wide:
                r = J.T @ r
            scale = np.linalg.norm(g) if wide else np.linalg.norm(J) * np.linalg.norm(g)      # (Frobenius: no SVD)
            if np.isfinite(lam).all() and np.linalg.norm(r) <= 1.0e-11 * max(scale, np.finfo(float).tiny):
                return lam
    except (np.linalg.LinAlgError, ValueError):
        pass
    return np.linalg.pinv(J) @ g


def _pinv_apply_bounded(J, g):
    import scipy.linalg
    n, m = J.shape
    wide = m >= n
    try:
        cf = scipy.linalg.cho_factor(J.gram(wide), lower=True, check_finite=False)
        d = np.abs(np.diag(cf[0]))
        if d.size and np.isfinite(d).all() and d.min() > 1.0e-3 * d.max():
            def apply(r):
                if wide:
                    return J.tdot(scipy.linalg.cho_solve(cf, r, check_finite=False))
                return scipy.linalg.cho_solve(cf, J.tdot(r), check_finite=False)
            lam = apply(g)
            lam = lam + apply(g - J.dot(lam))
            r = g - J.dot(lam)
            if not wide:
                r = J.tdot(r)
            scale = np.linalg.norm(g) if wide else J.fro() * np.linalg.norm(g)
            if np.isfinite(lam).all() and np.linalg.norm(r) <= 1.0e-11 * max(scale, np.finfo(float).tiny):
                return lam
    except (np.linalg.LinAlgError, ValueError):
        pass
    return np.linalg.pinv(J.dense()) @ g


class HipNewtonBackend(object):
    """Newton backend on the HIP core: the counterpart of ``reghess`` + ``sym_solve_cmp``
    (pyipm.py:1373-1406, 1717-1725).

    * Inertia comes from the block pivots of the factorisation instead of ``eigvalsh`` (Sylvester).
    * The reference solves with LU + partial pivoting over the WHOLE matrix (pyipm.py:18-20); the device pivots
      inside 64x64 tiles.  A pivot that cannot be avoided inside its tile and has cancelled to nothing (LPs and
      other problems with zero Hessian rows: the x-x tile is singular although the KKT matrix is not) becomes a
      *static pivot* (``n_zero``): the factor is that of a matrix perturbed by sqrt(eps)|Hc| in those diagonal
      entries, and the direction of the UNperturbed system is recovered by refinement against the KKT blocks
      (``solve(refine=-1)``).  Converged => the reference's own answer with its own "no shift" decision.  Not
      converged => Hc is singular to working precision, which is what the reference's ``rcond <= eps`` test
      detects (pyipm.py:1379-1381): the same delta / delta_c branch is taken.
    * Without static pivots the "rcond <= eps" trigger is "d_min/d_max <= eps" on the block pivots."""

    # the bars of the rule (reghess.py); the rule is given this instance's values
    suspect_spread, berr_tol, berr_fallback = reghess.SUSPECT_SPREAD, reghess.BERR_TOL, reghess.BERR_FALLBACK

    def __init__(self, n, me, mi, device=None, nb=256, refine=0, max_shift_tries=60, device_step=False,
                 condensed=False):
        from .newton import NewtonCore
        self.core = NewtonCore(n, me, mi, device=device, nb=nb)
        self.condensed_requested = bool(condensed and mi)
        self.condensed_on = self.condensed_requested
        self.condensed_tol = 1e-9           # backward-error bar a condensed direction must meet
        self.n_condensed_fallback = 0
        self.condensed_fallback_reason = None
        self.n_calls = 0
        if self.condensed_on:               # factor the (n+me) condensed system
            self.core.set_option("condensed", 1)
        self.n, self.me, self.mi = n, me, mi
        self.refine = refine
        self.device_step = device_step      # closed-form step lengths on the device
        self.max_shift_tries = max_shift_tries
        self.n_factor = 0
        self.n_static = 0                   # directions recovered from a statically pivoted factor
        self.n_unconverged = 0              # refined solves that missed berr_tol and were sent to the shift branch
        self.n_inertia_retries = 0          # shifted factorisations whose inertia was still wrong (delta *= 10, pyipm.py:1399-1403)
        self.n_inexact = 0                  # directions returned on berr_fallback after the shift budget was spent
        self.rcond_log = []                 # (call, rcond estimate, pivot spread) of every estimate taken
        self.last_solve_info = None

    def shape(self):
        return (self.n, self.me, self.mi)

    def new_solve(self):
        """Called at the start of every IPM.solve(): a condensed-form fallback lasts for one solve, not for the
        lifetime of the backend."""
        if self.condensed_requested and not self.condensed_on:
            self.condensed_on = True
            self.core.set_option("condensed", 1)

    def _factor(self):
        """factor(); a NaN/Inf met on the way is reported like a singular matrix (the host regularises and retries,
        as reghess would) instead of aborting the solve."""
        from .newton import NewtonError
        self.n_factor += 1
        try:
            return self.core.factor()
        except NewtonError as e:
            if e.code != -4 or e.stats is None:
                raise
            return e.stats

    def _singular(self, st, eps):
        """The reference's ``rcond <= eps`` test (pyipm.py:1379-1381, rcond = min|w|/max|w| over the eigenvalues).
        Block pivots of moderate spread cannot hide an eigenvalue ratio at the eps level (``reghess.suspect``); otherwise,
        and whenever static pivots were placed, the ratio is ESTIMATED from the factor and the blocks (``core.rcond``:
        inverse / power iterations) and judged by ``reghess.singular``.

        The estimate is taken with adaptive iteration counts (``core.rcond(-1, -1)``, include/pyipm_newton.h): late in an
        interior-point run the pivot spread stays below ``suspect_spread`` at EVERY iterate (Sigma = lda_i / s spans twenty
        decades by itself, the spread falls a thousandfold per iterate while rcond falls twentyfold: 2e-6 ... 3e-16 over the
        last seven iterates of the benchmark QP), so the estimate is part of every late step: 7.4 ms instead of 14.8 at
        N = 32768, and it leaves a right-hand side that was forward-substituted under the factorisation in place."""
        self.last_rcond = None
        if st["nonfinite"]:
            return True
        if not reghess.suspect(st, self.suspect_spread):
            return False
        # adaptive iteration counts (include/pyipm_newton.h): the threshold decision of the fixed 3 + 6 iterations at a
        # third of their cost when the matrix is far from singular -- every suspect iterate of a convex QP
        est = self.last_rcond = self.core.rcond(-1, -1) if st["n_zero"] == 0 else self.core.rcond()
        self.n_rcond += 1
        self.rcond_log.append((self.n_calls, est["rcond"], st["d_min"] / st["d_max"] if st["d_max"] > 0 else 1.0))
        return reghess.singular((est["w_min"], est["w_max"], est["rcond"], est["static_pivot"]), st, eps, nan_singular=False)

    n_rcond = n_rcond_reused = 0
    rcond_log = []

    _at_risk = staticmethod(reghess.at_risk)

    def _solve(self, st):
        """Substitution for the current factor; (dz tensor, converged)."""
        core = self.core
        if self._at_risk(st):
            dz = core.solve(flip=True, refine=-1)
            info = self.last_solve_info = core.solve_info()
            return dz, info["backward_error"] >= 0.0 and info["backward_error"] <= self.berr_tol
        self.last_solve_info = None
        return core.solve(flip=True, refine=self.refine), True

    def direction(self, d2L, Je, Ji, df, ce, ci, s, lda, mu, delta, mu_host, eta, beta, reg_coef, delta0, eps,
                  as_tensor=False, staged=False, g=None):
        """as_tensor: inputs may be device tensors (staged without copies) and dz stays on the device.
        staged: the caller has already staged the blocks (constant for a QP: once per solve) and this point's vectors and
        formed g = -grad in the handle (``core.residual()``, passed as ``g``) -- nothing is staged again here."""
        core, need = self.core, self.me + self.mi
        self.n_calls += 1
        self._dir_override = None          # set when the direction returned is NOT the handle's last solve (see step_lengths)
        if not staged:
            core.stage_blocks(d2L, Je, Ji)
            core.stage_vectors(df, ce, ci, s, lda, mu=mu, eps=eps)
            g = core.residual()
        elif g is None and self.condensed_on:
            g = core.residual()
        if self.condensed_on:
            # Condensed system first (2x fewer flops at the benchmark shape).  The block pivots are explicit
            # 64x64 inverses, so a dense ill-conditioned tile (Sigma spanning > ~1e8 late in a run) costs
            # accuracy ~ eps*sqrt(cond): accept only a direction whose backward error against the FULL blocks
            # is small and whose inertia is right; otherwise use the full system for the rest of this solve.
            core.assemble(0.0, 0.0)
            st = self._factor()
            ok = st["n_zero"] == 0 and st["n_neg"] == need and not st["nonfinite"]
            why = "inertia %d/%d, %d static pivots" % (st["n_neg"], need, st["n_zero"])
            if ok:
                gn = float(g.norm())
                for refine in (self.refine, max(self.refine, 1) + 3):      # second try: more refinement steps
                    dz = core.solve(flip=True, refine=refine)
                    raw = dz.clone()
                    raw[self.n + self.mi:] *= -1.0
                    rn = float((core.matvec(raw) - g).norm())
                    berr = rn / gn if gn > 0.0 else rn                     # zero residual: the zero direction is exact
                    ok = berr <= self.condensed_tol
                    why = "backward error %.1e after %d refinement steps" % (berr, max(refine, 1))
                    if ok:
                        break
            if ok:
                if not as_tensor:
                    dz = dz.cpu().numpy()
                return dz, 0.0 if delta == 0.0 else float(delta), st
            self.condensed_on = False
            self.n_condensed_fallback += 1
            self.condensed_fallback_reason = "call %d: %s" % (self.n_calls, why)
            core.set_option("condensed", 0)
        core.assemble(0.0, 0.0)
        st = self._factor()
        singular = self._singular(st, eps)
        dz = None
        loop = reghess.ShiftLoop(self.max_shift_tries, self.berr_fallback, retry_overrun_as_miss=True, stall_on_inf=True)

        def missed():
            """(backward error, how to copy the direction) of the solve that just missed berr_tol."""
            self.n_unconverged += 1
            info = self.last_solve_info
            return (info["backward_error"] if info else -1.0), (lambda: dz.clone() if hasattr(dz, "clone") else dz)

        if not singular and st["n_neg"] == need:
            dz, converged = self._solve(st)
            if not converged:
                # a statically pivoted / 2x2 / high-growth factor whose refinement against the blocks stalls above
                # berr_tol solves a nearby system, not this one: what the reference's LU would flag as rcond <= eps.
                # Take the branch reghess takes then (pyipm.py:1379-1403) instead of returning the direction silently.
                loop.remember(*missed(), 0.0, st)
                dz, singular = None, True
            elif st["n_zero"] > 0:
                self.n_static += 1         # reference: LU over the whole matrix, no shift (pyipm.py:1381 not taken)
        if dz is None:
            # the shift loop (reghess.ShiftLoop: the reference's delta *= 10 loop, :1399-1403, until the inertia is right AND
            # the direction satisfies the blocks)
            delta_c = reghess.delta_c(singular, self.me, reg_coef, eta, mu_host, beta)
            delta = reghess.first_shift(delta, delta0)
            while True:
                core.assemble(delta, delta_c)
                st = self._factor()
                if reghess.wrong(st, need):
                    self.n_inertia_retries += 1      # (an inertia retry, not an unconverged solve: counted on its own)
                    verdict = loop.inertia_retry()
                else:
                    dz, converged = self._solve(st)
                    if converged:                    # (no n_static here: that counter is the UNshifted recoveries')
                        break
                    verdict = loop.miss(*missed(), delta, st)
                if verdict == reghess.SETTLE:
                    self.n_inexact += 1
                    _, dz, delta, st = loop.best
                    self._dir_override = dz
                    break
                if verdict == reghess.LOST_INERTIA:
                    raise RuntimeError("inertia not corrected after %d diagonal shifts" % loop.tries)
                if verdict == reghess.LOST_SOLVE:
                    raise RuntimeError("refined solve did not reach backward error %.1e after %d diagonal shifts (last: %s)"
                                       % (self.berr_tol, loop.tries, self.last_solve_info))
                delta *= 10.0
        if not as_tensor:
            dz = dz.cpu().numpy()
        return dz, float(delta), st

    _dir_override = None

    def step_lengths(self, tau):
        """(alpha_smax, alpha_lmax) for the direction just returned, or None to let the host search.  When direction() gave up
        on shifting and returned an EARLIER, less shifted solve (n_inexact), the handle's last direction is another one: the
        lengths are then taken for the direction actually returned (they used to come from the most shifted
        solve, and s + a ds could leave the positive orthant)."""
        if not (self.device_step and self.mi):
            return None
        return self.core.step_lengths(tau, dz=self._dir_override)


class HipLbfgsBackend(object):
    """L-BFGS direction on the HIP library: the counterpart of ``lbfgs_dir_func`` (pyipm.py:872-875,
    1184-1246).  The "rcond <= eps" trigger on the equality block (:1108-1113, an ``eigh`` in the
    reference) is taken from the block pivots of the factorisation, as in ``HipNewtonBackend``."""

    def __init__(self, n, me, mi, memory, device=None, nb=256, linear_constraints=False, refine=0, bounds=None):
        """``bounds=(var, sign)``: simple bounds BEHIND the mi general inequalities, on a bounded handle
        (``LbfgsCore(bounds=...)``): Ji, the staged columns and a ``linear_constraints`` mask cover the me + mi general
        columns alone; s, lda, g and the direction count mi + len(var) inequalities."""
        from .lbfgs import LbfgsCore
        if bounds is not None and refine:
            raise NotImplementedError("lbfgs_refine with bounds: the quasi-Newton KKT operator has no bound block")
        self.core = LbfgsCore(n, me, mi, int(memory) + 1, device=device, nb=nb, bounds=bounds)   # storage grows to memory+1 (:1300)
        self.n, self.me, self.mi = n, me, mi
        self.mb = self.core.mb
        # linear_constraints: True = dce/dci do not depend on x (stage once, J'J is reused), False = they all may, or a boolean
        # mask over the me + mi columns of [Je | Ji], True where a column does not: after the first direction only the runs of
        # False columns are staged again, and only the tiles of J'J they reach are recomputed
        self.column_runs = None                # [(c0, c1), ...]: the maximal runs of columns that depend on x (a mixed mask only)
        if np.ndim(linear_constraints) > 0:
            mask = np.asarray(linear_constraints, dtype=bool).reshape(-1)
            if mask.size != me + mi:
                raise ValueError("linear_constraints: a mask needs me + mi = %d entries, got %d" % (me + mi, mask.size))
            linear_constraints = bool(mask.all())
            if not linear_constraints and mask.any():
                edges = np.flatnonzero(np.diff(np.concatenate([[True], mask, [True]]).astype(np.int8)))
                self.column_runs = [(int(a), int(b)) for a, b in zip(edges[0::2], edges[1::2])]
        self.linear_constraints = bool(linear_constraints)
        self.refine = int(refine)              # != 0: every constrained direction is refined against the quasi-Newton KKT operator
        self.last_refine_info = None
        self.n_calls = self.n_staged = 0
        self.n_cols_staged = 0                 # columns of [Je | Ji] copied to the device so far (a full staging: me + mi)
        self.pair_doubles_uploaded = 0         # S / Y entries that crossed from the host (none with a resident pair store)

    def shape(self):
        return (self.n, self.me, self.mi + self.mb)

    def lbfgs_direction(self, Je, Ji, s, lda, g, zeta, S, Y, SS, L, D, reg, eps):
        self.n_calls += 1
        self.pair_doubles_uploaded += sum(int(a.size) for a in (S, Y) if isinstance(a, np.ndarray))   # device tensors pass through
        if (self.me or self.mi) and self.n_staged and self.column_runs is not None:
            me = self.me
            for c0, c1 in self.column_runs:
                parts = ([Je[:, c0:min(c1, me)]] if c0 < me else []) + ([Ji[:, max(c0, me) - me:c1 - me]] if c1 > me else [])
                self.core.stage_jacobian_columns(c0, parts[0] if len(parts) == 1 else np.concatenate(parts, axis=1))
                self.n_cols_staged += c1 - c0
        elif (self.me or self.mi) and not (self.linear_constraints and self.n_staged):
            self.core.stage_jacobian(Je, Ji)
            self.n_staged += 1
            self.n_cols_staged += self.me + self.mi
        dz, self.last_stats = self.core.direction(g, s, lda, zeta, S, Y, SS, L, D, reg=reg, eps=eps, flip=False,
                                                  refine=self.refine)
        if self.refine and (self.me or self.mi):
            self.last_refine_info = self.core.refine_info()
        if S.shape[1] and self.last_stats["small_pivot_min"] == 0.0:
            # the reference's sym_solve raises on an exactly singular system (scipy.linalg.solve, pyipm.py:18-20)
            raise np.linalg.LinAlgError("L-BFGS: the 2m x 2m system is singular (zero pivot)")
        return dz.cpu().numpy()


class IPM(BarrierLoop):
    """Line-search primal-dual interior-point solver; see module docstring.  The barrier loop itself is
    ``pyipm_amd.loop.BarrierLoop``: this class is its NumPy / user-callable side."""

    def __init__(self, x0=None, x_dev=None, f=None, df=None, d2f=None, ce=None, dce=None, d2ce=None, ci=None,
                 dci=None, d2ci=None, lda0=None, lambda_dev=None, s0=None, mu=0.2, nu=10.0, rho=0.1, tau=0.995,
                 eta=1.0E-4, beta=0.4, miter=20, niter=10, Xtol=None, Ktol=1.0E-4, Ftol=None, lbfgs=False,
                 lbfgs_zeta=None, float_dtype=np.float64, verbosity=1, backend=None, device=None, nb=256, refine=0,
                 device_step=False, condensed=False, linear_constraints=False, resident_pairs=False, lbfgs_refine=0,
                 bounds=None):
        """``bounds=(lb, ub)`` (L-BFGS mode): simple bounds on x, length n each, -inf / +inf or None where there is none.
        They are the last inequalities -- lower bounds in ascending k, then upper bounds: ``nineq``, s and the returned
        multipliers count them -- and are never written as columns of ``dci`` (``BoundBlock``)."""
        if bounds is not None and not lbfgs:
            raise NotImplementedError("bounds need lbfgs=m: the exact-Hessian handle takes bounds as rows of ci only")
        if bounds is not None and lbfgs_refine:
            raise NotImplementedError("lbfgs_refine with bounds: the quasi-Newton KKT operator has no bound block")
        self.bounds, self._bb = bounds, None
        self.x0, self.s0, self.lda0 = x0, s0, lda0
        self.x_dev, self.lambda_dev = x_dev, lambda_dev        # accepted for signature parity; unused
        self.f, self.df, self.d2f = f, df, d2f
        self.ce, self.dce, self.d2ce = ce, dce, d2ce
        self.ci, self.dci, self.d2ci = ci, dci, d2ci
        self.nvar = self.neq = self.nineq = None
        self.float_dtype = float_dtype
        self.eps = float(np.finfo(float_dtype).eps)
        self.mu, self.nu, self.rho, self.tau, self.eta, self.beta = mu, nu, rho, tau, eta, beta
        self.miter, self.niter = miter, niter
        self.Xtol = Xtol if Xtol else self.eps
        self.Ktol, self.Ftol = Ktol, Ftol
        self.reg_coef = float(np.sqrt(self.eps))
        self.delta0 = self.reg_coef
        self.lbfgs = lbfgs
        self.lbfgs_zeta = 1.0 if (lbfgs and lbfgs_zeta is None) else lbfgs_zeta         # pyipm.py:355-359
        self.lbfgs_fail_max = lbfgs                                                     # :360
        self.verbosity = verbosity
        self.backend = backend
        self._own_backend = backend is None
        self._backend_opts = dict(device=device, nb=nb, refine=refine, device_step=device_step, condensed=condensed)
        self.linear_constraints = linear_constraints       # L-BFGS mode: Jacobians staged once, J'J reused; or a boolean mask over
                                                           # the me + mi columns of [Je | Ji] (HipLbfgsBackend): True = constant
        self.resident_pairs = bool(resident_pairs)         # L-BFGS mode: S, Y in the library's pair store (pyipm_amd.lbfgs.PairStore)
        self.lbfgs_refine = int(lbfgs_refine)              # L-BFGS mode: refinement of every direction (LbfgsCore.refine); 0 = none
        self._pairs = None
        self.compiled = False
        self.signal = 0

    # ------------------------------------------------------------------ setup
    def validate(self):
        assert self.f is not None
        assert (self.ce is not None) or (self.dce is None and self.d2ce is None)
        assert (self.ci is not None) or (self.dci is None and self.d2ci is None)
        assert self.mu > 0.0 and self.nu > 0.0
        assert 0.0 < self.eta < 1.0 and 0.0 < self.rho < 1.0 and 0.0 < self.tau < 1.0
        assert self.beta < 1.0
        assert isinstance(self.miter, int) and self.miter >= 0
        assert isinstance(self.niter, int) and self.niter >= 0
        assert self.Xtol >= self.eps and self.Ktol >= self.eps
        assert self.Ftol is None or self.Ftol >= 0.0
        assert self.lbfgs is False or self.lbfgs >= 0                                  # pyipm.py:405-408
        if self.lbfgs:
            assert isinstance(self.lbfgs, int) and not isinstance(self.lbfgs, bool)
            if self.lbfgs > 31:
                raise NotImplementedError("the device direction keeps the 2m x 2m system in one 64 x 64 tile: lbfgs <= 31")
        assert self.lbfgs_zeta is None or self.lbfgs_zeta > 0.0
        if self.float_dtype != np.float64:
            raise NotImplementedError("the Newton-step core computes in fp64 only")
        second = () if self.lbfgs else ("d2f",)
        for name in ("df",) + second:
            if getattr(self, name) is None:
                raise ValueError("%s must be supplied as a callable (no autodiff without Aesara)" % name)
        if self.ce is not None and (self.dce is None or (self.d2ce is None and not self.lbfgs)):
            raise ValueError("dce and d2ce must be supplied with ce")
        if self.ci is not None and (self.dci is None or (self.d2ci is None and not self.lbfgs)):
            raise ValueError("dci and d2ci must be supplied with ci")

    def compile(self, nvar=None, neq=None, nineq=None):
        """Infer constraint counts (pyipm.py:443-467) and bind the Newton backend."""
        if nvar is not None:
            self.nvar = nvar
        x0 = np.asarray(self.x0, dtype=np.float64)
        self.neq = int(np.size(self.ce(x0))) if (self.ce is not None and neq is None) else int(neq or 0)
        if self.bounds is not None:
            self._bb = BoundBlock(self.bounds[0], self.bounds[1], self.nvar)
        mb = self._bb.mb if self._bb is not None else 0
        self.nineq = (int(np.size(self.ci(x0))) if (self.ci is not None and nineq is None) else int(nineq or 0)) + mb
        if self.backend is not None and self._own_backend and hasattr(self.backend, "shape") and \
                self.backend.shape() != (self.nvar, self.neq, self.nineq):
            self.backend = None            # force_recompile with another problem shape: the handle is per shape
        if self.backend is None:
            self._own_backend = True
            if self.lbfgs:
                self.backend = HipLbfgsBackend(self.nvar, self.neq, self.nineq - mb, self.lbfgs,
                                               device=self._backend_opts["device"], nb=self._backend_opts["nb"],
                                               linear_constraints=self.linear_constraints, refine=self.lbfgs_refine,
                                               bounds=(self._bb.var, self._bb.sign) if mb else None)
            else:
                self.backend = HipNewtonBackend(self.nvar, self.neq, self.nineq, **self._backend_opts)
        self.compiled = True

    # ------------------------------------------------------------------ model pieces (host, O(n m))
    # the inequalities: the caller's ci / dci for the general ones, then the bound block, applied by index
    def _ci(self, x):
        mg = self.nineq - (self._bb.mb if self._bb is not None else 0)
        parts = [np.asarray(self.ci(x), dtype=np.float64).reshape(mg)] if mg else []
        if self._bb is not None:
            parts.append(self._bb.residual(np.asarray(x, dtype=np.float64)))
        return np.concatenate(parts) if len(parts) != 1 else parts[0]

    def _ji(self, x):
        """The inequality columns that ARE columns: dci(x), n x mg (None without general inequalities)."""
        mg = self.nineq - (self._bb.mb if self._bb is not None else 0)
        return np.asarray(self.dci(x), dtype=np.float64).reshape(self.nvar, mg) if mg else None

    def _ji_dot(self, x, v):
        """Ji v over all nineq inequalities."""
        Jg = self._ji(x)
        mg = 0 if Jg is None else Jg.shape[1]
        out = Jg @ v[:mg] if mg else np.zeros(self.nvar)
        return out + self._bb.dot(v[mg:]) if self._bb is not None else out

    def _con(self, x, s):
        parts = []
        if self.neq:
            parts.append(np.asarray(self.ce(x), dtype=np.float64).reshape(self.neq))
        if self.nineq:
            parts.append(self._ci(x) - s)
        return np.concatenate(parts) if parts else np.zeros(0)

    def _jac_x(self, x):
        """[Je | Ji]: a dense array, or with bounds the operator ``BoundedJacobian`` over the dense general columns."""
        cols = []
        if self.neq:
            cols.append(np.asarray(self.dce(x), dtype=np.float64).reshape(self.nvar, self.neq))
        Jg = self._ji(x) if self.nineq else None
        if Jg is not None:
            cols.append(Jg)
        Jd = np.concatenate(cols, axis=1) if cols else np.zeros((self.nvar, 0))
        return BoundedJacobian(Jd, self._bb) if self._bb is not None else Jd

    def _jaco(self, x):
        """(n+mi) x (me+mi) composite Jacobian [[Je, Ji],[0, -I]] (pyipm.py:582-607)."""
        top = self._jac_x(x)
        if not self.nineq:
            return top
        bottom = np.concatenate([np.zeros((self.nineq, self.neq)), -np.eye(self.nineq)], axis=1)
        return np.concatenate([top, bottom], axis=0)

    def grad(self, x, s, lda):
        """KKT residual on the host (same formula as K2; used by the KKT report and convergence tests)."""
        n, me, mi = self.nvar, self.neq, self.nineq
        gx = np.array(self.df(x), dtype=np.float64).reshape(n)
        out = [None]
        if me:
            gx = gx - np.asarray(self.dce(x), dtype=np.float64).reshape(n, me) @ lda[:me]
        if mi:
            gx = gx - self._ji_dot(x, lda[me:])
            out.append(lda[me:] - self.mu_host_dev / (s + self.eps))
        out[0] = gx
        if me:
            out.append(np.asarray(self.ce(x), dtype=np.float64).reshape(me))
        if mi:
            out.append(self._ci(x) - s)
        return np.concatenate(out)

    def KKT(self, x, s, lda):
        """First-order conditions split in four blocks, slack block scaled by s (pyipm.py:958-991)."""
        n, me, mi = self.nvar, self.neq, self.nineq
        k = self.grad(x, s, lda)
        zero = np.float64(0.0)
        k1 = k[:n]
        k2 = k[n:n + mi] * s if mi else zero
        k3 = k[n + mi:n + mi + me] if me else zero
        k4 = k[n + mi + me:] if mi else zero
        return k1, k2, k3, k4

    def phi(self, x, s):
        v = float(self.f(x))
        if self.neq:
            v += self.nu_host * np.sum(np.abs(self.ce(x)))
        if self.nineq:
            v += self.nu_host * np.sum(np.abs(self._ci(x) - s))
            v -= self.mu_host_dev * np.sum(np.log(s))
        return v

    def dphi(self, x, s, dz):
        n = self.nvar
        v = float(np.dot(np.asarray(self.df(x)).reshape(n), dz[:n]))
        if self.neq:
            v -= self.nu_host * np.sum(np.abs(self.ce(x)))
        if self.nineq:
            v -= self.nu_host * np.sum(np.abs(self._ci(x) - s))
            v -= float(np.dot(self.mu_host_dev / (s + self.eps), dz[n:]))
        return v

    # ------------------------------------------------------------------ line-search pieces
    def step(self, x, dx):
        """Fraction-to-the-boundary step by golden-section search on [0,1] (pyipm.py:1408-1436)."""
        gold = (np.sqrt(5.0) + 1.0) / 2.0
        floor = (1.0 - self.tau) * x

        def feasible(alpha):
            return bool(np.all(x + alpha * dx >= floor))

        lo, hi = 0.0, 1.0
        if feasible(hi):
            return hi
        c = hi - (hi - lo) / gold
        d = lo + (hi - lo) / gold
        while abs(hi - lo) > gold * self.Xtol:
            if feasible(d):
                lo = d
            else:
                hi = d
            if c > lo:
                if feasible(c):
                    lo = c
                else:
                    hi = c
            c = hi - (hi - lo) / gold
            d = lo + (hi - lo) / gold
        return lo

    def _restoration(self, x0, c_new):
        """Feasibility-restoration direction of the second-order correction (pyipm.py:1466-1477,
        1518-1529): a square solve when the Jacobian happens to be square, otherwise (the usual
        case) the minimum-norm least-squares solution."""
        if self._bb is not None:
            return self._restoration_bounded(x0, c_new)
        A = self._jaco(x0).T
        if A.shape[0] == A.shape[1]:
            try:
                import scipy.linalg
                return -scipy.linalg.solve(A, c_new.reshape(-1, 1)).reshape(-1)
            except Exception:
                pass
        return -np.linalg.lstsq(A, c_new, rcond=None)[0]

    def _restoration_bounded(self, x0, c_new):
        """The same minimum-norm solution of [J' | [0; -I]] d = c with the bound block eliminated by index: a bound's row
        gives ds_b,j = sigma_j dx_k - c_b,j, so d minimises dx'D dx - 2 b'dx + |ds_g|^2 (D = I + bounds per variable,
        b = E c_b) under the general rows alone -- order me + mg, O(n + mb) for the bounds."""
        n, bb = self.nvar, self._bb
        pg = self.neq + self.nineq - bb.mb
        mg = self.nineq - bb.mb
        cg, cb = c_new[:pg], c_new[pg:]
        hinv = np.concatenate([1.0 / (1.0 + bb.count), np.ones(mg)])
        h = np.concatenate([bb.dot(cb), np.zeros(mg)])
        z = hinv * h
        if pg:
            A = np.concatenate([self._jac_x(x0).Jd, np.concatenate([np.zeros((mg, self.neq)), -np.eye(mg)], axis=1)], axis=0).T
            nu = np.linalg.lstsq((A * hinv) @ A.T, cg - A @ z, rcond=None)[0]
            z = z + hinv * (A.T @ nu)
        return -np.concatenate([z, bb.tdot(z[:n]) - cb])

    def search(self, x0, s0, lda0, dz, alpha_smax, alpha_lmax, info=None):
        """Backtracking Armijo search on the merit function with an optional second-order
        feasibility correction (pyipm.py:1438-1565).  ``info`` is the loop's hand-over slot and carries nothing here."""
        n, me, mi = self.nvar, self.neq, self.nineq
        dx, ds = dz[:n], dz[n:n + mi]
        if not (me or mi):
            alpha_lmax = 0.0
        phi0 = self.phi(x0, s0)
        dphi0 = self.dphi(x0, s0, dz[:n + mi])
        armijo = lambda a: phi0 + a * self.eta * dphi0    # noqa: E731
        corrected, alpha_corr, dz_p = False, 1.0, None

        def trial(a):
            return self.phi(x0 + a * dx, s0 + a * ds) if mi else self.phi(x0 + a * dx, s0)

        if trial(alpha_smax) > armijo(alpha_smax):
            if me or mi:
                c_old = self._con(x0, s0)
                c_new = self._con(x0 + alpha_smax * dx, s0 + alpha_smax * ds if mi else s0)
                if np.sum(np.abs(c_new)) > np.sum(np.abs(c_old)):
                    dz_p = self._restoration(x0, c_new)
                    corrected, alpha_corr = self._second_order_correction(x0, s0, dx, ds, dz_p, alpha_smax,
                                                                          armijo(alpha_smax))
            if not corrected:
                alpha_smax *= self.tau
                alpha_lmax *= self.tau
                while trial(alpha_smax) > armijo(alpha_smax):
                    size = np.linalg.norm(alpha_smax * dx)
                    if mi:
                        size = np.sqrt(size ** 2 + np.linalg.norm(alpha_lmax * ds) ** 2)
                    if size < self.eps:
                        if self.verbosity > 2:
                            print('Search direction is unreliable to machine precision.')
                        self.signal = -2
                        return x0, s0, lda0
                    alpha_smax *= self.tau
                    alpha_lmax *= self.tau
        return self._step_to(x0, s0, lda0, dz, alpha_smax, alpha_lmax, alpha_corr, dz_p if corrected else None)

    # ------------------------------------------------------------------ the Newton step (hot path)
    def newton_direction(self, x, s, lda):
        """Counterpart of pyipm.py:1717-1725: host evaluates the derivative blocks, the backend
        assembles / regularises / factors / solves on the device and returns dz (sign-flipped)."""
        n, me, mi = self.nvar, self.neq, self.nineq
        d2L = np.array(self.d2f(x), dtype=np.float64).reshape(n, n)
        Je = Ji = ce = ci = None
        if me:
            d2L = d2L - np.asarray(self.d2ce(x, lda), dtype=np.float64).reshape(n, n)
            Je = np.asarray(self.dce(x), dtype=np.float64).reshape(n, me)
            ce = np.asarray(self.ce(x), dtype=np.float64).reshape(me)
        if mi:
            d2L = d2L - np.asarray(self.d2ci(x, lda), dtype=np.float64).reshape(n, n)
            Ji = np.asarray(self.dci(x), dtype=np.float64).reshape(n, mi)
            ci = np.asarray(self.ci(x), dtype=np.float64).reshape(mi)
        df = np.asarray(self.df(x), dtype=np.float64).reshape(n)
        dz, self.delta, self.last_stats = self.backend.direction(
            d2L, Je, Ji, df, ce, ci, s, lda, self.mu_host_dev, self.delta, self.mu_host, self.eta, self.beta,
            self.reg_coef, self.delta0, self.eps)
        return dz

    # ------------------------------------------------------------------ L-BFGS storage (host, O(n m))
    def lbfgs_init(self):
        """Empty displacement storage (pyipm.py:993-1005)."""
        if self.resident_pairs:
            return self._pair_store(reset=True).view()
        n, z = self.nvar, np.zeros
        return float(self.lbfgs_zeta), z((n, 0)), z((n, 0)), z((0, 0)), z((0, 0)), z((0, 0)), 0

    def lbfgs_update(self, x_old, x_new, g_old, g_new, zeta, S, Y, SS, L, D, lbfgs_fail):
        """Append the newest (dx, dg) pair and its inner products; pairs of non-positive curvature are
        skipped and counted, too many skips in a row reset the storage (pyipm.py:1282-1371).  For constrained
        problems SS = S'S, L = strictly-lower(S'Y), zeta scales the Hessian; for unconstrained ones the same
        arrays hold Y'Y and the upper-triangular S'Y and zeta scales the inverse Hessian."""
        if self.resident_pairs:                      # the same update as ONE offer to the device-resident store
            store = self._pair_store()
            if store.offer(x_old, x_new, g_old, g_new, self.eps) == 2 and self.verbosity > 2:
                print('Max failures reached, resetting storage arrays.')
            return store.view()
        n, con = self.nvar, bool(self.neq or self.nineq)
        dx = x_new - x_old
        dg = g_old[:n] - g_new[:n]
        drop = S.shape[1] > self.lbfgs                   # the reference lets the storage reach lbfgs+1 pairs (:1300)
        Sn = np.concatenate([S[:, 1:] if drop else S, dx[:, None]], axis=1)
        Yn = np.concatenate([Y[:, 1:] if drop else Y, dg[:, None]], axis=1)
        accepted, reset, zeta, SS, L, D, lbfgs_fail = lbfgs_pair_update(
            zeta, SS, L, D, lbfgs_fail, drop, Sn.T @ dx if con else Yn.T @ dg, dx @ Yn if con else Sn.T @ dg,
            float(np.dot(dg, dx)), np.dot(dx, dx) if con else np.dot(dg, dg), con, self.lbfgs_fail_max, self.eps)
        if accepted:
            S, Y = Sn, Yn
        if reset:
            if self.verbosity > 2:
                print('Max failures reached, resetting storage arrays.')
            return self.lbfgs_init()
        return zeta, S, Y, SS, L, D, lbfgs_fail

    def _pair_store(self, reset=False):
        """The store of this problem's shape, on the backend's device; created on first use."""
        from .lbfgs import PairStore
        key = (self.nvar, int(self.lbfgs), bool(self.neq or self.nineq), float(self.lbfgs_zeta))
        if self._pairs is None or self._pairs[0] != key:
            core = getattr(self.backend, "core", None)
            dev = core.device.index if core is not None else self._backend_opts["device"]
            self._pairs = (key, PairStore(key[0], key[1], key[2], zeta0=key[3], device=dev))
        elif reset:
            self._pairs[1].reset()
        return self._pairs[1]

    def lbfgs_dir(self, x, s, lda, g, zeta, S, Y, SS, L, D):
        """Counterpart of pyipm.py:1184-1246: the host evaluates the constraint Jacobians, the backend forms
        and solves the Woodbury system on the device and returns the RAW direction (the caller flips the
        multiplier rows, :1723-1725).  The square-Jacobian shortcut (:1188-1198) is not taken: it returns the
        same direction through inv(B) and, as written, cannot be compiled (duplicate input, :877-880)."""
        n, me, mi = self.nvar, self.neq, self.nineq
        Je = np.asarray(self.dce(x), dtype=np.float64).reshape(n, me) if me else None
        Ji = self._ji(x) if mi else None           # (the general columns alone: bounds are the handle's structure)
        reg = self.reg_coef * self.eta * (self.mu_host_dev ** self.beta)              # :1113
        return self.backend.lbfgs_direction(Je, Ji, s, lda, g, zeta, S, Y, SS, L, D, reg, self.eps)

    def _lbfgs_direction(self, x, s, lda, g, zeta, S, Y, SS, L, D):
        dz = self.lbfgs_dir(x, s, lda, g, zeta, S, Y, SS, L, D)
        if self.neq or self.nineq:
            dz[self.nvar + self.nineq:] = -dz[self.nvar + self.nineq:]                # :1723-1725
        return dz

    # ------------------------------------------------------------------ what the loop asks for (pyipm_amd.loop.BarrierLoop)
    def _kkt_norms(self, kkt):
        return (np.linalg.norm(k) for k in kkt)        # lazily: the smallness tests stop at the first block above tol

    def _neg_grad(self, x, s, lda):
        return -self.grad(x, s, lda)

    def _set_barrier(self, mu):
        self.mu_host = self.mu_host_dev = mu              # mu_host_dev: value of the reference's shared mu_dev

    def _step_lengths(self, s, lda, dz):
        n, me, mi = self.nvar, self.neq, self.nineq
        dev = self.backend.step_lengths(self.tau) if hasattr(self.backend, "step_lengths") else None
        if dev is not None:
            return dev
        return self.step(s, dz[n:n + mi]), self.step(lda[me:], dz[n + mi + me:])

    def _merit_threshold(self, x, s, lda, dz):
        n, mi = self.nvar, self.nineq
        if not (self.neq or mi):
            return None, None
        bcg = np.asarray(self.df(x), dtype=np.float64).reshape(n)
        if mi:
            bcg = np.concatenate([bcg, -self.mu_host_dev / (s + self.eps)])
        with np.errstate(divide='ignore', invalid='ignore'):
            return np.dot(bcg, dz[:n + mi]) / (1 - self.rho) / np.sum(np.abs(self._con(x, s))), None

    def _complementarity(self, x, s, lda):
        return float(np.dot(s, lda[self.neq:])), np.min(s * lda[self.neq:])

    # ------------------------------------------------------------------ driver
    def solve(self, x0=None, s0=None, lda0=None, force_recompile=False):
        if x0 is not None:
            self.x0 = x0
        if s0 is not None:
            self.s0 = s0
        if lda0 is not None:
            self.lda0 = lda0
        assert self.x0 is not None and np.size(self.x0) > 0
        self.x0 = np.asarray(self.x0, dtype=np.float64)
        assert self.x0.ndim == 1
        self.nvar = self.x0.size
        self.validate()
        if not self.compiled or force_recompile:
            self.compile()
        if hasattr(self.backend, "new_solve"):
            self.backend.new_solve()
        n, me, mi = self.nvar, self.neq, self.nineq

        # initial point (pyipm.py:1597-1625)
        x = self.x0
        if mi:
            s = (np.maximum(self._ci(x), self.Ktol)
                 if self.s0 is None else np.asarray(self.s0, dtype=np.float64))
            self._set_barrier(self.mu)
        else:
            s = np.zeros(0)
            self._set_barrier(self.Ktol)
        self.nu_host = self.nu
        if me or mi:
            if self.lda0 is None:
                lda = pinv_apply(self._jac_x(x), np.asarray(self.df(x), dtype=np.float64).reshape(n))
                if mi:
                    li = lda[me:]
                    li[li < 0.0] = self.Ktol
            else:
                lda = np.asarray(self.lda0, dtype=np.float64).copy()
        else:
            lda = np.zeros(0)
        Ftol_converged, outer, inner = self._barrier_loop(x, s, lda)
        if self.verbosity >= 0:
            self._report(self.kkt, Ftol_converged, outer, inner, self.iter_count)
        return self.x, self.s, self.lda, self.fval, self.kkt

    def _report(self, kkt, Ftol_converged, outer, inner, iter_count):
        mi = self.nineq
        words = []
        if self.signal == -2:
            words.append('Terminated due to bad direction in backtracking line search')
        elif self._small(kkt, self.Ktol):
            words.append('Converged to Ktol tolerance')
        elif self.Ftol is not None and Ftol_converged:
            words.append('Converged to Ftol tolerance')
        else:
            words.append('Maximum iterations reached')
            outer, inner = self.niter, 0
        if mi:
            if outer > 1:
                words += ['after {} outer'.format(outer - 1), 'iterations' if outer > 2 else 'iteration', 'and']
            else:
                words.append('after')
            words += ['{} inner'.format(inner), 'iterations' if inner > 1 else 'iteration',
                      '({} total).'.format(iter_count)]
        else:
            words += ['after {}'.format(iter_count), 'iterations.' if iter_count > 1 else 'iteration.']
        print(' '.join(words))
        if self.verbosity > 1:
            msg = ['FINAL: f(x) = {}'.format(self.f(self.x))]
            if self.verbosity > 2:
                msg += ['|dL/dx| = {}'.format(np.linalg.norm(kkt[0])), '|dL/ds| = {}'.format(np.linalg.norm(kkt[1])),
                        '|ce| = {}'.format(np.linalg.norm(kkt[2])), '|ci-s| = {}'.format(np.linalg.norm(kkt[3]))]
            print(', '.join(msg))
