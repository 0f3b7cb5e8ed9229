"""The interior-point loop of the reference (``/root/reference/pyipm.py:1567-1863``), stated once.

``BarrierLoop`` is the control flow that ``pyipm_amd.ipm.IPM`` (NumPy iterate, user callables) and
``pyipm_amd.qp.QPDeviceIPM`` (device-resident iterate, library reductions) both run: the outer / inner iteration, the
``Ktol`` / ``max(Ktol, mu)`` exits and ``signal`` codes (``:1656, 1665, 1680, 1761, 1781, 1796``), the ``Ftol`` test, the
transcript (``README.md:101-122``), the L-BFGS bookkeeping around the direction (``:1633-1637, 1702-1713``), the merit
parameter (``:1727-1735``) and the barrier update (``:1804-1814``).  A solver class brings its own initial point and final
report and supplies the primitives listed at ``BarrierLoop``; everything here is host arithmetic on scalars.

``lbfgs_pair_update`` is the accept / skip / reset decision and the ``SS / L / D`` update of ``:1282-1371`` over the small
host arrays, from inner products the caller computed where its (S, Y) live.
"""
from __future__ import annotations

import numpy as np


def lbfgs_pair_update(zeta, SS, L, D, fail, drop, inner, cross, curv, den, con, fail_max, eps):
    """One (dx, dg) pair offered to the storage.  ``curv = dg.dx``; ``den = dx.dx`` (constrained: zeta scales the Hessian,
    SS = S'S, L = strictly-lower S'Y) or ``dg.dg`` (unconstrained: zeta scales the inverse, "SS" = Y'Y, "L" = upper S'Y);
    ``inner`` / ``cross`` are the new last row of SS / of S'Y against the storage WITH the new pair appended, ``drop`` says
    that the oldest pair left to make room (the storage reaches lbfgs+1 pairs, ``:1300``).  A pair of non-positive curvature
    is skipped and counted; more than ``fail_max`` skips in a row ask for a reset of a non-empty storage.
    Returns (accepted, reset, zeta, SS, L, D, fail)."""
    zeta_new = curv / (den + eps)
    root = np.sqrt(eps)
    accepted = bool(curv > root and zeta_new > root)
    if accepted:
        if drop:
            SS, L, D = SS[1:, 1:], L[1:, 1:], D[1:, 1:]
        SS, L, D = (np.pad(Mx, ((0, 1), (0, 1))) for Mx in (SS, L, D))
        SS[:, -1] = SS[-1, :] = inner
        if con:
            L[-1, :] = cross
            L[-1, -1] = 0.0
        else:
            L[:, -1] = cross
        D[-1, -1] = curv
        zeta, fail = zeta_new, 0
    else:
        fail += 1
    return accepted, fail > fail_max and SS.shape[0] > 0, zeta, SS, L, D, fail


def _copy(v):
    return v.clone() if hasattr(v, "clone") else v.copy()


class BarrierLoop(object):
    """Mixin: ``_barrier_loop(x, s, lda)`` from the class's initial point to the final iterate.

    The class supplies (``nvar / neq / nineq``, the reference's parameters and ``lbfgs`` are attributes):

    * ``f(x)``; ``KKT(x, s, lda)`` -> the four first-order blocks, ``_kkt_norms(kkt)`` -> their four norms;
    * ``newton_direction(x, s, lda)``, or with ``lbfgs``: ``_neg_grad``, ``lbfgs_init``, ``lbfgs_update`` and
      ``_lbfgs_direction(x, s, lda, g, zeta, S, Y, SS, L, D)`` -- directions with the multiplier rows flipped;
    * ``_step_lengths(s, lda, dz)`` -> (alpha_s, alpha_l), asked right after the direction;
    * ``_merit_threshold(x, s, lda, dz)`` -> (the bound nu must reach or None, whatever ``search(..., info=)`` reuses);
    * ``search(x, s, lda, dz, alpha_s, alpha_l, info=)`` -> the next point, ``signal = -2`` on a dead direction;
    * ``_complementarity(x, s, lda)`` -> (s'lda_i, min s lda_i);
    * optionally ``_set_barrier(mu)`` (more than one name for the value) and the timer hooks ``_direction_begins()``,
      ``_direction_done()`` (after the step lengths) and ``_iteration_done()`` (after the KKT report)."""

    def _set_barrier(self, mu):
        self.mu_host = mu

    def _direction_begins(self):
        pass

    _direction_done = _iteration_done = _direction_begins

    def _small(self, kkt, tol):
        return all(k <= tol for k in self._kkt_norms(kkt))

    def _barrier_loop(self, x, s, lda):
        """Leaves ``x, s, lda, kkt, fval, iter_count, signal`` on self; returns (Ftol_converged, outer, inner) for the report."""
        me, mi = self.neq, self.nineq
        self.delta = 0.0
        kkt = self.KKT(x, s, lda)
        if self.lbfgs:                                           # pyipm.py:1633-1637
            store = self.lbfgs_init()
            x_old, g = _copy(x), self._neg_grad(x, s, lda)
        if self.verbosity > 0:
            print('Searching for a feasible local minimizer using L-BFGS to approximate the Hessian.' if self.lbfgs
                  else 'Searching for a feasible local minimizer using the exact Hessian.')
        iter_count = 0
        f_past = float(self.f(x)) if self.Ftol is not None else None
        Ftol_converged = False
        self.signal = 0
        outer = inner = 0

        for outer in range(self.niter):
            if self._small(kkt, self.Ktol):
                self.signal = 1
                break
            if self.verbosity > 0 and mi:
                print('OUTER ITERATION {}'.format(outer + 1))
            for inner in range(self.miter):
                if self._small(kkt, max(self.Ktol, self.mu_host)):
                    if not me and not mi:
                        self.signal = 1
                    break
                if self.verbosity > 0:
                    msg = ['* INNER ITERATION {}'.format(inner + 1) if mi else 'ITERATION {}'.format(iter_count + 1)]
                    if self.verbosity > 1:
                        msg.append('f(x) = {}'.format(self.f(x)))
                    if self.verbosity > 2:
                        msg += ['{} = {}'.format(*p) for p in zip(('|dL/dx|', '|dL/ds|', '|ce|', '|ci-s|'),
                                                                  self._kkt_norms(kkt))]
                    print(', '.join(msg))

                self._direction_begins()
                if self.lbfgs:                                    # pyipm.py:1702-1713, 1723-1725
                    if inner > 0 or outer > 0:
                        g_old, g_new = self._neg_grad(x_old, s, lda), self._neg_grad(x, s, lda)
                        store = self.lbfgs_update(x_old, x, g_old, g_new, *store)
                        x_old, g = _copy(x), g_new
                    dz = self._lbfgs_direction(x, s, lda, g, *store[:6])
                else:
                    dz = self.newton_direction(x, s, lda)        # <-- the accelerated hot path
                a_s, a_l = self._step_lengths(s, lda, dz) if mi else (1.0, 1.0)
                self._direction_done()
                nu_thres, info = self._merit_threshold(x, s, lda, dz)      # merit parameter (pyipm.py:1727-1735)
                if nu_thres is not None and self.nu_host < nu_thres:
                    self.nu_host = float(nu_thres)
                x, s, lda = self.search(x, s, lda, dz, float(a_s), float(a_l), info=info)
                iter_count += 1
                kkt = self.KKT(x, s, lda)
                self._iteration_done()

                if self.Ftol is not None and not mi and self.signal != -2:
                    f_new = float(self.f(x))
                    if abs(f_past - f_new) <= abs(self.Ftol):
                        self.signal = 2
                        Ftol_converged = True
                        break
                    f_past = f_new
                if self.signal == -2:
                    break
                if inner >= self.miter - 1 and self.verbosity > 0 and mi:
                    print('MAXIMUM INNER ITERATIONS EXCEEDED')

            if self.Ftol is not None and mi and self.signal != -2:
                f_new = float(self.f(x))
                if abs(f_past - f_new) <= abs(self.Ftol):
                    self.signal = 2
                    Ftol_converged = True
                else:
                    f_past = f_new
            if Ftol_converged or self.signal == -2:
                break
            if outer >= self.niter - 1:
                self.signal = -1
                if self.verbosity > 0:
                    print('MAXIMUM OUTER ITERATIONS EXCEEDED' if mi else 'MAXIMUM ITERATIONS EXCEEDED')
                break
            if mi:                                                # barrier update (pyipm.py:1804-1814)
                comp, mn = self._complementarity(x, s, lda)
                xi = mi * mn / (comp + self.eps)
                mu_new = 0.1 * min(0.05 * (1.0 - xi) / (xi + self.eps), 2.0) ** 3 * comp / mi
                self._set_barrier(max(float(mu_new), 0.0))

        self.x, self.s, self.lda, self.kkt = x, s, lda, kkt
        self.fval = self.f(x)
        self.iter_count = iter_count
        return Ftol_converged, outer, inner

    # ------------------------------------------------------------------ the parts of search() both classes word alike
    def _second_order_correction(self, x0, s0, dx, ds, dz_p, alpha_smax, bound):
        """Is the step alpha_smax dz + dz_p (dz_p: the class's feasibility restoration, pyipm.py:1466-1477, 1518-1529)
        within ``bound``, the Armijo line at alpha_smax?  (corrected, alpha_corr) -- :1478-1500, 1530-1533."""
        n, mi = self.nvar, self.nineq
        corrected, alpha_corr = False, 1.0
        if mi:
            xs = x0 + alpha_smax * dx + dz_p[:n]
            ss = s0 + alpha_smax * ds + dz_p[n:]
            if self.phi(xs, ss) <= bound:
                alpha_corr = self.step(s0, alpha_smax * ds + dz_p[n:])
                if (self.phi(x0 + alpha_corr * (alpha_smax * dx + dz_p[:n]),
                             s0 + alpha_corr * (alpha_smax * ds + dz_p[n:])) <= bound):
                    corrected = True
        else:
            if self.phi(x0 + alpha_smax * dx + dz_p[:n], s0) <= bound:
                alpha_corr, corrected = 1.0, True
        if corrected and self.verbosity > 2:
            print('Second-order feasibility correction accepted')
        return corrected, alpha_corr

    def _step_to(self, x0, s0, lda0, dz, alpha_smax, alpha_lmax, alpha_corr=1.0, dz_p=None):
        """The point the search settled on (pyipm.py:1550-1565); ``dz_p`` is set when the correction was accepted."""
        n, me, mi = self.nvar, self.neq, self.nineq
        dx, ds, dl = dz[:n], dz[n:n + mi], dz[n + mi:]
        if dz_p is not None:
            x = x0 + alpha_corr * (alpha_smax * dx + dz_p[:n])
            s = s0 + alpha_corr * (alpha_smax * ds + dz_p[n:]) if mi else _copy(s0)
        else:
            x = x0 + alpha_smax * dx
            s = s0 + alpha_smax * ds if mi else _copy(s0)
        lda = lda0 + alpha_lmax * dl if (me or mi) else _copy(lda0)
        return x, s, lda
