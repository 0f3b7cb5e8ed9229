"""The regularisation rule: the counterpart of the reference's ``reghess`` + solve (pyipm.py:1373-1406, 1717-1725), stated once.

When a factor is trusted, when a condition estimate is asked for, when a direction is refined, when and by how much the x
block is shifted, and what is returned when the shift budget runs out.  Plain floats and dicts only (no device, no library):
``HipNewtonBackend.direction`` (ipm.py) and ``BatchedNewton.direction_all`` (batched.py) own the launches and the counters
and ask this module for every decision; tests/test_shift_rule.py drives both through scripted factorisations on the CPU.

A statistics record is what ``factor`` returns (``n_neg, n_zero, n_2x2, d_min, d_max, growth, nonfinite``).  Where the scalar
and the batched driver decided differently before they shared this module, both behaviours are kept behind a named argument
(``nan_singular``, ``retry_overrun_as_miss``, ``stall_on_inf``): neither can be shown unreachable from the code."""
import math
import sys

EPS = sys.float_info.epsilon
SUSPECT_SPREAD = 1e-10            # pivot spread d_min / d_max at or below which the condition estimate is consulted
BERR_TOL = 1e-11                  # backward error a refined direction must meet to count as converged
BERR_FALLBACK = math.sqrt(EPS)    # ... and the bar of the LAST resort: when no shift within the budget yields a converged
                                  # direction, the best one seen is returned if it meets this (the reference returns its LU
                                  # direction whatever its accuracy, pyipm.py:1720-1721) and counted in n_inexact; only beyond
                                  # it the drivers give up
GROWTH_BAR = 64.0                 # entries of L above this: the tile-local pivot search no longer vouches for the direction
STATIC_RATIO = 100.0              # min|w| within this factor of the static pivot's magnitude: the unperturbed matrix is singular

AGAIN, SETTLE, LOST_INERTIA, LOST_SOLVE = "again", "settle", "lost: inertia", "lost: solve"


def wrong(st, need):
    """Not the inertia of a KKT matrix (``need`` = me + mi negative pivots), or a NaN / Inf met on the way: shift and retry."""
    return st["n_neg"] != need or bool(st["nonfinite"])


def suspect(st, bar=SUSPECT_SPREAD):
    """The pivots cannot rule out an eigenvalue ratio at the eps level: static pivots, or a pivot spread at or below ``bar``
    (no pivots at all, d_max <= 0, reads as spread 1).  The spread is never NaN: the kernels form d_min and d_max with fmin /
    fmax from finite seeds, which drop a NaN pivot (that one raises ``nonfinite``, which every caller looks at first)."""
    return st["n_zero"] > 0 or (st["d_max"] > 0 and st["d_min"] / st["d_max"] <= bar)


def at_risk(st):
    """Block pivots whose accuracy the tile-local pivot search does not guarantee: static pivots, 2x2 pivots (indefinite
    tiles) or large entries of L.  Such a direction is checked against the blocks and refined."""
    return st["n_zero"] > 0 or st["n_2x2"] > 0 or st["growth"] > GROWTH_BAR


def singular(est, st, eps, nan_singular):
    """The reference's ``rcond <= eps`` test (pyipm.py:1379-1381) on an estimate ``(w_min, w_max, rcond, static_pivot)``.  With
    static pivots the factor is that of a perturbed matrix, whose smallest eigenvalue sits at the perturbation level exactly
    when the unperturbed matrix is singular.  ``nan_singular``: how a NaN estimate reads (batched: singular; scalar: not)."""
    w_min, _, rcond, static = est
    at_most = (lambda a, b: not a > b) if nan_singular else (lambda a, b: a <= b)
    return (st["n_zero"] > 0 and at_most(w_min, STATIC_RATIO * static)) or at_most(rcond, eps)


def first_shift(delta, delta0):
    """The first shift of the x block (pyipm.py:1390-1397): delta0, or half of what the last call persisted."""
    return delta0 if delta == 0.0 else max(delta / 2.0, delta0)


def delta_c(is_singular, me, reg_coef, eta, mu, beta):
    """The shift of the equality-multiplier block (pyipm.py:1383-1388): only for a singular matrix with equalities."""
    return reg_coef * eta * mu ** beta if (is_singular and me) else 0.0


class ShiftLoop(object):
    """One problem's way through the ``delta *= 10`` loop (pyipm.py:1399-1403): the budget, the stall count and the best
    unconverged direction so far, ``best = (backward error, direction, delta, statistics)``.  The direction is the caller's
    own copy, opaque here.

    A factorisation whose inertia was wrong produced no direction: it is charged to the budget and takes no part in the
    stall count (two inertia retries used to count as "larger shifts stopped helping")."""

    def __init__(self, max_tries, berr_fallback=BERR_FALLBACK, retry_overrun_as_miss=False, stall_on_inf=False):
        self.max_tries, self.berr_fallback = max_tries, berr_fallback
        self.retry_overrun_as_miss = retry_overrun_as_miss    # scalar: once a shifted solve has happened, a budget that runs
                                                              # out on an inertia retry ends like one that runs out on a miss
        self.stall_on_inf = stall_on_inf                      # scalar: two infinite backward errors in a row count as a stall
        self.tries = self.stalled = self.solves = 0
        self.prev_be = self.best = None

    def in_hand(self):
        return self.best is not None and self.best[0] <= self.berr_fallback

    def remember(self, be, take, delta, st):
        """Keep ``take()`` -- a copy of the direction with backward error ``be``, made only if it is kept -- when it is the
        LEAST shifted one that meets ``berr_fallback`` (the reference does not shift such a system at all) or, below that
        bar, the most accurate one."""
        if be >= 0.0 and math.isfinite(be) and (self.best is None or (self.best[0] > self.berr_fallback and be < self.best[0])):
            self.best = (be, take(), float(delta), st)

    def _spend(self, lost):
        self.tries += 1
        if self.tries <= self.max_tries:
            return AGAIN
        return SETTLE if (lost == LOST_SOLVE and self.in_hand()) else lost

    def inertia_retry(self):
        """A shifted factorisation whose inertia was still wrong: AGAIN (with delta *= 10), or the budget is spent."""
        return self._spend(LOST_SOLVE if (self.retry_overrun_as_miss and self.solves) else LOST_INERTIA)

    def miss(self, be, take, delta, st):
        """A shifted solve missed ``berr_tol`` with backward error ``be`` (< 0: none measured).  AGAIN with a larger shift;
        SETTLE on ``best`` when the budget is spent, or as soon as larger shifts have stopped helping: two SOLVES in a row
        whose backward error did not fall tenfold with the tenfold shift, and a direction at ``berr_fallback`` in hand.
        (Exactly dependent equality constraints: no shift of the x block cures the multiplier block; waiting for delta ~ 1
        to dominate the system cost nine factorisations per iterate and returned a gradient-like step -- round 4.)"""
        self.solves += 1
        self.remember(be, take, delta, st)
        known = self.prev_be is not None and (self.stall_on_inf or math.isfinite(self.prev_be))
        self.stalled = self.stalled + 1 if (known and be >= 0.0 and be >= 0.1 * self.prev_be) else 0
        if be >= 0.0:
            self.prev_be = be
        if self.stalled >= 2 and self.in_hand():
            return SETTLE
        return self._spend(LOST_SOLVE)
