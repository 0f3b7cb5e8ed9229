"""The regularisation rule (pyipm_amd/reghess.py) and its drivers, on the CPU: ``HipNewtonBackend.direction`` over a scripted
core, ``BatchedNewton.direction_all`` over a scripted batch of four whose member 2 follows the same script.

A script is a list of factorisations in the order the problem meets them: ``F(statistics, be=..., est=...)`` -- the statistics
``factor`` returns, the backward error the refined solve on that factor reports, the condition estimate taken for it.  The
direction of factorisation k is the vector [k], so the test sees WHICH solve was returned.  Every expected value below was
recorded from the drivers as they stood before the rule was gathered into one module (three hand-written copies); where the
scalar and the batched copy disagreed then, both values are pinned (the scenarios named ``differs_*``)."""
import numpy as np
import pytest

from pyipm_amd import reghess

EPS = float(np.finfo(np.float64).eps)
D0 = float(np.sqrt(EPS))                 # reg_coef = delta0 (pyipm.py:353, 372)
MU, ETA, BETA = 0.2, 1e-4, 0.4
B, AT = 4, 2                             # the batch, and where the scripted problem sits in it
INF, NAN = float("inf"), float("nan")


def S(need, **kw):
    st = dict(n_neg=need, n_pos=2, n_zero=0, n_2x2=0, d_min=1.0, d_max=1.0, growth=1.0, nonfinite=0)
    st.update(kw)
    return st


def F(be=None, est=None, **kw):
    """One factorisation: statistics overrides (``wrong=True``: one negative pivot too many), backward error, estimate."""
    return dict(kw=kw, be=be, est=est)


def _event(f, need):
    kw = dict(f["kw"])
    if kw.pop("wrong", False):
        kw["n_neg"] = need + 1
    est = f["est"]
    return dict(st=S(need, **kw), be=f["be"],
                est=None if est is None else dict(zip(("w_min", "w_max", "rcond", "static_pivot"), est)))


RISKY = dict(n_2x2=1)                    # a factor whose direction is checked against the blocks and refined
STATIC = dict(n_zero=2)
FAR = (1e-3, 1.0, 1e-3, 1e-8)            # an estimate far from singular
NEAR = (1e-17, 1.0, 1e-17, 1e-8)         # ... and a singular one

#   name: (me, script, options)          options: delta (persisted), max_shift_tries, berr_tol, berr_fallback
SCENARIOS = {
    "clean": (1, [F()], {}),
    "wrong_inertia_then_right": (1, [F(wrong=True), F(wrong=True), F(wrong=True), F()], {}),
    "wrong_inertia_persisted_delta": (1, [F(wrong=True), F(wrong=True), F()], dict(delta=1e-3)),
    "wrong_inertia_small_persisted_delta": (1, [F(wrong=True), F()], dict(delta=1e-8)),
    "suspect_not_singular": (1, [F(d_min=1e-12, est=FAR)], {}),
    "singular_by_estimate_me": (1, [F(d_min=1e-12, est=NEAR), F()], {}),
    "singular_by_estimate_no_me": (0, [F(d_min=1e-12, est=NEAR), F()], {}),
    "singular_and_wrong_inertia": (1, [F(d_min=1e-12, est=NEAR, wrong=True), F(wrong=True), F()], {}),
    "nonfinite": (1, [F(nonfinite=1), F()], {}),
    "static_pivots_converge": (1, [F(be=1e-13, est=FAR, **STATIC)], {}),
    "miss_unshifted_meet_at_first_shift": (1, [F(be=1e-9, **RISKY), F(be=1e-12, **RISKY)], {}),
    "stall_settles_on_least_shifted": (1, [F(be=1e-9, **RISKY), F(be=5e-10, **RISKY), F(be=4e-10, **RISKY),
                                           F(be=3.5e-10, **RISKY)], {}),
    "stall_settles_on_first_at_fallback": (1, [F(be=1e-6, **RISKY), F(be=1e-9, **RISKY), F(be=9e-10, **RISKY),
                                               F(be=1e-10, **RISKY), F(be=9e-11, **RISKY), F(be=8e-11, **RISKY)], {}),
    "inertia_retries_are_not_stalls": (1, [F(be=1e-9, **RISKY), F(be=5e-10, **RISKY), F(be=4e-10, **RISKY), F(wrong=True),
                                           F(wrong=True), F(be=1e-12, **RISKY)], {}),
    "stall_after_inertia_retry": (1, [F(be=1e-9, **RISKY), F(be=5e-10, **RISKY), F(be=4e-10, **RISKY), F(wrong=True),
                                      F(be=3.9e-10, **RISKY)], {}),
    "budget_spent_direction_in_hand": (1, [F(be=1e-9, **RISKY), F(be=1e-10, **RISKY), F(be=1e-12, **RISKY),
                                           F(be=1e-14, **RISKY), F(be=1e-16, **RISKY)], dict(max_shift_tries=3, berr_tol=0.0)),
    "budget_spent_nothing_in_hand": (1, [F(be=1e-9, **RISKY), F(be=1e-10, **RISKY), F(be=1e-12, **RISKY),
                                         F(be=1e-14, **RISKY), F(be=1e-16, **RISKY)],
                                     dict(max_shift_tries=3, berr_tol=0.0, berr_fallback=0.0)),
    "differs_budget_spent_on_inertia_retry_in_hand": (1, [F(be=1e-9, **RISKY), F(be=1e-10, **RISKY), F(wrong=True),
                                                          F(wrong=True), F(wrong=True)], dict(max_shift_tries=3)),
    "differs_budget_spent_on_inertia_retry_nothing": (1, [F(be=1e-9, **RISKY), F(be=1e-10, **RISKY), F(wrong=True),
                                                          F(wrong=True), F(wrong=True)],
                                                      dict(max_shift_tries=3, berr_fallback=0.0)),
    "inertia_never_corrected": (1, [F(wrong=True)] * 5, dict(max_shift_tries=3)),
    "inertia_never_corrected_after_a_miss": (1, [F(be=1e-9, **RISKY)] + [F(wrong=True)] * 4, dict(max_shift_tries=3)),
    "differs_nan_estimate": (1, [F(d_min=1e-12, est=(NAN, NAN, NAN, 1e-8)), F()], {}),
    "differs_static_count_on_a_shifted_solve": (1, [F(est=NEAR, **STATIC), F(be=1e-13, **STATIC)], {}),
    "differs_infinite_backward_errors": (1, [F(be=1e-9, **RISKY), F(be=INF, **RISKY), F(be=INF, **RISKY), F(be=INF, **RISKY),
                                             F(be=1e-12, **RISKY)], {}),
    # the edges of the predicates, through the drivers
    "edge_spread_at_the_bar_is_suspect": (1, [F(d_min=1e-10, est=FAR)], {}),
    "edge_spread_above_the_bar": (1, [F(d_min=1.0000000001e-10)], {}),
    "edge_growth_64_is_not_at_risk": (1, [F(growth=64.0, be=1.0)], {}),
    "edge_growth_above_64": (1, [F(growth=64.00000000000001, be=1e-13)], {}),
    "edge_w_min_at_100_static_pivots": (1, [F(est=(1e-6, 1.0, 1e-6, 1e-8), **STATIC), F()], {}),
    "edge_w_min_above_100_static_pivots": (1, [F(est=(1.0000000000000002e-6, 1.0, 1e-6, 1e-8), be=1e-13, **STATIC)], {}),
    "edge_rcond_at_eps": (1, [F(d_min=1e-12, est=(EPS, 1.0, EPS, 0.0)), F()], {}),
    "edge_rcond_above_eps": (1, [F(d_min=1e-12, est=(EPS, 1.0, EPS * (1 + EPS), 0.0))], {}),
    "edge_d_max_zero": (1, [F(d_min=0.0, d_max=0.0)], {}),
    # what direction_all(refine=False) decides differently: its bar is eps, and static pivots are shifted (LP members)
    "spread_at_eps": (1, [F(d_min=EPS, est=FAR), F()], {}),
    "static_pivots_twice": (0, [F(be=1e-13, est=FAR, **STATIC), F(be=1e-13, **STATIC)], {}),
}


class Vec(object):
    """What the scripted core returns for a direction: a NumPy vector behind the three tensor calls the driver makes."""

    def __init__(self, a):
        self.a = np.array(a, dtype=np.float64)

    def clone(self):
        return Vec(self.a)

    def cpu(self):
        return self

    def numpy(self):
        return self.a


class FakeCore(object):
    def __init__(self, events):
        self.events, self.k, self.steps = events, -1, []

    def stage_blocks(self, *a, **k):
        pass

    stage_vectors = stage_blocks

    def residual(self):
        return None

    def assemble(self, delta, delta_c):
        self.steps.append((float(delta), float(delta_c)))

    def factor(self):
        self.k += 1
        return dict(self.events[self.k]["st"])

    def solve(self, flip=True, refine=0):
        return Vec([self.k])

    def solve_info(self):
        be = self.events[self.k]["be"]
        return {"steps": 1, "backward_error0": be, "backward_error": be, "converged": False}

    def rcond(self, it_inv=0, it_pow=0):
        return dict(self.events[self.k]["est"])


SCALAR_COUNTERS = ("n_factor", "n_rcond", "n_static", "n_unconverged", "n_inertia_retries", "n_inexact")
BATCHED_COUNTERS = ("n_factor", "n_inertia_retries", "n_rcond", "n_refined", "n_static", "n_unconverged", "n_inexact")


def run_scalar(name, monkeypatch):
    import pyipm_amd.newton
    from pyipm_amd.ipm import HipNewtonBackend
    me, script, opt = SCENARIOS[name]
    core = FakeCore([_event(f, me) for f in script])
    monkeypatch.setattr(pyipm_amd.newton, "NewtonCore", lambda *a, **k: core)
    be = HipNewtonBackend(2, me, 0, max_shift_tries=opt.get("max_shift_tries", 60))
    for k in ("berr_tol", "berr_fallback"):
        if k in opt:
            setattr(be, k, opt[k])
    got = {}
    try:
        dz, delta, st = be.direction(None, None, None, None, None, None, None, None, MU, opt.get("delta", 0.0), MU, ETA, BETA,
                                     D0, D0, EPS)
        assert st == core.events[int(dz[0])]["st"]               # the statistics of the factor whose direction is returned
        got["ret"] = (delta, int(dz[0]), be._dir_override is not None)
    except RuntimeError as e:
        got["error"] = str(e)
    got.update(steps=core.steps, counters=tuple(getattr(be, c) for c in SCALAR_COUNTERS))
    return got


def _fake_batch():
    import torch
    from pyipm_amd.batched import BatchedNewton

    class FakeBatch(BatchedNewton):
        def __init__(self, me, events):
            self.torch, self.n, self.me, self.mi, self.N, self.batch = torch, 2, me, 0, 2 + me, B
            self.guard, self.device = False, torch.device("cpu")
            self.events = [[_event(F(), me)] if b != AT else events for b in range(B)]
            self.k = [-1] * B
            self.steps = [[] for _ in range(B)]

        def stage(self, *a, **k):
            return B

        def _opts_get(self, name):
            return 0.0

        def backward_errors(self, dz):
            raise AssertionError("no condensed form in this test")

        def _rows(self, active):
            return [b for b in range(B) if active is None or active[b]]

        def step_each(self, mu, delta, delta_c, active=None, out=None):
            if out is None:
                out = torch.full((B, self.N), NAN, dtype=torch.float64)
            for b in self._rows(active):
                self.k[b] += 1
                self.steps[b].append((float(delta[b]), float(delta_c[b])))
                out[b] = float(self.k[b])
            return out, [dict(self.events[b][max(self.k[b], 0)]["st"]) for b in range(B)]

        def rcond_all(self, it_inv=0, it_pow=0, active=None):
            out = torch.full((B, 4), NAN, dtype=torch.float64)
            for b in self._rows(active):
                out[b] = torch.tensor(list(self.events[b][self.k[b]]["est"].values()), dtype=torch.float64)
            return out

        def refine_all(self, dz, active=None, flip=True, target=None, max_steps=None):
            out = torch.full((B, 4), NAN, dtype=torch.float64)
            for b in self._rows(active):
                be = self.events[b][self.k[b]]["be"]
                out[b] = torch.tensor([1.0, be, be, 0.0], dtype=torch.float64)
            return out

    return FakeBatch


def run_batched(name, refine=True):
    me, script, opt = SCENARIOS[name]
    bn = _fake_batch()(me, [_event(f, me) for f in script])
    for k in ("berr_tol", "berr_fallback"):
        if k in opt:
            setattr(bn, k, opt[k])
    delta_in = np.zeros(B)
    delta_in[AT] = opt.get("delta", 0.0)
    got = {}
    try:
        out, delta, stats = bn.direction_all(None, None, None, None, None, None, None, None, MU, delta=delta_in, eta=ETA, beta=BETA,
                                             max_shift_tries=opt.get("max_shift_tries", 60), refine=refine)
        k = int(out[AT, 0])
        assert stats[AT] == bn.events[AT][k]["st"]
        got["ret"] = (float(delta[AT]), k)
        assert [float(d) for b, d in enumerate(delta) if b != AT] == [0.0] * (B - 1)
        assert all(float(out[b, 0]) == 0.0 for b in range(B) if b != AT)
        info = bn.shift_info()
        got["info"] = tuple(None if v[AT] != v[AT] else v[AT].item() for _, v in sorted(info.items()))
        assert not any(info["failed"][b] for b in range(B) if b != AT)
    except RuntimeError as e:
        got["error"] = str(e)
    assert [bn.steps[b] for b in range(B) if b != AT] == [[(0.0, 0.0)]] * (B - 1)      # the clean neighbours: pass 1 and no more
    got.update(steps=bn.steps[AT], counters=tuple(getattr(bn, c) for c in BATCHED_COUNTERS))
    return got


UNREFINED = ("clean", "wrong_inertia_then_right", "wrong_inertia_persisted_delta", "wrong_inertia_small_persisted_delta",
             "suspect_not_singular", "singular_by_estimate_me", "singular_by_estimate_no_me", "nonfinite",
             "spread_at_eps", "static_pivots_twice", "inertia_never_corrected", "edge_d_max_zero")      # direction_all(refine=False)

# What the drivers did before the rule was gathered into reghess.py -- recorded, not derived.  D[k] = delta0 * 10^k as the
# `delta *= 10` loop forms it, DC = reg_coef * eta * mu ** beta.  counters: SCALAR_COUNTERS / BATCHED_COUNTERS; ret: (delta
# returned, which factorisation's direction[, _dir_override set]); info: shift_info() of the problem, keys in sorted order.
D = [1.4901161193847656e-08, 1.4901161193847656e-07, 1.4901161193847656e-06, 1.4901161193847656e-05, 0.00014901161193847656]
DC = 7.827662838708661e-13

EXPECTED_SCALAR = {'budget_spent_direction_in_hand': {'counters': (5, 0, 0, 5, 0, 1),
                                    'ret': (0.0, 0, True),
                                    'steps': [(0.0, 0.0), (D[0], DC),
                                              (D[1], DC),
                                              (D[2], DC),
                                              (D[3], DC)]},
 'budget_spent_nothing_in_hand': {'counters': (5, 0, 0, 5, 0, 0),
                                  'error': 'refined solve did not reach backward error 0.0e+00 after 4 diagonal shifts (last: '
                                           "{'steps': 1, 'backward_error0': 1e-16, 'backward_error': 1e-16, 'converged': "
                                           'False})',
                                  'steps': [(0.0, 0.0), (D[0], DC),
                                            (D[1], DC),
                                            (D[2], DC),
                                            (D[3], DC)]},
 'clean': {'counters': (1, 0, 0, 0, 0, 0), 'ret': (0.0, 0, False), 'steps': [(0.0, 0.0)]},
 'differs_budget_spent_on_inertia_retry_in_hand': {'counters': (5, 0, 0, 2, 3, 1),
                                                   'ret': (0.0, 0, True),
                                                   'steps': [(0.0, 0.0), (D[0], DC),
                                                             (D[1], DC),
                                                             (D[2], DC),
                                                             (D[3], DC)]},
 'differs_budget_spent_on_inertia_retry_nothing': {'counters': (5, 0, 0, 2, 3, 0),
                                                   'error': 'refined solve did not reach backward error 1.0e-11 after 4 '
                                                            "diagonal shifts (last: {'steps': 1, 'backward_error0': 1e-10, "
                                                            "'backward_error': 1e-10, 'converged': False})",
                                                   'steps': [(0.0, 0.0), (D[0], DC),
                                                             (D[1], DC),
                                                             (D[2], DC),
                                                             (D[3], DC)]},
 'differs_infinite_backward_errors': {'counters': (4, 0, 0, 4, 0, 1),
                                      'ret': (0.0, 0, True),
                                      'steps': [(0.0, 0.0), (D[0], DC),
                                                (D[1], DC),
                                                (D[2], DC)]},
 'differs_nan_estimate': {'counters': (1, 1, 0, 0, 0, 0), 'ret': (0.0, 0, False), 'steps': [(0.0, 0.0)]},
 'differs_static_count_on_a_shifted_solve': {'counters': (2, 1, 0, 0, 0, 0),
                                             'ret': (D[0], 1, False),
                                             'steps': [(0.0, 0.0), (D[0], DC)]},
 'edge_d_max_zero': {'counters': (1, 0, 0, 0, 0, 0), 'ret': (0.0, 0, False), 'steps': [(0.0, 0.0)]},
 'edge_growth_64_is_not_at_risk': {'counters': (1, 0, 0, 0, 0, 0), 'ret': (0.0, 0, False), 'steps': [(0.0, 0.0)]},
 'edge_growth_above_64': {'counters': (1, 0, 0, 0, 0, 0), 'ret': (0.0, 0, False), 'steps': [(0.0, 0.0)]},
 'edge_rcond_above_eps': {'counters': (1, 1, 0, 0, 0, 0), 'ret': (0.0, 0, False), 'steps': [(0.0, 0.0)]},
 'edge_rcond_at_eps': {'counters': (2, 1, 0, 0, 0, 0),
                       'ret': (D[0], 1, False),
                       'steps': [(0.0, 0.0), (D[0], DC)]},
 'edge_spread_above_the_bar': {'counters': (1, 0, 0, 0, 0, 0), 'ret': (0.0, 0, False), 'steps': [(0.0, 0.0)]},
 'edge_spread_at_the_bar_is_suspect': {'counters': (1, 1, 0, 0, 0, 0), 'ret': (0.0, 0, False), 'steps': [(0.0, 0.0)]},
 'edge_w_min_above_100_static_pivots': {'counters': (1, 1, 1, 0, 0, 0), 'ret': (0.0, 0, False), 'steps': [(0.0, 0.0)]},
 'edge_w_min_at_100_static_pivots': {'counters': (2, 1, 0, 0, 0, 0),
                                     'ret': (D[0], 1, False),
                                     'steps': [(0.0, 0.0), (D[0], DC)]},
 'inertia_never_corrected': {'counters': (5, 0, 0, 0, 4, 0),
                             'error': 'inertia not corrected after 4 diagonal shifts',
                             'steps': [(0.0, 0.0), (D[0], 0.0), (D[1], 0.0),
                                       (D[2], 0.0), (D[3], 0.0)]},
 'inertia_never_corrected_after_a_miss': {'counters': (5, 0, 0, 1, 4, 0),
                                          'error': 'inertia not corrected after 4 diagonal shifts',
                                          'steps': [(0.0, 0.0), (D[0], DC),
                                                    (D[1], DC),
                                                    (D[2], DC),
                                                    (D[3], DC)]},
 'inertia_retries_are_not_stalls': {'counters': (6, 0, 0, 3, 2, 0),
                                    'ret': (D[4], 5, False),
                                    'steps': [(0.0, 0.0), (D[0], DC),
                                              (D[1], DC),
                                              (D[2], DC),
                                              (D[3], DC),
                                              (D[4], DC)]},
 'miss_unshifted_meet_at_first_shift': {'counters': (2, 0, 0, 1, 0, 0),
                                        'ret': (D[0], 1, False),
                                        'steps': [(0.0, 0.0), (D[0], DC)]},
 'nonfinite': {'counters': (2, 0, 0, 0, 0, 0),
               'ret': (D[0], 1, False),
               'steps': [(0.0, 0.0), (D[0], DC)]},
 'singular_and_wrong_inertia': {'counters': (3, 1, 0, 0, 1, 0),
                                'ret': (D[1], 2, False),
                                'steps': [(0.0, 0.0), (D[0], DC),
                                          (D[1], DC)]},
 'singular_by_estimate_me': {'counters': (2, 1, 0, 0, 0, 0),
                             'ret': (D[0], 1, False),
                             'steps': [(0.0, 0.0), (D[0], DC)]},
 'singular_by_estimate_no_me': {'counters': (2, 1, 0, 0, 0, 0),
                                'ret': (D[0], 1, False),
                                'steps': [(0.0, 0.0), (D[0], 0.0)]},
 'spread_at_eps': {'counters': (1, 1, 0, 0, 0, 0), 'ret': (0.0, 0, False), 'steps': [(0.0, 0.0)]},
 'stall_after_inertia_retry': {'counters': (5, 0, 0, 4, 1, 1),
                               'ret': (0.0, 0, True),
                               'steps': [(0.0, 0.0), (D[0], DC),
                                         (D[1], DC),
                                         (D[2], DC),
                                         (D[3], DC)]},
 'stall_settles_on_first_at_fallback': {'counters': (4, 0, 0, 4, 0, 1),
                                        'ret': (D[0], 1, True),
                                        'steps': [(0.0, 0.0), (D[0], DC),
                                                  (D[1], DC),
                                                  (D[2], DC)]},
 'stall_settles_on_least_shifted': {'counters': (4, 0, 0, 4, 0, 1),
                                    'ret': (0.0, 0, True),
                                    'steps': [(0.0, 0.0), (D[0], DC),
                                              (D[1], DC),
                                              (D[2], DC)]},
 'static_pivots_converge': {'counters': (1, 1, 1, 0, 0, 0), 'ret': (0.0, 0, False), 'steps': [(0.0, 0.0)]},
 'static_pivots_twice': {'counters': (1, 1, 1, 0, 0, 0), 'ret': (0.0, 0, False), 'steps': [(0.0, 0.0)]},
 'suspect_not_singular': {'counters': (1, 1, 0, 0, 0, 0), 'ret': (0.0, 0, False), 'steps': [(0.0, 0.0)]},
 'wrong_inertia_persisted_delta': {'counters': (3, 0, 0, 0, 1, 0),
                                   'ret': (0.005, 2, False),
                                   'steps': [(0.0, 0.0), (0.0005, 0.0), (0.005, 0.0)]},
 'wrong_inertia_small_persisted_delta': {'counters': (2, 0, 0, 0, 0, 0),
                                         'ret': (D[0], 1, False),
                                         'steps': [(0.0, 0.0), (D[0], 0.0)]},
 'wrong_inertia_then_right': {'counters': (4, 0, 0, 0, 2, 0),
                              'ret': (D[2], 3, False),
                              'steps': [(0.0, 0.0), (D[0], 0.0), (D[1], 0.0),
                                        (D[2], 0.0)]}}

EXPECTED_BATCHED = {'budget_spent_direction_in_hand': {'counters': (5, 0, 0, 5, 0, 5, 1),
                                    'info': (1e-09, 0.0, DC, True, 4, True, True, False),
                                    'ret': (0.0, 0),
                                    'steps': [(0.0, 0.0), (D[0], DC),
                                              (D[1], DC),
                                              (D[2], DC),
                                              (D[3], DC)]},
 'budget_spent_nothing_in_hand': {'counters': (5, 0, 0, 5, 0, 5, 0),
                                  'error': 'refined solve did not reach backward error 0.0e+00 after 4 diagonal shifts: '
                                           'problems [np.int64(2)]',
                                  'steps': [(0.0, 0.0), (D[0], DC),
                                            (D[1], DC),
                                            (D[2], DC),
                                            (D[3], DC)]},
 'clean': {'counters': (1, 0, 0, 0, 0, 0, 0),
           'info': (None, 0.0, 0.0, False, 0, False, False, False),
           'ret': (0.0, 0),
           'steps': [(0.0, 0.0)]},
 'differs_budget_spent_on_inertia_retry_in_hand': {'counters': (5, 3, 0, 2, 0, 2, 0),
                                                   'error': 'inertia not corrected after 4 diagonal shifts: problems '
                                                            '[np.int64(2)]',
                                                   'steps': [(0.0, 0.0), (D[0], DC),
                                                             (D[1], DC),
                                                             (D[2], DC),
                                                             (D[3], DC)]},
 'differs_budget_spent_on_inertia_retry_nothing': {'counters': (5, 3, 0, 2, 0, 2, 0),
                                                   'error': 'inertia not corrected after 4 diagonal shifts: problems '
                                                            '[np.int64(2)]',
                                                   'steps': [(0.0, 0.0), (D[0], DC),
                                                             (D[1], DC),
                                                             (D[2], DC),
                                                             (D[3], DC)]},
 'differs_infinite_backward_errors': {'counters': (5, 0, 0, 5, 0, 4, 0),
                                      'info': (1e-12, D[3], DC, True, 4, True, True,
                                               False),
                                      'ret': (D[3], 4),
                                      'steps': [(0.0, 0.0), (D[0], DC),
                                                (D[1], DC),
                                                (D[2], DC),
                                                (D[3], DC)]},
 'differs_nan_estimate': {'counters': (2, 0, 1, 0, 0, 0, 0),
                          'info': (None, D[0], DC, True, 1, False, True, True),
                          'ret': (D[0], 1),
                          'steps': [(0.0, 0.0), (D[0], DC)]},
 'differs_static_count_on_a_shifted_solve': {'counters': (2, 0, 1, 1, 1, 0, 0),
                                             'info': (1e-13, D[0], DC, True, 1, True, True,
                                                      True),
                                             'ret': (D[0], 1),
                                             'steps': [(0.0, 0.0), (D[0], DC)]},
 'edge_d_max_zero': {'counters': (1, 0, 0, 0, 0, 0, 0),
                     'info': (None, 0.0, 0.0, False, 0, False, False, False),
                     'ret': (0.0, 0),
                     'steps': [(0.0, 0.0)]},
 'edge_growth_64_is_not_at_risk': {'counters': (1, 0, 0, 0, 0, 0, 0),
                                   'info': (None, 0.0, 0.0, False, 0, False, False, False),
                                   'ret': (0.0, 0),
                                   'steps': [(0.0, 0.0)]},
 'edge_growth_above_64': {'counters': (1, 0, 0, 1, 0, 0, 0),
                          'info': (1e-13, 0.0, 0.0, False, 0, True, False, False),
                          'ret': (0.0, 0),
                          'steps': [(0.0, 0.0)]},
 'edge_rcond_above_eps': {'counters': (1, 0, 1, 0, 0, 0, 0),
                          'info': (None, 0.0, 0.0, False, 0, False, False, True),
                          'ret': (0.0, 0),
                          'steps': [(0.0, 0.0)]},
 'edge_rcond_at_eps': {'counters': (2, 0, 1, 0, 0, 0, 0),
                       'info': (None, D[0], DC, True, 1, False, True, True),
                       'ret': (D[0], 1),
                       'steps': [(0.0, 0.0), (D[0], DC)]},
 'edge_spread_above_the_bar': {'counters': (1, 0, 0, 0, 0, 0, 0),
                               'info': (None, 0.0, 0.0, False, 0, False, False, False),
                               'ret': (0.0, 0),
                               'steps': [(0.0, 0.0)]},
 'edge_spread_at_the_bar_is_suspect': {'counters': (1, 0, 1, 0, 0, 0, 0),
                                       'info': (None, 0.0, 0.0, False, 0, False, False, True),
                                       'ret': (0.0, 0),
                                       'steps': [(0.0, 0.0)]},
 'edge_w_min_above_100_static_pivots': {'counters': (1, 0, 1, 1, 1, 0, 0),
                                        'info': (1e-13, 0.0, 0.0, False, 0, True, False, True),
                                        'ret': (0.0, 0),
                                        'steps': [(0.0, 0.0)]},
 'edge_w_min_at_100_static_pivots': {'counters': (2, 0, 1, 0, 0, 0, 0),
                                     'info': (None, D[0], DC, True, 1, False, True, True),
                                     'ret': (D[0], 1),
                                     'steps': [(0.0, 0.0), (D[0], DC)]},
 'inertia_never_corrected': {'counters': (5, 4, 0, 0, 0, 0, 0),
                             'error': 'inertia not corrected after 4 diagonal shifts: problems [np.int64(2)]',
                             'steps': [(0.0, 0.0), (D[0], 0.0), (D[1], 0.0),
                                       (D[2], 0.0), (D[3], 0.0)]},
 'inertia_never_corrected_after_a_miss': {'counters': (5, 4, 0, 1, 0, 1, 0),
                                          'error': 'inertia not corrected after 4 diagonal shifts: problems [np.int64(2)]',
                                          'steps': [(0.0, 0.0), (D[0], DC),
                                                    (D[1], DC),
                                                    (D[2], DC),
                                                    (D[3], DC)]},
 'inertia_retries_are_not_stalls': {'counters': (6, 2, 0, 4, 0, 3, 0),
                                    'info': (1e-12, D[4], DC, True, 5, True, True, False),
                                    'ret': (D[4], 5),
                                    'steps': [(0.0, 0.0), (D[0], DC),
                                              (D[1], DC),
                                              (D[2], DC),
                                              (D[3], DC),
                                              (D[4], DC)]},
 'miss_unshifted_meet_at_first_shift': {'counters': (2, 0, 0, 2, 0, 1, 0),
                                        'info': (1e-12, D[0], DC, True, 1, True, True,
                                                 False),
                                        'ret': (D[0], 1),
                                        'steps': [(0.0, 0.0), (D[0], DC)]},
 'nonfinite': {'counters': (2, 0, 0, 0, 0, 0, 0),
               'info': (None, D[0], DC, True, 1, False, True, False),
               'ret': (D[0], 1),
               'steps': [(0.0, 0.0), (D[0], DC)]},
 'singular_and_wrong_inertia': {'counters': (3, 1, 1, 0, 0, 0, 0),
                                'info': (None, D[1], DC, True, 2, False, True, True),
                                'ret': (D[1], 2),
                                'steps': [(0.0, 0.0), (D[0], DC),
                                          (D[1], DC)]},
 'singular_by_estimate_me': {'counters': (2, 0, 1, 0, 0, 0, 0),
                             'info': (None, D[0], DC, True, 1, False, True, True),
                             'ret': (D[0], 1),
                             'steps': [(0.0, 0.0), (D[0], DC)]},
 'singular_by_estimate_no_me': {'counters': (2, 0, 1, 0, 0, 0, 0),
                                'info': (None, D[0], 0.0, True, 1, False, True, True),
                                'ret': (D[0], 1),
                                'steps': [(0.0, 0.0), (D[0], 0.0)]},
 'spread_at_eps': {'counters': (1, 0, 1, 0, 0, 0, 0),
                   'info': (None, 0.0, 0.0, False, 0, False, False, True),
                   'ret': (0.0, 0),
                   'steps': [(0.0, 0.0)]},
 'stall_after_inertia_retry': {'counters': (5, 1, 0, 4, 0, 4, 1),
                               'info': (1e-09, 0.0, DC, True, 4, True, True, False),
                               'ret': (0.0, 0),
                               'steps': [(0.0, 0.0), (D[0], DC),
                                         (D[1], DC),
                                         (D[2], DC),
                                         (D[3], DC)]},
 'stall_settles_on_first_at_fallback': {'counters': (4, 0, 0, 4, 0, 4, 1),
                                        'info': (1e-09, D[0], DC, True, 3, True, True,
                                                 False),
                                        'ret': (D[0], 1),
                                        'steps': [(0.0, 0.0), (D[0], DC),
                                                  (D[1], DC),
                                                  (D[2], DC)]},
 'stall_settles_on_least_shifted': {'counters': (4, 0, 0, 4, 0, 4, 1),
                                    'info': (1e-09, 0.0, DC, True, 3, True, True, False),
                                    'ret': (0.0, 0),
                                    'steps': [(0.0, 0.0), (D[0], DC),
                                              (D[1], DC),
                                              (D[2], DC)]},
 'static_pivots_converge': {'counters': (1, 0, 1, 1, 1, 0, 0),
                            'info': (1e-13, 0.0, 0.0, False, 0, True, False, True),
                            'ret': (0.0, 0),
                            'steps': [(0.0, 0.0)]},
 'static_pivots_twice': {'counters': (1, 0, 1, 1, 1, 0, 0),
                         'info': (1e-13, 0.0, 0.0, False, 0, True, False, True),
                         'ret': (0.0, 0),
                         'steps': [(0.0, 0.0)]},
 'suspect_not_singular': {'counters': (1, 0, 1, 0, 0, 0, 0),
                          'info': (None, 0.0, 0.0, False, 0, False, False, True),
                          'ret': (0.0, 0),
                          'steps': [(0.0, 0.0)]},
 'wrong_inertia_persisted_delta': {'counters': (3, 1, 0, 0, 0, 0, 0),
                                   'info': (None, 0.005, 0.0, True, 2, False, False, False),
                                   'ret': (0.005, 2),
                                   'steps': [(0.0, 0.0), (0.0005, 0.0), (0.005, 0.0)]},
 'wrong_inertia_small_persisted_delta': {'counters': (2, 0, 0, 0, 0, 0, 0),
                                         'info': (None, D[0], 0.0, True, 1, False, False, False),
                                         'ret': (D[0], 1),
                                         'steps': [(0.0, 0.0), (D[0], 0.0)]},
 'wrong_inertia_then_right': {'counters': (4, 2, 0, 0, 0, 0, 0),
                              'info': (None, D[2], 0.0, True, 3, False, False, False),
                              'ret': (D[2], 3),
                              'steps': [(0.0, 0.0), (D[0], 0.0), (D[1], 0.0),
                                        (D[2], 0.0)]}}

EXPECTED_UNREFINED = {'clean': {'counters': (1, 0, 0, 0, 0, 0, 0), 'info': (0.0, 0.0, False, 0, False), 'ret': (0.0, 0), 'steps': [(0.0, 0.0)]},
 'edge_d_max_zero': {'counters': (1, 0, 0, 0, 0, 0, 0),
                     'info': (0.0, 0.0, False, 0, False),
                     'ret': (0.0, 0),
                     'steps': [(0.0, 0.0)]},
 'inertia_never_corrected': {'counters': (5, 4, 0, 0, 0, 0, 0),
                             'error': 'inertia not corrected after 4 diagonal shifts: problems [2]',
                             'steps': [(0.0, 0.0), (D[0], 0.0), (D[1], 0.0),
                                       (D[2], 0.0), (D[3], 0.0)]},
 'nonfinite': {'counters': (2, 0, 0, 0, 0, 0, 0),
               'info': (D[0], DC, True, 1, True),
               'ret': (D[0], 1),
               'steps': [(0.0, 0.0), (D[0], DC)]},
 'singular_by_estimate_me': {'counters': (1, 0, 0, 0, 0, 0, 0),
                             'info': (0.0, 0.0, False, 0, False),
                             'ret': (0.0, 0),
                             'steps': [(0.0, 0.0)]},
 'singular_by_estimate_no_me': {'counters': (1, 0, 0, 0, 0, 0, 0),
                                'info': (0.0, 0.0, False, 0, False),
                                'ret': (0.0, 0),
                                'steps': [(0.0, 0.0)]},
 'spread_at_eps': {'counters': (2, 0, 0, 0, 0, 0, 0),
                   'info': (D[0], DC, True, 1, True),
                   'ret': (D[0], 1),
                   'steps': [(0.0, 0.0), (D[0], DC)]},
 'static_pivots_twice': {'counters': (2, 0, 0, 0, 0, 0, 0),
                         'info': (D[0], 0.0, True, 1, True),
                         'ret': (D[0], 1),
                         'steps': [(0.0, 0.0), (D[0], 0.0)]},
 'suspect_not_singular': {'counters': (1, 0, 0, 0, 0, 0, 0),
                          'info': (0.0, 0.0, False, 0, False),
                          'ret': (0.0, 0),
                          'steps': [(0.0, 0.0)]},
 'wrong_inertia_persisted_delta': {'counters': (3, 1, 0, 0, 0, 0, 0),
                                   'info': (0.005, 0.0, True, 2, False),
                                   'ret': (0.005, 2),
                                   'steps': [(0.0, 0.0), (0.0005, 0.0), (0.005, 0.0)]},
 'wrong_inertia_small_persisted_delta': {'counters': (2, 0, 0, 0, 0, 0, 0),
                                         'info': (D[0], 0.0, True, 1, False),
                                         'ret': (D[0], 1),
                                         'steps': [(0.0, 0.0), (D[0], 0.0)]},
 'wrong_inertia_then_right': {'counters': (4, 2, 0, 0, 0, 0, 0),
                              'info': (D[2], 0.0, True, 3, False),
                              'ret': (D[2], 3),
                              'steps': [(0.0, 0.0), (D[0], 0.0), (D[1], 0.0),
                                        (D[2], 0.0)]}}


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_scalar_driver(name, monkeypatch):
    assert run_scalar(name, monkeypatch) == EXPECTED_SCALAR[name]


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_batched_driver(name):
    assert run_batched(name) == EXPECTED_BATCHED[name]


@pytest.mark.parametrize("name", UNREFINED)
def test_batched_driver_without_refinement(name):
    assert run_batched(name, refine=False) == EXPECTED_UNREFINED[name]


# ---- the module itself: bars and predicates at their edges (the same edges go through both drivers above) ----------------
def test_bars_are_stated_once():
    from pyipm_amd.batched import BatchedNewton
    from pyipm_amd.ipm import HipNewtonBackend
    assert (reghess.SUSPECT_SPREAD, reghess.BERR_TOL, reghess.BERR_FALLBACK) == (1e-10, 1e-11, D0)
    assert (reghess.GROWTH_BAR, reghess.STATIC_RATIO, reghess.EPS) == (64.0, 100.0, EPS)
    for cls in (HipNewtonBackend, BatchedNewton):
        assert (cls.suspect_spread, cls.berr_tol, cls.berr_fallback) == (1e-10, 1e-11, D0)
    assert HipNewtonBackend._at_risk(S(0, growth=65.0)) and not HipNewtonBackend._at_risk(S(0))      # callable on the class


@pytest.mark.parametrize("kw,bar,want", [
    (dict(d_min=1e-10), 1e-10, True),                # spread exactly at the bar
    (dict(d_min=1.0000000001e-10), 1e-10, False),
    (dict(d_min=0.0, d_max=0.0), 1e-10, False),      # no pivots: spread 1
    (dict(d_min=1.0, d_max=-1.0), 1e-10, False),
    (dict(n_zero=1), 1e-10, True),
    (dict(d_min=EPS), EPS, True),
    (dict(d_min=1e-12), EPS, False),
])
def test_suspect(kw, bar, want):
    assert reghess.suspect(S(0, **kw), bar) is want


@pytest.mark.parametrize("kw,want", [
    (dict(), False), (dict(growth=64.0), False), (dict(growth=64.00000000000001), True), (dict(n_2x2=1), True),
    (dict(n_zero=1), True), (dict(growth=NAN), False),
])
def test_at_risk(kw, want):
    assert reghess.at_risk(S(0, **kw)) is want


def test_wrong():
    assert not reghess.wrong(S(3), 3)
    assert reghess.wrong(S(2), 3) and reghess.wrong(S(4), 3) and reghess.wrong(S(3, nonfinite=1), 3)


@pytest.mark.parametrize("est,n_zero,want,want_nan_singular", [
    ((1.0, 1.0, EPS, 0.0), 0, True, True),                      # rcond == eps
    ((1.0, 1.0, EPS * (1 + EPS), 0.0), 0, False, False),
    ((1e-6, 1.0, 1e-3, 1e-8), 2, True, True),                   # w_min == 100 static_pivot, static pivots
    ((1e-6, 1.0, 1e-3, 1e-8), 0, False, False),                 # ... the same estimate without static pivots
    ((1.0000000000000002e-6, 1.0, 1e-3, 1e-8), 2, False, False),
    ((1.0, 1.0, NAN, 0.0), 0, False, True),                     # a NaN estimate: the one place the two drivers differ
    ((NAN, 1.0, 1e-3, 1e-8), 2, False, True),
    ((NAN, 1.0, 1e-3, 1e-8), 0, False, False),
])
def test_singular(est, n_zero, want, want_nan_singular):
    assert reghess.singular(est, S(0, n_zero=n_zero), EPS, nan_singular=False) is want
    assert reghess.singular(est, S(0, n_zero=n_zero), EPS, nan_singular=True) is want_nan_singular


def test_first_shift_and_delta_c():
    assert reghess.first_shift(0.0, D0) == D0
    assert reghess.first_shift(1e-3, D0) == 5e-4 and reghess.first_shift(1e-8, D0) == D0 and reghess.first_shift(2 * D0, D0) == D0
    assert reghess.delta_c(True, 1, D0, ETA, MU, BETA) == D0 * ETA * MU ** BETA == DC
    assert reghess.delta_c(True, 0, D0, ETA, MU, BETA) == 0.0 and reghess.delta_c(False, 1, D0, ETA, MU, BETA) == 0.0


def test_the_rule_imports_nothing_but_the_standard_library():
    import ast
    tree = ast.parse(open(reghess.__file__).read())
    names = {a.name for n in ast.walk(tree) if isinstance(n, ast.Import) for a in n.names}
    assert names <= {"math", "sys"} and not any(isinstance(n, ast.ImportFrom) for n in ast.walk(tree))
