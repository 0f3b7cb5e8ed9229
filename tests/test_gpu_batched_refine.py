"""Adaptive refinement per problem on the batched handle (``BatchedNewton.refine_all`` / ``pyipm_newton_refine_batched``), the
decisions of ``direction_all(refine=True)`` and ``BatchedQPIPM(refine=True)``.

Shapes: (24, 4, 40), N = 108, two tiles, and (48, 8, 72), N = 200, four tiles -- the smallest on which a left-looking pass, a
static pivot and a multi-tile sweep all occur.  Members come from ``make_qp``: a QP as it is; an LP (``d2L = 0``; ``df = c``
since the start is x = 0), whose x-x tile is singular although its KKT matrix is not; "zero rows" (the first 8 rows / columns of
``d2L`` zeroed: variables without curvature); a singular member (two identical constraint gradients); a wrong-inertia member as
``tests/test_gpu_batched_each.py`` builds its own.  The oracle's directions are computed once per batch and shared."""
import functools

import numpy as np
import pytest

from oracle import newton_oracle as orc
from pyipm_amd.problems import make_qp

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float64).eps)
KEYS = ("d2L", "Je", "Ji", "df", "ce", "ci", "s", "lam")
SHAPES = [(24, 4, 40), (48, 8, 72)]
PARITY = 1e-10                         # the project's parity bar against the oracle, relative to max|dz|
KINDS = ("qp", "lp", "zero", "qp", "lp", "zero")


def _args(qps, n, me, mi):
    on = {"d2L": True, "Je": me, "Ji": mi, "df": True, "ce": me, "ci": mi, "s": mi, "lam": me + mi}
    return [np.stack([q[k] for q in qps]) if on[k] else None for k in KEYS]


def _member(kind, n, me, mi, seed):
    q = make_qp(n, me, mi, seed=seed)
    if kind == "lp":
        q["d2L"] = np.zeros((n, n))
        q["df"] = q["c"].copy()
    elif kind == "zero":
        q["d2L"] = q["d2L"].copy()
        q["d2L"][:8, :] = 0.0
        q["d2L"][:, :8] = 0.0
    elif kind == "singular":
        q["Je"] = q["Je"].copy()
        q["Je"][:, 1] = q["Je"][:, 0]
    elif kind == "wrong":
        V = np.linalg.qr(np.random.default_rng(seed).standard_normal((n, 3)))[0]
        q["d2L"] = q["d2L"] - (np.linalg.eigvalsh(q["d2L"]).max() + 3e-4) * V @ V.T
    else:
        assert kind == "qp"
    return q


@functools.lru_cache(maxsize=None)
def _batch(n, me, mi):
    """The six members of tests 1-5 at one shape and the oracle's step of each: (qps, [(dz, delta)])."""
    qps = [_member(k, n, me, mi, 500 + 7 * b + n) for b, k in enumerate(KINDS)]
    want = []
    for q in qps:
        dz, delta, _, _ = orc.newton_step(q["d2L"], q["Je"], q["Ji"], q["df"], q["ce"], q["ci"], q["s"], q["lam"], q["mu"], n, me, mi)
        want.append((dz, delta))
    return qps, want


def _err(dz, ref):
    return float(np.abs(dz - ref).max() / np.abs(ref).max())


def _stepped(n, me, mi, qps, condensed=False):
    """A handle with one unshifted step of the batch behind it: (handle, dz, statistics as dicts)."""
    from pyipm_amd.batched import BatchedNewton
    bn = BatchedNewton(n, me, mi, condensed=condensed, guard=False)
    bn.stage(*_args(qps, n, me, mi), mu=0.2)
    dz, st = bn.step_each(0.2, 0.0, 0.0)
    return bn, dz, [dict(x) for x in st]


def _check_against_oracle(n, me, mi, kinds, want, dz0, dz, info, st, skip=()):
    from pyipm_amd.batched import BatchedNewton
    import torch
    dzh, ih = dz.cpu().numpy(), info.cpu().numpy()
    for b, kind in enumerate(kinds):
        if b in skip:
            continue
        steps, be0, be, conv = ih[b]
        print((n, me, mi), "member", b, kind, "n_zero", st[b]["n_zero"], "steps", steps, "berr0 %.2e berr %.2e" % (be0, be), "conv", conv,
              "err vs oracle %.2e" % _err(dzh[b], want[b][0]), "oracle delta", want[b][1])
        assert conv == 1.0, (b, ih[b])
        assert be <= 1e-14 and be <= be0
        assert _err(dzh[b], want[b][0]) <= PARITY, b
        assert want[b][1] == 0.0
        if kind == "qp":
            assert steps == 0.0 and be0 == be
            assert torch.equal(dz[b], dz0[b])                              # bit for bit what the step wrote
        else:
            assert st[b]["n_zero"] > 0
            assert be0 > BatchedNewton.berr_tol, "the unrefined direction already meets berr_tol: this member shows nothing"
            assert steps >= 1.0


# ---- 1. the entry against the oracle ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,me,mi", SHAPES)
def test_refine_all_against_the_oracle(n, me, mi):
    qps, want = _batch(n, me, mi)
    bn, dz0, st = _stepped(n, me, mi, qps)
    dz = dz0.clone()
    info = bn.refine_all(dz)
    assert tuple(info.shape) == (len(qps), 4) and bn.REFINE_KEYS[2] == "backward_error"
    _check_against_oracle(n, me, mi, KINDS, want, dz0, dz, info, st)
    # what the record says is what the blocks say
    be = bn.backward_errors(dz).cpu().numpy()
    assert np.all(be <= 1e-14)
    bn.close()


# ---- 2. independence ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,me,mi", SHAPES)
def test_a_problems_bits_do_not_depend_on_the_others(n, me, mi):
    import torch
    from pyipm_amd.batched import BatchedNewton
    qps, _ = _batch(n, me, mi)
    B = len(qps)
    bn, dz0, _ = _stepped(n, me, mi, qps)
    dz = dz0.clone()
    info = bn.refine_all(dz)
    # permuted
    perm = [4, 2, 5, 0, 3, 1]
    bp, dp0, _ = _stepped(n, me, mi, [qps[p] for p in perm])
    dp = dp0.clone()
    ip = bp.refine_all(dp)
    for k, p in enumerate(perm):
        assert torch.equal(dp[k], dz[p]) and torch.equal(ip[k], info[p]), (k, p)
    bp.close()
    # alone
    one = BatchedNewton(n, me, mi)
    for b in (1, 2, 3):
        one.stage(*_args([qps[b]], n, me, mi), mu=0.2)
        d1, _ = one.step_each(0.2, 0.0, 0.0)
        i1 = one.refine_all(d1)
        assert torch.equal(d1[0], dz[b]) and torch.equal(i1[0], info[b]), b
    one.close()
    # every other member masked out: the rows of the others keep their NaN prefill, in dz and in info
    for b in (1, 2, 3):
        act = np.zeros(B, dtype=np.int32)
        act[b] = 1
        dm = torch.full_like(dz0, float("nan"))
        dm[b] = dz0[b]
        im = bn.refine_all(dm, active=act)
        assert torch.equal(dm[b], dz[b]) and torch.equal(im[b], info[b]), b
        rest = [k for k in range(B) if k != b]
        assert bool(torch.isnan(dm[rest]).all()) and bool(torch.isnan(im[rest]).all())
    # a padded row (ld > N) and a flip-less (raw) direction
    wide = torch.full((B, bn.N + 5), float("nan"), dtype=torch.float64, device=dz0.device)
    wide[:, :bn.N] = dz0
    iw = bn.refine_all(wide)
    assert torch.equal(wide[:, :bn.N], dz) and torch.equal(iw, info) and bool(torch.isnan(wide[:, bn.N:]).all())
    raw = dz0.clone()
    raw[:, n + mi:] *= -1.0
    ir = bn.refine_all(raw, flip=False)
    raw[:, n + mi:] *= -1.0
    assert torch.equal(raw, dz) and torch.equal(ir, info)
    bn.close()


# ---- 3. nothing else moves ----------------------------------------------------------------------------------------------------
def test_refine_all_leaves_the_handle_alone():
    import torch
    n, me, mi = SHAPES[1]
    qps, _ = _batch(n, me, mi)
    bn, dz0, st0 = _stepped(n, me, mi, qps)
    R = torch.from_numpy(np.random.default_rng(5).standard_normal((len(qps), 3, bn.N))).to(dz0.device)
    x0 = bn.solve_all(R)
    be0 = bn.backward_errors(dz0).clone()
    a = dz0.clone()
    ia = bn.refine_all(a)
    assert torch.equal(bn.solve_all(R), x0)
    assert [dict(x) for x in bn._fetch_stats(bn._step_id)] == st0
    assert torch.equal(bn.backward_errors(dz0), be0)                       # (the kept residual and the shifts)
    b = dz0.clone()
    ib = bn.refine_all(b)
    assert torch.equal(a, b) and torch.equal(ia, ib)
    # a fixed budget below what the members need: stopped, not converged, the steps taken are counted
    c = dz0.clone()
    ic = bn.refine_all(c, max_steps=0).cpu().numpy()
    assert torch.equal(c, dz0)
    for k, kind in enumerate(KINDS):
        assert ic[k, 0] == 0.0 and ic[k, 3] == (1.0 if kind == "qp" else 0.0) and ic[k, 1] == ic[k, 2] == ia.cpu().numpy()[k, 1]
    bn.close()


# ---- 4. a NaN member ----------------------------------------------------------------------------------------------------------
def test_a_nan_member_is_left_alone():
    import torch
    n, me, mi = SHAPES[0]
    qps, want = _batch(n, me, mi)
    qps = [dict(q) for q in qps]
    qps[3]["df"] = qps[3]["df"].copy()
    qps[3]["df"][0] = np.nan
    bn, dz0, st = _stepped(n, me, mi, qps)
    dz = dz0.clone()
    info = bn.refine_all(dz)
    ih = info.cpu().numpy()
    print("NaN member:", ih[3])
    assert ih[3, 0] == 0.0 and ih[3, 3] == 0.0 and np.isnan(ih[3, 1]) and np.isnan(ih[3, 2])
    assert torch.equal(dz[3].isnan(), dz0[3].isnan()) and torch.equal(dz[3].nan_to_num(), dz0[3].nan_to_num())
    _check_against_oracle(n, me, mi, KINDS, want, dz0, dz, info, st, skip=(3,))
    bn.close()


# ---- 5. condensed factors -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,me,mi", SHAPES)
def test_a_condensed_member_is_corrected_through_its_condensed_factor(n, me, mi):
    import torch
    allq, allw = _batch(n, me, mi)
    idx = [b for b, k in enumerate(KINDS) if k == "qp"]
    qps, want = [allq[b] for b in idx], [allw[b] for b in idx]
    bn, dz0, st = _stepped(n, me, mi, qps, condensed=True)
    assert all(x["n_zero"] == 0 and x["n_neg"] == me + mi for x in st)
    be0 = bn.backward_errors(dz0).cpu().numpy()
    dz = dz0.clone()
    info = bn.refine_all(dz).cpu().numpy()                                 # the adaptive rule on condensed factors
    be = bn.backward_errors(dz).cpu().numpy()
    dzh = dz.cpu().numpy()
    for k in range(len(qps)):
        print((n, me, mi), "condensed member", k, info[k], "berr before %.2e after %.2e" % (be0[k], be[k]), "err %.2e" % _err(dzh[k], want[k][0]))
        assert be[k] <= be0[k] and _err(dzh[k], want[k][0]) <= PARITY
    # one member FORCED through its condensed factor: two steps whatever it measures (the target cannot be met ...)
    dz = dz0.clone()
    act = np.array([0, 1], dtype=np.int32)
    info = bn.refine_all(dz, active=act, max_steps=2, target=0).cpu().numpy()
    assert torch.equal(dz[0], dz0[0]) and np.isnan(info[0]).all()
    dz2 = dz0.clone()
    tiny = bn.refine_all(dz2, active=act, max_steps=2, target=1e-300).cpu().numpy()   # (... with this one)
    be2 = bn.backward_errors(dz2).cpu().numpy()
    print("forced:", tiny[1], "berr before %.2e after %.2e" % (be0[1], be2[1]))
    assert tiny[1, 3] == 0.0 and tiny[1, 2] <= tiny[1, 1] and be2[1] <= be0[1]
    assert _err(dz2.cpu().numpy()[1], want[1][0]) <= PARITY
    bn.close()


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals():
    import ctypes
    import torch
    from pyipm_amd.batched import BatchedNewton
    from pyipm_amd.newton import MEM_DEVICE, NewtonCore, NewtonError
    n, me, mi = SHAPES[0]
    qps, _ = _batch(n, me, mi)
    bn = BatchedNewton(n, me, mi)
    bn.stage(*_args(qps, n, me, mi), mu=0.2)
    dz = torch.zeros((len(qps), bn.N), dtype=torch.float64, device=bn.device)
    with pytest.raises(NewtonError):
        bn.refine_all(dz)                                                  # before any step
    out, _ = bn.step_each(0.2, 0.0, 0.0)
    bn.refine_all(out.clone())
    with pytest.raises(NewtonError):
        bn.refine_all(out[:, :bn.N - 1].contiguous())                      # ld < N
    bn.stage(*_args(qps, n, me, mi), mu=0.2)
    with pytest.raises(NewtonError):
        bn.refine_all(out.clone())                                         # after restaging
    bn.close()
    core = NewtonCore(n, me, mi)
    info = torch.zeros(4, dtype=torch.float64, device=dz.device)
    rc = core.lib.pyipm_newton_refine_batched(core.h, ctypes.c_void_p(dz.data_ptr()), core.N, core.N, None, 1, 0.0, -1,
                                              ctypes.c_void_p(info.data_ptr()), MEM_DEVICE)
    assert rc == -1
    with pytest.raises(NewtonError):
        core._ck(rc)                                                       # a single-system handle
    core.close()


# ---- 7. direction_all(refine=True) on a mixed batch ---------------------------------------------------------------------------
MIXED = ("qp", "lp", "wrong", "qp", "singular", "lp")


@functools.lru_cache(maxsize=None)
def _mixed():
    n, me, mi = SHAPES[0]
    qps = [_member(k, n, me, mi, 900 + 11 * b) for b, k in enumerate(MIXED)]
    want = []
    for q, kind in zip(qps, MIXED):
        if kind == "singular":
            want.append(None)                                              # (the oracle's LU fails there)
            continue
        stats = {}
        dz, delta, Hc, _ = orc.newton_step(q["d2L"], q["Je"], q["Ji"], q["df"], q["ce"], q["ci"], q["s"], q["lam"], q["mu"], n, me, mi,
                                           stats=stats)
        margin = 1.0
        if kind == "wrong":                    # every matrix whose inertia the loop looks at: no decision is a marginal one
            x, tried = float(np.sqrt(EPS)), [0.0]
            for _ in range(stats["n_eigh"] - 1):
                tried.append(x)
                x *= 10.0
            assert tried[-1] == delta and not stats["delta_c_used"]
            for x in tried:
                H = orc.kkt_matrix(q["d2L"], q["Je"], q["Ji"], q["s"], q["lam"], n, me, mi)
                H[:n, :n] += x * np.eye(n)
                w = np.abs(np.linalg.eigvalsh(H))
                margin = min(margin, w.min() / w.max())
        want.append({"dz": dz, "delta": delta, "margin": margin, "cond": np.linalg.cond(Hc)})
    return qps, want


def test_direction_all_refined_on_a_mixed_batch():
    import torch
    from pyipm_amd.batched import BatchedNewton
    n, me, mi = SHAPES[0]
    qps, want = _mixed()
    B, need = len(qps), me + mi
    reg = float(np.sqrt(EPS))
    wrong, sing = MIXED.index("wrong"), MIXED.index("singular")
    lps = [b for b, k in enumerate(MIXED) if k == "lp"]
    qs = [b for b, k in enumerate(MIXED) if k == "qp"]
    assert want[wrong]["margin"] >= 1e-5 and want[wrong]["delta"] > 0.0, want[wrong]
    old = BatchedNewton(n, me, mi)
    dz_old, delta_old, st_old = old.direction_all(*_args(qps, n, me, mi), mu=0.2)
    new = BatchedNewton(n, me, mi)
    dz, delta, stats = new.direction_all(*_args(qps, n, me, mi), mu=0.2, refine=True)
    info = new.shift_info()
    dzh = dz.cpu().numpy()
    print("refine=False delta", delta_old, "\nrefine=True  delta", delta, "\npasses", info["passes"], "singular", info["singular"],
          "refined", info["refined"], "berr", info["backward_error"])
    print("counters: rcond", new.n_rcond, "refined", new.n_refined, "static", new.n_static, "unconverged", new.n_unconverged,
          "inexact", new.n_inexact)
    for b in lps:                              # not shifted at all, as the reference; today's path shifts them
        assert delta[b] == 0.0 and info["passes"][b] == 0 and info["refined"][b] and not info["failed"][b] and not info["singular"][b]
        assert info["backward_error"][b] <= BatchedNewton.berr_tol
        assert want[b]["delta"] == 0.0 and _err(dzh[b], want[b]["dz"]) <= PARITY, b
        assert delta_old[b] == reg
        assert stats[b]["n_zero"] > 0
    assert new.n_static >= len(lps) and new.n_rcond >= len(lps) and new.n_refined >= len(lps)
    for b in qs:                               # nobody looked at them: the bits of pass 1
        assert torch.equal(dz[b], dz_old[b]) and dict(stats[b]) == dict(st_old[b]) and delta[b] == 0.0
        assert not info["refined"][b] and info["passes"][b] == 0
    assert delta[wrong] == want[wrong]["delta"], (delta[wrong], want[wrong]["delta"])
    assert stats[wrong]["n_neg"] == need and info["failed"][wrong] and info["delta_c"][wrong] == 0.0
    tol = max(PARITY, 20 * want[wrong]["cond"] * EPS)
    assert _err(dzh[wrong], want[wrong]["dz"]) <= tol, (_err(dzh[wrong], want[wrong]["dz"]), tol)
    # the singular member: the decision only
    assert info["failed"][sing] and info["singular"][sing] and info["passes"][sing] >= 1 and stats[sing]["n_neg"] == need
    assert info["delta_c"][sing] == reg * 1e-4 * 0.2 ** 0.4 and delta[sing] > 0.0
    old.close(); new.close()
    # an all-QP batch: no extra launch, the bits of refine=False
    qq = [qps[b] for b in qs] + [make_qp(n, me, mi, seed=77)]
    a, b_ = BatchedNewton(n, me, mi), BatchedNewton(n, me, mi)
    d0, l0, s0 = a.direction_all(*_args(qq, n, me, mi), mu=0.2)
    d1, l1, s1 = b_.direction_all(*_args(qq, n, me, mi), mu=0.2, refine=True)
    assert b_.n_rcond == 0 and b_.n_refined == 0 and b_.n_factor == 1
    assert torch.equal(d0, d1) and np.array_equal(l0, l1) and [dict(x) for x in s0] == [dict(x) for x in s1]
    a.close(); b_.close()


# ---- 8. BatchedQPIPM(refine=True) on LPs --------------------------------------------------------------------------------------
# Bounded by construction: c = G'w with w ~ U(0.5, 2) makes w dual feasible, and x = 0 is strictly feasible in make_qp.  Seeds
# 40 .. 45 were checked on the CPU with the host IPM over the oracle backend of tests/backends.py (miter = 20, niter = 10,
# Ktol = 1e-4): every one ends with signal 1.
LP_SEEDS = (40, 41, 42, 43, 44, 45)
SOLO_SPREAD_X, SOLO_SPREAD_F = 2.78e-4, 7.62e-6      # the solo solver's own spread at this Ktol (tests/test_gpu_batched_qp.py)
BOUND_X, BOUND_F = 100 * SOLO_SPREAD_X, 100 * SOLO_SPREAD_F


def lp_problem(seed, n=24, me=4, mi=40):
    q = make_qp(n, me, mi, seed=seed)
    w = np.random.default_rng(10000 + seed).uniform(0.5, 2.0, mi)
    q["Q"] = np.zeros((n, n))
    q["c"] = q["G"].T @ w
    return q


def test_batched_qp_ipm_solves_lps_without_a_shift():
    from pyipm_amd.batched_qp import BatchedQPIPM
    from pyipm_amd.qp import QPDeviceIPM
    probs = [lp_problem(s) for s in LP_SEEDS]
    kw = {k: np.stack([p[k] for p in probs]) for k in ("Q", "c", "A", "b", "G", "h")}
    ipm = BatchedQPIPM(x0=np.stack([p["x"] for p in probs]), s0=np.stack([p["s"] for p in probs]),
                       lda0=np.stack([p["lam"] for p in probs]), Ktol=1e-4, refine=True, **kw)
    seen = []
    real = ipm.core.direction_all

    def spy(*a, **k):
        out = real(*a, **k)
        seen.append(out[1].copy())
        return out

    ipm.core.direction_all = spy
    res = ipm.solve()
    print("signal", res["signal"], "iterations", res["iter_count"], "static", ipm.core.n_static, "rcond", ipm.core.n_rcond,
          "refined", ipm.core.n_refined, "unconverged", ipm.core.n_unconverged, "inexact", ipm.core.n_inexact)
    assert np.all(res["signal"] == 1), res["signal"]
    assert ipm.core.n_static > 0
    assert seen and all(not d.any() for d in seen)                         # no member's delta ever leaves 0
    xs = res["x"].cpu().numpy()
    worst_x = worst_f = 0.0
    for b, q in enumerate(probs):
        solo = QPDeviceIPM(q["Q"], q["c"], A=q["A"], b=q["b"], G=q["G"], h=q["h"], x0=q["x"], s0=q["s"], lda0=q["lam"], Ktol=1e-4,
                           verbosity=-1, warm=False)
        x, _, _, fval, _ = solo.solve()
        dx, dfv = float(np.linalg.norm(x.cpu().numpy() - xs[b])), abs(float(fval) - res["fval"][b])
        print(b, "solo iterations", solo.iter_count, "signal", solo.signal, "|dx|", dx, "|dfval|", dfv)
        assert solo.signal == 1
        worst_x, worst_f = max(worst_x, dx), max(worst_f, dfv)
        solo.close()
    print("worst |dx|", worst_x, "bound", BOUND_X, "worst |dfval|", worst_f, "bound", BOUND_F)
    assert worst_x <= BOUND_X and worst_f <= BOUND_F
