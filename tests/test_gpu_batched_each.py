"""The batched handle with per-problem mu / delta / delta_c, an active mask, the per-problem shift loop (reghess,
pyipm.py:1373-1406) and the batched fraction-to-the-boundary rule (pyipm.py:1408-1436)."""
import numpy as np
import pytest

from oracle import newton_oracle as orc
from pyipm_amd.problems import make_qp

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float64).eps)
KEYS = ("d2L", "Je", "Ji", "df", "ce", "ci", "s", "lam")


def _args(qps, n, me, mi):
    on = {"d2L": True, "Je": me, "Ji": mi, "df": True, "ce": me, "ci": mi, "s": mi, "lam": me + mi}
    return [np.stack([q[k] for q in qps]) if on[k] else None for k in KEYS]


def _records(stats):
    return [dict(x) for x in stats]


def _shifted_oracle(q, n, me, mi, mu, delta, delta_c):
    """The reference's step on Hc shifted by hand: + delta on the x block, - delta_c on the lambda_e block."""
    g = -orc.kkt_residual(q["df"], q["Je"], q["Ji"], q["ce"], q["ci"], q["s"], q["lam"], mu, n, me, mi)
    Hc = orc.kkt_matrix(q["d2L"], q["Je"], q["Ji"], q["s"], q["lam"], n, me, mi)
    Hc[:n, :n] += delta * np.eye(n)
    Hc[n + mi:n + mi + me, n + mi:n + mi + me] -= delta_c * np.eye(me)
    return orc.flip_multipliers(orc.sym_solve(Hc, g.reshape(-1, 1)).reshape(-1), n, mi)


# ---- 1. constant arrays are the scalar step -----------------------------------------------------------------------------------
@pytest.mark.parametrize("shifts", [(0.0, 0.0), (1e-3, 1e-9)])
@pytest.mark.parametrize("condensed", [False, True])
@pytest.mark.parametrize("n,me,mi", [(65, 63, 1), (130, 40, 100)])
def test_constant_arrays_are_the_scalar_step(n, me, mi, condensed, shifts):
    import torch
    from pyipm_amd.batched import BatchedNewton
    B, (delta, delta_c) = 5, shifts
    qps = [make_qp(n, me, mi, seed=700 + 13 * b + n) for b in range(B)]
    bn = BatchedNewton(n, me, mi, condensed=condensed)
    dz0, st0 = bn.step_all(*_args(qps, n, me, mi), mu=0.2, delta=delta, delta_c=delta_c)
    st0 = _records(st0)
    assert bn.n_condensed_fallback == 0
    dz1, st1 = bn.step_each(np.full(B, 0.2), np.full(B, delta), np.full(B, delta_c))
    assert dz1.data_ptr() != dz0.data_ptr()
    assert torch.equal(dz1, dz0)
    assert _records(st1) == st0
    dz2, st2 = bn.step_each(0.2, delta, delta_c, active=np.ones(B, dtype=np.int32))       # (scalars broadcast; an all-ones mask)
    assert torch.equal(dz2, dz0) and _records(st2) == st0
    bn.close()


# ---- 2. per-problem values reach the right problem ----------------------------------------------------------------------------
def test_per_problem_values_reach_the_right_problem():
    from pyipm_amd.batched import BatchedNewton
    n, me, mi, B = 48, 8, 24, 6
    qps = [make_qp(n, me, mi, seed=100 + b) for b in range(B)]
    mu = np.array([0.2, 0.05, 1e-3, 0.7, 3e-2, 1e-5])
    delta = np.array([0.0, 1e-6, 1e-2, 3e-4, 0.5, 1e-8])
    delta_c = np.array([0.0, 1e-9, 1e-4, 0.0, 2e-6, 1e-12])
    bn = BatchedNewton(n, me, mi)
    bn.stage(*_args(qps, n, me, mi), mu=0.2)
    dz, st = bn.step_each(mu, delta, delta_c)
    st = _records(st)
    be = bn.backward_errors(dz).cpu().numpy()
    dz = dz.cpu().numpy()
    print("backward errors", be)
    assert be.max() <= 1e-12                       # (k_b_berr applies each problem's OWN shifts)
    one = BatchedNewton(n, me, mi)
    for b, q in enumerate(qps):
        d1, s1 = one.step_all(*_args([q], n, me, mi), mu=mu[b], delta=delta[b], delta_c=delta_c[b])
        assert np.array_equal(d1.cpu().numpy()[0], dz[b]), b
        assert _records(s1)[0] == st[b]
        ref = _shifted_oracle(q, n, me, mi, mu[b], delta[b], delta_c[b])
        err = np.linalg.norm(dz[b] - ref) / np.linalg.norm(ref)
        print("problem", b, "rel. err vs oracle", err)
        assert err <= 1e-10
        assert st[b]["n_neg"] == me + mi and st[b]["n_zero"] == 0
    bn.close(); one.close()


# ---- 3. the mask leaves the others alone --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,me,mi,condensed", [(48, 8, 24, False), (48, 8, 24, True), (5, 2, 0, False), (3, 0, 9, False), (3, 0, 9, True),
                                               (1020, 0, 2, False), (1020, 0, 2, True)])
def test_mask_leaves_the_others_alone(n, me, mi, condensed):
    import torch
    from pyipm_amd.batched import BatchedNewton
    B = 6
    qps = [make_qp(n, me, mi, seed=100 + b) for b in range(B)]
    bn = BatchedNewton(n, me, mi, condensed=condensed)
    out, st0 = bn.step_all(*_args(qps, n, me, mi), mu=0.2)
    st0 = _records(st0)
    assert bn.n_condensed_fallback == 0
    before = out.clone()
    mu = np.array([0.2, 0.1, 0.2, 0.2, 0.01, 0.2])
    delta = np.array([7.0, 1e-3, 7.0, 7.0, 1e-2, 7.0])           # (the 7s belong to problems that sit out: nothing may read them)
    delta_c = np.array([7.0, 1e-8, 7.0, 7.0, 0.0, 7.0])
    active = np.array([0, 1, 0, 0, 1, 0], dtype=np.int32)
    ret, st1 = bn.step_each(mu, delta, delta_c, active, out=out)
    st1 = _records(st1)
    assert ret.data_ptr() == out.data_ptr()
    idle, busy = [0, 2, 3, 5], [1, 4]
    assert torch.equal(out[idle], before[idle])
    assert [st1[b] for b in idle] == [st0[b] for b in idle]
    assert not torch.equal(out[busy], before[busy])
    # nobody takes part: a no-op
    after = out.clone()
    _, st2 = bn.step_each(mu, delta, delta_c, np.zeros(B, dtype=np.int32), out=out)
    assert torch.equal(out, after) and _records(st2) == st1
    # the handle kept the shifts each problem last stepped with: 0 for the idle ones, its own for the busy ones
    if mi or me:
        assert float(bn.backward_errors(out).max()) <= 1e-10
    # a fresh all-active step with the busy problems' parameters (the idle ones: their step_all values)
    fresh, st3 = bn.step_each(mu, np.where(active, delta, 0.0), np.where(active, delta_c, 0.0))
    st3 = _records(st3)
    assert torch.equal(fresh[busy], after[busy])
    assert [st3[b] for b in busy] == [st1[b] for b in busy]
    assert torch.equal(fresh[idle], before[idle])
    # a new tensor under a mask: the rows that are not written are NaN, the others the same bits
    part, _ = bn.step_each(mu, delta, delta_c, active)
    assert torch.equal(part[busy], after[busy]) and bool(torch.isnan(part[idle]).all())
    bn.close()
    # a batch of one
    one = BatchedNewton(n, me, mi, condensed=condensed)
    o1, s1 = one.step_all(*_args(qps[1:2], n, me, mi), mu=0.2)
    keep = o1.clone()
    one.step_each(0.1, 1e-3, 1e-8, np.zeros(1, dtype=np.int32), out=o1)
    assert torch.equal(o1, keep)
    o2, s2 = one.step_each(0.1, 1e-3, 1e-8, np.ones(1, dtype=np.int32), out=o1)
    assert torch.equal(o2[0], after[1]) and _records(s2)[0] == st1[1]
    one.close()


# ---- 4. the shift loop, per problem, against the oracle -----------------------------------------------------------------------
_N4, _ME4, _MI4, _B4 = 48, 8, 24, 8
_shift_cache = {}


def _shift_batch():
    """Convex and non-convex members; computed once."""
    if "qps" not in _shift_cache:
        n = _N4
        qps = [make_qp(n, _ME4, _MI4, seed=300 + b) for b in range(_B4)]
        for b, q in enumerate(qps):
            if b % 4 in (1, 3):
                V = np.linalg.qr(np.random.default_rng(b).standard_normal((n, 3)))[0]
                a = 3e-4 if b % 4 == 1 else 40.0
                q["d2L"] = q["d2L"] - (np.linalg.eigvalsh(q["d2L"]).max() + a) * V @ V.T
        _shift_cache["qps"] = qps
    return _shift_cache["qps"]


def _oracle_shift(delta_in):
    """Per problem the oracle's reghess + solve for the incoming delta, and the margin of every matrix it decided on."""
    key = tuple(delta_in)
    if key not in _shift_cache:
        n, me, mi = _N4, _ME4, _MI4
        res = []
        for b, q in enumerate(_shift_batch()):
            stats = {}
            ref, d, Hc, _ = orc.newton_step(q["d2L"], q["Je"], q["Ji"], q["df"], q["ce"], q["ci"], q["s"], q["lam"], q["mu"],
                                            n, me, mi, delta=delta_in[b], regularise=True, stats=stats)
            # every matrix whose inertia the loop looked at: no shift, then the sequence of shifts up to the accepted one
            tried = [0.0]
            if stats["n_eigh"] > 1:
                reg = float(np.sqrt(EPS))
                x = reg if delta_in[b] == 0.0 else max(delta_in[b] / 2, reg)
                for _ in range(stats["n_eigh"] - 1):
                    tried.append(x)
                    x *= 10.0
                assert tried[-1] == d
            assert not stats["delta_c_used"]
            margin = 1.0
            for x in tried:
                H = orc.kkt_matrix(q["d2L"], q["Je"], q["Ji"], q["s"], q["lam"], n, me, mi)
                H[:n, :n] += x * np.eye(n)
                w = np.abs(np.linalg.eigvalsh(H))
                margin = min(margin, w.min() / w.max())
            res.append({"dz": ref, "delta": d, "cond": np.linalg.cond(Hc), "shifts": stats["n_eigh"] - 1, "margin": margin})
        _shift_cache[key] = res
    return _shift_cache[key]


@pytest.mark.parametrize("case", ["fresh", "incoming", "condensed"])
def test_shift_loop_per_problem_vs_oracle(case):
    import torch
    from pyipm_amd.batched import BatchedNewton
    n, me, mi, B = _N4, _ME4, _MI4, _B4
    qps = _shift_batch()
    delta_in = np.array([0.0, 8.0, 0.0, 0.5] * 2) if case == "incoming" else np.zeros(B)
    want = _oracle_shift(delta_in)
    # No decision below is a marginal one: at every shift the oracle tried, the eigenvalue nearest zero is at least this
    # fraction of the largest.  1e-5 for the runs that start from delta = 0; the incoming deltas lead through other shifts
    # (0.25, 2.5, 25: min|w| / max|w| = 6e-6 there), for which 1e-6 is asked -- block pivots can miscount an eigenvalue's sign
    # only within their rounding, N * eps * growth ~ 1e-13 of the largest entry: seven decades below either bar.
    bar = 1e-6 if case == "incoming" else 1e-5
    for b, w in enumerate(want):
        print("oracle: problem", b, "delta", w["delta"], "shifts", w["shifts"], "margin", w["margin"])
        assert w["margin"] >= bar, (b, w["margin"])
    if case != "incoming":
        assert [w["shifts"] for w in want] == [0, 10, 0, 11] * 2
        assert all(w["delta"] == 0.0 for w in want[0::2])
    bn = BatchedNewton(n, me, mi, condensed=(case == "condensed"))
    dz, delta, stats = bn.direction_all(*_args(qps, n, me, mi), mu=0.2, delta=delta_in)
    dzh = dz.cpu().numpy()
    for b, w in enumerate(want):
        assert delta[b] == w["delta"], (b, delta[b], w["delta"])
        tol = max(1e-10, 20 * w["cond"] * EPS)
        err = np.linalg.norm(dzh[b] - w["dz"]) / np.linalg.norm(w["dz"])
        print("problem", b, "delta", delta[b], "rel. err", err, "tol", tol)
        assert err <= tol, (b, err, tol)
        assert stats[b]["n_neg"] == me + mi
    assert bn.n_factor == 1 + max(w["shifts"] for w in want)
    assert bn.n_inertia_retries == sum(max(w["shifts"] - 1, 0) for w in want)
    info = bn.shift_info()
    assert info["passes"].tolist() == [w["shifts"] for w in want]
    if case != "condensed":
        plain = BatchedNewton(n, me, mi)
        ref, st = plain.step_all(*_args(qps, n, me, mi), mu=0.2)
        st = _records(st)
        for b in range(0, B, 2):
            assert torch.equal(dz[b], ref[b]) and dict(stats[b]) == st[b]
        plain.close()
    else:
        assert bn.n_condensed_fallback == 1
    bn.close()


def test_shift_loop_gives_up_naming_the_problems():
    from pyipm_amd.batched import BatchedNewton
    n, me, mi = _N4, _ME4, _MI4
    bn = BatchedNewton(n, me, mi)
    with pytest.raises(RuntimeError, match=r"problems \[3, 7\]"):
        bn.direction_all(*_args(_shift_batch(), n, me, mi), mu=0.2, max_shift_tries=9)      # (problems 1, 5 need 10 shifts, 3, 7 eleven)
    bn.close()


# ---- 5. a singular member: the decision only ----------------------------------------------------------------------------------
def test_singular_member_decision():
    import torch
    from pyipm_amd.batched import BatchedNewton
    n, me, mi, B, bad = 48, 8, 24, 5, 2
    qps = [make_qp(n, me, mi, seed=100 + b) for b in range(B)]
    qps[bad]["Je"] = qps[bad]["Je"].copy()
    qps[bad]["Je"][:, 1] = qps[bad]["Je"][:, 0]                 # two identical constraint gradients: Hc is singular
    mu = np.array([0.2, 0.1, 0.05, 0.3, 0.02])
    bn = BatchedNewton(n, me, mi)
    dz, delta, stats = bn.direction_all(*_args(qps, n, me, mi), mu=mu)
    info = bn.shift_info()
    reg = float(np.sqrt(EPS))
    print("singular member: delta", delta[bad], "delta_c", info["delta_c"][bad], "passes", info["passes"][bad], "stats", stats[bad])
    assert info["suspect"].tolist() == [b == bad for b in range(B)] and info["failed"].tolist() == info["suspect"].tolist()
    assert info["delta_c"][bad] == reg * 1e-4 * mu[bad] ** 0.4 and not info["delta_c"][[0, 1, 3, 4]].any()
    ladder, x = [], reg
    for _ in range(61):
        ladder.append(x); x *= 10.0
    assert delta[bad] in ladder and delta[bad] == ladder[info["passes"][bad] - 1]
    assert stats[bad]["n_neg"] == me + mi
    assert not delta[[0, 1, 3, 4]].any()
    rest = [b for b in range(B) if b != bad]
    other = BatchedNewton(n, me, mi)
    dz4, delta4, st4 = other.direction_all(*_args([qps[b] for b in rest], n, me, mi), mu=mu[rest])
    assert other.n_factor == 1 and not delta4.any()
    assert torch.equal(dz[rest], dz4)
    assert [dict(stats[b]) for b in rest] == [dict(x) for x in st4]
    bn.close(); other.close()


# ---- 6. step lengths ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [5, 3])
@pytest.mark.parametrize("n,me,mi", [(3, 0, 9), (65, 63, 1), (130, 40, 100), (200, 0, 400), (5, 2, 0)])
def test_step_lengths_all(n, me, mi, B):
    import torch
    from pyipm_amd.batched import BatchedNewton
    from pyipm_amd.newton import NewtonCore
    tau = 0.995
    qps = [make_qp(n, me, mi, seed=700 + 13 * b + n) for b in range(B)]
    bn = BatchedNewton(n, me, mi)
    dz, _ = bn.step_all(*_args(qps, n, me, mi), mu=0.2)
    al = bn.step_lengths_all(tau)
    assert tuple(al.shape) == (B, 2)
    assert torch.equal(bn.step_lengths_all(tau, dz=dz), al)
    al = al.cpu().numpy()
    if mi == 0:
        assert (al == 1.0).all()
        bn.close()
        return
    # a second set of directions: problem 0 without a negative entry, the others rescaled so that some lengths fall below 1
    dz2 = dz.clone()
    dz2[1:, n:n + mi] *= 8.0
    dz2[1:, n + mi + me:] *= 8.0
    dz2[0, n:n + mi] = dz2[0, n:n + mi].abs()
    dz2[0, n + mi + me:] = dz2[0, n + mi + me:].abs()
    al2 = bn.step_lengths_all(tau, dz=dz2).cpu().numpy()
    assert al2[0].tolist() == [1.0, 1.0]
    if mi >= 100:
        assert (al2[1:] < 1.0).any()
    core = NewtonCore(n, me, mi)

    def closed_form(v, dv):
        neg = dv < 0.0
        return min(1.0, float(np.min(-tau * v[neg] / dv[neg]))) if neg.any() else 1.0

    for d, a in ((dz, al), (dz2, al2)):
        dh = d.cpu().numpy()
        for b, q in enumerate(qps):
            want = (closed_form(q["s"], dh[b, n:n + mi]), closed_form(q["lam"][me:], dh[b, n + mi + me:]))
            assert (a[b, 0], a[b, 1]) == want, (b, a[b], want)
            core.stage_vectors(q["df"], q["ce"] if me else None, q["ci"], q["s"], q["lam"], mu=0.2)
            assert core.step_lengths(tau, dz=d[b]) == want, b
    core.close(); bn.close()
