"""The batched handle's per-problem products and merit pieces (pyipm_newton_block_products_batched / _t_batched,
merit_info_batched, merit_ray_batched; kernels_batched.hpp) against host references, against the single-system handle, and for
independence of a problem's bits from the batch around it.

The bound of every sum is a-priori: for a sum of m terms t_i,  |got - ref| <= (m + 8) u sum|t_i|,  u = 2^-53: summation in any
order contributes at most (m - 1) u of that, the 8 covers the few roundings that form a term.  ``ref`` is math.fsum over the
float64 terms formed as the kernel forms them (abs_change, log1p, d / (s + eps)); two valid summations (batched handle against
single-system handle) differ by at most twice the bound.  Where a term is itself built on a device sum the error of that sum,
by the same formula, is carried into the bound:
 * entry 5 (|dL/dx|^2 = sum g_j^2): g_j = -(df_j - sum_a J[j][a] lda_a) from the step's residual kernel carries
   e_j = (me + mi + 8) u (|df_j| + sum_a |J[j][a] lda_a|), so the square carries e_j (2 |g_j| + e_j);
 * the ray: dce_i = Je' dx and dci_i = Ji' dx carry E_i = (n + 8) u sum_j |J[j][i] dx_j|, and |c + a d| - |c| is 1-Lipschitz in
   a d: a E_i per element (times nu).  abs_change returns sign(c) a d (one rounding of the change) unless c + a d leaves the sign
   of c; only then it subtracts two magnitudes of size <= |c| + |a d|: elements with |a d| >= |c| / 2 -- every such element and
   every one a perturbation of d by E_i could turn into one -- get 4 u (|c| + |a d|) <= 12 u |a d| more.  For the a = 1e-12
   candidates no element of these problems is of that kind: the whole bound is relative to the CHANGE of phi.
Norms are compared as squares, with 4 u more for the square root and the squaring back."""
import functools
import math
from fractions import Fraction

import numpy as np
import pytest

from pyipm_amd.problems import make_qp

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
EPS = float(np.finfo(np.float64).eps)
SHAPES = [(40, 0, 0), (48, 12, 0), (40, 0, 12), (96, 24, 40), (200, 30, 90), (300, 100, 300)]
BATCHES = [1, 5, 67]
FRACS = (1.0, 0.5, 0.1, 1e-3, 1e-6)          # candidates alpha_s * f, and 1e-12 itself
KEYS = ("d2L", "Je", "Ji", "df", "ce", "ci", "s", "lam")
SQ = (5, 6, 7, 8, 11, 12)                    # entries returned as norms


@functools.lru_cache(maxsize=None)
def qp(n, me, mi, seed):
    q = make_qp(n, me, mi, seed=seed)
    rng = np.random.default_rng(seed + 100000)
    q["v"], q["le"], q["li"] = rng.standard_normal(n), rng.standard_normal(me), rng.standard_normal(mi)
    q["nu"], q["mu_b"] = 10.0 + seed % 7, 0.2 / (1 + seed % 3)
    return q


def seeds_of(shape, B):
    return tuple(1000 * shape[0] + 7 * b + 3 for b in range(B))


def _args(qps, me, mi):
    on = {"d2L": True, "Je": me, "Ji": mi, "df": True, "ce": me, "ci": mi, "s": mi, "lam": me + mi}
    return [np.stack([q[k] for q in qps]) if on[k] else None for k in KEYS]


def _np(t):
    return None if t is None else t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def run(shape, seeds, dz_from=None):
    """Everything the batched handle says about the problems ``seeds`` of ``shape`` (NumPy).  ``dz_from``: (seeds, dz) of an
    earlier run whose directions are handed in (row by seed) instead of this run's own."""
    import torch
    from pyipm_amd.batched import BatchedNewton
    n, me, mi = shape
    qps = [qp(n, me, mi, sd) for sd in seeds]
    B = len(seeds)
    bn = BatchedNewton(n, me, mi)
    dz, _ = bn.step_all(*_args(qps, me, mi), mu=0.2)
    if dz_from is not None:
        src = dict(zip(dz_from[0], dz_from[1]))
        dz = torch.from_numpy(np.stack([src[sd] for sd in seeds])).cuda()
    al = _np(bn.step_lengths_all(0.995, dz))
    alphas = np.array([[al[b, 0] * f for f in FRACS] + [1e-12] for b in range(B)])
    nu, mu = np.array([q["nu"] for q in qps]), np.array([q["mu_b"] for q in qps])
    out = {"dz": _np(dz), "alphas": alphas, "nu": nu, "mu": mu, "seeds": seeds}
    out["info"] = _np(bn.merit_info_all(dz))
    out["info_nodz"] = _np(bn.merit_info_all(use_last=False))
    out["ray"] = _np(bn.merit_ray_all(alphas, nu, mu, dz))
    out["ray_again"] = _np(bn.merit_ray_all(alphas, nu, mu, dz))
    out["info_again"] = _np(bn.merit_info_all(dz))
    quad = np.array([3.7 + 0.1 * (sd % 11) for sd in seeds])
    out["quad"], out["ray_quad"] = quad, _np(bn.merit_ray_all(alphas, nu, mu, dz, quad=quad))
    v = np.stack([q["v"] for q in qps])
    out["prod"] = tuple(_np(t) for t in bn.products_all(v))
    out["prod_again"] = tuple(_np(t) for t in bn.products_all(v))
    out["prod_part"] = tuple(_np(t) for t in bn.products_all(v, want=(False, True, True)))
    le = np.stack([q["le"] for q in qps]) if me else None
    li = np.stack([q["li"] for q in qps]) if mi else None
    out["prod_t"] = _np(bn.products_t_all(le, li))
    out["prod_t_e"] = _np(bn.products_t_all(le, None))
    bn.close()
    return out


# ---- host references -------------------------------------------------------------------------------------------------------------
def fsum_b(terms, extra=0.0):
    """(fsum, (m + 8) u sum|t| + extra)"""
    t = np.asarray(terms, dtype=np.float64).ravel()
    return math.fsum(t), (t.size + 8) * U * float(np.abs(t).sum()) + extra


def sym(Q):
    return np.triu(Q) + np.triu(Q, 1).T


def ref_info(q, dz, mu):
    """(values, bounds) of the 13 entries -- sums of squares where the entry is a norm."""
    n, me, mi = q["n"], q["me"], q["mi"]
    s, lam, ce, ci = q["s"], q["lam"], q["ce"], q["ci"]
    dx, ds = dz[:n], dz[n:n + mi]
    r = ci - s
    val, bnd = np.zeros(13), np.zeros(13)
    J = np.concatenate([q["Je"], q["Ji"]], axis=1) if (me + mi) else np.zeros((n, 0))
    T = J * lam[None, :]
    acc = np.array([math.fsum(row) for row in T]) if (me + mi) else np.zeros(n)
    gx = -(q["df"] - acc)
    ej = (me + mi + 8) * U * (np.abs(q["df"]) + np.abs(T).sum(axis=1))
    v6 = (lam[me:] - mu / (s + EPS)) * s
    sl = s * lam[me:]
    for k, terms, extra in ((0, np.abs(ce), 0.0), (1, np.abs(r), 0.0), (2, q["df"] * dx, 0.0), (3, ds / (s + EPS), 0.0),
                            (4, np.log(s), 0.0), (5, gx * gx, float((ej * (2 * np.abs(gx) + ej)).sum())), (6, v6 * v6, 0.0),
                            (7, ce * ce, 0.0), (8, r * r, 0.0), (9, sl, 0.0), (11, dx * dx, 0.0), (12, ds * ds, 0.0)):
        val[k], bnd[k] = fsum_b(terms, extra)
    val[10] = sl.min() if mi else np.nan
    for k in SQ:
        bnd[k] += 4 * U * val[k]
    return val, bnd


def check_info(got, val, bnd, mi, factor=1.0, what=""):
    for k in range(13):
        if k == 10:
            assert (np.isnan(got[10]) and mi == 0) or got[10] == val[10], (what, k, got[10], val[10])
            continue
        g = got[k] * got[k] if k in SQ else got[k]
        assert abs(g - val[k]) <= factor * bnd[k], (what, k, g, val[k], abs(g - val[k]), bnd[k])
    assert np.all(got[13:] == 0.0)


def abs_change(c, d, a):
    """kernels_merit.hpp's abs_change, element by element, in float64."""
    c, d = np.asarray(c, dtype=np.float64), np.asarray(d, dtype=np.float64)
    out = np.sign(c) * (a * d)                               # c + a d keeps the sign of c wherever |a d| < |c|
    for i in np.flatnonzero(np.abs(a * d) >= 0.5 * np.abs(c)):
        ci, di = float(c[i]), float(d[i])
        exact = Fraction(a) * Fraction(di) + Fraction(ci)    # its rounding is the kernel's fma(a, d, c): same sign, same value
        if ci > 0.0 and exact >= 0:
            out[i] = a * di
        elif ci < 0.0 and exact <= 0:
            out[i] = -(a * di)
        else:
            out[i] = abs(float(exact)) - abs(ci)
    return out


def ref_ray(q, dz, alphas, nu, mu, quad=None):
    n, me, mi = q["n"], q["me"], q["mi"]
    dx, ds = dz[:n], dz[n:n + mi]
    t1 = q["df"] * dx
    S = sym(q["d2L"])
    t2 = dx[:, None] * S * dx[None, :]
    dce = np.array([math.fsum(q["Je"][:, i] * dx) for i in range(me)])
    dci = np.array([math.fsum(q["Ji"][:, i] * dx) for i in range(mi)])
    Ee = (n + 8) * U * np.abs(q["Je"] * dx[:, None]).sum(axis=0) if me else np.zeros(0)
    Ei = (n + 8) * U * np.abs(q["Ji"] * dx[:, None]).sum(axis=0) if mi else np.zeros(0)
    r, dr = q["ci"] - q["s"], dci - ds
    vals, bnds = [], []
    for a in alphas:
        a = float(a)
        p1, b1 = fsum_b(a * t1)
        if quad is None:
            p2, b2 = fsum_b((0.5 * a * a) * t2)
        else:
            p2 = (0.5 * a * a) * quad
            b2 = 8 * U * abs(p2)
        p3 = b3 = p4 = b4 = p5 = b5 = 0.0
        if me:
            te = abs_change(q["ce"], dce, a)
            flip = np.abs(a * dce) >= 0.5 * np.abs(q["ce"])
            p3, b3 = fsum_b(nu * te, nu * float((a * Ee).sum() + (4 * U * (np.abs(q["ce"]) + np.abs(a * dce)))[flip].sum()))
        if mi:
            ti = abs_change(r, dr, a)
            flip = np.abs(a * dr) >= 0.5 * np.abs(r)
            p4, b4 = fsum_b(nu * ti, nu * float((a * Ei).sum() + (4 * U * (np.abs(r) + np.abs(a * dr)))[flip].sum()))
            p5, b5 = fsum_b(-mu * np.log1p(a * (ds / q["s"])))
        vals.append(math.fsum([p1, p2, p3, p4, p5]))
        bnds.append(b1 + b2 + b3 + b4 + b5 + 8 * U * (abs(p1) + abs(p2) + abs(p3) + abs(p4) + abs(p5)))
    return np.array(vals), np.array(bnds)


def ref_products(q):
    n, me, mi = q["n"], q["me"], q["mi"]
    v = q["v"]
    out = []
    for M in (sym(q["d2L"]), q["Je"].T, q["Ji"].T):
        T = M * v[None, :]
        out.append((np.array([math.fsum(row) for row in T]), (n + 8) * U * np.abs(T).sum(axis=1)))
    T = np.concatenate([q["Je"] * q["le"][None, :], q["Ji"] * q["li"][None, :]], axis=1)
    out.append((np.array([math.fsum(row) for row in T]) if me + mi else np.zeros(n), (me + mi + 8) * U * np.abs(T).sum(axis=1)))
    Te = q["Je"] * q["le"][None, :]
    out.append((np.array([math.fsum(row) for row in Te]) if me else np.zeros(n), (me + 8) * U * np.abs(Te).sum(axis=1)))
    return out


@functools.lru_cache(maxsize=None)
def refs(shape, seed, B):
    return {}


def problem_refs(shape, seed, R, b):
    """The host references of one problem for the direction of the run it belongs to: computed once, shared by the tests."""
    c = refs(shape, seed, len(R["seeds"]))
    if not c:
        q = qp(*shape, seed)
        c["info"] = ref_info(q, R["dz"][b], 0.2)
        c["ray"] = ref_ray(q, R["dz"][b], R["alphas"][b], R["nu"][b], R["mu"][b])
        c["ray_quad"] = ref_ray(q, R["dz"][b], R["alphas"][b], R["nu"][b], R["mu"][b], quad=R["quad"][b])
        c["prod"] = ref_products(q)
    return c


# ---- 1. accuracy against the host references -------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("shape", SHAPES)
def test_every_quantity_meets_its_a_priori_bound(shape, B):
    n, me, mi = shape
    seeds = seeds_of(shape, B)
    R = run(shape, seeds)
    worst = {"ray": 0.0, "prod": 0.0}
    for b, sd in enumerate(seeds):
        c = problem_refs(shape, sd, R, b)
        val, bnd = c["info"]
        check_info(R["info"][b], val, bnd, mi, what="info b=%d" % b)
        for name in ("ray", "ray_quad"):
            val, bnd = c[name]
            err = np.abs(R[name][b] - val)
            assert np.all(err <= bnd), (name, b, err, bnd, val)
            worst["ray"] = max(worst["ray"], float((err / np.maximum(bnd, 1e-300)).max()))
        # the a = 1e-12 candidate: the bound, and so the error, is relative to the change of phi itself
        val, bnd = c["ray"]
        assert bnd[-1] <= 1e-9 * abs(val[-1]), (b, bnd[-1], val[-1])
        got = list(R["prod"]) + [R["prod_t"], R["prod_t_e"]]
        for k, (val, bnd) in enumerate(c["prod"]):
            if got[k] is None:
                assert (k == 1 and me == 0) or (k == 2 and mi == 0)
                continue
            err = np.abs(got[k][b] - val)
            assert np.all(err <= bnd), ("products", k, b, float(err.max()))
            worst["prod"] = max(worst["prod"], float((err / np.maximum(bnd, 1e-300)).max()))
    print("shape", shape, "B", B, "worst error / bound:", worst)
    # absent outputs, absent directions
    assert R["prod_part"][0] is None
    for k in (1, 2):
        assert (R["prod_part"][k] is None and R["prod"][k] is None) or np.array_equal(R["prod_part"][k], R["prod"][k])
    nd = R["info_nodz"]
    assert np.isnan(nd[:, [2, 3, 11, 12]]).all()
    keep = [0, 1, 4, 5, 6, 7, 8, 9] + ([10] if mi else [])
    assert np.array_equal(nd[:, keep], R["info"][:, keep])
    # two identical calls on the NaN-poisoned workspace
    assert np.array_equal(R["ray"], R["ray_again"]) and np.array_equal(R["info"], R["info_again"], equal_nan=True)
    for x, y in zip(R["prod"], R["prod_again"]):
        assert (x is None and y is None) or np.array_equal(x, y)


# ---- 2. against the single-system handle -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("shape", SHAPES)
def test_rows_agree_with_the_problem_staged_alone_on_a_single_system_handle(shape, B):
    import torch
    from pyipm_amd.newton import NewtonCore
    n, me, mi = shape
    seeds = seeds_of(shape, B)
    R = run(shape, seeds)
    core = NewtonCore(n, me, mi)
    for b, sd in enumerate(seeds):
        q = qp(n, me, mi, sd)
        c = problem_refs(shape, sd, R, b)
        core.stage_blocks(q["d2L"], q["Je"] if me else None, q["Ji"] if mi else None)
        core.stage_vectors(q["df"], q["ce"] if me else None, q["ci"] if mi else None, q["s"] if mi else None,
                           q["lam"] if (me + mi) else None, mu=0.2)
        core.residual()
        dzb = torch.from_numpy(R["dz"][b]).cuda()
        single = core.merit_info(dz=dzb)
        single = np.array([single[k] for k in core.MERIT_KEYS] + [0.0] * 3)
        val, bnd = c["info"]
        got = R["info"][b]
        for k in range(13):
            if k == 10:
                assert (np.isnan(got[10]) and np.isnan(single[10])) or got[10] == single[10]
                continue
            x, y = (got[k] ** 2, single[k] ** 2) if k in SQ else (got[k], single[k])
            assert abs(x - y) <= 2 * bnd[k], ("info", b, k, x, y, bnd[k])
        ray1 = np.array(core.merit_ray(list(R["alphas"][b]), float(R["nu"][b]), float(R["mu"][b]), dz=dzb))
        assert np.all(np.abs(ray1 - R["ray"][b]) <= 2 * c["ray"][1]), ("ray", b)
        nodz = core.merit_info()                                         # (this handle has solved nothing: no direction)
        for k, name in ((2, "df_dx"), (3, "ds_over_s"), (11, "dx_norm"), (12, "ds_norm")):
            assert np.isnan(nodz[name]) and np.isnan(R["info_nodz"][b, k])
        p1 = core.block_products(q["v"])
        for k in range(3):
            if p1[k] is None:
                assert R["prod"][k] is None
                continue
            assert np.all(np.abs(_np(p1[k]) - R["prod"][k][b]) <= 2 * c["prod"][k][1]), ("products", b, k)
        part = core.block_products(q["v"], want=(False, True, True))
        assert part[0] is None and R["prod_part"][0] is None
        t1 = _np(core.block_products_t(q["le"] if me else None, q["li"] if mi else None))
        assert np.all(np.abs(t1 - R["prod_t"][b]) <= 2 * c["prod"][3][1]), ("products_t", b)
    core.close()


# ---- 3. a problem's bits do not depend on the batch around it --------------------------------------------------------------------
@pytest.mark.parametrize("B", [5, 67])
@pytest.mark.parametrize("shape", SHAPES)
def test_rows_are_bit_identical_under_permutation_and_alone(shape, B):
    seeds = seeds_of(shape, B)
    R = run(shape, seeds)
    perm = np.random.default_rng(B).permutation(B)
    dz_from = (seeds, tuple(R["dz"]))

    def same(P, pb, b):
        for name in ("info", "info_nodz"):
            assert np.array_equal(P[name][pb], R[name][b], equal_nan=True), (name, b)
        for name in ("ray", "ray_quad", "prod_t", "prod_t_e"):
            assert np.array_equal(P[name][pb], R[name][b]), (name, b)
        for x, y in zip(P["prod"], R["prod"]):
            assert (x is None and y is None) or np.array_equal(x[pb], y[b])

    P = run.__wrapped__(shape, tuple(seeds[i] for i in perm), dz_from)
    for pb, b in enumerate(perm):
        same(P, pb, b)
    for b in sorted({0, B // 2, B - 1}):
        same(run.__wrapped__(shape, (seeds[b],), dz_from), 0, b)


@pytest.mark.parametrize("shape", [(40, 0, 12), (200, 30, 90), (300, 100, 300)])
def test_a_ray_value_does_not_depend_on_K_or_on_its_place(shape):
    from pyipm_amd.batched import BatchedNewton
    n, me, mi = shape
    B = 5
    seeds = seeds_of(shape, B)
    qps = [qp(n, me, mi, sd) for sd in seeds]
    bn = BatchedNewton(n, me, mi)
    dz, _ = bn.step_all(*_args(qps, me, mi), mu=0.2)
    al = _np(bn.step_lengths_all(0.995, dz))
    a = 0.37 * al[:, 0]
    nu, mu = np.full(B, 10.0), np.linspace(0.01, 0.2, B)
    rng = np.random.default_rng(5)
    got = []
    for K, pos in ((1, 0), (64, 17), (1024, 1000)):
        alphas = al[:, :1] * rng.uniform(0.0, 1.0, (B, K))
        alphas[:, pos] = a
        got.append(_np(bn.merit_ray_all(alphas, nu, mu, dz))[:, pos])
    bn.close()
    assert np.isfinite(got[0]).all()
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2])


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------------
def test_every_badarg_case():
    import ctypes
    import torch
    from pyipm_amd.batched import BatchedNewton
    from pyipm_amd.newton import MEM_DEVICE, NewtonCore
    n, me, mi, B = 40, 0, 12, 3
    f64 = torch.float64
    buf = lambda *shape: torch.zeros(shape, dtype=f64, device="cuda")           # noqa: E731
    p = lambda t: ctypes.c_void_p(t.data_ptr())                                 # noqa: E731
    v, Qv, JiTv, li, out_n = buf(B, n), buf(B, n), buf(B, mi), buf(B, mi), buf(B, n)
    info, dz, nu, mu, al, ray = buf(B, 16), buf(B, n + 2 * mi + me), buf(B), buf(B), buf(B, 4), buf(B, 4)

    def four(lib, h, K=4, v_=v, out_=out_n, info_=info, nu_=nu, mu_=mu, al_=al, ray_=ray, dz_=dz):
        q = lambda t: None if t is None else p(t)                               # noqa: E731
        return (lib.pyipm_newton_block_products_batched(h, q(v_), p(Qv), None, p(JiTv)),
                lib.pyipm_newton_block_products_t_batched(h, None, p(li), q(out_)),
                lib.pyipm_newton_merit_info_batched(h, p(dz), q(info_), MEM_DEVICE),
                lib.pyipm_newton_merit_ray_batched(h, q(dz_), q(nu_), q(mu_), None, q(al_), K, q(ray_), MEM_DEVICE))

    # not a batched handle
    core = NewtonCore(n, me, mi)
    assert four(core.lib, core.h) == (-1, -1, -1, -1)
    assert b"not a batched handle" in core.lib.pyipm_newton_last_error(core.h)
    # nothing staged
    bn = BatchedNewton(n, me, mi, batch=B)
    assert four(bn.lib, bn.h) == (-1, -1, -1, -1)
    qps = [qp(n, me, mi, 50 + b) for b in range(B)]
    bn.stage(*_args(qps, me, mi), mu=0.2)
    assert four(bn.lib, bn.h) == (0, 0, 0, 0)
    # K out of range
    assert four(bn.lib, bn.h, K=0)[3] == -1 and four(bn.lib, bn.h, K=1025)[3] == -1 and four(bn.lib, bn.h, K=-3)[3] == -1
    # a required pointer is NULL
    assert four(bn.lib, bn.h, v_=None)[0] == -1
    assert four(bn.lib, bn.h, out_=None)[1] == -1
    assert four(bn.lib, bn.h, info_=None)[2] == -1
    for kw in ("nu_", "mu_", "al_", "ray_", "dz_"):
        assert four(bn.lib, bn.h, **{kw: None})[3] == -1, kw
    assert bn.lib.pyipm_newton_merit_info_batched(bn.h, p(dz), p(info), 7) == -1            # neither host nor device
    torch.cuda.synchronize()
    bn.close()


def test_host_outputs_are_the_device_outputs():
    """memkind = host: the same launches, staged through the library's scratch, synchronised."""
    import ctypes
    from pyipm_amd.batched import BatchedNewton
    from pyipm_amd.newton import MEM_HOST
    shape, B = (96, 24, 40), 5
    n, me, mi = shape
    seeds = seeds_of(shape, B)
    R = run(shape, seeds)
    qps = [qp(n, me, mi, sd) for sd in seeds]
    bn = BatchedNewton(n, me, mi)
    dz, _ = bn.step_all(*_args(qps, me, mi), mu=0.2)
    dp = lambda a: a.ctypes.data_as(ctypes.c_void_p)                            # noqa: E731
    info = np.zeros((B, 16))
    assert bn.lib.pyipm_newton_merit_info_batched(bn.h, ctypes.c_void_p(dz.data_ptr()), dp(info), MEM_HOST) == 0
    assert np.array_equal(info, R["info"], equal_nan=True)
    K = R["alphas"].shape[1]
    ray, al = np.zeros((B, K)), np.ascontiguousarray(R["alphas"])
    assert bn.lib.pyipm_newton_merit_ray_batched(bn.h, ctypes.c_void_p(dz.data_ptr()), dp(R["nu"]), dp(R["mu"]), None, dp(al), K,
                                                 dp(ray), MEM_HOST) == 0
    assert np.array_equal(ray, R["ray"])
    bn.close()
