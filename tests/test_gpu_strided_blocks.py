"""Caller-owned DEVICE blocks that are not packed: padded leading dimensions, odd ones, bases aligned to 8 bytes only, batch
strides with gaps (include/pyipm_newton.h, "Layout of a retained device block").  Every kernel that reads d2L, Je, Ji (S, Y for
L-BFGS) takes the leading dimension as an argument, and before this module those arguments had only ever carried the width.

Method.  ``padded`` lays a block out in a flat buffer of NaN: the padding of every row, the gaps between batch members, the
doubles in front of the base, a short tail and -- for d2L -- everything below the diagonal are NaN, so whatever the library may
not use poisons the result if it is used.  A handle on such views and a handle on packed tensors get the same numbers, and
every output is compared BIT FOR BIT: all these kernels index by element (M[j * ld + a]) and split their sums by element
index, never by address (k_assemble's 16-byte loads of d2L, taken only when ld is even and the base 16-byte aligned, fetch
the same two doubles), so the layout cannot change a bit.  So that the packed run is anchored to something else than the code
under test, it is compared with the CPU oracle (directions: relative error <= 1e-10, the suite's bar; L-BFGS: 1e-9), with the
NumPy-built triu(H) (assembly, bit for bit) and with math.fsum references under the a-priori bound of
tests/test_gpu_batched_merit.py: a sum of m terms t_i is within (m + 8) u sum|t_i| of fsum, u = 2^-53.

Layouts, named by what d2L gets; Je and Ji get the next ones in turn, so the three blocks never share a padding:
 a  ld = width + 1, off = 0           odd ld for an even width and the other way round: flips the parity k_assemble looks at
 b  ld = width + 2, off = 1           even ld, base 8-byte aligned only: k_assemble's second condition
 c  ld = roundup(width, 64) + 64, off = 2     aligned, even, far from the width: the vector loads with ld != n
Batched handles add a batch stride of rows * ld + 3 (odd: the alignment of the members alternates).
Shapes: the smallest at which the work splits (nb = 128: several panels, more than one 512-row assembly patch at N = 660), an
odd n, an even n (the packed run then takes the vector loads, a and b the scalar ones), and one inside a single tile."""
import ctypes
import functools
import math

import numpy as np
import pytest

from oracle import newton_oracle as orc
from pyipm_amd.problems import make_qp

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
EPS = float(np.finfo(np.float64).eps)
NAN = float("nan")
SHAPES = [(330, 70, 130), (301, 37, 0), (256, 0, 61), (64, 8, 16)]
BSHAPES = [(65, 63, 1), (130, 40, 100), (3, 0, 9)]
LSHAPES = [(777, 65, 191, 5), (300, 64, 64, 0)]
B = 5
LAYOUTS = {"a": lambda w: (w + 1, 0), "b": lambda w: (w + 2, 1), "c": lambda w: ((w + 63) // 64 * 64 + 64, 2)}
ORDER = "abc"
DELTA, DELTA_C = 1e-3, 1e-9
BADARG = -1
TAIL = 8


def padded(block, ld, off, batch_stride=None, poison=NAN, triu_only=False):
    """``block`` ((rows, width), or (batch, rows, width) with ``batch_stride``) inside one flat fp64 device buffer filled with
    ``poison``: row r at off + [b * batch_stride +] r * ld.  Returns the as_strided view.  ``triu_only`` (d2L): the strictly
    lower triangle inside the view is poisoned too."""
    import torch
    block = np.asarray(block, dtype=np.float64)
    rows, width = block.shape[-2:]
    assert ld >= width
    if block.ndim == 2:
        shape, strides, span = (rows, width), (ld, 1), (rows - 1) * ld + width
    else:
        assert batch_stride >= rows * ld
        shape, strides = block.shape, (batch_stride, ld, 1)
        span = (block.shape[0] - 1) * batch_stride + (rows - 1) * ld + width
    buf = torch.full((off + span + TAIL,), poison, dtype=torch.float64, device="cuda")
    view = buf.as_strided(shape, strides, off)
    view.copy_(torch.from_numpy(np.ascontiguousarray(block)).cuda())
    if triu_only:
        r, c = np.tril_indices(rows, -1)
        view[..., torch.from_numpy(r).cuda(), torch.from_numpy(c).cuda()] = poison
    assert int(torch.isnan(buf).sum()) >= buf.numel() - view.numel()
    return view


def lay(name, k, block, batch=False, triu_only=False):
    """Block number k (0: d2L, 1: Je, 2: Ji, ...) of the case ``name``; None for an empty block; 'packed': a plain tensor."""
    import torch
    if block is None or block.shape[-1] == 0:
        return None
    if name == "packed":
        return torch.from_numpy(np.ascontiguousarray(block)).cuda()
    ld, off = LAYOUTS[ORDER[(ORDER.index(name) + k) % 3]](block.shape[-1])
    return padded(block, ld, off, block.shape[-2] * ld + 3 if batch else None, triu_only=triu_only)


def _np(t):
    return None if t is None else t.detach().cpu().numpy().copy()


def same(a, b):
    """Bit for bit (NaN equal to the same NaN; None to None)."""
    if a is None or b is None:
        return a is None and b is None
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


@functools.lru_cache(maxsize=None)
def problem(n, me, mi, seed=None):
    q = make_qp(n, me, mi, seed=n + 7 if seed is None else seed)
    N = n + 2 * mi + me
    rng = np.random.default_rng(n + 1000 + (seed or 0))
    q["v"], q["vx"], q["le"], q["li"] = rng.standard_normal(N), rng.standard_normal(n), rng.standard_normal(me), rng.standard_normal(mi)
    q["rhs3"] = rng.standard_normal((N, 3))
    return q


def step_vectors(q, k):
    """Vectors of step k of the reuse sequence: other s, lda, mu and right-hand side each time."""
    n, me, mi = q["n"], q["me"], q["mi"]
    rng = np.random.default_rng(1000 + k)
    return dict(df=q["df"] + 0.1 * rng.standard_normal(n), ce=q["ce"] + 0.1 * rng.standard_normal(me),
                ci=q["ci"] + 0.1 * rng.standard_normal(mi), s=q["s"] * rng.uniform(0.5, 2.0, mi),
                lda=q["lam"] * rng.uniform(0.5, 2.0, me + mi), mu=0.2 / (k + 1))


def staged(shape, name, **kw):
    from pyipm_amd.newton import NewtonCore
    n, me, mi = shape
    q = problem(*shape)
    core = NewtonCore(n, me, mi, device=0, nb=128, **kw)
    blocks = (lay(name, 0, q["d2L"], triu_only=True), lay(name, 1, q["Je"]), lay(name, 2, q["Ji"]))
    core.stage_blocks(*blocks)
    if name != "packed":                                       # the views went through as they are: the test tests what it says
        for k, t in zip(("d2L", "Je", "Ji"), blocks):
            assert t is None or (core._keep[k].data_ptr() == t.data_ptr() and core._keep[k].stride() == t.stride())
    core.stage_vectors(q["df"], q["ce"], q["ci"], q["s"], q["lam"], mu=q["mu"])
    return core, q


@functools.lru_cache(maxsize=None)
def single(shape, name):
    """Everything a single-system handle on the layout ``name`` says about the problem of ``shape`` (NumPy)."""
    n, me, mi = shape
    out = {}
    # -- products, steps, solve_many, merit
    core, q = staged(shape, name)
    out["residual"] = _np(core.residual())
    dz, st = core.step(0.0, 0.0, refine=0)
    out["dz0"], out["st0"] = _np(dz), st
    out["matvec"] = _np(core.matvec(q["v"]))
    out["prod"] = tuple(_np(t) for t in core.block_products(q["vx"]))
    out["prod_t"] = _np(core.block_products_t(q["le"] if me else None, q["li"] if mi else None))
    out["many"] = _np(core.solve_many(q["rhs3"], refine=1))
    a_s, a_l = core.step_lengths(0.995) if mi else (1.0, 1.0)
    out["alphas"] = [a_s * f for f in (1.0, 0.5, 0.1)]
    out["merit"] = core.merit_info()
    out["ray"] = core.merit_ray(out["alphas"], 10.0, 0.2)
    dz, st = core.step(0.0, 0.0, refine=-1)
    out["dz1"], out["st1"], out["info1"] = _np(dz), st, core.solve_info()
    if mi:
        core.set_option("condensed", 1)
        dz, st = core.step(0.0, 0.0, refine=0)
        out["cdz0"], out["cst0"] = _np(dz), st
        dz, st = core.step(0.0, 0.0, refine=-1)
        out["cdz1"], out["cst1"] = _np(dz), st
    core.close()
    # -- the same products on a provider-only handle
    core, q = staged(shape, name, provider_only=True)
    out["p_residual"], out["p_matvec"] = _np(core.residual()), _np(core.matvec(q["v"]))
    out["p_prod"] = tuple(_np(t) for t in core.block_products(q["vx"]))
    out["p_prod_t"] = _np(core.block_products_t(q["le"] if me else None, q["li"] if mi else None))
    core.close()
    # -- three steps on one staging: the later ones re-read the retained blocks (reassemble_slack, the refinement)
    core, q = staged(shape, name)
    core.set_option("expert", 1)
    core.set_option("group", 2)
    out["reuse"] = []
    for k in range(3):
        v = step_vectors(q, k)
        core.stage_vectors(v["df"], v["ce"], v["ci"], v["s"], v["lda"], mu=v["mu"])
        dz, st = core.step(0.0, 0.0, refine=1 if k == 2 else 0)
        out["reuse"].append((_np(dz), st, core.reuse_info()["last"]))
    core.close()
    # -- assembly with both shifts (a handle of its own: reading the storage switches the reuse off)
    core, q = staged(shape, name)
    core.assemble(DELTA, DELTA_C)
    out["storage"], out["anorm"] = _np(core.kkt_storage()), _np(core.anorm())
    core.close()
    return out


@functools.lru_cache(maxsize=None)
def oracle(shape, seed=None):
    n, me, mi = shape
    q = problem(n, me, mi, seed)
    dz, _, Hc, g = orc.newton_step(q["d2L"], q["Je"], q["Ji"], q["df"], q["ce"], q["ci"], q["s"], q["lam"], q["mu"], n, me, mi,
                                   regularise=False)
    return dz, Hc, g


def relerr(got, ref):
    return float(np.linalg.norm(got - ref) / np.linalg.norm(ref))


def rows_fsum(T, m=None):
    """(fsum of every row of the term matrix T, (m + 8) u sum|t|)"""
    T = np.atleast_2d(T)
    m = T.shape[1] if m is None else m
    return np.array([math.fsum(r) for r in T]), (m + 8) * U * np.abs(T).sum(axis=1)


def sym(Q):
    return np.triu(Q) + np.triu(Q, 1).T


CASES = [(s, l) for s in SHAPES for l in ORDER]
IDS = ["%dx%dx%d-%s" % (s + (l,)) for s, l in CASES]


# ---- 1. assembly -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,name", CASES, ids=IDS)
def test_assembly_is_the_packed_one_and_triu_of_the_reference(shape, name):
    n, me, mi = shape
    N = n + 2 * mi + me
    got, ref = single(shape, name), single(shape, "packed")
    # the storage is (columns, Npad) row-major: row j = column j of the lower triangle = row j of triu(H); what lies left of the
    # diagonal belongs to other columns' rows and is not written by the assembly
    assert same(np.triu(got["storage"]), np.triu(ref["storage"]))
    assert same(got["anorm"], ref["anorm"]) and np.isfinite(got["anorm"]).all() and got["anorm"][0] > 0.0
    H = oracle(shape)[1].copy()
    H[np.arange(n), np.arange(n)] += DELTA
    e0 = n + mi
    H[np.arange(e0, e0 + me), np.arange(e0, e0 + me)] -= DELTA_C
    for pack in (got, ref):
        assert np.array_equal(np.triu(pack["storage"][:N, :N]), np.triu(H))
        pad = np.triu(pack["storage"][N:, :pack["storage"].shape[0]], N)          # identity pad
        assert np.array_equal(pad[:, N:], np.eye(pad.shape[0]))


# ---- 2. products that read the blocks --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,name", CASES, ids=IDS)
def test_products_are_the_packed_ones(shape, name):
    got, ref = single(shape, name), single(shape, "packed")
    for k in ("residual", "matvec", "prod_t", "p_residual", "p_matvec", "p_prod_t"):
        assert same(got[k], ref[k]), k
        assert np.isfinite(got[k]).all(), k
    for k in ("prod", "p_prod"):
        for a, b in zip(got[k], ref[k]):
            assert same(a, b), k


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_packed_products_meet_the_a_priori_bound(shape):
    n, me, mi = shape
    N = n + 2 * mi + me
    q, R = problem(*shape), single(shape, "packed")
    _, Hc, g = oracle(shape)
    lam, s = q["lam"], q["s"]
    worst = 0.0

    def check(got, val, bnd, what):
        nonlocal worst
        err = np.abs(got - val)
        print(what, "worst error / bound: %.3f" % float((err / np.maximum(bnd, 1e-300)).max()) if err.size else "empty")
        assert np.all(err <= bnd), (what, float(err.max()), float(bnd[np.argmax(err)]))
        worst = max(worst, float((err / np.maximum(bnd, 1e-300)).max()) if err.size else 0.0)

    # residual g = -grad: x rows -(df_j - sum_a J[j][a] lda_a); the rows below are formed from two or three numbers
    J = np.concatenate([q["Je"], q["Ji"]], axis=1)
    val, bnd = rows_fsum(np.concatenate([-q["df"][:, None], J * lam[None, :]], axis=1))
    low_b = 8 * U * np.concatenate([np.abs(lam[me:]) + np.abs(q["mu"] / (s + EPS)), np.abs(q["ce"]), np.abs(q["ci"]) + np.abs(s)])
    for key in ("residual", "p_residual"):
        check(R[key][:n], val, bnd, key + " x")
        check(R[key][n:N], g[n:], low_b, key + " s, lambda")
        assert np.all(R[key][N:] == 0.0)
    # kkt_matvec: row i of Hc (N terms at the most) times v
    val, bnd = rows_fsum(Hc * q["v"][None, :])
    for key in ("matvec", "p_matvec"):
        check(R[key][:N], val, bnd, key)
    # block products: sym(triu d2L) v, Je' v, Ji' v (n terms), Je le + Ji li (me + mi terms)
    refs = [rows_fsum(M * q["vx"][None, :]) for M in (sym(q["d2L"]), q["Je"].T, q["Ji"].T)]
    reft = rows_fsum(np.concatenate([q["Je"] * q["le"][None, :], q["Ji"] * q["li"][None, :]], axis=1))
    for key in ("prod", "p_prod"):
        for k, (val, bnd) in enumerate(refs):
            if R[key][k] is None:
                assert (k == 1 and me == 0) or (k == 2 and mi == 0)
            else:
                check(R[key][k], val, bnd, "%s[%d]" % (key, k))
        check(R[key + "_t"], reft[0], reft[1], key + "_t")
    assert worst > 0.0 or N == 0


# ---- 3. steps ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,name", CASES, ids=IDS)
def test_steps_are_the_packed_ones_and_the_oracles(shape, name):
    n, me, mi = shape
    got, ref = single(shape, name), single(shape, "packed")
    want = oracle(shape)[0]
    keys = [("dz0", "st0"), ("dz1", "st1")] + ([("cdz0", "cst0"), ("cdz1", "cst1")] if mi else [])
    for dz, st in keys:
        assert same(got[dz], ref[dz]), dz
        assert got[st] == ref[st], (st, got[st], ref[st])
        assert got[st]["n_neg"] == me + mi and got[st]["n_zero"] == 0 and got[st]["nonfinite"] == 0
        for pack in (got, ref):
            err = relerr(pack[dz], want)
            print(dz, "relative error against the oracle: %.3e" % err)
            assert err <= 1e-10, (dz, err)
    assert got["info1"] == ref["info1"]


# ---- 4. reuse ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,name", CASES, ids=IDS)
def test_reusing_steps_reread_the_retained_blocks(shape, name):
    n, me, mi = shape
    got, ref = single(shape, name), single(shape, "packed")
    # (a system of one panel -- N <= 128 -- has no group inside the x block: prefix_mode runs it in full, whatever the layout)
    kinds = ["recording", "reusing", "reusing"] if n + 2 * mi + me > 128 else ["full"] * 3
    assert [r[2] for r in got["reuse"]] == kinds == [r[2] for r in ref["reuse"]]
    for k, ((dz, st, _), (rdz, rst, _)) in enumerate(zip(got["reuse"], ref["reuse"])):
        assert np.isfinite(dz).all(), k
        assert same(dz, rdz), k
        assert st == rst, (k, st, rst)
    assert not same(got["reuse"][0][0], got["reuse"][1][0])


# ---- 5. solve_many and merit -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,name", CASES, ids=IDS)
def test_solve_many_and_merit_are_the_packed_ones(shape, name):
    got, ref = single(shape, name), single(shape, "packed")
    assert same(got["many"], ref["many"]) and np.isfinite(got["many"]).all() and got["many"].shape[1] == 3
    assert got["alphas"] == ref["alphas"]
    for k, v in got["merit"].items():
        assert same(np.array([v]), np.array([ref["merit"][k]])), k
    assert same(np.array(got["ray"]), np.array(ref["ray"])) and np.isfinite(got["ray"]).all()
    # anchor: Hc x = b for the refined columns (Hc from the oracle's blocks; the columns come back multiplier-flipped)
    n, me, mi = shape
    q, Hc = problem(*shape), oracle(shape)[1]
    X = ref["many"].copy()
    X[n + mi:] *= -1.0
    res = np.linalg.norm(Hc @ X - q["rhs3"], axis=0) / np.linalg.norm(q["rhs3"], axis=0)
    print("solve_many residuals", res)
    assert np.all(res <= 1e-10)


# ---- 6. batched -------------------------------------------------------------------------------------------------------------------
def bproblems(shape):
    return [problem(*shape, seed=31 * shape[0] + 5 * b + 1) for b in range(B)]


@functools.lru_cache(maxsize=None)
def batched(shape, name, condensed, flipped=False):
    import torch
    from pyipm_amd.batched import BatchedNewton
    n, me, mi = shape
    qs = bproblems(shape)
    if flipped:
        qs = qs[::-1]
    st = lambda k: np.stack([q[k] for q in qs])                  # noqa: E731
    blocks = (lay(name, 0, st("d2L"), True, triu_only=True), lay(name, 1, st("Je"), True), lay(name, 2, st("Ji"), True))
    vecs = dict(df=st("df"), ce=st("ce") if me else None, ci=st("ci") if mi else None, s=st("s") if mi else None,
                lda=st("lam") if me + mi else None)
    bn = BatchedNewton(n, me, mi, condensed=condensed)
    out = {}
    dz, stats = bn.step_all(*blocks, **vecs, mu=0.2)
    if name != "packed":
        for kept, t in zip(bn._keep[0], blocks):
            assert t is None or (kept.data_ptr() == t.data_ptr() and kept.stride() == t.stride())
    out["dz"], out["stats"], out["fallback"] = _np(dz), list(stats), bn.n_condensed_fallback
    out["berr"] = _np(bn.backward_errors(dz))
    al = _np(bn.step_lengths_all(0.995, dz)) if mi else np.ones((B, 2))
    alphas = np.stack([al[:, 0] * f for f in (1.0, 0.5, 0.1)], axis=1)
    out["ray"] = _np(bn.merit_ray_all(alphas, 10.0, 0.2, dz))
    out["prod"] = tuple(_np(t) for t in bn.products_all(st("vx")))
    out["prod_t"] = _np(bn.products_t_all(st("le") if me else None, st("li") if mi else None))
    dz2, delta, stats2 = bn.direction_all(*blocks, vecs["df"], vecs["ce"], vecs["ci"], vecs["s"], vecs["lda"], 0.2)
    out["ddz"], out["ddelta"], out["dstats"] = _np(dz2), np.array(delta), list(stats2)
    bn.close()
    torch.cuda.synchronize()
    return out


BCASES = [(s, l, c) for s in BSHAPES for l in ORDER for c in (False, True)]
BIDS = ["%dx%dx%d-%s-%s" % (s + (l, "condensed" if c else "full")) for s, l, c in BCASES]
BKEYS = ("dz", "berr", "ray", "prod_t", "ddz", "ddelta")


def _same_batch(got, ref, order):
    for k in BKEYS:
        assert same(got[k][order], ref[k]), k
        assert np.isfinite(got[k]).all(), k
    for a, b in zip(got["prod"], ref["prod"]):
        assert same(None if a is None else a[order], b)
    for k in ("stats", "dstats"):
        assert [got[k][i] for i in order] == ref[k], k
    assert got["fallback"] == ref["fallback"]


@pytest.mark.parametrize("shape,name,condensed", BCASES, ids=BIDS)
def test_batched_handle_is_the_packed_one_and_the_oracles(shape, name, condensed):
    n, me, mi = shape
    got, ref = batched(shape, name, condensed), batched(shape, "packed", condensed)
    _same_batch(got, ref, np.arange(B))
    for b, q in enumerate(bproblems(shape)):
        want = oracle(shape, q["seed"])[0]
        for k in ("dz", "ddz"):
            err = relerr(ref[k][b], want)
            assert err <= 1e-10, (k, b, err)
        assert ref["stats"][b]["n_neg"] == me + mi
    print("backward errors", ref["berr"])


@pytest.mark.parametrize("condensed", [False, True], ids=["full", "condensed"])
def test_batch_members_in_reverse_order_in_memory(condensed):
    """The same problems laid out the other way round (layout b, stride rows * ld + 3): problem b's result does not depend on
    where it lies -- b * stride is what is used, not a position."""
    shape = BSHAPES[1]
    got, ref = batched(shape, "b", condensed, flipped=True), batched(shape, "packed", condensed)
    _same_batch(got, ref, np.arange(B)[::-1])


# ---- 7. L-BFGS --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lproblem(n, me, mi, m):
    q = problem(n, me, mi)
    rng = np.random.default_rng(3 + n)
    S = rng.standard_normal((n, m)) / np.sqrt(n)
    Y = 0.7 * S + 0.05 * rng.standard_normal((n, 4)) @ (rng.standard_normal((4, n)) @ S)
    SY = S.T @ Y
    SS, L, D = np.ascontiguousarray(S.T @ S), np.ascontiguousarray(np.tril(SY, -1)), np.ascontiguousarray(np.diag(np.diag(SY)))
    zeta = float(SY[-1, -1] / SS[-1, -1]) if m else 1.3
    return q, dict(S=S, Y=Y, SS=SS, L=L, D=D, zeta=zeta, g=rng.standard_normal(n + 2 * mi + me))


@functools.lru_cache(maxsize=None)
def lbfgs_run(shape, name):
    from pyipm_amd.lbfgs import LbfgsCore
    n, me, mi, m = shape
    q, p = lproblem(*shape)
    lb = LbfgsCore(n, me, mi, m + 2, device=0, nb=128)
    lb.stage_jacobian(lay(name, 1, q["Je"]), lay(name, 2, q["Ji"]))
    S, Y = (lay(name, 3, p["S"]), lay(name, 4, p["Y"])) if m else (None, None)
    dz, st = lb.direction(p["g"], q["s"], q["lam"], p["zeta"], S, Y, p["SS"], p["L"], p["D"], reg=1e-12)
    out = (_np(dz), st)
    lb.close()
    return out


@pytest.mark.parametrize("name", ORDER)
@pytest.mark.parametrize("shape", LSHAPES, ids=lambda s: "%dx%dx%d-m%d" % s)
def test_lbfgs_direction_is_the_packed_one_and_the_oracles(shape, name):
    from oracle import lbfgs_oracle as lo
    n, me, mi, m = shape
    q, p = lproblem(*shape)
    (dz, st), (rdz, rst) = lbfgs_run(shape, name), lbfgs_run(shape, "packed")
    assert same(dz, rdz) and np.isfinite(dz).all()
    assert st == rst and st["m"] == m and st["n_neg"] == 0 and st["n_zero"] == 0
    ref = lo.direction(p["g"], p["zeta"], p["S"], p["Y"], p["SS"], p["L"], p["D"], Je=q["Je"], Ji=q["Ji"], s=q["s"], lda=q["lam"],
                       reg=1e-12)
    err = float(np.linalg.norm(rdz - ref) / np.linalg.norm(ref))
    print("L-BFGS relative error against the oracle: %.3e" % err)
    assert err <= 1e-9, err


# ---- 8. argument errors (DEVICE memory, raw ctypes) ------------------------------------------------------------------------------
def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def test_a_leading_dimension_below_the_width_is_refused():
    import torch
    shape = SHAPES[3]
    n, me, mi = shape
    core, q = staged(shape, "b")
    dz, _ = core.step(0.0, 0.0)
    H, E, I = (core._keep[k] for k in ("d2L", "Je", "Ji"))
    ld = [H.stride(0), E.stride(0), I.stride(0)]
    for k, w in enumerate((n, me, mi)):
        bad = list(ld)
        bad[k] = w - 1
        assert core.lib.pyipm_newton_stage_blocks(core.h, _p(H), bad[0], _p(E), bad[1], _p(I), bad[2], 0) == BADARG, k
        assert b"leading dimension" in core.lib.pyipm_newton_last_error(core.h)
    assert core.lib.pyipm_newton_stage_blocks(core.h, _p(H), ld[0], _p(E), ld[1], _p(I), ld[2], 0) == 0
    again, _ = core.step(0.0, 0.0)
    assert torch.equal(again, dz)
    core.close()


def test_a_leading_dimension_below_the_width_is_refused_batched():
    import torch
    from pyipm_amd.batched import BatchedNewton
    shape = BSHAPES[0]
    n, me, mi = shape
    qs = bproblems(shape)
    st = lambda k: np.stack([q[k] for q in qs])                  # noqa: E731
    H, E, I = lay("b", 0, st("d2L"), True, triu_only=True), lay("b", 1, st("Je"), True), lay("b", 2, st("Ji"), True)
    bn = BatchedNewton(n, me, mi)
    args = (H, E, I, st("df"), st("ce"), st("ci"), st("s"), st("lam"))
    dz, _ = bn.step_all(*args, mu=0.2)
    dz = dz.clone()
    good = [_p(H), H.stride(1), H.stride(0), _p(E), E.stride(1), E.stride(0), _p(I), I.stride(1), I.stride(0)]
    for k, w in enumerate((n, me, mi)):
        bad = list(good)
        bad[3 * k + 1] = w - 1
        assert bn.lib.pyipm_newton_stage_blocks_batched(bn.h, *bad) == BADARG, k
        assert b"leading dimension" in bn.lib.pyipm_newton_last_error(bn.h)
    assert bn.lib.pyipm_newton_stage_blocks_batched(bn.h, *good) == 0
    again, _ = bn.step_all(*args, mu=0.2)
    assert torch.equal(again, dz)
    bn.close()


def test_a_leading_dimension_below_the_width_is_refused_lbfgs():
    import torch
    from pyipm_amd.lbfgs import LbfgsCore, LbfgsStats
    from pyipm_amd.newton import MEM_DEVICE
    shape = LSHAPES[0]
    n, me, mi, m = shape
    q, p = lproblem(*shape)
    lb = LbfgsCore(n, me, mi, m + 2, device=0, nb=128)
    E, I, S, Y = lay("b", 1, q["Je"]), lay("b", 2, q["Ji"]), lay("b", 3, p["S"]), lay("b", 4, p["Y"])
    lib, h = lb.lib, lb.h
    assert lib.pyipm_lbfgs_stage_jacobian(h, _p(E), me - 1, _p(I), I.stride(0), MEM_DEVICE) == BADARG
    assert lib.pyipm_lbfgs_stage_jacobian(h, _p(E), E.stride(0), _p(I), mi - 1, MEM_DEVICE) == BADARG
    assert b"leading dimension" in lib.pyipm_lbfgs_last_error(h)
    lb.stage_jacobian(E, I)
    want, _ = lb.direction(p["g"], q["s"], q["lam"], p["zeta"], S, Y, p["SS"], p["L"], p["D"], reg=1e-12)
    g, s, lda = (torch.from_numpy(a).cuda() for a in (p["g"], q["s"], q["lam"]))
    out = torch.empty_like(g)
    hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)           # noqa: E731
    st = LbfgsStats()
    for ldS, ldY in ((m - 1, Y.stride(0)), (S.stride(0), m - 1)):
        rc = lib.pyipm_lbfgs_direction(h, _p(g), _p(s), _p(lda), p["zeta"], m, _p(S), ldS, _p(Y), ldY, hp(p["SS"]), hp(p["L"]),
                                       hp(p["D"]), 1e-12, EPS, _p(out), 0, MEM_DEVICE, ctypes.byref(st))
        assert rc == BADARG and b"bad storage pointers" in lib.pyipm_lbfgs_last_error(h)
    again, _ = lb.direction(p["g"], q["s"], q["lam"], p["zeta"], S, Y, p["SS"], p["L"], p["D"], reg=1e-12)
    assert torch.equal(again, want)
    lb.close()
