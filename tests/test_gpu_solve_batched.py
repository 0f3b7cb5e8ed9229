"""The kept factors of a batched handle as a solver: ``BatchedNewton.solve_all`` (pyipm_newton_solve_batched),
``kkt_matvec_all`` (pyipm_newton_kkt_matvec_batched) and ``rcond_all`` (pyipm_newton_rcond_batched) against dense fp64
matrices built on the host from the blocks and Sigma.

Bars: 1e-10 per column on known solutions (the project's bar for directions), 1e-12 against the step's own direction (the bar
``test_gpu_solve_many.py`` holds ``solve_many`` to against ``solve``), 1e-13 for the products, ``condensed_tol`` for the
refined condensed solve, the band (0.2, 5) of ``tests/test_gpu_pivoting.py`` for the condition estimate."""
import numpy as np
import pytest

from oracle import newton_oracle as orc
from pyipm_amd.problems import make_qp

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float64).eps)
KEYS = ("d2L", "Je", "Ji", "df", "ce", "ci", "s", "lam")
B = 5
SHAPES = [(40, 8, 24), (70, 10, 20), (203, 37, 61), (256, 0, 256), (300, 100, 312)]
KS = (1, 2, 15, 16, 17, 40)
KMAX = 40
MU = 0.2


def _seed(shape, b):
    return 4100 + 17 * b + shape[0]


def _args(qps, n, me, mi):
    on = {"d2L": True, "Je": me, "Ji": mi, "df": True, "ce": me, "ci": mi, "s": mi, "lam": me + mi}
    return [np.stack([q[k] for q in qps]) if on[k] else None for k in KEYS]


def _dense(q, n, me, mi, delta=0.0, delta_c=0.0):
    Hc = orc.kkt_matrix(q["d2L"], q["Je"], q["Ji"], q["s"], q["lam"], n, me, mi)
    Hc[:n, :n] += delta * np.eye(n)
    Hc[n + mi:n + mi + me, n + mi:n + mi + me] -= delta_c * np.eye(me)
    return Hc


def _colerr(x, ref):
    """Per-column relative error of (..., k, N) arrays: the worst column."""
    return float((np.linalg.norm(x - ref, axis=-1) / np.linalg.norm(ref, axis=-1)).max())


_CASES = {}


def _case(shape):
    """Problems, dense matrices, known solutions and their right-hand sides of one shape: built once, never changed.  Before
    anything is asked of the GPU: numpy.linalg.solve on the dense matrix recovers X_true to 1e-11 for every problem."""
    if shape in _CASES:
        return _CASES[shape]
    n, me, mi = shape
    N = n + 2 * mi + me
    qps = [make_qp(n, me, mi, seed=_seed(shape, b)) for b in range(B)]
    Hc = np.stack([_dense(q, n, me, mi) for q in qps])
    rng = np.random.default_rng(99 + n)
    X = rng.standard_normal((B, KMAX, N))
    R = np.einsum("bij,bkj->bki", Hc, X)
    for b in range(B):
        back = np.linalg.solve(Hc[b], R[b].T).T
        assert _colerr(back, X[b]) <= 1e-11, (shape, b, _colerr(back, X[b]))
    g = np.stack([-orc.kkt_residual(q["df"], q["Je"], q["Ji"], q["ce"], q["ci"], q["s"], q["lam"], MU, n, me, mi) for q in qps])
    c = _CASES[shape] = {"qps": qps, "Hc": Hc, "X": X, "R": R, "g": g, "N": N}
    return c


def _handle(shape, qps, condensed=False, delta=0.0, delta_c=0.0, step=True):
    from pyipm_amd.batched import BatchedNewton
    n, me, mi = shape
    bn = BatchedNewton(n, me, mi, condensed=condensed)
    bn.stage(*_args(qps, n, me, mi), mu=MU)
    dz = bn.step_each(MU, delta, delta_c)[0] if step else None
    return bn, dz


def _flip(a, n, mi):
    a = np.array(a)
    a[..., n + mi:] = -a[..., n + mi:]
    return a


# ---- 1. known solutions, and the bits of a column ------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_known_solutions_and_column_bits(shape):
    import torch
    c = _case(shape)
    n, me, mi = shape
    bn, _ = _handle(shape, c["qps"])
    R = torch.from_numpy(c["R"]).to(bn.device)
    full = bn.solve_all(R, flip=False)
    assert full.shape == R.shape
    err = _colerr(full.cpu().numpy(), c["X"])
    print("known solutions", shape, "k = %d: worst column %.3e" % (KMAX, err))
    assert err <= 1e-10
    for k in KS:
        xk = bn.solve_all(R[:, :k].contiguous(), flip=False)
        e = _colerr(xk.cpu().numpy(), c["X"][:, :k])
        print("  k = %d: worst column %.3e" % (k, e))
        assert e <= 1e-10
        assert torch.equal(xk, full[:, :k]), "a column's bits depend on k (k = %d)" % k
    perm = torch.from_numpy(np.random.default_rng(3).permutation(KMAX)).to(bn.device)
    assert torch.equal(bn.solve_all(R[:, perm].contiguous(), flip=False), full[:, perm]), "bits depend on the column's position"
    assert torch.equal(bn.solve_all(R, flip=False), full), "two identical calls differ"
    one = bn.solve_all(R[:, 3].contiguous(), flip=False)                    # (B, N) in, (B, N) out
    assert one.shape == (B, c["N"]) and torch.equal(one, full[:, 3])
    fl = bn.solve_all(R, flip=True)
    ref = full.clone(); ref[..., n + mi:] = -ref[..., n + mi:]
    assert torch.equal(fl, ref)
    out = torch.empty_like(R)
    assert bn.solve_all(R, flip=False, out=out) is out and torch.equal(out, full)
    bn.close()
    # the batch size and the problem's place in the batch
    b1, _ = _handle(shape, [c["qps"][2]])
    assert torch.equal(b1.solve_all(R[2:3].contiguous(), flip=False), full[2:3]), "bits depend on the batch size"
    b1.close()
    order = [3, 0, 4, 2, 1]
    bp, _ = _handle(shape, [c["qps"][b] for b in order])
    assert torch.equal(bp.solve_all(R[order].contiguous(), flip=False), full[order]), "bits depend on the problem's place"
    bp.close()


# ---- 2. the step's own system --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("condensed", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_the_steps_own_system(shape, condensed):
    c = _case(shape)
    bn, dz = _handle(shape, c["qps"], condensed=condensed)
    x = bn.solve_all(c["g"], flip=True)
    dz, x = dz.cpu().numpy(), x.cpu().numpy()
    err = np.linalg.norm(x - dz, axis=1) / np.linalg.norm(dz, axis=1)
    print("step's own system", shape, "condensed" if condensed else "full", "per problem:", err)
    assert err.max() <= 1e-12
    bn.close()


# ---- 3. mask -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("condensed", [False, True])
def test_mask_leaves_the_others_alone(condensed):
    import torch
    shape = SHAPES[2]
    c = _case(shape)
    bn, _ = _handle(shape, c["qps"], condensed=condensed)
    R = torch.from_numpy(c["R"][:, :17]).to(bn.device).contiguous()
    full = bn.solve_all(R)
    act = np.array([1, 0, 1, 1, 0], dtype=np.int32)
    out = torch.full_like(R, -7.25)
    bn.solve_all(R, active=act, out=out)
    on = torch.from_numpy(act.astype(bool)).to(bn.device)
    assert torch.equal(out[on], full[on])
    assert torch.equal(out[~on], torch.full_like(out[~on], -7.25))
    fresh = bn.solve_all(R, active=act, refine=1)
    assert bool(torch.isnan(fresh[~on]).all()) and not bool(torch.isnan(fresh[on]).any())
    bn.close()


# ---- 4. every problem against its own shifts; products ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2], SHAPES[3]])
def test_own_shifts_and_products(shape):
    import torch
    c = _case(shape)
    n, me, mi = shape
    delta = 1e-3 * (1.0 + np.arange(B))
    delta_c = 1e-4 * (1.0 + np.arange(B)) if me else np.zeros(B)
    bn, _ = _handle(shape, c["qps"], delta=delta, delta_c=delta_c)
    Hs = np.stack([_dense(q, n, me, mi, delta[b], delta_c[b]) for b, q in enumerate(c["qps"])])
    X = c["X"][:, :17]
    R = np.einsum("bij,bkj->bki", Hs, X)
    x = bn.solve_all(R, flip=False).cpu().numpy()
    res = np.einsum("bij,bkj->bki", Hs, x) - R
    r = float((np.linalg.norm(res, axis=-1) / np.linalg.norm(R, axis=-1)).max())
    print("own shifts", shape, "worst residual %.3e, worst error %.3e" % (r, _colerr(x, X)))
    assert r <= 1e-10 and _colerr(x, X) <= 1e-10
    for k in (1, 17):
        y = bn.kkt_matvec_all(torch.from_numpy(X[:, :k]).to(bn.device).contiguous())
        e = _colerr(y.cpu().numpy(), R[:, :k])
        print("products", shape, "k = %d: %.3e" % (k, e))
        assert e <= 1e-13
        if k == 17:
            assert torch.equal(bn.kkt_matvec_all(torch.from_numpy(X[:, 5]).to(bn.device).contiguous()), y[:, 5])
    bn.close()


# ---- 5. refinement in the condensed form -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[3]])
def test_refinement_condensed(shape):
    import torch
    from pyipm_amd.batched import BatchedNewton
    c = _case(shape)
    bn, _ = _handle(shape, c["qps"], condensed=True)
    R = torch.from_numpy(np.random.default_rng(5).standard_normal((B, 17, c["N"]))).to(bn.device)

    def berr(x):
        return (torch.linalg.norm(R - bn.kkt_matvec_all(x), dim=-1) / torch.linalg.norm(R, dim=-1)).cpu().numpy()

    e0, e2 = berr(bn.solve_all(R, flip=False, refine=0)), berr(bn.solve_all(R, flip=False, refine=2))
    print("refinement", shape, "backward error per column: refine=0 [%.3e, %.3e], refine=2 [%.3e, %.3e]"
          % (e0.min(), e0.max(), e2.min(), e2.max()))
    assert e2.max() <= BatchedNewton.condensed_tol
    assert (e2 <= e0).all()                                      # no worse than unrefined, column by column
    x2 = bn.solve_all(R, flip=True, refine=2).cpu().numpy()
    assert np.array_equal(x2, _flip(bn.solve_all(R, flip=False, refine=2).cpu().numpy(), shape[0], shape[2]))
    bn.close()


# ---- 5b. in place ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("condensed", [False, True])
def test_in_place_is_the_out_of_place_call(condensed):
    """x may BE rhs: the bits of the out-of-place call, unrefined and refined (the residuals of a refined in-place solve still
    see the right-hand sides); any other overlap of the two blocks is refused."""
    import ctypes
    import torch
    shape = SHAPES[2]
    c = _case(shape)
    N = c["N"]
    bn, _ = _handle(shape, c["qps"], condensed=condensed)
    R = torch.from_numpy(c["R"][:, :17]).to(bn.device).contiguous()
    keep = R.clone()
    for refine in (0, 2):
        ref = bn.solve_all(R, refine=refine)
        assert torch.equal(R, keep)
        X = R.clone()
        assert bn.solve_all(X, refine=refine, out=X) is X
        assert torch.equal(X, ref), "in place differs (refine = %d)" % refine
    act = np.array([0, 1, 1, 0, 1], dtype=np.int32)
    ref = bn.solve_all(R, refine=1, active=act)
    X = R.clone()
    bn.solve_all(X, refine=1, active=act, out=X)
    on = torch.from_numpy(act.astype(bool)).to(bn.device)
    assert torch.equal(X[on], ref[on]) and torch.equal(X[~on], R[~on])
    buf = torch.zeros(B * 17 * N + 8, dtype=torch.float64, device=bn.device)
    p0, p1 = ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(buf.data_ptr() + 64)
    assert bn.lib.pyipm_newton_solve_batched(bn.h, 17, p0, N, 17 * N, p1, N, 17 * N, None, 1, 0, 0) == -1     # shifted overlap
    assert bn.lib.pyipm_newton_solve_batched(bn.h, 17, p0, N, 17 * N, p0, N, 17 * N, None, 1, 0, 0) == 0
    bn.close()


# ---- 5c. host pointers, padded leading dimensions, a host mask -----------------------------------------------------------------------
@pytest.mark.parametrize("condensed", [False, True])
def test_host_pointers_padded_strides_and_host_mask(condensed):
    """The three entries with host memory: the bits of the device path; entries N .. ld - 1, the gaps between problems and
    the rows of inactive problems keep a sentinel."""
    import ctypes
    import torch
    shape = SHAPES[1]
    c = _case(shape)
    N, k, S = c["N"], 5, -3.5
    bn, _ = _handle(shape, c["qps"], condensed=condensed)
    lib, hp = bn.lib, lambda a: ctypes.c_void_p(a.ctypes.data)      # noqa: E731
    Rk = np.ascontiguousarray(c["R"][:, :k])
    ld_r, ld_x = N + 3, N + 1
    st_r, st_x = k * ld_r + 5, k * ld_x + 2
    rb = np.full(B * st_r, S)
    for b in range(B):
        for j in range(k):
            rb[b * st_r + j * ld_r: b * st_r + j * ld_r + N] = Rk[b, j]
    act = np.array([1, 0, 1, 1, 0], dtype=np.int32)
    for refine in (0, 1):
        ref = bn.solve_all(Rk, refine=refine).cpu().numpy()
        xb = np.full(B * st_x, S)
        rc = lib.pyipm_newton_solve_batched(bn.h, k, hp(rb), ld_r, st_r, hp(xb), ld_x, st_x, hp(act), 1, refine, 1)
        assert rc == 0
        seen = np.zeros(B * st_x, dtype=bool)
        for b in range(B):
            for j in range(k):
                o = b * st_x + j * ld_x
                if act[b]:
                    assert np.array_equal(xb[o:o + N], ref[b, j]), (refine, b, j)
                    seen[o:o + N] = True
        assert (xb[~seen] == S).all()
    Xk = np.ascontiguousarray(c["X"][:, :k])
    vb = np.full(B * st_r, S)
    for b in range(B):
        for j in range(k):
            vb[b * st_r + j * ld_r: b * st_r + j * ld_r + N] = Xk[b, j]
    ref = bn.kkt_matvec_all(Xk).cpu().numpy()
    yb = np.full(B * st_x, S)
    assert lib.pyipm_newton_kkt_matvec_batched(bn.h, k, hp(vb), ld_r, st_r, hp(yb), ld_x, st_x, 1) == 0
    seen = np.zeros(B * st_x, dtype=bool)
    for b in range(B):
        for j in range(k):
            o = b * st_x + j * ld_x
            assert np.array_equal(yb[o:o + N], ref[b, j])
            seen[o:o + N] = True
    assert (yb[~seen] == S).all()
    if not condensed:
        ref = bn.rcond_all().cpu().numpy()
        out = np.full((B, 4), S)
        assert lib.pyipm_newton_rcond_batched(bn.h, 0, 0, hp(act), hp(out), 1) == 0
        on = act.astype(bool)
        assert np.array_equal(out[on], ref[on]) and (out[~on] == S).all()
    bn.close()


# ---- 6. the call leaves the handle's state alone; argument checks --------------------------------------------------------------
@pytest.mark.parametrize("condensed", [False, True])
def test_non_interference(condensed):
    import torch
    shape = SHAPES[1]
    c = _case(shape)
    bn, dz = _handle(shape, c["qps"], condensed=condensed)
    be0, al0 = bn.backward_errors(dz).clone(), bn.step_lengths_all(0.995).clone()
    bn.solve_all(c["R"], refine=1)
    bn.kkt_matvec_all(c["X"])
    if not condensed:
        bn.rcond_all()
    assert torch.equal(bn.backward_errors(dz), be0) and torch.equal(bn.step_lengths_all(0.995), al0)
    dz2 = bn.step_each(MU, 0.0, 0.0)[0]
    assert torch.equal(dz2, dz)
    bn.close()


def test_argument_checks():
    import ctypes
    from pyipm_amd.newton import NewtonError
    shape = SHAPES[0]
    c = _case(shape)
    N = c["N"]
    bn, _ = _handle(shape, c["qps"], step=False)
    for call in (lambda: bn.solve_all(c["R"]), lambda: bn.kkt_matvec_all(c["X"]), lambda: bn.rcond_all()):
        with pytest.raises(NewtonError):                       # no step yet
            call()
    bn.step_each(MU, 0.0, 0.0)
    bn.solve_all(c["R"][:, :2])
    n, me, mi = shape
    bn.stage(*_args(c["qps"], n, me, mi), mu=MU)               # staged again: the kept factors belong to the step's blocks and vectors
    with pytest.raises(NewtonError):
        bn.solve_all(c["R"][:, :2])
    bn.step_each(MU, 0.0, 0.0)
    with pytest.raises(NewtonError):
        bn.solve_all(c["R"], refine=-1)
    with pytest.raises(NewtonError):
        bn.rcond_all(it_inv=-1)
    with pytest.raises(NewtonError):
        bn.solve_all(c["R"][:, :, :-1])
    x = bn.solve_all(c["R"][:, :2])
    p = ctypes.c_void_p(x.data_ptr())
    lib = bn.lib
    assert lib.pyipm_newton_solve_batched(bn.h, 0, None, 0, 0, None, 0, 0, None, 1, 0, 0) == 0          # k == 0
    assert lib.pyipm_newton_solve_batched(bn.h, 2, p, N - 1, 2 * N, p, N, 2 * N, None, 1, 0, 0) == -1   # ld < N
    assert lib.pyipm_newton_solve_batched(bn.h, -1, p, N, 2 * N, p, N, 2 * N, None, 1, 0, 0) == -1      # k < 0
    assert lib.pyipm_newton_solve_batched(bn.h, 2, None, N, 2 * N, p, N, 2 * N, None, 1, 0, 0) == -1    # NULL
    assert lib.pyipm_newton_kkt_matvec_batched(bn.h, 2, p, N, 2 * N, None, N, 2 * N, 0) == -1
    assert lib.pyipm_newton_rcond_batched(bn.h, 0, 0, None, None, 0) == -1
    bn.close()
    from pyipm_amd.newton import NewtonCore
    core = NewtonCore(*shape, device=0)                        # not a batched handle
    assert lib.pyipm_newton_solve_batched(core.h, 2, p, N, 2 * N, p, N, 2 * N, None, 1, 0, 0) == -1
    bc, _ = _handle(shape, c["qps"], condensed=True)
    with pytest.raises(NewtonError, match="condensed"):
        bc.rcond_all()
    bc.close()


# ---- 7. the condition estimate ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_condition_estimate(shape):
    c = _case(shape)
    bn, _ = _handle(shape, c["qps"])
    out = bn.rcond_all().cpu().numpy()
    assert out.shape == (B, 4) and len(bn.RCOND_KEYS) == 4
    for b in range(B):
        w = np.abs(np.linalg.eigvalsh(c["Hc"][b]))
        wmin, wmax = w.min(), w.max()
        print("rcond", shape, b, "est (%.4e, %.4e, %.4e) true (%.4e, %.4e, %.4e)" % (out[b, 0], out[b, 1], out[b, 2], wmin, wmax, wmin / wmax))
        assert out[b, 1] <= wmax * (1 + 1e-10)
        assert out[b, 0] >= wmin * (1 - 1e-8)
        assert 0.2 < out[b, 2] / (wmin / wmax) < 5
        assert out[b, 2] == out[b, 0] / out[b, 1]
        assert out[b, 3] > 0
    bn.close()


def _singular_batch():
    from pyipm_amd.batched import BatchedNewton
    n, me, mi, bad = 48, 8, 24, 2
    qps = [make_qp(n, me, mi, seed=100 + b) for b in range(B)]
    qps[bad]["Je"] = qps[bad]["Je"].copy()
    qps[bad]["Je"][:, 1] = qps[bad]["Je"][:, 0]                 # two identical constraint gradients: Hc is singular
    bn = BatchedNewton(n, me, mi)
    bn.stage(*_args(qps, n, me, mi), mu=0.05)
    _, st = bn.step_each(0.05, 0.0, 0.0)
    return bn, bad, [dict(x) for x in st]


def test_condition_estimate_separates_a_singular_member():
    """The singular member's estimate <= 1e-12, its neighbours' > 1e-8.  Its zero pivot is replaced by a static pivot of
    sqrt(eps) max|Hc| at factorisation, so inverse iteration with the kept factor alone finds w_min ~ 2e-8 (rcond 4.7e-9):
    the estimate has to come back to the unperturbed blocks (k_b_rc_fix_begin) to read the member as singular."""
    bn, bad, _ = _singular_batch()
    out = bn.rcond_all(active=[0, 1, 1, 1, 0]).cpu().numpy()
    print("separation: rcond estimates", out[:, 2], "w_min", out[:, 0], "static pivot", out[:, 3])
    assert np.isnan(out[[0, 4]]).all()                           # the mask restricts the work: their rows are not written
    assert out[1, 2] > 1e-8 and out[3, 2] > 1e-8
    assert out[bad, 2] <= 1e-12
    bn.close()


def test_condition_estimate_singular_member_by_the_static_pivot_rule():
    """The decision a single-system caller takes from the same four quantities (the rcond <= eps test of reghess where static
    pivots were placed: w_min <= 100 static_pivot) singles the singular member out of its batch."""
    bn, bad, st = _singular_batch()
    out = bn.rcond_all().cpu().numpy()
    hit = [bool(st[b]["n_zero"] > 0 and out[b, 0] <= 100.0 * out[b, 3]) or bool(out[b, 2] <= EPS) for b in range(B)]
    print("static-pivot rule:", hit, "n_zero", [x["n_zero"] for x in st], "w_min", out[:, 0], "static pivot", out[:, 3])
    assert hit == [b == bad for b in range(B)]
    bn.close()
