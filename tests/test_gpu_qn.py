"""The quasi-Newton KKT operator of an L-BFGS direction (include/pyipm_newton.h, pyipm_qn_*): product, kept-state solve,
backward error and refinement, against the operator built here in NumPy from the same inputs,

    K = [ B_k   0      J        ]      B_k = zeta I - W inv(M) W',  W = [zeta S, Y],  M = [[zeta SS, L], [L', -D]]
        [ 0     Sigma  [0 | -I] ]      Sigma = lda_i / (s + eps),  J = [Je | Ji]
        [ J'    [0;-I]  0       ]

block by block (a dense N x N array would only add zeros), with every product and residual in numpy.longdouble.

Figures measured on the MI355X are printed before each assertion; DESIGN.md section 7d records them."""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(float).eps)
LD = np.longdouble
# |out - K v|_2 <= C_OP * eps * | |K| |v| |_2.  The largest ratio measured on the MI355X over SHAPES and both values of flip is
# 0.217, at (96, 24, 40, 5); the constant is 8 x that.  It depends on the order of the sums over n and p.
C_OP = 1.74

SHAPES = [(200, 30, 90, 8, 8), (96, 24, 40, 5, 5), (130, 0, 129, 3, 3), (64, 20, 0, 2, 2), (300, 64, 64, 0, 1), (5, 1, 2, 3, 3),
          (777, 65, 191, 31, 32),
          (8300, 100, 200, 4, 4)]       # p_pad = 384 > 256 and n > 8192: two column blocks, several row splits, six wave partials
IDS = ["n%d_me%d_mi%d_m%d" % s[:4] for s in SHAPES]
# the cases of the CPU probe behind DESIGN.md section 7d: (n, me, mi, m, decades of Sigma either side of 1, seed)
REFINE_CASES = [(600, 40, 200, 4, 8, 99), (200, 30, 90, 8, 6, 2), (130, 0, 129, 3, 6, 1), (96, 24, 40, 5, 6, 3)]


def _storage(n, m, rng, memory):
    from oracle import lbfgs_oracle as lo
    zeta, S, Y, SS, L, D, fail = lo.lbfgs_init(n)
    Mq = rng.standard_normal((n, 32)) / np.sqrt(32.0)
    x_old = rng.standard_normal(n)
    for _ in range(m):
        x_new = x_old + rng.standard_normal(n) / np.sqrt(n)
        hv = lambda v: Mq @ (Mq.T @ v) + 0.5 * v           # noqa: E731
        zeta, S, Y, SS, L, D, fail = lo.lbfgs_update(x_old, x_new, -hv(x_old), -hv(x_new), zeta, S, Y, SS, L, D, fail,
                                                     n, True, memory, EPS)
        x_old = x_new
    return zeta, S, Y, SS, L, D


def _ld_solve(A, B):
    """inv(A) B by Gaussian elimination with partial pivoting in longdouble (numpy.linalg has no longdouble)."""
    A, B = np.array(A, dtype=LD), np.array(B, dtype=LD).reshape(A.shape[0], -1)
    k = A.shape[0]
    for c in range(k):
        piv = c + int(np.argmax(np.abs(A[c:, c])))
        A[[c, piv]], B[[c, piv]] = A[[piv, c]], B[[piv, c]]
        f = A[c + 1:, c] / A[c, c]
        A[c + 1:] -= np.outer(f, A[c])
        B[c + 1:] -= np.outer(f, B[c])
    for c in range(k - 1, -1, -1):
        B[c] = (B[c] - A[c, c + 1:] @ B[c + 1:]) / A[c, c]
    return B


class Operator(object):
    """K of one direction, block by block in longdouble."""

    def __init__(self, n, me, mi, zeta, S, Y, SS, L, D, J, s, lda):
        self.n, self.me, self.mi, self.zeta = n, me, mi, LD(zeta)
        self.J = J.astype(LD)
        self.sig = (lda[me:] / (s + EPS)).astype(LD) if mi else np.zeros(0, dtype=LD)
        self.m = S.shape[1]
        if self.m:
            self.W = np.concatenate([zeta * S, Y], axis=1).astype(LD)
            M = np.block([[zeta * SS, L], [L.T, -D]])
            self.MinvWT = _ld_solve(M, self.W.T)                                # 2m x n

    def apply(self, v):
        n, me, mi = self.n, self.me, self.mi
        v = np.asarray(v, dtype=LD)
        vx, vs, vl = v[:n], v[n:n + mi], v[n + mi:]
        ox = self.zeta * vx + self.J @ vl
        if self.m:
            ox = ox - self.W @ (self.MinvWT @ vx)
        ol = self.J.T @ vx
        ol[me:] -= vs
        return np.concatenate([ox, self.sig * vs - vl[me:], ol])

    def abs_apply(self, v):
        """|K| |v| in float64 (a bound needs no more)."""
        n, me, mi = self.n, self.me, self.mi
        a = np.abs(np.asarray(v, dtype=float))
        ax, as_, al = a[:n], a[n:n + mi], a[n + mi:]
        Ja = np.abs(self.J).astype(float)
        if getattr(self, "absBk", None) is None:           # (n x n, formed once)
            Bk = float(self.zeta) * np.eye(n)
            if self.m:
                Bk -= self.W.astype(float) @ self.MinvWT.astype(float)
            self.absBk = np.abs(Bk, out=Bk)
        ol = Ja.T @ ax
        ol[me:] += as_
        return np.concatenate([self.absBk @ ax + Ja @ al, self.sig.astype(float) * as_ + al[me:], ol])

    def berr(self, x, g):
        r = np.asarray(g, dtype=LD) - self.apply(x)
        return float(np.linalg.norm(r) / np.linalg.norm(np.asarray(g, dtype=LD)))


class Case(object):
    pass


def _make(n, me, mi, m, cap, spread=0, seed=None, qp_seed=3, dup=False):
    """Inputs, the operator and a handle that has run the direction.  Built once per argument list and shared (nothing below
    writes into a case's arrays)."""
    from pyipm_amd.lbfgs import LbfgsCore
    from pyipm_amd.problems import make_qp
    c = Case()
    rng = np.random.default_rng(n + 7 * me + 13 * mi + m if seed is None else seed)
    qp = make_qp(n, me, mi, qp_seed)
    c.n, c.me, c.mi, c.m, c.N = n, me, mi, m, n + 2 * mi + me
    c.store = _storage(n, m, rng, max(m, 1))
    assert c.store[1].shape[1] == m
    c.s = rng.uniform(0.5, 2.0, mi)
    if spread:
        sig = np.exp(rng.uniform(np.log(10.0 ** -spread), np.log(10.0 ** spread), mi))
        c.lda = np.concatenate([qp["lam"][:me], sig * c.s])
    else:
        c.lda = qp["lam"]
        c.s = qp["s"] if mi else c.s
    c.g = rng.standard_normal(c.N)
    c.Je = qp["Je"].copy() if me else None
    c.Ji = qp["Ji"] if mi else None
    if dup:                                                # a duplicated equality gradient: G_ee is singular, and so is K -- a
        c.Je[:, -1] = c.Je[:, 0]                           # residual means something for a consistent right-hand side only
        c.g[n + mi + me - 1] = c.g[n + mi]
    c.J = np.concatenate([a for a in (c.Je, c.Ji) if a is not None], axis=1)
    c.K = Operator(n, me, mi, *c.store, c.J, c.s, c.lda)
    c.rng = rng
    c.core = LbfgsCore(n, me, mi, cap, device=0, nb=128 if n < 1000 else 256)
    c.core.stage_jacobian(c.Je, c.Ji)
    c.direct = lambda g=None, **kw: c.core.direction(c.g if g is None else g, c.s, c.lda, *c.store, reg=1e-12, **kw)
    c.dz, c.st = c.direct()
    c.dz = c.dz.cpu().numpy()
    return c


@functools.lru_cache(maxsize=None)
def _shape_case(shape):
    n, me, mi, m, cap = shape
    return _make(n, me, mi, m, cap)


@functools.lru_cache(maxsize=None)
def _refine_case(case):
    n, me, mi, m, spread, seed = case
    return _make(n, me, mi, m, max(m, 1), spread=spread, seed=seed, qp_seed=8)


def _flipped(c, v):
    w = np.array(v, dtype=float)
    w[c.n + c.mi:] = -w[c.n + c.mi:]
    return w


@pytest.mark.parametrize("flip", [False, True], ids=["raw", "flip"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_operator_against_the_dense_blocks(shape, flip):
    """out = K v for a random v (not a solution), within the rounding bound of the sums; two calls give the same bits."""
    c = _shape_case(shape)
    v = np.random.default_rng(17).standard_normal(c.N)
    arg = _flipped(c, v) if flip else v
    out = c.core.matvec(arg, flip=flip).cpu().numpy()
    again = c.core.matvec(arg, flip=flip).cpu().numpy()
    ref = c.K.apply(v)
    err = float(np.linalg.norm(out.astype(LD) - ref))
    scale = float(np.linalg.norm(c.K.abs_apply(v)))
    print("operator %s flip=%d: |out - K v| = %.3e = %.3f eps | |K||v| |" % (shape[:4], flip, err, err / (EPS * scale)))
    np.testing.assert_array_equal(out, again)
    assert err <= C_OP * EPS * scale


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_kept_state_solve_reproduces_the_direction_bit_for_bit(shape):
    """solve(g) after direction(g): the same bits, raw and flipped; no Gram launch is added by any of the new calls; a
    direction after them returns the bits it returned before."""
    c = _shape_case(shape)
    launches = c.core.last_timings()["gram_launches"]
    np.testing.assert_array_equal(c.core.solve(c.g).cpu().numpy(), c.dz)
    np.testing.assert_array_equal(c.core.solve(c.g, flip=True).cpu().numpy(), _flipped(c, c.dz))
    c.core.matvec(c.dz)
    c.core.refine(c.dz, refine=-1)
    dz2, _ = c.direct()
    assert c.core.last_timings()["gram_launches"] == launches
    np.testing.assert_array_equal(dz2.cpu().numpy(), c.dz)


@pytest.mark.parametrize("shape", SHAPES[:7], ids=IDS[:7])
def test_kept_state_solve_of_a_fresh_right_hand_side_matches_the_oracle(shape):
    """solve(rhs2) for another right-hand side against the oracle's direction for it (the well-conditioned shapes)."""
    from oracle import lbfgs_oracle as lo
    c = _shape_case(shape)
    rhs2 = np.random.default_rng(23).standard_normal(c.N)
    ref = lo.direction(rhs2, *c.store, Je=c.Je, Ji=c.Ji, s=c.s, lda=c.lda, reg=1e-12)
    got = c.core.solve(rhs2).cpu().numpy()
    rel = float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
    print("solve(rhs2) %s: rel. difference to the oracle %.3e" % (shape[:4], rel))
    assert rel <= 1e-9


@pytest.mark.parametrize("case", REFINE_CASES, ids=["n%d_me%d_mi%d_m%d_sig1e%d" % k[:5] for k in REFINE_CASES])
def test_adaptive_refinement_recovers_the_backward_error(case):
    c = _refine_case(case)
    b0 = c.K.berr(c.dz, c.g)
    dz, info = c.core.refine(c.dz, refine=-1)
    dz = dz.cpu().numpy()
    b1 = c.K.berr(dz, c.g)
    print("refine %s: test-side berr %.3e -> %.3e; library %s" % (case[:5], b0, b1, info))
    assert info == c.core.refine_info()
    assert info["converged"] and info["berr"] <= 1e-14 and 1 <= info["steps"] <= 3
    assert b1 <= 1e-13
    assert 0.5 * b0 <= info["berr0"] <= 2.0 * b0
    if case == REFINE_CASES[0]:
        assert b0 > 1e-11                                  # a gain, not a no-op (the CPU probe: 1.2e-9)
    # flipped in, flipped out: the same bits
    dzf, _ = c.core.refine(_flipped(c, c.dz), refine=-1, flip=True)
    np.testing.assert_array_equal(dzf.cpu().numpy(), _flipped(c, dz))
    # an explicit right-hand side equal to g: the same bits as rhs = None
    dzg, _ = c.core.refine(c.dz, rhs=c.g, refine=-1)
    np.testing.assert_array_equal(dzg.cpu().numpy(), dz)


def test_fixed_count_measure_only_and_the_direction_keyword():
    c = _refine_case(REFINE_CASES[1])
    dz2, info = c.core.refine(c.dz, refine=2)
    assert info["steps"] == 2 and info["berr0"] == -1.0 and info["berr"] == -1.0
    assert c.K.berr(dz2.cpu().numpy(), c.g) <= 1e-13
    dz0, info = c.core.refine(c.dz, refine=0)
    np.testing.assert_array_equal(dz0.cpu().numpy(), c.dz)
    assert info["steps"] == 0 and info["berr0"] == info["berr"] and 0.5 * c.K.berr(c.dz, c.g) <= info["berr"] <= 2.0 * c.K.berr(c.dz, c.g)
    # direction(..., refine=-1) = direction, then refine; refine=0 is the direction as it was
    ref, _ = c.core.refine(c.dz, refine=-1)
    got, st = c.direct(refine=-1)
    np.testing.assert_array_equal(got.cpu().numpy(), ref.cpu().numpy())
    assert c.core.refine_info()["converged"]
    plain, _ = c.direct(refine=0)
    np.testing.assert_array_equal(plain.cpu().numpy(), c.dz)
    # the options are the Newton handle's, forwarded: a target nobody meets ends on the budget or on stagnation, not converged
    c.core.set_option("refine_target", 1e-30)
    c.core.set_option("refine_max", 1)
    _, info = c.core.refine(c.dz, refine=-1)
    assert not info["converged"] and info["steps"] <= 1
    c.core.set_option("refine_target", 1e-14)
    c.core.set_option("refine_max", 8)


def test_regularised_factor_is_only_the_preconditioner():
    """A duplicated equality column: the direction regularises G_ee, K stays unregularised.  The refined direction is finite and
    no worse against K than the unrefined one; convergence is reported either way."""
    c = _make(96, 24, 40, 5, 5, dup=True, qp_seed=4)
    assert c.st["regularised"] == 1
    b0 = c.K.berr(c.dz, c.g)
    dz, info = c.core.refine(c.dz, refine=-1)
    dz = dz.cpu().numpy()
    b1 = c.K.berr(dz, c.g)
    print("regularised: test-side berr %.3e -> %.3e; library %s" % (b0, b1, info))
    assert np.all(np.isfinite(dz))
    assert b1 <= b0
    assert info["converged"] in (False, True) and info["steps"] >= 0
    c.core.close()


def test_errors_are_codes_with_a_message():
    from pyipm_amd.lbfgs import ALLREDUCE_FN, LbfgsCore
    from pyipm_amd.newton import MEM_DEVICE
    import torch
    c = _make(96, 24, 40, 5, 5, qp_seed=4)
    lib = c.core.lib
    buf = torch.zeros(c.N, dtype=torch.float64, device="cuda:0")
    p = ctypes.c_void_p(buf.data_ptr())
    info = (ctypes.c_double * 4)()

    def refused(core, word):
        for rc in (lib.pyipm_qn_matvec(core.h, p, 0, MEM_DEVICE, p), lib.pyipm_qn_solve(core.h, p, p, 0, MEM_DEVICE),
                   lib.pyipm_qn_refine(core.h, None, p, 0, -1, MEM_DEVICE)):
            assert rc == -1 and word in lib.pyipm_lbfgs_last_error(core.h).decode()
        assert lib.pyipm_qn_info(core.h, info) == 0

    fresh = LbfgsCore(96, 24, 40, 5, device=0)
    fresh.stage_jacobian(c.Je, c.Ji)
    refused(fresh, "no direction")                         # before any direction
    fresh.close()
    c.core.stage_jacobian(c.Je, c.Ji)
    refused(c.core, "no direction")                        # staged again, no new direction
    dz, _ = c.direct()
    np.testing.assert_array_equal(dz.cpu().numpy(), c.dz)  # ... and the handle works on
    assert c.core.refine(dz, refine=0)[1]["berr"] >= 0.0
    # an all-reduce callback (here: one rank, nothing to add) makes the handle a row-sharded one
    cb = ALLREDUCE_FN(lambda user, ptr, count, stream: 0)
    assert lib.pyipm_lbfgs_set_allreduce(c.core.h, ctypes.cast(cb, ctypes.c_void_p), None) == 0
    c.direct()
    refused(c.core, "row-sharded")
    assert lib.pyipm_lbfgs_set_allreduce(c.core.h, None, None) == 0
    c.core.close()
    # no constraints: an explicit formula, no system
    rng = np.random.default_rng(5)
    unc = LbfgsCore(40, 0, 0, 3, device=0)
    from oracle import lbfgs_oracle as lo
    zeta, S, Y, SS, L, D, _ = lo.lbfgs_init(40)
    unc.direction(rng.standard_normal(40), None, None, zeta, S, Y, SS, L, D)
    buf40 = ctypes.c_void_p(buf.data_ptr())
    assert lib.pyipm_qn_matvec(unc.h, buf40, 0, MEM_DEVICE, buf40) == -1
    assert "no constraints" in lib.pyipm_lbfgs_last_error(unc.h).decode()
    with pytest.raises(Exception):
        unc.matvec(np.zeros(40))
    unc.direction(rng.standard_normal(40), None, None, zeta, S, Y, SS, L, D, refine=-1)      # (ignored where there is no system)
    unc.close()


@pytest.mark.parametrize("k", [2, 7])
def test_ipm_with_refined_directions_ends_where_it_ended(k):
    from pyipm_amd.ipm import IPM
    from pyipm_amd.problems import example_problem, unit_test_x0
    p = example_problem(k)

    def run(**kw):
        ipm = IPM(x0=unit_test_x0()[k], f=p["f"], df=p["df"], ce=p["ce"], dce=p["dce"], ci=p["ci"], dci=p["dci"],
                  lbfgs=4, Ftol=1.0e-8, verbosity=-1, device=0, **kw)
        with np.errstate(all="ignore"):
            x = ipm.solve()[0]
        return ipm, x

    plain, x0 = run()
    refined, x1 = run(lbfgs_refine=-1)
    assert plain.backend.last_refine_info is None
    if refined.neq or refined.nineq:
        assert set(refined.backend.last_refine_info) == {"steps", "berr0", "berr", "converged"}
    assert refined.signal == plain.signal
    np.testing.assert_allclose(x1, x0, rtol=1e-5, atol=1e-6)


def test_qp_loop_with_refined_directions_ends_where_it_ended():
    from pyipm_amd.problems import make_qp
    from pyipm_amd.qp import QPDeviceIPM
    n, me, mi, seed = 24, 8, 16, 0
    qp = make_qp(n, me, mi, seed)

    def run(**kw):
        q = QPDeviceIPM(qp["Q"], qp["c"], A=qp["A"], b=qp["b"], G=qp["G"], h=qp["h"], verbosity=-1, lbfgs=4, niter=20, miter=30,
                        resident_pairs=True, **kw)
        return q, q.solve()[0].cpu().numpy()

    plain, x0 = run()
    refined, x1 = run(lbfgs_refine=-1)
    assert plain.last_refine_info is None and set(refined.last_refine_info) == {"steps", "berr0", "berr", "converged"}
    assert refined.signal == plain.signal
    np.testing.assert_allclose(x1, x0, rtol=1e-5, atol=1e-6)
