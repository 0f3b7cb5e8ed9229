"""Simple bounds of the L-BFGS direction as structure (include/pyipm_newton.h, pyipm_lbfgs_bounded_*; LbfgsCore(bounds=...)).

The yardsticks are code of the parent commit: the oracle (oracle/lbfgs_oracle.direction) and the plain handle, both fed the
explicit columns +-e_k of the bounds behind the general inequalities.  The judge is the dense system

    K dz = g ,  K = [[B_k, 0, J], [0, Sigma, [0 | -I]], [J', [0; -I], 0]] ,  J = [Je | Ji_general | +-e_var[j]]

applied block by block in numpy.longdouble (tests/test_gpu_qn.Operator for the general columns, the bound columns by index:
the same K, without mb dense columns of zeros).  Inputs as tests/test_gpu_qn.py builds them: make_qp, the storage from the
oracle's lbfgs_update, Sigma spread over 1e-6 .. 1e6.  Figures are printed before each assertion; DESIGN.md section 7d has them.

Every workspace is NaN-poisoned (tests/conftest.py).  The scaled operand's padding -- rows n .. n_pad-1, which the Gram
launch's K loop reads, and columns p .. p_pad-1, which are rows of the Gram matrix -- has no accessor: a NaN left there reaches
every entry of G, so the finite and accurate directions below at n < n_pad and p < p_pad are the check that it is zero."""
import contextlib
import ctypes
import functools

import numpy as np
import pytest

from test_gpu_qn import EPS, LD, Operator, _storage

pytestmark = pytest.mark.gpu


def _box(n):
    return np.concatenate([np.arange(n), np.arange(n)]), np.concatenate([np.ones(n), -np.ones(n)])


def _some(n, count, seed):
    rng = np.random.default_rng(seed)
    return rng.permutation(n)[:count], rng.choice([-1.0, 1.0], count)


# name -> (n, me, mg, m, max_pairs, (var, sign))
SHAPES = {
    "n1_lower": (1, 0, 0, 0, 1, (np.array([0]), np.array([1.0]))),
    "n5_mixed": (5, 1, 2, 3, 3, (np.array([0, 4, 1, 3, 4, 0]), np.array([1.0, 1.0, 1.0, -1.0, 1.0, -1.0]))),
    "n96_box": (96, 24, 40, 5, 5, _box(96)),
    "n130_bounds_only": (130, 0, 0, 3, 3, _box(130)),
    "n130_two_tiles": (130, 0, 129, 3, 3, _some(130, 40, 5)),
    "n200_upper": (200, 30, 0, 8, 8, (np.arange(200), -np.ones(200))),
    "n8300_9000": (8300, 100, 200, 4, 4, (np.concatenate([np.arange(8300), np.arange(700)]),
                                          np.concatenate([np.ones(8300), -np.ones(700)]))),
    "n96_box_m0": (96, 24, 40, 0, 1, _box(96)),
    "n96_box_m31": (96, 24, 40, 31, 32, _box(96)),
}


class Case(object):
    pass


def _unflip(dz, c, flip):
    dz = np.array(dz, dtype=float)
    if flip:
        dz[c.n + c.mi:] *= -1.0
    return dz


def _inputs(name, dup=False, active=None):
    return _inputs_cached(name, dup, active)


def _yardsticks(name, dup=False, active=None):
    return _yardsticks_cached(name, dup, active)


@functools.lru_cache(maxsize=None)
def _inputs_cached(name, dup, active):
    """The inputs of one shape and its operator: arrays only, built once and shared (nothing below writes into them).  Handles
    are made and closed per test (_handle)."""
    from pyipm_amd.problems import make_qp
    n, me, mg, m, cap, (var, sign) = SHAPES[name]
    c = Case()
    c.var, c.sign = np.asarray(var, dtype=np.int64), np.asarray(sign, dtype=float)
    mb = c.var.shape[0]
    c.n, c.me, c.mg, c.mb, c.m, c.cap, c.mi = n, me, mg, mb, m, cap, mg + mb
    c.N = n + 2 * c.mi + me
    rng = np.random.default_rng(n + 7 * me + 13 * mg + m)
    # (dup: a seed at which the oracle's own rank test on the duplicated equality block, eigh's rcond <= eps, fires -- 3e-17 at
    #  seed 7; at seed 3 eigh returns 2.8e-16, the oracle does not regularise and its LU meets an exactly singular matrix)
    qp = make_qp(n, me, mg, 7 if dup else 3) if me + mg else None
    c.store = _storage(n, m, rng, max(m, 1))
    assert c.store[1].shape[1] == m
    c.s = rng.uniform(0.5, 2.0, c.mi)
    sig = np.exp(rng.uniform(np.log(1e-6), np.log(1e6), c.mi))
    c.lda = np.concatenate([qp["lam"][:me] if me else np.zeros(0), sig * c.s])
    if active is not None:                                 # Sigma_j = 1e12: the bound is all but active
        c.s[mg + active] = 1e-12 * c.lda[me + mg + active]
    c.g = rng.standard_normal(c.N)
    c.Je = qp["Je"].copy() if me else None
    c.Jg = qp["Ji"] if mg else None
    if dup:                                                # a duplicated equality gradient and a consistent right-hand side
        c.Je[:, -1] = c.Je[:, 0]
        c.g[n + c.mi + me - 1] = c.g[n + c.mi]
    general = [a for a in (c.Je, c.Jg) if a is not None]
    c.Kg = Operator(n, me, mg, *c.store, np.concatenate(general, axis=1) if general else np.zeros((n, 0)),
                    c.s[:mg], c.lda[:me + mg])
    c.sigb = (c.lda[me + mg:] / (c.s[mg:] + EPS)).astype(LD)
    return c


@contextlib.contextmanager
def _handle(c):
    """(core, direct): a bounded handle of the case with its Jacobians staged, closed when the test is done."""
    from pyipm_amd.lbfgs import LbfgsCore
    core = LbfgsCore(c.n, c.me, c.mg, c.cap, device=0, nb=128 if c.n < 1000 else 256, bounds=(c.var, c.sign))
    try:
        core.stage_jacobian(c.Je, c.Jg)
        yield core, lambda **kw: core.direction(c.g, c.s, c.lda, *c.store, reg=1e-12, **kw)
    finally:
        core.close()


@functools.lru_cache(maxsize=None)
def _yardsticks_cached(name, dup, active):
    """(oracle, plain handle): the RAW directions of the parent commit's two paths, fed the explicit columns +-e_k.  Computed once
    per case (the oracle forms dense matrices of order n + mi: some 40 s of host time at n = 8300, mb = 9000, paid once)."""
    from oracle import lbfgs_oracle as lo
    from pyipm_amd.lbfgs import LbfgsCore
    c = _inputs(name, dup, active)
    E = np.zeros((c.n, c.mb))
    E[c.var, np.arange(c.mb)] = c.sign
    Ji = np.concatenate([c.Jg, E], axis=1) if c.mg else E
    dz_oracle = lo.direction(c.g, *c.store, Je=c.Je, Ji=Ji, s=c.s, lda=c.lda, reg=1e-12)
    core = LbfgsCore(c.n, c.me, c.mi, c.cap, device=0, nb=128 if c.n < 1000 else 256)
    core.stage_jacobian(c.Je, Ji)
    dz = core.direction(c.g, c.s, c.lda, *c.store, reg=1e-12)[0].cpu().numpy()
    core.close()
    return dz_oracle, dz


def _berr(c, dz):
    """|g - K dz|_2 / |g|_2 in longdouble, K with the explicit bound columns (dz RAW)."""
    n, me, mg, mb, mi = c.n, c.me, c.mg, c.mb, c.mi
    v = np.asarray(dz, dtype=LD)
    vx, vs, vle, vli = v[:n], v[n:n + mi], v[n + mi:n + mi + me], v[n + mi + me:]
    red = c.Kg.apply(np.concatenate([vx, vs[:mg], vle, vli[:mg]]))
    ox = red[:n].copy()
    np.add.at(ox, c.var, c.sign.astype(LD) * vli[mg:])
    out = np.concatenate([ox, red[n:n + mg], c.sigb * vs[mg:] - vli[mg:], red[n + mg:],
                          c.sign.astype(LD) * vx[c.var] - vs[mg:]])
    g = c.g.astype(LD)
    return float(np.linalg.norm(g - out) / np.linalg.norm(g))


def _check_against_the_dense_system(c, dz, what, key):
    """The two assertions of the dense-system check, with the figures printed first.  key: the arguments of the case."""
    dz_oracle, dz_explicit = _yardsticks(*key)
    be, bo, bb = _berr(c, dz_explicit), _berr(c, dz_oracle), _berr(c, dz)
    nrm = np.linalg.norm(dz_explicit)
    spread = max(np.linalg.norm(dz_explicit - dz_oracle), 1e-13 * nrm)
    dist = np.linalg.norm(dz - dz_explicit)
    print("%s: berr bounded %.3e explicit %.3e oracle %.3e ratio %.3f | |dz - dz_explicit| %.3e, |explicit - oracle| (floored) "
          "%.3e ratio %.3f" % (what, bb, be, bo, bb / max(be, bo), dist, spread, dist / spread))
    assert np.all(np.isfinite(dz))
    assert bb <= 8.0 * max(be, bo)
    assert dist <= 8.0 * spread


@pytest.mark.parametrize("flip", [False, True], ids=["raw", "flip"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_direction_against_the_dense_system(name, flip):
    c = _inputs(name)
    with _handle(c) as (core, direct):
        dz, st = direct(flip=flip)
        launches = core.last_timings()["gram_launches"]
    dz = _unflip(dz.cpu().numpy(), c, flip)
    _check_against_the_dense_system(c, dz, "%s flip=%d" % (name, flip), (name,))
    assert st["m"] == c.m
    if c.me + c.mg == 0:                                   # no Gram matrix, no factorisation
        assert (st["n_factor"], st["regularised"], st["n_neg"], st["n_zero"], st["d_min"], st["d_max"]) == (0, 0, 0, 0, 0.0, 0.0)
        assert launches == 0
    else:
        assert st["n_factor"] == 1 and st["regularised"] == 0 and launches == 1


def test_an_active_bound():
    """Sigma_j = 1e12 on one lower bound.  Its row of K is sigma_j dx_k - ds_j = g_li,j and ds_j = (g_s,j + dlambda_j) / Sigma_j
    vanishes, so dx_k = sigma_j g_li,j to 1e-9 (the sign the system K dz = g of include/pyipm_newton.h gives)."""
    j = 7
    c = _inputs("n96_box", active=j)
    with _handle(c) as (_, direct):
        dz = direct()[0].cpu().numpy()
    k, sg, gl = int(c.var[j]), c.sign[j], c.g[c.n + c.mi + c.me + c.mg + j]
    print("active bound: dx_k %.15e sigma g_li %.15e difference %.3e" % (dz[k], sg * gl, abs(dz[k] - sg * gl)))
    assert abs(dz[k] - sg * gl) <= 1e-9 * (1.0 + abs(gl))
    _check_against_the_dense_system(c, dz, "active bound", ("n96_box", False, j))


def test_a_duplicated_equality_column_under_the_bounds():
    c = _inputs("n96_box", dup=True)
    with _handle(c) as (_, direct):
        dz, st = direct()
    assert st["regularised"] == 1 and st["n_factor"] == 2
    _check_against_the_dense_system(c, dz.cpu().numpy(), "duplicated equality", ("n96_box", True))


@pytest.mark.parametrize("name", ["n96_box", "n8300_9000"])
def test_no_bounds_is_the_plain_handle_to_the_bit(name):
    from pyipm_amd.lbfgs import LbfgsCore
    c = _inputs(name)
    n, me, mg = c.n, c.me, c.mg
    s, lda = c.s[:mg], c.lda[:me + mg]
    g = np.concatenate([c.g[:n + mg], c.g[n + c.mi:n + c.mi + me + mg]])
    out = []
    for bounds in (None, (np.zeros(0, dtype=np.int64), np.zeros(0))):
        core = LbfgsCore(n, me, mg, c.cap, device=0, nb=128 if n < 1000 else 256, bounds=bounds)
        core.stage_jacobian(c.Je, c.Jg)
        res = []
        for rhs in (g, g[::-1].copy()):                    # the second direction reuses J'J
            dz, st = core.direction(rhs, s, lda, *c.store, reg=1e-12, flip=True)
            res.append((dz.cpu().numpy(), st, core.last_timings()["gram_launches"]))
        out.append(res)
        core.close()
    for (dz_a, st_a, n_a), (dz_b, st_b, n_b) in zip(*out):
        assert np.array_equal(dz_a, dz_b) and st_a == st_b
        assert n_a == n_b == 1


def test_equal_calls_give_equal_bits_and_every_direction_launches_the_gram():
    c = _inputs("n96_box")
    with _handle(c) as (core, direct):
        a, sa = direct()
        n0 = core.last_timings()["gram_launches"]
        b, sb = direct()
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy()) and sa == sb
        assert n0 == 1 and core.last_timings()["gram_launches"] == 2
        core.stage_jacobian_columns(3, c.Je[:, 3:9])       # accepted; copies; nothing saved
        d, _ = direct()
        assert np.array_equal(a.cpu().numpy(), d.cpu().numpy())
        assert core.last_timings()["gram_launches"] == 3


def test_restaging_permuted_bounds_permutes_the_bound_rows_alone():
    c = _inputs("n130_two_tiles")                          # 40 bounds on 40 different variables
    n, me, mg, mb, mi = c.n, c.me, c.mg, c.mb, c.mi
    perm = np.random.default_rng(11).permutation(mb)
    rows_s, rows_l = n + mg + np.arange(mb), n + mi + me + mg + np.arange(mb)
    g, s, lda = c.g.copy(), c.s.copy(), c.lda.copy()
    g[rows_s], g[rows_l] = c.g[rows_s[perm]], c.g[rows_l[perm]]
    s[mg:], lda[me + mg:] = c.s[mg:][perm], c.lda[me + mg:][perm]
    with _handle(c) as (core, direct):
        a = direct()[0].cpu().numpy()
        core.stage_bounds(c.var[perm], c.sign[perm])
        b = core.direction(g, s, lda, *c.store, reg=1e-12)[0].cpu().numpy()
        core.stage_bounds(c.var, c.sign)
        again = direct()[0].cpu().numpy()
    want = a.copy()
    want[rows_s], want[rows_l] = a[rows_s[perm]], a[rows_l[perm]]
    assert np.array_equal(b, want)
    assert np.array_equal(again, a)


def test_what_a_bounded_handle_refuses():
    from pyipm_amd.newton import NewtonError
    c = _inputs("n96_box")
    with _handle(c) as (core, direct):
        a = direct()[0].cpu().numpy()
        v = np.ones(core.N)
        for call in (lambda: core.matvec(v), lambda: core.solve(v), lambda: core.refine(v),
                     lambda: core.solve_many(np.ones((core.N, 2))), lambda: core.matvec_many(np.ones((core.N, 2))),
                     lambda: core._ck(core.lib.pyipm_lbfgs_set_allreduce(core.h, None, None)),
                     lambda: direct(refine=1)):
            with pytest.raises(NewtonError, match="bounded") as e:
                call()
            assert "bad argument" in str(e.value)
        assert np.array_equal(direct()[0].cpu().numpy(), a)
        # a bad index or sign, too many bounds on one variable: refused, and the bounds staged before still hold
        j = np.arange(c.mb)
        for var, sign in ((np.where(j == 5, c.n, c.var), c.sign), (np.where(j == 5, -1, c.var), c.sign),
                          (c.var, np.where(j == 9, 0.5, c.sign)), (c.var, np.where(j == 9, np.nan, c.sign)),
                          (np.where(j < 65, 3, c.var), c.sign)):
            with pytest.raises(NewtonError, match="bounded_stage"):
                core.stage_bounds(var, sign)
            assert np.array_equal(direct()[0].cpu().numpy(), a)
        rc = core.lib.pyipm_lbfgs_bounded_stage(core.h, None, None)
        assert rc == -1 and b"null" in core.lib.pyipm_lbfgs_last_error(core.h)
        assert np.array_equal(direct()[0].cpu().numpy(), a)


def test_a_direction_before_the_bounds_are_staged_is_refused():
    from pyipm_amd import lbfgs
    from pyipm_amd.newton import MEM_HOST
    lib = lbfgs.load()
    h = ctypes.c_void_p()
    assert lib.pyipm_lbfgs_bounded_create(ctypes.byref(h), 130, 0, 0, 3, 2, 0, 0, ctypes.c_void_p(0)) == 0
    try:
        N = 130 + 2 * 3
        g, dz, s, lda = (np.ones(k) for k in (N, N, 3, 3))
        p = lambda a: ctypes.c_void_p(a.ctypes.data)       # noqa: E731
        args = (h, p(g), p(s), p(lda), 1.0, 0, None, 1, None, 1, None, None, None, 0.0, EPS, p(dz), 0, MEM_HOST, None)
        assert lib.pyipm_lbfgs_direction(*args) == -1
        assert b"bounds" in lib.pyipm_lbfgs_last_error(h)
        var, sign = np.array([0, 129, 0], dtype=np.int64), np.array([1.0, -1.0, -1.0])
        assert lib.pyipm_lbfgs_bounded_stage(h, p(var), p(sign)) == 0
        assert lib.pyipm_lbfgs_direction(*args) == 0
        assert np.all(np.isfinite(dz))
    finally:
        lib.pyipm_lbfgs_destroy(h)


def test_ipm_with_bounds_tracks_the_hand_written_form():
    """A boxed QP (n = 40, 3 equalities, 4 general inequalities, |x_k| <= 0.5 with three sides left open; 15 bounds are active at
    the solution) solved by IPM(lbfgs=4, bounds=(lb, ub)) and with the same bounds written into ci / dci by hand, in the order
    IPM gives them.  Same signal and iteration count; x and fval within 100 x the distance between IPM(lbfgs=4) and
    IPM(lbfgs=4, resident_pairs=True) on the hand-written form (the yardstick and margin of DESIGN section 7d's pair-store
    paragraph, measured here).  The bounded run never stages more than me + mg columns."""
    from pyipm_amd.ipm import IPM
    from pyipm_amd.problems import make_qp, qp_callables
    n, me, mg = 40, 3, 4
    p = qp_callables(make_qp(n, me, mg, 5))
    lb, ub = np.full(n, -0.5), np.full(n, 0.5)
    lb[5], ub[7:9] = -np.inf, np.inf
    kl, ku = np.flatnonzero(np.isfinite(lb)), np.flatnonzero(np.isfinite(ub))
    E = np.zeros((n, kl.size + ku.size))
    E[kl, np.arange(kl.size)] = 1.0
    E[ku, kl.size + np.arange(ku.size)] = -1.0
    ci = lambda x: np.concatenate([np.asarray(p["ci"](x)).reshape(mg), x[kl] - lb[kl], ub[ku] - x[ku]])      # noqa: E731
    dci = lambda x: np.concatenate([np.asarray(p["dci"](x)).reshape(n, mg), E], axis=1)                       # noqa: E731
    kw = dict(x0=np.zeros(n), f=p["f"], df=p["df"], ce=p["ce"], dce=p["dce"], lbfgs=4, verbosity=-1, device=0, niter=20, miter=30)

    def run(ipm):
        with np.errstate(all="ignore"):
            x, s, lda, fval, _ = ipm.solve()
        return ipm, x, float(fval), s, lda

    hand, xh, fh, sh, ldh = run(IPM(ci=ci, dci=dci, **kw))
    res, xr, fr, _, _ = run(IPM(ci=ci, dci=dci, resident_pairs=True, **kw))
    bnd, xb, fb, sb, ldb = run(IPM(ci=p["ci"], dci=p["dci"], bounds=(lb, ub), **kw))
    dx_yard, df_yard = float(np.linalg.norm(xr - xh)), abs(fr - fh)
    dx, df = float(np.linalg.norm(xb - xh)), abs(fb - fh)
    print("boxed QP: iterations hand %d resident %d bounded %d | |x_res - x_hand| %.3e |f| %.3e | |x_bounded - x_hand| %.3e |f| %.3e"
          % (hand.iter_count, res.iter_count, bnd.iter_count, dx_yard, df_yard, dx, df))
    assert bnd.signal == hand.signal and bnd.iter_count == hand.iter_count
    assert dx <= 100 * dx_yard and df <= 100 * df_yard
    assert bnd.nineq == hand.nineq == mg + kl.size + ku.size and sb.shape == sh.shape and ldb.shape == ldh.shape
    assert bnd.backend.n_cols_staged == bnd.backend.n_staged * (me + mg) and bnd.backend.core.mi == mg
    assert np.all(xb[kl] > lb[kl]) and np.all(xb[ku] < ub[ku])
    with pytest.raises(NotImplementedError):
        IPM(ci=p["ci"], dci=p["dci"], bounds=(lb, ub), **dict(kw, lbfgs=False))
    with pytest.raises(NotImplementedError):
        IPM(ci=p["ci"], dci=p["dci"], bounds=(lb, ub), lbfgs_refine=1, **kw)
