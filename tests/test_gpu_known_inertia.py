"""Indefinite, singular and LP-like KKT systems at the sizes where the schedule switches code paths, judged against
manufactured systems of known inertia and known solution (tests/kkt_manufactured.py; its predictions are checked against
LAPACK in tests/test_kkt_manufactured_model.py).

The convex generator (make_qp / make_qp_device) only ever sees the inertia (n + mi, me + mi, 0): no negative pivot outside
the multiplier block, no 2x2 or static pivot.  Here the x block carries negative curvature, 2x2 pairs with zero diagonals
and exactly zero rows, at shapes that reach every regime of the single-rank schedule (csrc/ctx.hpp):

    N (Npad)         shape (n, me, mi)          path
    6144             (2048, 0, 2048)            early0, tail groups of 8 (Npad <= 8192)
    8118 (8192)      (3001, 517, 2300)          ragged, tail groups of 8
    9216             (1024, 0, 4096)            early0, tail groups of 4
    11504 (11520)    (5003, 701, 2900), nb 512  every chain exposed (<= tile8_rows), groups of 4
    17001 (17024)    (9001, 0, 4000), nb 128    non-exposed chains as k_tile_step, reserved CUs (> persist_rows)
    17000 (17024)    (12007, 4993, 0)           no slack block: no panels enqueued up front / no fast group (GroupSched::fast)
    23545 (23552)    (12345, 2000, 4600)        128 x 256 bulk tiles (> BULK_BN_ROWS)
    29928 (29952)    (14001, 3001, 6463)        groups of 8 panels before the tail (> TAIL_COLS)

Every reference is an O(N n) host product from the blocks; no LU or eigensolver at these sizes."""
import numpy as np
import pytest

from kkt_manufactured import EPS, Manufactured

pytestmark = pytest.mark.gpu

DELTA0 = float(np.sqrt(EPS))


def relerr(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(b))


def _system(n, me, mi, **kw):
    """The manufactured system on cuda:0, or a skip when free HBM is short (as test_gpu_configs._run)."""
    import torch
    dev = torch.device("cuda", 0)
    free, _ = torch.cuda.mem_get_info(dev)
    N = n + me + 2 * mi
    # generator transient (D, M, M D, M D M', d2L) or the resident set (KKT storage + panel buffers, blocks), with margin
    need = 8.0 * max(5.0 * n * n, 1.06 * N * N + n * n) + 8.0 * n * (me + mi) + 6e9
    if free < need:
        pytest.skip("needs %.0f GB of free HBM, %.0f available" % (need / 1e9, free / 1e9))
    m = Manufactured(n, me, mi, device=dev, seed=n + 3 * me + 7 * mi, **kw)
    torch.cuda.empty_cache()
    return m


def _core(m, nb=256, **opts):
    from pyipm_amd.newton import NewtonCore
    core = NewtonCore(m.n, m.me, m.mi, device=0, nb=nb)
    for k, v in opts.items():
        core.set_option(k, v)
    m.stage(core)
    return core


def _close(core):
    import torch
    core.close()
    torch.cuda.empty_cache()


def _inertia_ok(st, m, delta=0.0, delta_c=0.0):
    neg, zero, pos = m.inertia(delta, delta_c)
    assert zero == 0
    assert st["nonfinite"] == 0 and (st["n_pos"], st["n_neg"]) == (pos, neg), (st, (pos, neg), m.counts())


NEG_SHAPES = [((2048, 0, 2048), 256), ((3001, 517, 2300), 256), ((1024, 0, 4096), 256), ((5003, 701, 2900), 256),
              ((5003, 701, 2900), 512), ((9001, 0, 4000), 256), ((9001, 0, 4000), 128), ((12007, 4993, 0), 256),
              ((12345, 2000, 4600), 256), ((14001, 3001, 6463), 256)]


@pytest.mark.parametrize("shape,nb", NEG_SHAPES, ids=["%d-%d-%d-nb%d" % (s + (nb,)) for s, nb in NEG_SHAPES])
def test_negative_curvature_inertia_and_forward_error(shape, nb):
    """Q mixer, a third of the x block with negative curvature (including the last two rows): the pivots count exactly
    (n_pos, n_neg) = (|P| + mi, |Nn| + me + mi) -- every pivot kernel that ran adds to these counts, so a sign counted
    wrong in any of them shows --; solve(b) returns x_true to 1e-10; step(0, 0) satisfies the blocks to 1e-12.  Both
    substitution schedules (one-launch sweeps and per-panel launches).  Where the 128 x 256 bulk tiles must run
    (Npad > BULK_BN_ROWS), they did, and nowhere else.

    The solves are those the backend makes for this factor: indefinite tiles pivot 2x2 inside their 64 x 64 tile and reach
    growth ~1e3 here, so HipNewtonBackend._at_risk sends them through adaptive refinement against the blocks (refine < 0).
    A plain substitution of such a factor is ~1e-8 from x_true (measured: 1e-9 .. 8e-9 at these shapes) and is not what any
    caller returns; 1e-10 applies to the refined solve, and the plain one is held to 1e-7."""
    n, me, mi = shape
    m = _system(n, me, mi, mixer="Q", n_neg=n // 3)
    core = _core(m, nb=nb, profile=1)
    core.assemble(0.0, 0.0)
    st = core.factor()
    _inertia_ok(st, m)
    assert st["n_zero"] == 0
    inst = core.trailing_instances()
    if core.Npad > 20480:
        assert core.Npad % 256 == 0 and inst[256]["launches"] >= 1, inst
    else:
        assert inst[256]["launches"] == 0, inst
    from pyipm_amd.ipm import HipNewtonBackend
    refine = -1 if HipNewtonBackend._at_risk(st) else 0
    g = m.residual()
    for sweep in (1, 0):
        core.set_option("sweep_persist", sweep)
        x = core.solve(rhs=m.b, flip=False).cpu().numpy()
        assert relerr(x, m.x_true) <= 1e-7, (sweep, relerr(x, m.x_true), st)
        x = core.solve(rhs=m.b, flip=False, refine=refine).cpu().numpy()
        assert relerr(x, m.x_true) <= 1e-10, (sweep, relerr(x, m.x_true), st, core.solve_info())
        dz, st2 = core.step(0.0, 0.0, refine=refine)
        _inertia_ok(st2, m)
        berr = m.backward_error(m.unflip(dz.cpu().numpy()), g)
        assert berr <= 1e-12, (sweep, berr, st2)
    _close(core)


PLAIN = dict(expert=1, lookahead=0, group=1, tile_chain=0, tile_waves=4, bulk_bn=128, reserve_cus=0, skip_zeros=0,
             keep_zeros=0, sweep_persist=0)


@pytest.mark.parametrize("shape", [(12007, 4993, 0), (14001, 3001, 6463)])
def test_schedule_options_give_the_same_bits_on_indefinite_systems(shape):
    """test_random_schedule_options_give_the_same_bits (tests/test_gpu_symmetric.py) where the row thresholds act, on an
    indefinite system: default options against a plain schedule (one panel per group, no lookahead, no chains, four waves,
    128 x 128 tiles only, no reserved CUs, nothing skipped), three steps per handle: dz and every pivot statistic bit for
    bit."""
    import torch
    n, me, mi = shape
    m = _system(n, me, mi, mixer="Q", n_neg=n // 3)
    out = []
    for opts in (dict(expert=1, sweep_persist=0), PLAIN):
        core = _core(m, **opts)
        runs = [core.step(0.0, 0.0) for _ in range(3)]
        for dz, st in runs:
            assert torch.equal(dz, runs[0][0]) and st == runs[0][1], opts
        _inertia_ok(runs[0][1], m)
        out.append((runs[0][0].clone(), runs[0][1]))
        _close(core)
    keys = ("n_pos", "n_neg", "n_2x2", "n_zero", "d_min", "d_max")
    assert torch.equal(out[0][0], out[1][0])
    assert [out[0][1][k] for k in keys] == [out[1][1][k] for k in keys], (out[0][1], out[1][1])


def _backend(m, **kw):
    from pyipm_amd.ipm import HipNewtonBackend
    return HipNewtonBackend(m.n, m.me, m.mi, device=0, **kw)


@pytest.mark.parametrize("shape", [(5003, 701, 2900), (12345, 2000, 4600)])
def test_reghess_shift_loop_at_scale(shape):
    """reghess (pyipm.py:1373-1406) on a system whose spectrum is known: the x block's eigenvalues are D (Q mixer), the
    most negative is above -1.2, so the first shift delta0 * 10^k that corrects the inertia is k = 8 (delta0 = sqrt(eps)),
    after k wrong inertias.  The direction satisfies K + delta I_x."""
    n, me, mi = shape
    m = _system(n, me, mi, mixer="Q", n_neg=n // 3)
    want, k = DELTA0, 0
    while want <= np.max(np.abs(m.d[m.role == 1])):
        want *= 10.0
        k += 1
    assert k == 8
    be = _backend(m)
    dz, delta, st = be.direction(*m.direction_args())
    assert delta == want and be.n_inertia_retries == k, (delta, want, be.n_inertia_retries)
    assert st["n_neg"] == me + mi and st["nonfinite"] == 0
    _inertia_ok(st, m, delta)
    berr = m.backward_error(m.unflip(dz), m.residual(), delta=delta)
    assert berr <= 1e-12, berr
    _close(be.core)


@pytest.mark.parametrize("variant", ["zero", "pairs"])
@pytest.mark.parametrize("shape", [(5003, 701, 2900), (9001, 0, 4000)])
def test_lp_like_zero_rows_and_pairs(shape, variant):
    """T mixer: d2L keeps exact zero rows (one whole 64-row tile of them plus the last two rows) or the zero diagonals of
    2x2 pairs (across 63|64, 255|256 and the last two rows, plus random ones) while both stay densely coupled.  The
    zero-row tile is singular inside its tile although K is not: static pivots, counted by their sign
    (test_tile_local_pivoting_falls_back_to_static_pivots).  The refined solve recovers x_true, and the backend returns
    the unshifted direction through the static-pivot path (test_reference_direction_without_a_shift at scale)."""
    n, me, mi = shape
    kw = dict(zero_tile=True, n_zero=2) if variant == "zero" else dict(n_pairs=40, n_neg=n // 6)
    m = _system(n, me, mi, mixer="T", **kw)
    core = _core(m)
    core.assemble(0.0, 0.0)
    st = core.factor()
    _inertia_ok(st, m)
    if variant == "zero":
        assert st["n_zero"] >= 1, st
    else:
        assert st["n_2x2"] >= 1 or st["n_zero"] >= 1, st
    x = core.solve(rhs=m.b, flip=False, refine=-1).cpu().numpy()
    info = core.solve_info()
    with_host = m.backward_error(x, m.b)
    assert info["converged"] and info["backward_error"] <= 1e-11 and with_host <= 1e-11, (info, with_host)
    assert max(info["backward_error"], 1e-16) <= 10.0 * max(with_host, 1e-16) and \
        max(with_host, 1e-16) <= 10.0 * max(info["backward_error"], 1e-16), (info, with_host)
    assert relerr(x, m.x_true) <= 1e-9, relerr(x, m.x_true)
    _close(core)
    if variant == "zero":
        be = _backend(m)
        dz, delta, st = be.direction(*m.direction_args())
        assert delta == 0.0 and be.n_static == 1 and st["n_zero"] >= 1, (delta, be.n_static, st)
        _inertia_ok(st, m)
        assert m.backward_error(m.unflip(dz), m.residual()) <= 1e-11
        _close(be.core)


def test_dependent_equalities_take_the_singular_branch():
    """Three equality columns duplicated (exact copies in floating point): K is singular, reghess' rcond <= eps test fires
    (pyipm.py:1379-1384), delta_c = reg_coef * eta * mu^beta goes on the equality block and delta = delta0 on the x block,
    which restores n_neg = me + mi with a convex x block."""
    n, me, mi = 5003, 701, 2900
    m = _system(n, me, mi, mixer="Q", dependent_eq=3)
    be = _backend(m)
    calls = []
    assemble = be.core.assemble

    def spy(delta=0.0, delta_c=0.0):
        calls.append((float(delta), float(delta_c)))
        return assemble(delta, delta_c)

    be.core.assemble = spy
    dz, delta, st = be.direction(*m.direction_args())
    dc = DELTA0 * 1e-4 * m.mu ** 0.4
    assert calls[0] == (0.0, 0.0) and calls[-1] == (DELTA0, dc), calls
    assert delta == DELTA0
    assert st["n_neg"] == me + mi and st["n_zero"] == 0 and st["nonfinite"] == 0, st
    _inertia_ok(st, m, DELTA0, dc)
    assert m.backward_error(m.unflip(dz), m.residual(), DELTA0, dc) <= 1e-11
    _close(be.core)


@pytest.mark.parametrize("n", [12000, 17000])
def test_rcond_at_scale(n):
    """rcond = min|w| / max|w| (pyipm.py:1379-1381) with the spectrum pinned (Q mixer, me = mi = 0): an isolated largest
    |D| = 4 and smallest 1e-3 (all others in [0.25, 2]).  The smallest eigenvalue (inverse iteration through the factor)
    is within 5 %; the adaptive estimate never reports a rcond below exact / 1.1.  The ratio itself is held to 25 %, not 5 %:
    max|w| comes from six power iterations from a random start, whose component along an isolated largest eigenvalue is
    ~1/sqrt(N); (4/2)^6 / sqrt(N) < 1 at these sizes, so the estimate of max|w| is pulled toward the bulk at 2 (measured
    3.35 .. 3.5 for 4).  That error is harmless for the rcond <= eps test this estimate serves, which needs decades.  At min|D| = 1e-13 max|D| (450 eps: the rounding of the assembled matrix is two decades
    below) the backend's rcond <= eps test says "not singular"; with one exact zero row (T mixer) it says "singular".
    (No case within 100x of eps: there the reference's own decision is not sharp.)"""
    exact = 1e-3 / 4.0
    m = _system(n, 0, 0, mixer="Q", n_neg=n // 3, pin=(4.0, 1e-3))
    spec = np.abs(m.spectrum())
    assert spec.min() / spec.max() == exact
    core = _core(m)
    core.assemble(0.0, 0.0)
    st = core.factor()
    _inertia_ok(st, m)
    est = core.rcond()
    assert abs(est["w_min"] / 1e-3 - 1.0) <= 0.05, (est, exact)
    assert 2.0 < est["w_max"] <= 4.0 * 1.05 and abs(est["rcond"] / exact - 1.0) <= 0.25, (est, exact)
    ada = core.rcond(-1, -1)
    assert ada["rcond"] >= exact / 1.1, (ada, exact)
    _close(core)
    del m
    m = _system(n, 0, 0, mixer="Q", n_neg=n // 3, pin=(4.0, 4e-13))
    be = _backend(m)
    m.stage(be.core)
    be.core.assemble(0.0, 0.0)
    st = be._factor()
    # (no inertia check here: an eigenvalue at 1e-13 max|w| is below the backward error of a factor with growth ~1e3 --
    # measured: its sign came out wrong at both sizes -- so the count is not sharp; the rcond <= eps decision still is)
    assert st["nonfinite"] == 0 and st["n_neg"] + st["n_pos"] == m.N
    assert not be._singular(st, EPS), (st, be.last_rcond)
    _close(be.core)
    del m
    if n == 12000:
        m = _system(n, 0, 0, mixer="T", n_zero=1, n_neg=n // 3)
        assert not m.h["d2L"][m.role == 3].any()
        be = _backend(m)
        m.stage(be.core)
        be.core.assemble(0.0, 0.0)
        st = be._factor()
        assert be._singular(st, EPS), (st, be.last_rcond)
        _close(be.core)


@pytest.mark.parametrize("shape", [(5003, 701, 2900), (12345, 2000, 4600)])
def test_condensed_form_keeps_the_full_inertia(shape):
    """set_option("condensed", 1) factors [[H + Ji Sigma Ji', Je], [Je', 0]] and reports the inertia of the FULL matrix:
    with negative curvature in H that is (|P| + mi, |Nn| + me + mi).  The direction meets the backend's condensed_tol
    against the full blocks (HipNewtonBackend.direction: refine as the backend does, then 4 steps)."""
    n, me, mi = shape
    m = _system(n, me, mi, mixer="Q", n_neg=n // 3)
    core = _core(m, condensed=1)
    core.residual()
    core.assemble(0.0, 0.0)
    st = core.factor()
    _inertia_ok(st, m)
    g = m.residual()
    tol = 1e-9                                                   # HipNewtonBackend's condensed_tol
    for refine in (0, 4):
        berr = m.backward_error(m.unflip(core.solve(flip=True, refine=refine).cpu().numpy()), g)
        if berr <= tol:
            break
    assert berr <= tol, berr
    _close(core)


def test_late_iterate_sigma_over_twelve_decades():
    """Sigma = lam_i / s spread over 1e-6 .. 1e6 (late interior-point iterates), negative curvature, T mixer: inertia exact;
    the adaptive refinement either converges (and the host agrees: backward error <= 1e-11) or says it did not; the
    backward error it reports is never contradicted by the host's by more than 10x."""
    n, me, mi = 9001, 0, 4000
    m = _system(n, me, mi, mixer="T", n_neg=n // 3, sigma_decades=12.0)
    core = _core(m)
    core.assemble(0.0, 0.0)
    st = core.factor()
    _inertia_ok(st, m)
    x = core.solve(rhs=m.b, flip=False, refine=-1).cpu().numpy()
    info = core.solve_info()
    host = m.backward_error(x, m.b)
    if info["converged"]:
        assert host <= 1e-11, (info, host)
    assert info["backward_error"] >= 0.0
    assert max(info["backward_error"], 1e-16) <= 10.0 * max(host, 1e-16) and \
        max(host, 1e-16) <= 10.0 * max(info["backward_error"], 1e-16), (info, host)
    _close(core)
