"""The device-resident L-BFGS pair store (pyipm_pairs_* of include/pyipm_newton.h, pyipm_amd.lbfgs.PairStore) against the
oracle's restatement of lbfgs_update (oracle/lbfgs_oracle.py:24-75), offer by offer; into the direction; inside the two solvers.

Bounds.  S and Y are element-wise differences: bit-equal.  Every new entry of SS / L / D is a dot product of length n, so in
ANY summation order, with or without fused multiply-adds, |computed - exact| <= n eps sum|a_i b_i|; "exact" is evaluated in
np.longdouble.  zeta = curv / (den + eps) carries the propagated bound of its two dots plus four roundings of its own.  Entries
an offer does not touch must keep their bits.  A decision can differ from the oracle's only when curv or zeta_new lies within
that bound of sqrt(eps): every sequence asserts, from oracle values alone, a margin of 1e3 bounds on every offer."""
import ctypes
import os

import numpy as np
import pytest

import pairs_cases as pc

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS = pc.EPS
# kernels_pairs.hpp: rows a workgroup takes per round, and workgroups of the products kernel
PAIRS_ROWCHUNK = 64
PAIRS_GBLK = 1024
GRID_ROUND = PAIRS_ROWCHUNK * PAIRS_GBLK


def _store(n, memory, con, zeta0=1.0):
    from pyipm_amd.lbfgs import PairStore
    return PairStore(n, memory, con, zeta0=zeta0, device=0)


def _odd(a):
    """``a`` as a device tensor that starts an odd number of doubles into a larger buffer."""
    import torch
    buf = torch.full((a.size + 5,), float("nan"), dtype=torch.float64, device="cuda:0")
    buf[3:3 + a.size] = torch.from_numpy(a).to("cuda:0")
    t = buf[3:3 + a.size]
    assert t.data_ptr() % 16 == 8
    return t


def _dot_bound(a, b):
    """(exact a.b in extended precision, n eps sum|a_i b_i|)."""
    al, bl = a.astype(np.longdouble), b.astype(np.longdouble)
    return np.sum(al * bl), float(a.size * EPS * np.sum(np.abs(al * bl)))


def _oracle_outcome(before_m, after):
    if after[1].shape[1] == 0 and before_m > 0:
        return 2
    return 1 if (after[6] == 0 and after[1].shape[1] > 0) else 0


def _exact_new_entries(con, want):
    """Extended-precision values and bounds of what an ACCEPTED offer writes, from the oracle's storage (computed once per offer
    and shared by the stores under test)."""
    wS, wY = want[1], want[2]
    m = wS.shape[1]
    dx, dg = wS[:, -1], wY[:, -1]
    v, A, B = (dx, wS, wY) if con else (dg, wY, wS)    # SS = A'A, "L" from v against B
    e = {"ss": [_dot_bound(A[:, j], v) for j in range(m)], "l": [_dot_bound(B[:, j], v) for j in range(m - 1)]}
    curv, bc = e["curv"] = _dot_bound(dg, dx)
    den, bden = e["ss"][m - 1]
    z = curv / (den + EPS)
    e["zeta"] = (float(z), float((bc + abs(z) * bden) / (den + EPS - bden) + 4 * EPS * abs(z)))
    return e


def _check_offer(t, con, prev, got, want, outcome, exact):
    """One store's view after offer t against the oracle's state ``want`` = (zeta, S, Y, SS, L, D, fail); ``prev`` is the store's
    own (zeta, SS, L, D) before the offer."""
    zeta, S, Y, SS, L, D, fail = got
    wz, wS, wY, wSS, wL, wD, wfail = want
    m = wS.shape[1]
    assert S.shape == Y.shape == wS.shape and fail == wfail, (t, S.shape, wS.shape, fail, wfail)
    assert SS.shape == L.shape == D.shape == (m, m)
    Sh, Yh = S.cpu().numpy(), Y.cpu().numpy()
    assert Sh.tobytes() == wS.tobytes() and Yh.tobytes() == wY.tobytes(), (t, "S / Y differ from the oracle's bits")
    if outcome == 2:                                   # reset: empty, zeta0
        assert zeta == wz
        return
    if outcome == 0:                                   # skipped: nothing moves
        assert zeta == prev[0]
        for a, b in zip((SS, L, D), prev[1:]):
            assert a.tobytes() == b.tobytes(), (t, "a skipped pair changed SS / L / D")
        return
    # accepted: the old entries keep their bits (moved up and left by one when the oldest pair left) ...
    pm = prev[1].shape[0]
    off = 1 if pm + 1 > m else 0
    for name, a, b in zip(("SS", "L", "D"), (SS, L, D), prev[1:]):
        assert np.ascontiguousarray(a[:m - 1, :m - 1]).tobytes() == np.ascontiguousarray(b[off:, off:]).tobytes(), \
            (t, name, "old entries moved wrongly")
    # ... and the new row / column are dots of the newest pair with the storage
    for j in range(m):
        ex, bd = exact["ss"][j]
        assert abs(SS[m - 1, j] - ex) <= bd and SS[j, m - 1] == SS[m - 1, j], (t, "SS", j, float(SS[m - 1, j] - ex), bd)
        if j < m - 1:
            ex, bd = exact["l"][j]
            l_new, l_other = (L[m - 1, j], L[j, m - 1]) if con else (L[j, m - 1], L[m - 1, j])
            assert abs(l_new - ex) <= bd and l_other == 0.0, (t, "L", j, float(l_new - ex), bd)
            assert D[m - 1, j] == 0.0 and D[j, m - 1] == 0.0
    curv, bc = exact["curv"]
    assert abs(D[m - 1, m - 1] - curv) <= bc
    assert L[m - 1, m - 1] == (0.0 if con else D[m - 1, m - 1])
    z, bz = exact["zeta"]
    assert abs(zeta - z) <= bz, (t, zeta, z, bz)
    np.testing.assert_allclose(zeta, wz, rtol=1e-9)    # (and the oracle's own value, loosely: a gross error shows here first)


def _margins(t, x_old, x_new, g_old, g_new, n, con):
    """The oracle's own distance from the two thresholds against 1e3 x the bound: a seed that fails here is to be replaced."""
    dx, dg = x_new - x_old, g_old[:n] - g_new[:n]
    v = dx if con else dg
    curv, den = float(np.dot(dg, dx)), float(np.dot(v, v))
    _, bc = _dot_bound(dg, dx)
    _, bden = _dot_bound(v, v)
    z = curv / (den + EPS)
    bz = (bc + abs(z) * bden) / (den + EPS - bden) + 4 * EPS * abs(z)
    assert abs(curv - pc.ROOT_EPS) >= 1e3 * bc, ("seed too close to the curvature threshold", t, curv, bc)
    assert curv <= pc.ROOT_EPS or abs(z - pc.ROOT_EPS) >= 1e3 * bz, ("seed too close to the zeta threshold", t, z, bz)


SMALL_N = [1, 2, 63, 64, 65, 257, PAIRS_ROWCHUNK + 1]
CASES = [(n, memory) for n in SMALL_N for memory in (1, 2, 4, 31)]
CASES += [(GRID_ROUND + 1, 1), (GRID_ROUND + 1, 4), (8193, 2), (8193, 31)]
CASES = sorted(set(CASES))


@pytest.mark.parametrize("pattern", ["accepts", "reset"])
@pytest.mark.parametrize("con", [True, False])
@pytest.mark.parametrize("n,memory", CASES)
def test_replay_against_the_oracle(n, memory, con, pattern):
    """Two stores -- one fed host arrays, one fed device tensors at an odd 8-byte offset -- and the oracle, offer by offer."""
    from oracle import lbfgs_oracle as lo
    seq = pc.offers(n, memory, pattern, pc.seed_of(n, memory, con, pattern))
    assert len(seq) == 3 * (memory + 1) + 2
    host, dev = _store(n, memory, con), _store(n, memory, con)
    state = lo.lbfgs_init(n)
    prev = {id(st): (1.0,) + (np.zeros((0, 0)),) * 3 for st in (host, dev)}
    outcomes, top = [], 0
    for t, (x_old, x_new, g_old, g_new) in enumerate(seq):
        assert g_old.size > n and g_new.size > n
        _margins(t, x_old, x_new, g_old, g_new, n, con)
        before_m = state[1].shape[1]
        state = lo.lbfgs_update(x_old, x_new, g_old, g_new, *state, n, con, memory, EPS)
        want_outcome = _oracle_outcome(before_m, state)
        o_h = host.offer(x_old, x_new, g_old, g_new, EPS)
        o_d = dev.offer(_odd(x_old), _odd(x_new), _odd(g_old), _odd(g_new), EPS)
        assert o_h == o_d == want_outcome, (t, o_h, o_d, want_outcome)
        exact = _exact_new_entries(con, state) if want_outcome == 1 else None
        views = {}
        for st in (host, dev):
            views[id(st)] = got = st.view()
            _check_offer(t, con, prev[id(st)], got, state, want_outcome, exact)
            prev[id(st)] = (got[0],) + tuple(got[3:6])
        a, b = views[id(host)], views[id(dev)]
        assert a[0] == b[0] and all(p.tobytes() == q.tobytes() for p, q in zip(a[3:6], b[3:6])), (t, "the two stores differ")
        outcomes.append(want_outcome)
        top = max(top, state[1].shape[1])
    assert top == memory + 1 and 0 in outcomes and 1 in outcomes and ((2 in outcomes) == (pattern == "reset"))
    host.close(); dev.close()


@pytest.mark.parametrize("con", [True, False])
def test_reset_and_same_sequence_again_reproduces_the_first_pass(con):
    n, memory = 1000, 4
    seq = pc.offers(n, memory, "accepts", pc.seed_of(n, memory, con, "accepts"))
    st = _store(n, memory, con, zeta0=0.5)
    passes = []
    for _ in range(2):
        st.reset()
        z0, S0, _, SS0, _, _, f0 = st.view()
        assert (z0, S0.shape, SS0.shape, f0) == (0.5, (n, 0), (0, 0), 0)
        rec = []
        for x_old, x_new, g_old, g_new in seq:
            o = st.offer(x_old, x_new, g_old, g_new, EPS)
            zeta, S, Y, SS, L, D, fail = st.view()
            rec.append((o, zeta, fail, S.cpu().numpy().tobytes(), Y.cpu().numpy().tobytes(), SS.tobytes(), L.tobytes(), D.tobytes()))
        passes.append(rec)
    assert passes[0] == passes[1]
    st.close()


@pytest.mark.parametrize("n,me,mi,m", [(300, 20, 44, 9), (8193, 5, 9, 9), (300, 0, 0, 32)])
def test_view_goes_straight_into_the_direction(n, me, mi, m):
    """LbfgsCore.direction on the store's strided view is bit-equal to the same call on contiguous clones of S and Y -- on the
    full store, and again after one more accepted pair pushed the oldest one out."""
    from pyipm_amd.lbfgs import LbfgsCore
    from pyipm_amd.problems import make_qp
    memory, con = m - 1, bool(me or mi)
    rng = np.random.default_rng(n + m)
    qp = make_qp(n, me, mi, 3)
    core = LbfgsCore(n, me, mi, m, device=0, nb=128 if n < 1000 else 256)
    core.stage_jacobian(qp["Je"] if me else None, qp["Ji"] if mi else None)
    g = rng.standard_normal(n + 2 * mi + me)
    s = qp["s"] if mi else None
    lda = qp["lam"] if con else None
    st = _store(n, memory, con)
    seq = pc.offers(n, memory, "empty", pc.seed_of(n, memory, con, "empty"))[memory + 1:]       # accepts only
    assert len(seq) >= m + 1
    for k, (x_old, x_new, g_old, g_new) in enumerate(seq[:m + 1]):
        assert st.offer(x_old, x_new, g_old, g_new, EPS) == 1
        if k < m - 1:
            continue
        zeta, S, Y, SS, L, D, _ = st.view()
        assert S.shape == (n, m) and S.stride() == (2 * m, 1) and not S.is_contiguous()
        dz1, st1 = core.direction(g, s, lda, zeta, S, Y, SS, L, D, reg=1e-12)
        dz2, st2 = core.direction(g, s, lda, zeta, S.clone().contiguous(), Y.clone().contiguous(), SS, L, D, reg=1e-12)
        a, b = dz1.cpu().numpy(), dz2.cpu().numpy()
        assert np.isfinite(a).all() and a.tobytes() == b.tobytes(), (k, np.abs(a - b).max())
        assert st1["m"] == m
    st.close(); core.close()


@pytest.mark.parametrize("k", range(1, 11))
def test_ipm_with_resident_pairs_solves_the_example_problems(k):
    """The assertions of test_ipm_lbfgs_solves_example_problems_on_the_device, with the storage in the pair store; the same
    number of iterations as the NumPy storage; nothing of S / Y uploaded."""
    import torch
    from pyipm_amd.ipm import IPM
    from pyipm_amd.problems import example_problem, unit_test_x0
    d = np.load(os.path.join(GOLD, "lbfgs_trace_p%02d.npz" % k))
    p = example_problem(k)
    runs = {}
    for resident in (False, True):
        ipm = IPM(x0=unit_test_x0()[k], f=p["f"], df=p["df"], ce=p["ce"], dce=p["dce"], ci=p["ci"], dci=p["dci"],
                  lbfgs=4, Ftol=1.0e-8, verbosity=-1, device=0, resident_pairs=resident)
        with np.errstate(all="ignore"):
            x, s, lda, fval, kkt = ipm.solve()
        runs[resident] = (ipm, x)
    ipm, x = runs[True]
    assert min(np.linalg.norm(x - gt) for gt in p["ground_truth"]) <= 1e-3
    assert ipm.signal == int(d["signal"])
    assert ipm.backend.n_calls == ipm.iter_count
    np.testing.assert_allclose(x, d["x"], rtol=1e-5, atol=1e-6)
    assert ipm.iter_count == runs[False][0].iter_count
    assert ipm.backend.pair_doubles_uploaded == 0 and ipm._pairs[1].n_offers == max(ipm.iter_count - 1, 0)
    if runs[False][0].iter_count > 1:
        assert runs[False][0].backend.pair_doubles_uploaded > 0            # (the counter does count)
    assert isinstance(ipm._pair_store().view()[1], torch.Tensor)


@pytest.mark.parametrize("shape", [(40, 12, 0, 2), (40, 0, 12, 1), (24, 8, 16, 0)])      # the qp_n* fixtures: me only, mi only, both
def test_qp_loop_with_resident_pairs_tracks_the_torch_storage(shape):
    """QPDeviceIPM(lbfgs=4, resident_pairs=True) against resident_pairs=False: same signal, same iteration count; x and fval within
    100 x the distance between the two EXISTING paths QPDeviceIPM(lbfgs=4) and IPM(lbfgs=4) on the same QP -- they differ only in
    where the products are rounded, as the resident store does (the margin of DESIGN section 7e).  Measured on the parent
    (DESIGN section 7d has the figures); the two existing paths are run here again so that the bound is theirs, not a constant."""
    from pyipm_amd.ipm import IPM
    from pyipm_amd.problems import make_qp, qp_callables
    from pyipm_amd.qp import QPDeviceIPM
    n, me, mi, seed = shape
    qp = make_qp(n, me, mi, seed)
    p = qp_callables(qp)
    kw = dict(niter=20, miter=30)

    def dev(**more):
        q = QPDeviceIPM(qp["Q"], qp["c"], A=qp["A"] if me else None, b=qp["b"] if me else None, G=qp["G"] if mi else None,
                        h=qp["h"] if mi else None, verbosity=-1, lbfgs=4, **kw, **more)
        x, _, _, f, _ = q.solve()
        return q, x.cpu().numpy(), float(f)

    host = IPM(x0=np.zeros(n), f=p["f"], df=p["df"], ce=p["ce"], dce=p["dce"], ci=p["ci"], dci=p["dci"], lbfgs=4, verbosity=-1,
               device=0, **kw)
    with np.errstate(all="ignore"):
        xh, _, _, fh, _ = host.solve()
    q0, x0, f0 = dev()
    q1, x1, f1 = dev(resident_pairs=True)
    dx_paths, df_paths = float(np.linalg.norm(x0 - xh)), abs(f0 - float(fh))
    dx_res, df_res = float(np.linalg.norm(x1 - x0)), abs(f1 - f0)
    print("QP %s: existing paths |dx| = %.3e |df| = %.3e (iters %d / %d); resident vs torch storage |dx| = %.3e |df| = %.3e (iters %d)"
          % (shape, dx_paths, df_paths, q0.iter_count, host.iter_count, dx_res, df_res, q1.iter_count))
    assert q1.signal == q0.signal and q1.iter_count == q0.iter_count
    assert dx_res <= 100 * dx_paths and df_res <= 100 * df_paths
    assert q1.pairs.n_offers == max(q1.iter_count - 1, 0)


def test_errors_leave_the_store_usable():
    from pyipm_amd import newton
    from pyipm_amd.lbfgs import PairStore, PairsView
    from pyipm_amd.newton import NewtonError
    lib = newton.load_library()
    for memory in (0, 32):
        with pytest.raises(NewtonError):
            PairStore(50, memory, True, device=0)
        h = ctypes.c_void_p()
        assert lib.pyipm_pairs_create(ctypes.byref(h), 50, memory, 1, 1.0, 0, None) == -1 and not h.value
    n, memory = 50, 2
    st = _store(n, memory, True)
    seq = pc.offers(n, memory, "accepts", 5)
    assert st.offer(*seq[0], EPS) == 1
    before = st.view()
    out = ctypes.c_int(9)
    x = np.zeros(n)
    px = ctypes.c_void_p(x.ctypes.data)
    for bad in range(4):
        args = [px] * 4
        args[bad] = None
        assert lib.pyipm_pairs_offer(st.h, *args, EPS, newton.MEM_HOST, ctypes.byref(out)) == -1
        assert b"null" in lib.pyipm_pairs_last_error(st.h) and out.value == 9
    assert lib.pyipm_pairs_offer(st.h, px, px, px, px, EPS, newton.MEM_HOST, None) == -1
    assert lib.pyipm_pairs_view_get(st.h, None) == -1 and b"null" in lib.pyipm_pairs_last_error(st.h)
    after = st.view()
    assert after[0] == before[0] and after[6] == before[6] and after[1].shape == (n, 1)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(after[3:6], before[3:6]))
    assert st.offer(*seq[1], EPS) == 1 and st.view()[1].shape == (n, 2)          # still usable
    v = PairsView()
    assert lib.pyipm_pairs_view_get(st.h, ctypes.byref(v)) == 0 and (v.m, v.ld) == (2, 2 * (memory + 1))
    st.close()
