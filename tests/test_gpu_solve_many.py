"""solve_many: many right-hand sides against one factor (pyipm_newton_solve_many; sym_solve_cmp with a matrix b,
pyipm.py:911-914), judged against manufactured systems of known solution (tests/kkt_manufactured.py): B = K X_true from
the blocks on the host, so every check runs at any size without a dense LU."""
import ctypes

import numpy as np
import pytest

from kkt_manufactured import Manufactured, blas_threads

pytestmark = pytest.mark.gpu


def _kmat(m, X, delta=0.0, delta_c=0.0):
    """(K + delta I_x - delta_c I_e) X for an (N, k) matrix: Manufactured.matvec column-blocked."""
    n, me, mi, h = m.n, m.me, m.mi, m.h
    X = np.asarray(X, dtype=np.float64)
    xx, xs, xe, xi = X[:n], X[n:n + mi], X[n + mi:n + mi + me], X[n + mi + me:]
    Y = np.empty_like(X)
    with blas_threads():
        Y[:n] = h["d2L"] @ xx + delta * xx
        if me:
            Y[:n] += h["Je"] @ xe
            Y[n + mi:n + mi + me] = h["Je"].T @ xx - delta_c * xe
        if mi:
            Y[:n] += h["Ji"] @ xi
            Y[n:n + mi] = m.sigma[:, None] * xs - xi
            Y[n + mi + me:] = h["Ji"].T @ xx - xs
    return Y


def _colerr(A, B):
    A, B = np.asarray(A), np.asarray(B)
    return np.linalg.norm(A - B, axis=0) / np.linalg.norm(B, axis=0)


def _factored(m, nb=256, **opts):
    import torch
    from pyipm_amd.newton import NewtonCore
    core = NewtonCore(m.n, m.me, m.mi, device=0, nb=nb)
    for k, v in opts.items():
        core.set_option(k, v)
    m.stage(core)
    core.residual()
    core.assemble(0.0, 0.0)
    st = core.factor()
    torch.cuda.synchronize()
    return core, st


def _rhs(m, k, seed=1):
    X = np.random.default_rng(seed).standard_normal((m.N, k))
    return X, _kmat(m, X)


SHAPES = [
    # (n, me, mi, nb): ragged N, N below one panel, me = 0, mi = 0, wide_sub in effect (nb = 512)
    (203, 37, 61, 256),          # N = 362: not a multiple of 64 / 128 / 256
    (70, 10, 20, 256),           # N = 120: below one panel
    (611, 0, 300, 256),          # me = 0
    (700, 130, 0, 128),          # mi = 0
    (1301, 211, 517, 512),       # N = 2546, wide panels swept in sub-panels
]


@pytest.mark.parametrize("shape", SHAPES)
def test_columns_match_x_true_and_solve(shape):
    n, me, mi, nb = shape
    m = Manufactured(n, me, mi, n_pairs=3 if n >= 300 else 0, seed=n + me + mi)
    core, _ = _factored(m, nb=nb)
    X, B = _rhs(m, 200)
    for k in (1, 2, 63, 64, 65, 200):
        Xs = core.solve_many(B[:, :k], flip=False).cpu().numpy()
        assert Xs.shape == (m.N, k)
        assert _colerr(Xs, X[:, :k]).max() <= 1e-10
    for j in (0, 64, 199):
        xj = core.solve(B[:, j], flip=False).cpu().numpy()
        assert _colerr(Xs[:, j:j + 1], xj[:, None])[0] <= 1e-12
    core.close()


def test_ragged_last_sub_panel_of_a_wide_panel():
    """nb = 384 at wide_sub = 256: every panel is swept as sub-panels of 256 + 128 columns, forward and last first, by the
    per-panel sweeps of solve (sweep_persist = 0) and by solve_many.  N = 768: two such panels."""
    m = Manufactured(448, 64, 128, seed=7)
    core, _ = _factored(m, nb=384, wide_sub=256, sweep_persist=0)
    X, B = _rhs(m, 3)
    x0 = core.solve(B[:, 0], flip=False).cpu().numpy()
    assert _colerr(x0[:, None], X[:, :1])[0] <= 1e-10
    Xs = core.solve_many(B, flip=False).cpu().numpy()
    assert Xs.shape == (m.N, 3)
    assert _colerr(Xs, X).max() <= 1e-10
    assert _colerr(Xs[:, :1], x0[:, None])[0] <= 1e-12
    core.close()


def test_flip_negates_exactly_the_multiplier_rows():
    m = Manufactured(403, 57, 99, seed=5)
    core, _ = _factored(m)
    _, B = _rhs(m, 9)
    raw = core.solve_many(B, flip=False).cpu().numpy()
    fl = core.solve_many(B, flip=True).cpu().numpy()
    split = m.n + m.mi
    assert np.array_equal(fl[:split], raw[:split]) and np.array_equal(fl[split:], -raw[split:])
    core.close()


def test_static_pivots_adaptive_refinement_recovers_x_true():
    m = Manufactured(1100, 150, 600, mixer="T", zero_tile=True, n_zero=2, seed=11)
    core, st = _factored(m)
    assert st["n_zero"] >= 1, st
    X, B = _rhs(m, 70)
    Xs = core.solve_many(B, flip=False, refine=-1).cpu().numpy()
    info = core.solve_info()
    assert info["converged"] and info["steps"] >= 1, info
    assert _colerr(Xs, X).max() <= 1e-9
    assert np.max(_colerr(_kmat(m, Xs), B)) <= 10.0 * max(info["backward_error"], 1e-16)
    core.close()


def test_fixed_refinement_on_flagged_tiles_lowers_the_worst_backward_error():
    m = Manufactured(900, 100, 400, sigma_decades=12.0, seed=13)
    core, _ = _factored(m)
    _, B = _rhs(m, 17)
    X0 = core.solve_many(B, flip=False).cpu().numpy()
    core.set_option("block_refine", 0)                     # flagged tiles exist: their refinement in k_ms_diag changes bits
    assert not np.array_equal(core.solve_many(B, flip=False).cpu().numpy(), X0)
    core.set_option("block_refine", 2)                     # (the default)
    assert np.array_equal(core.solve_many(B, flip=False).cpu().numpy(), X0)
    e0 = _colerr(_kmat(m, X0), B)
    e2 = _colerr(_kmat(m, core.solve_many(B, flip=False, refine=2).cpu().numpy()), B)
    assert np.all(e2 <= np.maximum(e0, 1e-15)), (e0, e2)
    assert e2.max() <= e0.max()
    core.close()


@pytest.mark.parametrize("shape", [(203, 37, 61), (611, 0, 300), (1201, 173, 480)])
@pytest.mark.parametrize("smax", [None, 1.0])
def test_condensed_option(shape, smax):
    n, me, mi = shape
    m = Manufactured(n, me, mi, n_pairs=2, seed=17 + n)
    opts = dict(condensed=1)
    if smax is not None:
        opts["condensed_sigma_max"] = smax                 # part of the inequalities stay explicit (active) rows
    core, _ = _factored(m, **opts)
    X, B = _rhs(m, 65)
    for k in (1, 2, 64, 65):
        Xs = core.solve_many(B[:, :k], flip=False).cpu().numpy()
        assert _colerr(Xs, X[:, :k]).max() <= 1e-10
    xj = core.solve(B[:, 7], flip=False).cpu().numpy()
    assert _colerr(Xs[:, 7:8], xj[:, None])[0] <= 1e-12
    core.close()


def test_skip_zeros_off_agrees():
    m = Manufactured(777, 99, 333, seed=19)
    a, _ = _factored(m)
    b, _ = _factored(m, skip_zeros=0)
    _, B = _rhs(m, 40)
    xa, xb = a.solve_many(B).cpu().numpy(), b.solve_many(B).cpu().numpy()
    assert _colerr(xa, xb).max() <= 1e-12
    a.close(); b.close()


def test_columns_are_bitwise_independent_of_the_batch():
    m = Manufactured(1500, 200, 600, n_pairs=4, seed=23)
    core, _ = _factored(m)
    _, B = _rhs(m, 130)
    full = core.solve_many(B).cpu().numpy()
    again = core.solve_many(B).cpu().numpy()
    assert np.array_equal(full, again)
    for j in (0, 63, 64, 129):
        one = core.solve_many(B[:, j:j + 1]).cpu().numpy()
        assert np.array_equal(one[:, 0], full[:, j])
    perm = np.random.default_rng(3).permutation(130)
    shuffled = core.solve_many(B[:, perm]).cpu().numpy()
    assert np.array_equal(shuffled, full[:, perm])
    core.close()


def test_state_is_left_alone_full_form():
    """The factor, the fused forward pass, the kept residual and the last direction survive solve_many: every later
    result has the bits it has without it."""
    import torch
    m = Manufactured(1700, 230, 700, seed=29)
    a, _ = _factored(m)
    b, _ = _factored(m)
    _, B = _rhs(m, 33)
    S = a.kkt_storage()
    before = S.view(torch.int64).clone()                   # (bit patterns: unused storage may hold NaN)
    a.solve_many(B)
    torch.cuda.synchronize()
    assert torch.equal(S.view(torch.int64), before)
    dza1 = a.solve()                                       # consumes the fused forward pass
    dzb1 = b.solve()
    assert torch.equal(dza1, dzb1)
    la, ma = b.step_lengths(0.99), b.merit_info()
    b.solve_many(B)
    assert b.step_lengths(0.99) == la and b.merit_info() == ma
    assert torch.equal(a.solve(), b.solve())               # the kept residual, solved again without the fused pass
    a.close(); b.close()


def test_state_is_left_alone_condensed_form():
    m = Manufactured(1200, 150, 500, seed=31)
    a, _ = _factored(m, condensed=1)
    b, _ = _factored(m, condensed=1)
    _, B = _rhs(m, 10)
    a.solve_many(B)
    dza, dzb = a.solve().cpu().numpy(), b.solve().cpu().numpy()
    assert _colerr(dza[:, None], dzb[:, None])[0] <= 1e-12
    a.close(); b.close()


def test_memory_kinds_and_leading_dimensions():
    import torch
    from pyipm_amd.newton import MEM_DEVICE, MEM_HOST
    m = Manufactured(500, 60, 140, seed=37)
    core, _ = _factored(m)
    X, B = _rhs(m, 11)
    ref = core.solve_many(torch.from_numpy(B).cuda()).cpu().numpy()
    assert np.array_equal(core.solve_many(B).cpu().numpy(), ref)              # numpy in
    N, k, ld_r, ld_z = m.N, 11, m.N + 5, m.N + 9
    lib = core.lib
    # host memory, padded leading dimensions
    rh = np.full((k, ld_r), np.nan)
    rh[:, :N] = B.T
    zh = np.full((k, ld_z), 7.0)
    rc = lib.pyipm_newton_solve_many(core.h, k, rh.ctypes.data_as(ctypes.c_void_p), ld_r,
                                     zh.ctypes.data_as(ctypes.c_void_p), ld_z, 1, 0, MEM_HOST)
    assert rc == 0
    assert np.array_equal(zh[:, :N].T, ref) and np.all(zh[:, N:] == 7.0)
    # device memory, padded leading dimensions
    rd = torch.from_numpy(rh).cuda()
    zd = torch.full((k, ld_z), 7.0, dtype=torch.float64, device="cuda")
    rc = lib.pyipm_newton_solve_many(core.h, k, ctypes.c_void_p(rd.data_ptr()), ld_r, ctypes.c_void_p(zd.data_ptr()),
                                     ld_z, 1, 0, MEM_DEVICE)
    assert rc == 0
    torch.cuda.synchronize()
    z = zd.cpu().numpy()
    assert np.array_equal(z[:, :N].T, ref) and np.all(z[:, N:] == 7.0)
    core.close()


def test_errors_and_edge_cases():
    import torch
    from pyipm_amd.newton import MEM_DEVICE, NewtonCore, NewtonError
    m = Manufactured(300, 40, 90, seed=41)
    B = np.ones((m.N, 3))

    def bad(core):
        with pytest.raises(NewtonError) as e:
            core.solve_many(B)
        assert e.value.code == -1

    prov = NewtonCore(m.n, m.me, m.mi, device=0, provider_only=True)
    bad(prov)
    prov.close()
    dist = NewtonCore(m.n, m.me, m.mi, device=0, nb=128, world=2, rank=0)
    bad(dist)
    dist.close()
    core = NewtonCore(m.n, m.me, m.mi, device=0)
    m.stage(core)
    bad(core)                                              # before factor()
    core.assemble(0.0, 0.0)
    core.factor()
    rd = torch.zeros((3, m.N), dtype=torch.float64, device="cuda")
    zd = torch.zeros((3, m.N), dtype=torch.float64, device="cuda")
    p_r, p_z = ctypes.c_void_p(rd.data_ptr()), ctypes.c_void_p(zd.data_ptr())
    assert core.lib.pyipm_newton_solve_many(core.h, 3, p_r, m.N - 1, p_z, m.N, 1, 0, MEM_DEVICE) == -1
    assert core.lib.pyipm_newton_solve_many(core.h, 3, p_r, m.N, p_z, m.N - 1, 1, 0, MEM_DEVICE) == -1
    assert core.lib.pyipm_newton_solve_many(core.h, -1, p_r, m.N, p_z, m.N, 1, 0, MEM_DEVICE) == -1
    zd.fill_(5.0)
    assert core.lib.pyipm_newton_solve_many(core.h, 0, p_r, m.N, p_z, m.N, 1, 0, MEM_DEVICE) == 0
    torch.cuda.synchronize()
    assert bool((zd == 5.0).all())
    # a NaN in one column stays in that column
    _, Bm = _rhs(m, 5)
    clean = core.solve_many(Bm).cpu().numpy()
    Bn = Bm.copy()
    Bn[17, 2] = np.nan
    dirty = core.solve_many(Bn).cpu().numpy()
    assert np.isnan(dirty[:, 2]).any()
    others = [0, 1, 3, 4]
    assert np.array_equal(dirty[:, others], clean[:, others])
    core.close()


def test_bench_shape_backward_error():
    """N = 32768 (the bench shape), k = 64: backward error per column from the blocks."""
    import torch
    free, _ = torch.cuda.mem_get_info(0)
    if free < 40e9:
        pytest.skip("needs 40 GB of free HBM")
    m = Manufactured(16384, 4096, 6144, seed=43, device="cuda")
    torch.cuda.empty_cache()
    core, _ = _factored(m)
    _, B = _rhs(m, 64)
    Xs = core.solve_many(B, flip=False).cpu().numpy()
    assert _colerr(_kmat(m, Xs), B).max() <= 1e-13
    core.close()
