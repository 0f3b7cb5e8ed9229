"""Partial restaging of the Jacobians of an L-BFGS direction (include/pyipm_newton.h, pyipm_lbfgs_stage_jacobian_columns): the
direction after columns of J = [Je | Ji] were replaced must be, bit for bit, the direction a handle gives that staged the
whole of the new J; only the 128 x 128 lower-triangle tiles of J'J that those columns reach may be computed again.

Inputs are built as tests/test_gpu_lbfgs_depth.py builds its own (Jacobians, s and lambda of make_qp(n, me, mi, 3), storage
through the oracle's lbfgs_update, g standard normal, reg = 1e-12).  J1 is J0 with the chosen columns replaced by fresh
N(0, 1) / sqrt(n) columns, the scale of make_qp's own.  The oracle bound is that module's rule: 1e-9 relative in the 2-norm
where 4 (me + mi) <= n, 1e-6 otherwise."""
import ctypes
import functools

import numpy as np
import pytest

from test_gpu_lbfgs import _core, _rel, _storage
from test_gpu_lbfgs_depth import _shape, _tol

pytestmark = pytest.mark.gpu

BADARG = -1
TILE = 128


def _pads(n, p):
    return (p + TILE - 1) // TILE * TILE, (n + 8191) // 8192 * 8192


def _ksplit(p_pad, n_pad):
    """lb_ksplit of pyipm_amd/csrc/lbfgs_impl.hpp, restated: the split-K factor of the Gram launch."""
    nt = p_pad // TILE
    T, cnt = nt * (nt + 1) // 2, float(p_pad) * float(p_pad)
    best, bc, ks = 1, 1e300, 1
    while ks <= 512:
        if ks > 1 and (n_pad // ks < 1024 or ks * cnt * 8.0 > 1073741824.0):
            break
        t_tile = 2.0 * 128.0 * 128.0 * float(n_pad // ks) / (62.0e12 / 512.0)
        c = float((T * ks + 511) // 512) * t_tile + ((2.0 * ks + 1.0) * cnt * 8.0 / 3.0e12 + 5.0e-6 if ks > 1 else 0.0)
        if c < bc:
            bc, best = c, ks
        ks *= 2
    return best


def _tiles(p_pad, ranges=None):
    """Lower-triangle tiles with a row or column index the column ranges reach (None: all of them)."""
    nt = p_pad // TILE
    full = nt * (nt + 1) // 2
    if ranges is None:
        return full
    dirty = set()
    for a, b in ranges:
        dirty.update(range(a // TILE, (b - 1) // TILE + 1))
    clean = nt - len(dirty)
    return full - clean * (clean + 1) // 2


def _flops(n_pad, tiles):
    return 2.0 * 128.0 * 128.0 * n_pad * tiles


@functools.lru_cache(maxsize=None)
def _inputs(n, me, mi, m):
    """One direction's inputs, built once per shape and shared (read only)."""
    rng = np.random.default_rng(n + 7 * me + 13 * mi + m)
    c = dict(_shape(n, me, mi))
    zeta, S, Y, SS, L, D = _storage(n, m, rng, True, max(m, 1))
    assert S.shape[1] == m
    c.update(n=n, me=me, mi=mi, m=m, zeta=zeta, S=S, Y=Y, SS=SS, L=L, D=D, g=rng.standard_normal(n + 2 * mi + me))
    c["J0"] = np.concatenate([a for a in (c["Je"], c["Ji"]) if a is not None], axis=1)
    c["J0"].setflags(write=False)
    return c


def _j1(c, ranges, seed=11):
    rng = np.random.default_rng(seed)
    J1 = c["J0"].copy()
    for a, b in ranges:
        J1[:, a:b] = rng.standard_normal((c["n"], b - a)) / np.sqrt(c["n"])
    return J1


def _stage(core, c, J):
    me = c["me"]
    core.stage_jacobian(J[:, :me] if me else None, J[:, me:] if c["mi"] else None)


def _direct(core, c, g=None):
    dz, st = core.direction(c["g"] if g is None else g, c["s"], c["lda"], c["zeta"], c["S"], c["Y"], c["SS"], c["L"], c["D"],
                            reg=1e-12)
    return dz.cpu().numpy(), st


def _handle(c, nb=128):
    return _core(c["n"], c["me"], c["mi"], max(c["m"], 1), nb=nb)


SHAPE_A = (600, 100, 200, 4, 128)                 # p_pad = 384: three tile indices, ksplit > 1
CASES = [
    ("inside_one_tile", SHAPE_A, [(130, 135)], False),
    ("across_a_tile_boundary", SHAPE_A, [(120, 140)], True),
    ("across_je_ji", SHAPE_A, [(95, 110)], False),
    ("last_column", SHAPE_A, [(299, 300)], True),
    ("one_whole_tile", SHAPE_A, [(128, 256)], False),
    ("all_columns", SHAPE_A, [(0, 300)], False),
    ("two_calls", SHAPE_A, [(3, 8), (260, 271)], True),
    ("single_split", (600, 40, 3500, 0, 256), [(250, 260), (3000, 3001)], False),      # test_single_split_gram_vs_oracle's shape
    ("tiny", (3, 1, 1, 0, 128), [(1, 2)], False),
    ("two_row_pads", (8300, 100, 200, 4, 256), [(120, 140)], True),                    # n_pad = 16384
]


@pytest.mark.parametrize("name,shape,ranges,as_view", CASES, ids=[k[0] for k in CASES])
def test_partial_restage_is_a_full_restage_bit_for_bit(name, shape, ranges, as_view):
    """1. handle A (J0 staged, a direction, columns of J1 restaged, a direction) against handle B (J1 staged, a direction):
    the same dz and the same stats record.  2. the Gram launch of A's second direction computed the dirty tiles and no
    other: its flop count is 2 * 128 * 128 * n_pad per dirty tile, counted here from the ranges."""
    import torch
    n, me, mi, m, nb = shape
    c = _inputs(n, me, mi, m)
    p = me + mi
    p_pad, n_pad = _pads(n, p)
    ks = _ksplit(p_pad, n_pad)
    J1 = _j1(c, ranges)
    A, B = _handle(c, nb), _handle(c, nb)
    _stage(A, c, c["J0"])
    dz0, _ = _direct(A, c)
    t0 = A.last_timings()
    full = _flops(n_pad, _tiles(p_pad))
    assert t0["gram_launches"] == 1 and t0["gram_flops"] == full
    J1d = torch.from_numpy(J1).cuda()
    for a, b in ranges:
        A.stage_jacobian_columns(a, J1d[:, a:b] if as_view else J1[:, a:b])       # a row-strided device view / a NumPy slice
    dzA, stA = _direct(A, c)
    tA = A.last_timings()
    _stage(B, c, J1)
    dzB, stB = _direct(B, c)
    t_dirty = _tiles(p_pad, ranges)
    print("%s: p_pad=%d n_pad=%d ksplit=%d dirty tiles %d of %d, gram_flops %.6g (full %.6g)"
          % (name, p_pad, n_pad, ks, t_dirty, _tiles(p_pad), tA["gram_flops"], full))
    assert np.array_equal(dzA, dzB)
    assert stA == stB
    assert not np.array_equal(dzA, dz0)
    if name == "single_split":
        assert ks == 1
    elif shape == SHAPE_A:
        assert ks > 1
    assert tA["gram_flops"] == _flops(n_pad, t_dirty)
    assert tA["gram_launches"] == 2
    if t_dirty == _tiles(p_pad):
        assert tA["gram_flops"] == full
    else:
        assert tA["gram_flops"] < full
    again, _ = _direct(A, c)                                   # nothing restaged: J'J is reused
    assert np.array_equal(again, dzA) and A.last_timings()["gram_launches"] == 2
    A.stage_jacobian_columns(min(5, p), J1[:, :0])             # count == 0: nothing changes
    again, _ = _direct(A, c)
    assert np.array_equal(again, dzA) and A.last_timings()["gram_launches"] == 2
    A.close(); B.close()


def test_partial_restage_against_the_oracle():
    from oracle import lbfgs_oracle as lo
    n, me, mi, m, nb = SHAPE_A
    c = _inputs(n, me, mi, m)
    ranges = [(120, 140)]
    J1 = _j1(c, ranges)
    ref = lo.direction(c["g"], c["zeta"], c["S"], c["Y"], c["SS"], c["L"], c["D"], Je=J1[:, :me], Ji=J1[:, me:], s=c["s"],
                       lda=c["lda"], reg=1e-12)
    A = _handle(c, nb)
    _stage(A, c, c["J0"])
    _direct(A, c)
    A.stage_jacobian_columns(120, J1[:, 120:140])
    dz, st = _direct(A, c)
    A.close()
    err = _rel(dz, ref)
    print("partial restage n=%d me=%d mi=%d m=%d: rel.err vs oracle %.3e (bound %.0e)" % (n, me, mi, m, err, _tol(n, me, mi)))
    assert st["regularised"] == 0 and st["n_neg"] == 0 and st["n_zero"] == 0
    assert err <= _tol(n, me, mi)


def test_regularised_retry_after_a_partial_restage():
    """An equality column duplicated through a partial restage: the factorisation rejects a pivot, the retry adds reg and
    runs on the same J'J -- one Gram launch, the bits of a handle that staged the whole J1.  The Jacobians are those of
    tests/test_gpu_qn.py::test_regularised_factor_is_only_the_preconditioner (make_qp(96, 24, 40, 4)): the pivots of the
    equality block depend on Je alone, and with these the factorisation is known to reject one."""
    from pyipm_amd.problems import make_qp
    n, me, mi, m, nb = 96, 24, 40, 5, 128
    rng = np.random.default_rng(n + 7 * me + 13 * mi + m)
    qp = make_qp(n, me, mi, 4)
    zeta, S, Y, SS, L, D = _storage(n, m, rng, True, m)
    c = dict(n=n, me=me, mi=mi, m=m, zeta=zeta, S=S, Y=Y, SS=SS, L=L, D=D, s=qp["s"], lda=qp["lam"],
             g=rng.standard_normal(n + 2 * mi + me), J0=np.concatenate([qp["Je"], qp["Ji"]], axis=1))
    J1 = c["J0"].copy()
    J1[:, me - 1] = J1[:, 0]
    A, B = _handle(c, nb), _handle(c, nb)
    _stage(A, c, c["J0"])
    _, st0 = _direct(A, c)
    assert st0["regularised"] == 0 and A.last_timings()["gram_launches"] == 1
    A.stage_jacobian_columns(me - 1, J1[:, me - 1:me])
    dzA, stA = _direct(A, c)
    assert stA["regularised"] == 1 and stA["n_factor"] == 2
    assert A.last_timings()["gram_launches"] == 2
    _stage(B, c, J1)
    dzB, stB = _direct(B, c)
    assert np.all(np.isfinite(dzA))
    assert np.array_equal(dzA, dzB) and stA == stB
    A.close(); B.close()


def test_operator_state_ends_with_a_partial_restage():
    from pyipm_amd.newton import ERRORS, NewtonError
    n, me, mi, m, nb = SHAPE_A
    c = _inputs(n, me, mi, m)
    J1 = _j1(c, [(130, 135)])
    A, F = _handle(c, nb), _handle(c, nb)
    _stage(A, c, c["J0"]); _direct(A, c)
    _stage(F, c, c["J0"]); _direct(F, c)
    _stage(F, c, c["J0"])
    with pytest.raises(NewtonError) as after_full:
        F.solve(c["g"])
    A.stage_jacobian_columns(130, J1[:, 130:135])
    with pytest.raises(NewtonError) as after_columns:
        A.solve(c["g"])
    assert str(after_columns.value) == str(after_full.value)                 # the code and the message
    assert str(after_full.value).startswith(ERRORS[BADARG])
    dz, _ = _direct(A, c)
    assert np.array_equal(A.solve(c["g"]).cpu().numpy(), dz)
    A.close(); F.close()


def test_refusals_leave_the_handle_as_it_was():
    import torch
    from pyipm_amd.newton import MEM_DEVICE
    n, me, mi, m, nb = SHAPE_A
    c = _inputs(n, me, mi, m)
    p = me + mi
    A = _handle(c, nb)
    lib = A.lib
    blk = torch.from_numpy(_j1(c, [(0, p)])).cuda()               # other columns than J0's: a refused call that copied would show
    ptr = ctypes.c_void_p(blk.data_ptr())

    def refused(core, c0, count, pointer, ld, memkind=MEM_DEVICE):
        assert lib.pyipm_lbfgs_stage_jacobian_columns(core.h, c0, count, pointer, ld, memkind) == BADARG
        assert lib.pyipm_lbfgs_last_error(core.h)

    refused(A, 0, 5, ptr, p)                                      # before any full staging
    _stage(A, c, c["J0"])
    dz0, st0 = _direct(A, c)
    for args in ((-1, 5, ptr, p), (p - 4, 5, ptr, p), (0, 5, ptr, 4), (0, 5, ctypes.c_void_p(0), p), (0, -1, ptr, p),
                 (0, 5, ptr, p, 7)):
        refused(A, *args)
        dz, st = _direct(A, c)
        assert np.array_equal(dz, dz0) and st == st0
        assert A.last_timings()["gram_launches"] == 1             # ... on the J'J it had
    assert np.array_equal(A.solve(c["g"]).cpu().numpy(), dz0)     # (a refused call does not end the operator state either)
    A.close()
    # no constraints: count == 0 is the only accepted form
    from oracle import lbfgs_oracle as lo
    U = _core(40, 0, 0, 3)
    zeta, S, Y, SS, L, D, _ = lo.lbfgs_init(40)
    g = np.random.default_rng(5).standard_normal(40)
    before = U.direction(g, None, None, zeta, S, Y, SS, L, D)[0].cpu().numpy()
    refused(U, 0, 1, ptr, 1)
    assert lib.pyipm_lbfgs_stage_jacobian_columns(U.h, 0, 0, None, 0, MEM_DEVICE) == 0
    assert np.array_equal(U.direction(g, None, None, zeta, S, Y, SS, L, D)[0].cpu().numpy(), before)
    U.close()


def test_row_sharded_handle_falls_back_to_the_full_launch():
    """A world of one: the callback returns 0 and leaves the buffer alone.  The columns are copied, the whole of J'J is
    computed (and would be exchanged) again."""
    from pyipm_amd.lbfgs import ALLREDUCE_FN
    n, me, mi, m, nb = SHAPE_A
    c = _inputs(n, me, mi, m)
    p_pad, n_pad = _pads(n, me + mi)
    J1 = _j1(c, [(130, 135)])
    A, B = _handle(c, nb), _handle(c, nb)
    cb = ALLREDUCE_FN(lambda user, ptr, count, stream: 0)
    assert A.lib.pyipm_lbfgs_set_allreduce(A.h, ctypes.cast(cb, ctypes.c_void_p), None) == 0
    _stage(A, c, c["J0"]); _direct(A, c)
    A.stage_jacobian_columns(130, J1[:, 130:135])
    dzA, stA = _direct(A, c)
    tA = A.last_timings()
    _stage(B, c, J1)
    dzB, stB = _direct(B, c)
    assert np.array_equal(dzA, dzB) and stA == stB
    assert tA["gram_flops"] == _flops(n_pad, _tiles(p_pad)) and tA["gram_launches"] == 2
    assert A.lib.pyipm_lbfgs_set_allreduce(A.h, None, None) == 0
    A.close(); B.close()


def _nlp():
    """n = 40: 8 linear equalities, 12 inequalities of which the two in the middle (columns 5 and 6 of Ji) are balls."""
    rng = np.random.default_rng(21)
    n = 40
    xs = 0.3 * rng.standard_normal(n)                      # strictly feasible by construction
    t = xs + 0.5 * rng.standard_normal(n)
    Ae = rng.standard_normal((8, n)) / np.sqrt(n)
    be = Ae @ xs
    G = rng.standard_normal((10, n)) / np.sqrt(n)
    h = G @ xs - 1.0
    c1, c2 = np.zeros(n), np.zeros(n)
    c1[:20], c2[20:] = 1.0, 1.0
    r1, r2 = float(c1 @ xs ** 2) + 1.0, float(c2 @ (xs - 0.1) ** 2) + 1.0

    def ci(x):
        lin = G @ x - h
        return np.concatenate([lin[:5], [r1 - c1 @ x ** 2, r2 - c2 @ (x - 0.1) ** 2], lin[5:]])

    def dci(x):
        return np.concatenate([G[:5].T, (-2.0 * c1 * x)[:, None], (-2.0 * c2 * (x - 0.1))[:, None], G[5:].T], axis=1)

    mask = np.ones(8 + 12, dtype=bool)
    mask[8 + 5:8 + 7] = False
    return dict(x0=xs + 0.01 * rng.standard_normal(n), f=lambda x: 0.5 * float((x - t) @ (x - t)), df=lambda x: x - t,
                ce=lambda x: Ae @ x - be, dce=lambda x: Ae.T.copy(), ci=ci, dci=dci), mask


@pytest.mark.parametrize("resident", [False, True], ids=["host_pairs", "resident_pairs"])
def test_ipm_with_a_column_mask_is_the_unmasked_run(resident):
    from pyipm_amd.ipm import IPM
    prob, mask = _nlp()
    runs = []
    for lin in (False, mask):
        ipm = IPM(lbfgs=4, Ftol=1.0e-8, verbosity=-1, device=0, linear_constraints=lin, resident_pairs=resident, **prob)
        with np.errstate(all="ignore"):
            x, s, lda, fval, kkt = ipm.solve()
        runs.append((x, s, lda, ipm.iter_count, ipm.backend))
    (x0, s0, l0, it0, b0), (x1, s1, l1, it1, b1) = runs
    print("iterations %d, columns staged %d unmasked, %d with the mask" % (it0, b0.n_cols_staged, b1.n_cols_staged))
    assert it0 == it1 and it0 > 2
    assert np.array_equal(x0, x1) and np.array_equal(s0, s1) and np.array_equal(l0, l1)
    assert b1.column_runs == [(13, 15)] and b0.column_runs is None
    assert b0.n_cols_staged == 20 * b0.n_calls and b1.n_cols_staged == 20 + 2 * (b1.n_calls - 1)
    assert b1.n_cols_staged < b0.n_cols_staged
    assert b1.n_staged == 1 and b0.n_staged == b0.n_calls


def test_all_true_and_all_false_masks_are_the_bools():
    from pyipm_amd.ipm import HipLbfgsBackend
    for mask, want in ((np.ones(7, dtype=bool), True), (np.zeros(7, dtype=bool), False), ([True] * 7, True)):
        b = HipLbfgsBackend(30, 3, 4, 2, device=0, linear_constraints=mask)
        assert b.linear_constraints is want and b.column_runs is None
        b.core.close()
    with pytest.raises(ValueError):
        HipLbfgsBackend(30, 3, 4, 2, device=0, linear_constraints=[True, False])
