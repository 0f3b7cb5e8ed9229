"""The quasi-Newton KKT operator of an L-BFGS direction for k columns per call (include/pyipm_newton.h,
pyipm_lbfgs_kkt_matvec_many / pyipm_lbfgs_kkt_solve_many; LbfgsCore.matvec_many / solve_many) against the longdouble operator of
tests/test_gpu_qn.py, against the single-column entries on the same handle, and bit for bit against itself.

Shapes: the smallest at which each partition can go wrong -- n below every chunk, mi = 0, me = 0 with two 128-column tiles,
no pairs, full memory with p_pad = 384 and a ragged n, more than one split of n.  Column counts: one column, a ragged block,
a full block of 64, a block plus one, three blocks.  The longdouble references are formed once per shape for the 130 columns
and shared; the smaller column counts take the leading columns of the same block.

Figures measured on the MI355X are printed before each assertion; DESIGN.md section 7d records them: the product's worst
ratio to eps | |K||v| | is 0.705 (at n = 5) against C_OP = 1.74; the solve's backward error is at most 2.42 x the single-column
solve's (2.27 x after one refinement step) against the bound of 8."""
import ctypes
import functools

import numpy as np
import pytest

from test_gpu_qn import C_OP, EPS, LD, REFINE_CASES, Operator, _make      # noqa: F401  (Operator: the type of case.K)

pytestmark = pytest.mark.gpu

SHAPES = [(5, 1, 2, 3, 3), (64, 20, 0, 2, 2), (130, 0, 129, 3, 3), (300, 64, 64, 0, 1), (777, 65, 191, 31, 32),
          (8300, 100, 200, 4, 4)]
IDS = ["n%d_me%d_mi%d_m%d" % s[:4] for s in SHAPES]
KS = [1, 3, 64, 65, 130]
KMAX = 130
# columns whose solves are compared one by one with the single-column entries: both ends of each block of 64 and the ragged tail
PICK = [0, 1, 2, 63, 64, 65, 127, 128, 129]
E_BADARG = -1


@functools.lru_cache(maxsize=None)
def _case(shape):
    n, me, mi, m, cap = shape
    c = _make(n, me, mi, m, cap)
    rng = np.random.default_rng(1000 + n)
    c.Vm = rng.standard_normal((c.N, KMAX))                 # solution-space columns (not solutions)
    c.Bm = rng.standard_normal((c.N, KMAX))                 # right-hand sides
    return c


@functools.lru_cache(maxsize=None)
def _product_reference(shape):
    """K v_j in longdouble for the 130 columns, and | |K||v_j| |_2 in float64 (the matrix form of Operator.abs_apply)."""
    c = _case(shape)
    K, n, me, mi = c.K, c.n, c.me, c.mi
    ref = np.stack([K.apply(c.Vm[:, j]) for j in range(KMAX)], axis=1)
    K.abs_apply(c.Vm[:, 0])                                 # (forms K.absBk)
    a = np.abs(c.Vm)
    ax, as_, al = a[:n], a[n:n + mi], a[n + mi:]
    Ja = np.abs(K.J).astype(float)
    ol = Ja.T @ ax
    ol[me:] += as_
    full = np.concatenate([K.absBk @ ax + Ja @ al, K.sig.astype(float)[:, None] * as_ + al[me:], ol])
    return ref, np.linalg.norm(full, axis=0)


def _flip_rows(c, A):
    W = np.array(A, dtype=float)
    W[c.n + c.mi:] = -W[c.n + c.mi:]
    return W


def _np(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("flip", [False, True], ids=["raw", "flip"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_product_against_extended_precision(shape, flip):
    """Every column of every column count: |out_j - K v_j|_2 <= C_OP eps | |K||v_j| |_2, the single-column product's constant."""
    c = _case(shape)
    ref, scale = _product_reference(shape)
    arg = _flip_rows(c, c.Vm) if flip else c.Vm
    worst = 0.0
    for k in KS:
        out = _np(c.core.matvec_many(arg[:, :k], flip=flip))
        assert out.shape == (c.N, k)
        err = np.linalg.norm(out.astype(LD) - ref[:, :k], axis=0).astype(float)
        ratio = err / (EPS * scale[:k])
        worst = max(worst, float(ratio.max()))
        print("product %s flip=%d k=%d: worst column %.3f eps | |K||v| |" % (shape[:4], flip, k, ratio.max()))
        assert np.all(err <= C_OP * EPS * scale[:k]), (k, int(np.argmax(ratio)), float(ratio.max()))
    print("product %s flip=%d: worst ratio over all k %.3f (bound %.2f)" % (shape[:4], flip, worst, C_OP))


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_solve_against_the_single_column_solve(shape):
    """Backward error |rhs_j - K x_j|_2 / |rhs_j|_2 in longdouble: the many-column value at most 8 x what pyipm_qn_solve reaches
    for the same column on the same handle (the margin: solve_many_plain instead of solve_plain); with refine = 1 against
    LbfgsCore.refine(refine=1) of that column.  The columns of PICK of the k = 130 call one by one; every smaller k gives the
    bits of those columns (the property test_bits states), so it is held to the same figures."""
    c = _case(shape)
    for refine in (0, 1):
        X = _np(c.core.solve_many(c.Bm, refine=refine))
        for k in KS[:-1]:
            np.testing.assert_array_equal(_np(c.core.solve_many(c.Bm[:, :k], refine=refine)), X[:, :k])
        worst = 0.0
        for j in PICK:
            b = c.Bm[:, j]
            x1 = c.core.solve(b)
            if refine:
                x1, _ = c.core.refine(x1, rhs=b, refine=1)
            e1, ek = c.K.berr(_np(x1), b), c.K.berr(X[:, j], b)
            worst = max(worst, ek / e1)
            print("solve %s refine=%d column %d: berr many %.3e, single %.3e, ratio %.2f" % (shape[:4], refine, j, ek, e1, ek / e1))
            assert ek <= 8.0 * e1, (refine, j, ek, e1)
        print("solve %s refine=%d: worst ratio many / single %.2f (bound 8)" % (shape[:4], refine, worst))


@pytest.mark.parametrize("case", REFINE_CASES, ids=["n%d_me%d_mi%d_m%d_sig1e%d" % k[:5] for k in REFINE_CASES])
def test_adaptive_refinement_of_a_block(case):
    """refine = -1 on 65 columns (the direction's g first): wherever every single-column refine(-1) converges the block does,
    every column then meets the bound the single-column test sets (1e-13 test-side), and the block takes at least as many
    steps as the slowest single column."""
    n, me, mi, m, spread, seed = case
    c = _make(n, me, mi, m, max(m, 1), spread=spread, seed=seed, qp_seed=8)
    k = 65
    B = np.random.default_rng(seed).standard_normal((c.N, k))
    B[:, 0] = c.g
    single = []
    for j in range(k):
        x, info = c.core.refine(c.core.solve(B[:, j]), rhs=B[:, j], refine=-1)
        single.append(info)
    X = _np(c.core.solve_many(B, refine=-1))
    info = c.core.refine_info()
    berr = [c.K.berr(X[:, j], B[:, j]) for j in range(k)]
    steps1 = max(i["steps"] for i in single)
    print("adaptive %s k=%d: block %s; single-column steps max %d, converged %d of %d, worst single berr %.3e; "
          "test-side block berr worst %.3e" % (case[:5], k, info, steps1, sum(i["converged"] for i in single), k,
                                               max(i["berr"] for i in single), max(berr)))
    assert info["steps"] >= steps1
    if all(i["converged"] for i in single):
        assert info["converged"] and info["berr"] <= 1e-14
        assert max(berr) <= 1e-13
    c.core.close()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_bits(shape):
    """Column j of a k = 130 call = the same vector alone = at another position = beside a NaN and an all-zero column, for the
    product and for the solve with refine 0 and 2; two identical calls agree; flip only changes the sign of the multiplier rows."""
    c = _case(shape)
    j, other = 70, 5
    calls = [("matvec", lambda A, **kw: c.core.matvec_many(A, **kw), c.Vm, {}),
             ("solve", lambda A, **kw: c.core.solve_many(A, **kw), c.Bm, {"refine": 0}),
             ("solve+2", lambda A, **kw: c.core.solve_many(A, **kw), c.Bm, {"refine": 2})]
    for name, fn, A, kw in calls:
        full = _np(fn(A, **kw))
        np.testing.assert_array_equal(_np(fn(A, **kw)), full, err_msg=name + ": two identical calls")
        np.testing.assert_array_equal(_np(fn(A[:, j:j + 1], **kw))[:, 0], full[:, j], err_msg=name + ": alone")
        moved = np.random.default_rng(3).standard_normal(A.shape)
        moved[:, other] = A[:, j]
        np.testing.assert_array_equal(_np(fn(moved, **kw))[:, other], full[:, j], err_msg=name + ": another position")
        trio = np.stack([np.full(c.N, np.nan), A[:, j], np.zeros(c.N)], axis=1)
        got = _np(fn(trio, **kw))
        np.testing.assert_array_equal(got[:, 1], full[:, j], err_msg=name + ": beside NaN and zero")
        assert np.isnan(got[:, 0]).any() and np.all(got[:, 2] == 0.0), name + ": the NaN column stays in its column"
    # flip: solution-space blocks have their multiplier rows negated on read (v) and on write (dz)
    np.testing.assert_array_equal(_np(c.core.matvec_many(_flip_rows(c, c.Vm), flip=True)), _np(c.core.matvec_many(c.Vm)))
    np.testing.assert_array_equal(_np(c.core.solve_many(c.Bm, flip=True, refine=2)), _flip_rows(c, _np(c.core.solve_many(c.Bm, refine=2))))


def _raw(c, entry, A, ld, memkind, flip=0, refine=0):
    """The C entry on blocks of leading dimension ld >= N, gaps and outputs poisoned with NaN; returns the (k, ld) output."""
    import torch
    from pyipm_amd.newton import MEM_HOST
    k = A.shape[1]
    src = np.full((k, ld), np.nan)
    src[:, :c.N] = A.T
    dst = np.full((k, ld), np.nan)
    lib = c.core.lib
    c.core._stream()
    if memkind == MEM_HOST:
        pin, pout = ctypes.c_void_p(src.ctypes.data), ctypes.c_void_p(dst.ctypes.data)
    else:
        tin, tout = torch.from_numpy(src).to(c.core.device), torch.from_numpy(dst).to(c.core.device)
        pin, pout = ctypes.c_void_p(tin.data_ptr()), ctypes.c_void_p(tout.data_ptr())
    if entry == "matvec":
        rc = lib.pyipm_lbfgs_kkt_matvec_many(c.core.h, k, pin, ld, pout, ld, flip, memkind)
    else:
        rc = lib.pyipm_lbfgs_kkt_solve_many(c.core.h, k, pin, ld, pout, ld, flip, refine, memkind)
    assert rc == 0, lib.pyipm_lbfgs_last_error(c.core.h)
    if memkind != MEM_HOST:
        torch.cuda.synchronize()
        dst = tout.cpu().numpy()
    return dst


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[4], SHAPES[5]], ids=[IDS[0], IDS[4], IDS[5]])
def test_padded_leading_dimension_and_host_blocks(shape):
    """ld > N gives the bits of ld = N and leaves the entries N .. ld-1 of every output column untouched (NaN before, NaN after);
    PYIPM_MEM_HOST blocks give the bits of device blocks."""
    from pyipm_amd.newton import MEM_DEVICE, MEM_HOST
    c = _case(shape)
    k = 67
    for entry, A, kw in (("matvec", c.Vm[:, :k], {}), ("solve", c.Bm[:, :k], {"refine": 0}), ("solve", c.Bm[:, :k], {"refine": 2})):
        want = _raw(c, entry, A, c.N, MEM_DEVICE, **kw)
        assert not np.isnan(want).any()
        for memkind in (MEM_DEVICE, MEM_HOST):
            got = _raw(c, entry, A, c.N + 3, memkind, **kw)
            np.testing.assert_array_equal(got[:, :c.N], want)
            assert np.all(np.isnan(got[:, c.N:]))
        np.testing.assert_array_equal(_raw(c, entry, A, c.N, MEM_HOST, flip=1, **kw),
                                      _raw(c, entry, A, c.N, MEM_DEVICE, flip=1, **kw))


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_kept_state_survives(shape):
    """After both calls (a refined solve included) pyipm_qn_solve(rhs = g) still returns the direction bit for bit, no Gram
    launch was added, and a repeated direction returns the bits of the first."""
    c = _case(shape)
    launches = c.core.last_timings()["gram_launches"]
    c.core.matvec_many(c.Vm)
    c.core.solve_many(c.Bm, refine=-1)
    c.core.solve_many(c.Bm[:, :3])
    np.testing.assert_array_equal(_np(c.core.solve(c.g)), c.dz)
    dz2, _ = c.direct()
    assert c.core.last_timings()["gram_launches"] == launches
    np.testing.assert_array_equal(_np(dz2), c.dz)


def test_wrong_shapes_raise_value_error():
    c = _case(SHAPES[1])
    for bad in (np.zeros(c.N), np.zeros((c.N + 1, 2)), np.zeros((2, c.N))):
        with pytest.raises(ValueError):
            c.core.matvec_many(bad)
        with pytest.raises(ValueError):
            c.core.solve_many(bad)


def test_refusals_are_codes_with_a_message():
    import torch
    from pyipm_amd.lbfgs import ALLREDUCE_FN, LbfgsCore
    from pyipm_amd.newton import MEM_DEVICE
    from oracle import lbfgs_oracle as lo
    c = _make(96, 24, 40, 5, 5, qp_seed=4)
    lib, N, k = c.core.lib, c.N, 3
    vin = torch.ones((k, N + 2), dtype=torch.float64, device="cuda:0")
    out = torch.full((k, N + 2), 7.0, dtype=torch.float64, device="cuda:0")
    pv, po = ctypes.c_void_p(vin.data_ptr()), ctypes.c_void_p(out.data_ptr())

    def both(core, kk, a, lda, b, ldb, memkind=MEM_DEVICE):
        return (lib.pyipm_lbfgs_kkt_matvec_many(core.h, kk, a, lda, b, ldb, 0, memkind),
                lib.pyipm_lbfgs_kkt_solve_many(core.h, kk, a, lda, b, ldb, 0, 0, memkind))

    def refused(core, word, *args, **kw):
        for rc in both(core, *args, **kw):
            msg = lib.pyipm_lbfgs_last_error(core.h).decode()
            assert rc == E_BADARG and msg and word in msg, (rc, msg)

    ok = (k, pv, N + 2, po, N + 2)
    fresh = LbfgsCore(96, 24, 40, 5, device=0)
    fresh.stage_jacobian(c.Je, c.Ji)
    refused(fresh, "no direction", *ok)                    # no direction since create
    fresh.close()
    c.core.stage_jacobian_columns(3, c.Je[:, 3:5])
    refused(c.core, "no direction", *ok)                   # ... since a restaging
    np.testing.assert_array_equal(_np(c.direct()[0]), c.dz)
    unc = LbfgsCore(40, 0, 0, 3, device=0)                 # me + mi = 0
    zeta, S, Y, SS, L, D, _ = lo.lbfgs_init(40)
    unc.direction(np.ones(40), None, None, zeta, S, Y, SS, L, D)
    refused(unc, "no constraints", k, pv, 40, po, 40)
    unc.close()
    refused(c.core, "null", k, None, N, po, N)
    refused(c.core, "null", k, pv, N, None, N)
    refused(c.core, "leading dimension", k, pv, N - 1, po, N + 2)
    refused(c.core, "leading dimension", k, pv, N + 2, po, N - 1)
    refused(c.core, "k < 0", -1, pv, N + 2, po, N + 2)
    refused(c.core, "memkind", k, pv, N + 2, po, N + 2, memkind=7)
    inside = ctypes.c_void_p(vin.data_ptr() + 8 * (N + 2))  # out = column 1 of v
    rc = lib.pyipm_lbfgs_kkt_matvec_many(c.core.h, k, pv, N + 2, inside, N + 2, 0, MEM_DEVICE)
    assert rc == E_BADARG and "overlap" in lib.pyipm_lbfgs_last_error(c.core.h).decode()
    assert both(c.core, 0, pv, N + 2, po, N + 2) == (0, 0)  # k == 0: nothing to do
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((vin == 1.0).all())          # no refusal wrote anything
    np.testing.assert_array_equal(_np(c.direct()[0]), c.dz)               # ... and the handle still produces the same direction
    # an all-reduce callback makes the handle a row-sharded one: refused until it is taken out and a direction has run
    cb = ALLREDUCE_FN(lambda user, ptr, count, stream: 0)
    assert lib.pyipm_lbfgs_set_allreduce(c.core.h, ctypes.cast(cb, ctypes.c_void_p), None) == 0
    c.direct()
    refused(c.core, "row-sharded", *ok)
    assert lib.pyipm_lbfgs_set_allreduce(c.core.h, None, None) == 0
    refused(c.core, "no direction", *ok)
    np.testing.assert_array_equal(_np(c.direct()[0]), c.dz)
    assert both(c.core, *ok) == (0, 0)
    torch.cuda.synchronize()
    c.core.close()
