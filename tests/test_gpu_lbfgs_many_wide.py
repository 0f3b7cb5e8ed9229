"""The many-column quasi-Newton KKT operator of an L-BFGS direction (pyipm_lbfgs_kkt_matvec_many / pyipm_lbfgs_kkt_solve_many;
kernels_qnmany.hpp, qnmany_impl.hpp) in the column-count regimes tests/test_gpu_lbfgs_many.py never enters, and on three edges
of its geometry:

  1. 256 < k: qm_jt loops over groups of QM_GROUP columns; the second and later k_qm_jt / k_qm_jt_reduce launches reuse the
     partial buffer with another kcols (its stride) and work at P + j0 * ldo, B + j0 * ldb; the last group is ragged.
  2. 4096 < k: every column-walking kernel (grid.y = QM_YMAX) takes a second trip of its column loop, k_qm_gram through its
     shared staging between two barriers.
  3. m = 32 (r = 2m = 64, the upper edge of k_qm_gram, k_qm_hs and small_solve_body) on a shape whose qm_nsplit is two splits
     with a last split of one K step plus one row.
  4. matvec / solve / matvec_many / solve_many after a partial restage that CHANGED J: they must use the new J.

No tolerance is new here.  Every assertion is either bit equality -- a wide call against the concatenation of calls on
consecutive chunks of at most 130 columns of the same block, the regime test_gpu_lbfgs_many.py holds to extended precision and
whose columns the project states to be independent of k, of position and of the other columns -- or one of that module's two
bounds with its constants: C_OP of tests/test_gpu_qn.py for the product against the longdouble Operator, and the factor 8 over
the single-column solve of the same column on the same handle for the backward error.  The columns held to those bounds in
parts 1 and 2 are columns of the existing module's own blocks (c.Vm, c.Bm), placed at the edges of the groups and of the walk.

An adaptive call (refine = -1) decides on the worst column of ITS block, so a wide call may take more steps than a chunk;
its bits are therefore those of the chunked calls with the fixed count refine = steps of the wide call (a step taken back
leaves the saved iterate, bit for bit the one after that many steps), and of a chunk's own adaptive call wherever that
chunk took as many steps.

Figures measured on the MI355X are printed before each assertion; DESIGN.md section 7d records them."""
import functools

import numpy as np
import pytest

from test_gpu_qn import C_OP, EPS, LD, Operator, _make
from test_gpu_lbfgs_many import KS, PICK, _case, _flip_rows, _raw

pytestmark = pytest.mark.gpu

# Restated from pyipm_amd/csrc/kernels_qnmany.hpp: QM_GROUP (columns per launch of k_qm_jt), QM_YMAX (grid.y of the
# column-walking kernels), QM_TR / QM_KC (rows of a tile / the K step, which qm_nsplit rounds to).  REGIME is worked out by hand
# from them: (launch groups = ceil(k / QM_GROUP), second trip of the column walk = k > QM_YMAX).  A change of either constant
# in the library leaves these tests in another regime than their names say: look here then.
QM_GROUP = 256
QM_YMAX = 4096
QM_TR = 64
QM_KC = 64
REGIME = {257: (2, False), 300: (2, False), 512: (2, False), 577: (3, False), 4097: (17, True), 4200: (17, True)}
CHUNK = 130                                   # KMAX of tests/test_gpu_lbfgs_many.py: one group, one trip of every loop

SHAPE_SPLITS = (777, 65, 191, 31, 32)         # four row splits, p_pad = 256
SHAPE_TILES = (130, 0, 129, 3, 3)             # me = 0, two 128-column tiles (a padding column of p_pad), N = 388
SHAPE_TINY = (5, 1, 2, 3, 3)                  # me > 0, mi > 0, n below every chunk, N = 10
SHAPE_M32 = (257, 33, 64, 32, 32)             # r = 64, p = 97 (31 padding columns), two row splits: 192 + 65 rows
SHAPE_RESTAGE = (600, 100, 200, 4, 4)         # SHAPE_A of tests/test_gpu_lbfgs_columns.py, p_pad = 384

EDGE_GROUP = [0, 255, 256, 257, 319, 320]     # ... and k - 1: both sides of the first group's end and of its first 64 columns
EDGE_WALK = [0, 4095, 4096, 4097]             # ... and k - 1, and 4150 inside the second trip where k reaches it
WIDE = [(s, k) for s in (SHAPE_SPLITS, SHAPE_TILES) for k in (257, 300, 512, 577)] + \
       [(s, k) for s in (SHAPE_TINY, SHAPE_TILES) for k in (4097, 4200)]
WIDE_IDS = ["n%d_me%d_mi%d_m%d-k%d" % (s[:4] + (k,)) for s, k in WIDE]


def _np(t):
    return t.cpu().numpy()


def _regime(k):
    return (-(-k // QM_GROUP), k > QM_YMAX)


def _nsplit(n, p_pad):
    """qm_nsplit of pyipm_amd/csrc/qnmany_impl.hpp, restated: (splits of n in k_qm_jt, rows per split)."""
    tiles = p_pad // QM_TR
    s = max(1, min(-(-1024 // tiles), (n + 255) // 256))
    per = -(-(-(-n // s)) // QM_KC) * QM_KC
    return -(-n // per), per


def _edges(k):
    base = (EDGE_WALK + [k - 1, 4150]) if k > QM_YMAX else (EDGE_GROUP + [k - 1])
    out = []
    for e in base:
        if 0 <= e < k and e not in out:
            out.append(e)
    return out


def _block(c, k, src, seed):
    """Standard-normal columns with column i of `src` (c.Vm or c.Bm of the existing module) at the i-th edge position."""
    A = np.random.default_rng(seed).standard_normal((c.N, k))
    for i, e in enumerate(_edges(k)):
        A[:, e] = src[:, i]
    return A


def _chunks(k):
    return [(a, min(a + CHUNK, k)) for a in range(0, k, CHUNK)]


def _chunked(fn, A, **kw):
    return np.concatenate([_np(fn(A[:, a:b], **kw)) for a, b in _chunks(A.shape[1])], axis=1)


def _product_error(K, V, out):
    """|out_j - K v_j|_2 with K v_j in longdouble, and | |K||v_j| |_2 in float64 (the matrix form of Operator.abs_apply, as
    _product_reference of tests/test_gpu_lbfgs_many.py), for every column."""
    n, me, mi = K.n, K.me, K.mi
    ref = np.stack([K.apply(V[:, j]) for j in range(V.shape[1])], axis=1)
    K.abs_apply(V[:, 0])                                    # (forms K.absBk)
    a = np.abs(V)
    ax, as_, al = a[:n], a[n:n + mi], a[n + mi:]
    Ja = np.abs(K.J).astype(float)
    ol = Ja.T @ ax
    ol[me:] += as_
    full = np.concatenate([K.absBk @ ax + Ja @ al, K.sig.astype(float)[:, None] * as_ + al[me:], ol])
    return np.linalg.norm(out.astype(LD) - ref, axis=0).astype(float), np.linalg.norm(full, axis=0)


def _check_product(c, k, tag, all_columns=False):
    """matvec_many raw and flipped on a k-column block: the bits of the chunked calls over every column; the C_OP bound of
    tests/test_gpu_qn.py at the edge columns (columns of c.Vm).  Returns the worst edge ratio."""
    edges = _edges(k)
    V = _block(c, k, c.Vm, 2000 + k)
    out = _np(c.core.matvec_many(V))
    assert out.shape == (c.N, k)
    np.testing.assert_array_equal(out, _chunked(c.core.matvec_many, V), err_msg="%s: raw, wide against chunks" % tag)
    Vf = _flip_rows(c, V)
    outf = _np(c.core.matvec_many(Vf, flip=True))
    np.testing.assert_array_equal(outf, _chunked(c.core.matvec_many, Vf, flip=True), err_msg="%s: flipped, wide against chunks" % tag)
    np.testing.assert_array_equal(outf, out, err_msg="%s: flip changes the reading of v only" % tag)
    for i, e in enumerate(edges):
        np.testing.assert_array_equal(V[:, e], c.Vm[:, i])
    err, scale = _product_error(c.K, V[:, edges], out[:, edges])
    ratio = err / (EPS * scale)
    print("product %s: edge columns %s: ratios to eps | |K||v| | %s, worst %.3f (bound C_OP = %.2f)"
          % (tag, edges, np.array2string(ratio, precision=3), ratio.max(), C_OP))
    assert np.all(err <= C_OP * EPS * scale), (edges, ratio)
    if all_columns:
        # a record, not an assertion: C_OP was measured on the vectors of the existing suite, which the edge columns are
        assert np.all(np.isfinite(out))
        err, scale = _product_error(c.K, V, out)
        ratio = err / (EPS * scale)
        print("RECORD product %s: all %d columns: worst ratio %.3f at column %d (C_OP = %.2f, asserted at the edge columns)"
              % (tag, k, ratio.max(), int(np.argmax(ratio)), C_OP))
    return float(ratio.max())


def _check_solves(c, k, tag):
    """solve_many with refine 0, 1 and -1 on a k-column block: the bits of the chunked calls over every column; at the edge
    columns (columns of c.Bm) the backward error in longdouble at most 8 x that of the single-column solve of the same
    column on the same handle (refine(refine=1) of it where refine = 1), the bound of tests/test_gpu_lbfgs_many.py.
    Returns the worst many / single ratio."""
    edges = _edges(k)
    B = _block(c, k, c.Bm, 3000 + k)
    solve = c.core.solve_many
    worst = 0.0
    for refine in (0, 1):
        X = _np(solve(B, refine=refine))
        assert X.shape == (c.N, k)
        np.testing.assert_array_equal(X, _chunked(solve, B, refine=refine), err_msg="%s: refine=%d, wide against chunks" % (tag, refine))
        if refine == 0:
            np.testing.assert_array_equal(_np(solve(B, flip=True)), _flip_rows(c, X), err_msg="%s: flipped output" % tag)
        for i, e in enumerate(edges):
            b = c.Bm[:, i]
            np.testing.assert_array_equal(B[:, e], b)
            x1 = c.core.solve(b)
            if refine:
                x1, _ = c.core.refine(x1, rhs=b, refine=1)
            e1, ek = c.K.berr(_np(x1), b), c.K.berr(X[:, e], b)
            worst = max(worst, ek / e1)
            print("solve %s refine=%d column %d: berr many %.3e, single %.3e, ratio %.2f" % (tag, refine, e, ek, e1, ek / e1))
            assert ek <= 8.0 * e1, (refine, e, ek, e1)
    # adaptive: the chunks first (each with its own outcome), then the wide call
    parts, infos = [], []
    for a, b in _chunks(k):
        parts.append(_np(solve(B[:, a:b], refine=-1)))
        infos.append(c.core.refine_info())
    Xa = _np(solve(B, refine=-1))
    info = c.core.refine_info()
    steps = [i["steps"] for i in infos]
    print("solve %s refine=-1: wide %s; chunks: steps %d .. %d, converged %d of %d"
          % (tag, info, min(steps), max(steps), sum(i["converged"] for i in infos), len(infos)))
    assert info["steps"] >= max(steps)
    if all(i["converged"] for i in infos):
        assert info["converged"]
    np.testing.assert_array_equal(Xa, _chunked(solve, B, refine=info["steps"]),
                                  err_msg="%s: adaptive, wide against chunks at its step count" % tag)
    for (a, b), part, i in zip(_chunks(k), parts, infos):
        if i["steps"] == info["steps"]:
            np.testing.assert_array_equal(Xa[:, a:b], part, err_msg="%s: adaptive, columns %d .. %d" % (tag, a, b - 1))
    # The default target (1e-14) is met before the first step on these shapes.  Under a target nobody meets the loop saves,
    # corrects and stops on stagnation, or takes a worse step back; either way the wide call leaves what its step count says.
    c.core.set_option("refine_target", 1e-30)
    try:
        Xt = _np(solve(B, refine=-1))
        forced = c.core.refine_info()
    finally:
        c.core.set_option("refine_target", 1e-14)          # (the library's default: the handles of _case are shared)
    print("solve %s refine=-1 under refine_target 1e-30: wide %s" % (tag, forced))
    assert not forced["converged"]
    np.testing.assert_array_equal(Xt, _chunked(solve, B, refine=forced["steps"]),
                                  err_msg="%s: adaptive under a target nobody meets, wide against chunks at its step count" % tag)
    print("RECORD solve %s: worst berr ratio many / single %.2f (bound 8)" % (tag, worst))
    return worst


# ---- 1 and 2: past one launch group, past one column walk

@pytest.mark.parametrize("shape,k", WIDE, ids=WIDE_IDS)
def test_wide_product(shape, k):
    assert _regime(k) == REGIME[k]
    c = _case(shape)
    tag = "%s k=%d" % (shape[:4], k)
    # the all-column longdouble reference: 4200 Operator.apply calls of N = 388, about a second on the host
    _check_product(c, k, tag, all_columns=(shape == SHAPE_TILES and k > QM_YMAX))


@pytest.mark.parametrize("shape,k", WIDE, ids=WIDE_IDS)
def test_wide_solve(shape, k):
    assert _regime(k) == REGIME[k]
    c = _case(shape)
    _check_solves(c, k, "%s k=%d" % (shape[:4], k))


def test_wide_host_blocks_with_a_padded_leading_dimension():
    """k = 4097 through the C entry: PYIPM_MEM_HOST blocks with ld = N + 3 give the bits of device blocks with ld = N, and the
    gap entries N .. ld-1 of every output column keep their NaN."""
    from pyipm_amd.newton import MEM_DEVICE, MEM_HOST
    k = 4097
    assert _regime(k) == REGIME[k]
    c = _case(SHAPE_TINY)
    for entry, A, kw in (("matvec", _block(c, k, c.Vm, 2000 + k), {}), ("solve", _block(c, k, c.Bm, 3000 + k), {"refine": 2})):
        want = _raw(c, entry, A, c.N, MEM_DEVICE, **kw)
        assert want.shape == (k, c.N) and not np.isnan(want).any()
        got = _raw(c, entry, A, c.N + 3, MEM_HOST, **kw)
        np.testing.assert_array_equal(got[:, :c.N], want, err_msg=entry)
        assert np.all(np.isnan(got[:, c.N:])), entry
        call = c.core.matvec_many(A) if entry == "matvec" else c.core.solve_many(A, **kw)
        np.testing.assert_array_equal(_np(call).T, want, err_msg=entry + ": the Python call")


# ---- 3: m = 32 and the two-split edge

@functools.lru_cache(maxsize=None)
def _m32():
    n, me, mi, m, cap = SHAPE_M32
    c = _make(n, me, mi, m, cap)                  # (asserts that the oracle's lbfgs_update kept all 32 pairs)
    rng = np.random.default_rng(1000 + n)         # as _case of tests/test_gpu_lbfgs_many.py
    c.Vm = rng.standard_normal((c.N, CHUNK))
    c.Bm = rng.standard_normal((c.N, CHUNK))
    return c


@functools.lru_cache(maxsize=None)
def _restage_inputs():
    return _make(*SHAPE_RESTAGE)


@pytest.fixture(scope="module", autouse=True)
def _close_own_handles():
    """The handles of _case are shared with tests/test_gpu_lbfgs_many.py and stay open; this module's own are closed."""
    yield
    for cached in (_m32, _restage_inputs):
        if cached.cache_info().currsize:
            cached().core.close()
        cached.cache_clear()


def test_m32_geometry():
    n, me, mi, m, cap = SHAPE_M32
    p = me + mi
    p_pad = (p + 127) // 128 * 128
    nsplit, kper = _nsplit(n, p_pad)
    assert (2 * m, p, p_pad, p_pad - p) == (64, 97, 128, 31)
    assert (nsplit, kper, n - (nsplit - 1) * kper) == (2, 192, 65)          # the last split: one K step plus one row
    assert _nsplit(777, 256)[0] == 4 and _nsplit(130, 256)[0] == 1 and _nsplit(5, 128)[0] == 1 and _nsplit(600, 384) == (3, 256)
    c = _m32()
    assert c.store[1].shape[1] == 32 and c.core.cap == 32


@pytest.mark.parametrize("flip", [False, True], ids=["raw", "flip"])
def test_m32_product_against_extended_precision(flip):
    """test_product_against_extended_precision of tests/test_gpu_lbfgs_many.py on the m = 32 shape: every column of every
    column count of KS within C_OP.  (A ratio above C_OP here would be a finding about the r = 64 sums, not a reason to
    widen the constant.)  Then the single-column product of tests/test_gpu_qn.py, as that module tests it."""
    c = _m32()
    arg = _flip_rows(c, c.Vm) if flip else c.Vm
    worst = 0.0
    for k in KS:
        out = _np(c.core.matvec_many(arg[:, :k], flip=flip))
        assert out.shape == (c.N, k)
        err, scale = _product_error(c.K, c.Vm[:, :k], out)
        ratio = err / (EPS * scale)
        worst = max(worst, float(ratio.max()))
        print("product m32 flip=%d k=%d: worst column %.3f eps | |K||v| |" % (flip, k, ratio.max()))
        assert np.all(err <= C_OP * EPS * scale), (k, int(np.argmax(ratio)), float(ratio.max()))
    print("RECORD product m32 %s flip=%d: worst ratio over all k %.3f (bound C_OP = %.2f)" % (SHAPE_M32[:4], flip, worst, C_OP))
    v = np.random.default_rng(17).standard_normal(c.N)
    arg = _flip_rows(c, v[:, None])[:, 0] if flip else v
    out = _np(c.core.matvec(arg, flip=flip))
    np.testing.assert_array_equal(out, _np(c.core.matvec(arg, flip=flip)))
    err, scale = _product_error(c.K, v[:, None], out[:, None])
    print("RECORD operator m32 single column flip=%d: %.3f eps | |K||v| | (bound C_OP = %.2f)" % (flip, err[0] / (EPS * scale[0]), C_OP))
    assert err[0] <= C_OP * EPS * scale[0]


def test_m32_solve_against_the_single_column_solve():
    """test_solve_against_the_single_column_solve of tests/test_gpu_lbfgs_many.py on the m = 32 shape."""
    c = _m32()
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
            print("solve m32 refine=%d column %d: berr many %.3e, single %.3e, ratio %.2f" % (refine, j, ek, e1, ek / e1))
            assert ek <= 8.0 * e1, (refine, j, ek, e1)
        print("RECORD solve m32 refine=%d: worst ratio many / single %.2f (bound 8)" % (refine, worst))
    np.testing.assert_array_equal(_np(c.core.solve(c.g)), c.dz)              # the kept state is as the direction left it


def test_m32_past_one_group():
    k = 257
    assert _regime(k) == REGIME[k]
    c = _m32()
    _check_product(c, k, "m32 k=%d" % k)
    _check_solves(c, k, "m32 k=%d" % k)


# ---- 4: the operator after a partial restage that changed J

RANGES = [("across_a_tile_boundary", [(120, 140)]), ("across_je_ji", [(95, 110)]), ("all_columns", [(0, 300)])]


@pytest.mark.parametrize("name,ranges", RANGES, ids=[r[0] for r in RANGES])
def test_operator_after_a_restage_that_changed_j(name, ranges):
    """Handle A (J0 staged, a direction, the ranges of J1 restaged, a direction) against handle B (J1 staged whole, a direction):
    the four entries give the same bits on 67 columns; A's product is K(J1) v within C_OP and is NOT K(J0) v (further than
    100 x the bound wherever v reaches a changed column; the last column of V reaches none and stays within C_OP of K(J0) v);
    A's solves meet the factor 8 of tests/test_gpu_lbfgs_many.py against K(J1)."""
    from pyipm_amd.lbfgs import LbfgsCore
    c = _restage_inputs()
    n, me, mi, N, k = c.n, c.me, c.mi, c.N, 67
    J0 = c.J
    rng = np.random.default_rng(11)                                          # _j1 of tests/test_gpu_lbfgs_columns.py
    J1 = J0.copy()
    for a, b in ranges:
        J1[:, a:b] = rng.standard_normal((n, b - a)) / np.sqrt(n)
    K0, K1 = c.K, Operator(n, me, mi, *c.store, J1, c.s, c.lda)
    rng = np.random.default_rng(41)
    V, B = rng.standard_normal((N, k)), rng.standard_normal((N, k))
    V[:n, k - 1] = 0.0                                                       # the control: v_x = 0 and v_lambda = 0 on the
    for a, b in ranges:                                                      # changed columns, so K(J0) v = K(J1) v exactly
        V[n + mi + a:n + mi + b, k - 1] = 0.0

    def handle(stages):
        core = LbfgsCore(n, me, mi, SHAPE_RESTAGE[4], device=0, nb=128)
        for stage in stages:
            stage(core)
            dz, _ = core.direction(c.g, c.s, c.lda, *c.store, reg=1e-12)
        return core, _np(dz)

    def whole(J):
        return lambda core: core.stage_jacobian(J[:, :me], J[:, me:])

    def columns(core):
        for a, b in ranges:
            core.stage_jacobian_columns(a, J1[:, a:b])

    A, dzA = handle([whole(J0), columns])
    Bh, dzB = handle([whole(J1)])
    try:
        np.testing.assert_array_equal(dzA, dzB)
        assert not np.array_equal(dzA, c.dz)
        got = {}
        for core in (A, Bh):
            got[core] = dict(
                matvec=np.stack([_np(core.matvec(V[:, j])) for j in range(k)], axis=1),
                solve=np.stack([_np(core.solve(B[:, j])) for j in range(k)], axis=1),
                matvec_many=_np(core.matvec_many(V)), solve_many=_np(core.solve_many(B, refine=0)),
                solve_many2=_np(core.solve_many(B, refine=2)))
        for entry in got[A]:
            np.testing.assert_array_equal(got[A][entry], got[Bh][entry], err_msg=entry)
        for entry in ("matvec", "matvec_many"):
            out = got[A][entry]
            err1, scale1 = _product_error(K1, V, out)
            err0, scale0 = _product_error(K0, V, out)
            bound1 = C_OP * EPS * scale1
            print("RECORD restage %s %s: against K(J1) worst %.3f eps | |K||v| | (bound C_OP = %.2f); against K(J0) the nearest "
                  "column is %.3g x that bound away, the control column %.3f eps | |K0||v| |"
                  % (name, entry, (err1 / (EPS * scale1)).max(), C_OP, (err0[:-1] / bound1[:-1]).min(),
                     err0[-1] / (EPS * scale0[-1])))
            assert np.all(err1 <= bound1), (entry, int(np.argmax(err1 / scale1)))
            assert np.all(err0[:-1] > 100.0 * bound1[:-1]), (entry, int(np.argmin(err0[:-1] / bound1[:-1])))
            assert err0[-1] <= C_OP * EPS * scale0[-1], entry
        worst = 0.0
        for j in range(k):
            e1, ek = K1.berr(got[A]["solve"][:, j], B[:, j]), K1.berr(got[A]["solve_many"][:, j], B[:, j])
            worst = max(worst, ek / e1)
            assert ek <= 8.0 * e1, (j, ek, e1)
        print("RECORD restage %s: solve_many against K(J1): worst berr ratio many / single %.2f (bound 8)" % (name, worst))
    finally:
        A.close()
        Bh.close()
