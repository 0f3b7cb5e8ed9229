"""The product and merit kernels of the single-system handle past one column segment, one element per thread, one wave and
one stride: kkt_matvec, residual, block_products, block_products_t (k_symv_tiles / k_jac_tiles / k_coldot_partial /
k_rowdot2 and their finish kernels, kernels_assemble.hpp), merit_info, merit_ray, dots (kernels_merit.hpp) and step_lengths.
The other modules value-check them where the tiling collapses to one piece (n <= 330, me, mi <= 141; a handful of
variables for merit_info; less than one wave for merit_ray); here every shape is the smallest that reaches a further path:

* rowcol_tiles: a block owns SYMV_SEG = 1024 columns in four 256-column windows and streams 16-row groups of a chunk of rpc
  rows (64 up to 8192 rows, 128 above).  n = 1025: the second segment is one column and row 1024 the one-row group below
  segment 0; n = 2100: three segments, the windows left of the diagonal skipped, zero row partials below a segment;
  me = 1030 / mi = 1100 with n = 300: two segments of a Jacobian block; n = 8201: rpc = 128.
* k_merit_info: 64 blocks of ceil(len / 64) contiguous elements, 256 threads striding through them, so a thread takes a
  second element only when a vector is longer than 16384: one vector at a time is.
* k_merit_ray, k_step_lengths: one block striding by 256, sums / minima over four waves.
* k_dots: one block of 1024 threads per pair, sixteen waves.

Yardstick: no measured tolerance.  Every reference is formed on the host in np.longdouble (or by math.fsum: rows_fsum of
tests/test_gpu_strided_blocks.py) from exactly the float64 data handed to the device.
  products   |got - ref| <= T eps sum|a_i b_i| + ulp(ref), T the number of entries of that row of the matrix: holds for any
             order of summation (the rule of tests/test_gpu_kkt_matvec_many.py);
  sums       (T + 8) eps sum|term_i|, T the number of summands: rows_fsum's (T + 8) u sum|t| restated with eps = 2 u; the 8
             allows a few ulps for the log, log1p, division and fma behind a term.  Norms are compared as squares.
             merit_ray: T = n + me + mi and the magnitudes are the ``scale`` of test_gpu_merit._qp_numpy_ray;
  minima     comp_min and step_lengths: the bits of NumPy float64 in the kernel's order of operations.
Each test prints its worst error / bound."""
import functools

import numpy as np
import pytest

from kkt_manufactured import Manufactured
from pyipm_amd.problems import make_qp
from test_gpu_merit import _qp_numpy_ray
from test_gpu_strided_blocks import U, rows_fsum, same, sym

pytestmark = pytest.mark.gpu

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
DELTA, DELTA_C = 1e-3, 1e-7
SHAPES = [
    (1025, 0, 0),          # segment 1 is one column; row 1024 is a one-row group wholly below segment 0
    (2100, 37, 59),        # three segments of the triangle
    (300, 1030, 0),        # two segments of Je, five row chunks
    (300, 0, 1100),        # the same for Ji
    (1500, 1100, 1300),    # everything at once
]
BIG = (8201, 3, 5)         # more than 8192 rows: rpc = 128
KINDS = ("full", "provider")


def _ids(shape):
    return "%dx%dx%d" % shape


# ---- data --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def system(shape):
    """Blocks and vectors of the case (float64 NumPy) and the vectors the products are taken with.  make_qp, except for
    the large case: there the O(n^3) construction runs on the device (Manufactured)."""
    import torch
    n, me, mi = shape
    seed = n + 3 * me + 5 * mi
    if n > 4096:
        m = Manufactured(n, me, mi, seed=seed, device="cuda" if torch.cuda.is_available() else "cpu")
        q = dict(m.h, mu=m.mu)
        m.free_device()
    else:
        q = make_qp(n, me, mi, seed=seed)
    q = {k: q[k] for k in ("d2L", "Je", "Ji", "df", "ce", "ci", "s", "lam", "mu")}
    rng = np.random.default_rng(seed + 1)
    q.update(v=rng.standard_normal(n + 2 * mi + me), vx=rng.standard_normal(n), le=rng.standard_normal(me),
             li=rng.standard_normal(mi))
    return q


def handle(shape, kind):
    """A handle with the case staged and the shifts its kkt_matvec applies: a full one has been assembled with
    (DELTA, DELTA_C), a provider-only one has no assembly and keeps (0, 0)."""
    from pyipm_amd.newton import NewtonCore
    n, me, mi = shape
    q = system(shape)
    core = NewtonCore(n, me, mi, device=0, provider_only=(kind == "provider"))
    core.stage_blocks(q["d2L"], q["Je"] if me else None, q["Ji"] if mi else None)
    core.stage_vectors(q["df"], q["ce"], q["ci"], q["s"], q["lam"], mu=q["mu"])
    if kind == "provider":
        return core, (0.0, 0.0)
    core.residual()
    core.assemble(DELTA, DELTA_C)
    return core, (DELTA, DELTA_C)


def _np(t):
    return t.detach().cpu().numpy()


# ---- references --------------------------------------------------------------------------------------------------------------------
def ld_rows(M, V, chunk=1024):
    """(M V, |M| |V|) in np.longdouble for a float64 matrix M and the columns V, a chunk of rows at a time (no
    extended-precision copy of the whole block)."""
    Vl = np.asarray(V, dtype=np.float64).astype(LD)
    Va = np.abs(Vl)
    val = np.zeros((M.shape[0],) + Vl.shape[1:], dtype=LD)
    mag = np.zeros_like(val)
    for i in range(0, M.shape[0], chunk):
        blk = M[i:i + chunk].astype(LD)
        val[i:i + chunk] = blk @ Vl
        mag[i:i + chunk] = np.abs(blk) @ Va
    return val, mag


@functools.lru_cache(maxsize=None)
def block_terms(shape):
    """The block products behind every reference of the case, block by block (never an N x N matrix): for the two
    columns (x part of v | vx), S = sym(triu d2L) times them and J' times them; Je v_e, Ji v_i, Je lam_e, Ji lam_i,
    Je le, Ji li."""
    n, me, mi = shape
    q = system(shape)
    d2L = q["d2L"]
    S = d2L if np.array_equal(d2L, d2L.T) else sym(d2L)                  # the library reads the upper triangle
    v, lam = q["v"], q["lam"]
    ve, vi = v[n + mi:n + mi + me], v[n + mi + me:]
    X = np.stack([v[:n], q["vx"]], axis=1)
    return dict(S=ld_rows(S, X), diag=np.diagonal(S).astype(LD), JeT=ld_rows(q["Je"].T, X), JiT=ld_rows(q["Ji"].T, X),
                Je=ld_rows(q["Je"], np.stack([ve, lam[:me], q["le"]], axis=1)),
                Ji=ld_rows(q["Ji"], np.stack([vi, lam[me:], q["li"]], axis=1)))


def ref_matvec(shape, delta, delta_c):
    """(Hc v, sum of the magnitudes, entries of the row) for Hc of pyipm.py:824-842 with delta on the diagonal of the x
    block, -delta_c on that of the equality multipliers, Sigma = lam_i / (s + eps)."""
    n, me, mi = shape
    q, t = system(shape), block_terms(shape)
    v = q["v"].astype(LD)
    vx, vs, ve = v[:n], v[n:n + mi], v[n + mi:n + mi + me]
    sig = q["lam"][me:].astype(LD) / (q["s"].astype(LD) + LD(EPS))
    d = t["diag"]
    val = [t["S"][0][:, 0] + LD(delta) * vx + t["Je"][0][:, 0] + t["Ji"][0][:, 0],
           sig * vs - v[n + mi + me:], t["JeT"][0][:, 0] - LD(delta_c) * ve, t["JiT"][0][:, 0] - vs]
    mag = [t["S"][1][:, 0] + (np.abs(d + LD(delta)) - np.abs(d)) * np.abs(vx) + t["Je"][1][:, 0] + t["Ji"][1][:, 0],
           np.abs(sig * vs) + np.abs(v[n + mi + me:]), t["JeT"][1][:, 0] + np.abs(LD(delta_c) * ve), t["JiT"][1][:, 0] + np.abs(vs)]
    T = [np.full(n, n + me + mi), np.full(mi, 2), np.full(me, n + 1), np.full(mi, n + 1)]
    return np.concatenate(val), np.concatenate(mag), np.concatenate(T)


def ref_residual(shape):
    """g = -grad (pyipm.py:655-668): -(df - Je lam_e - Ji lam_i), -(lam_i - mu / (s + eps)), -ce, -(ci - s)."""
    n, me, mi = shape
    q, t = system(shape), block_terms(shape)
    L = lambda a: a.astype(LD)                                           # noqa: E731
    inv = LD(q["mu"]) / (L(q["s"]) + LD(EPS))
    val = [-(L(q["df"]) - t["Je"][0][:, 1] - t["Ji"][0][:, 1]), -(L(q["lam"][me:]) - inv), -L(q["ce"]), -(L(q["ci"]) - L(q["s"]))]
    mag = [np.abs(L(q["df"])) + t["Je"][1][:, 1] + t["Ji"][1][:, 1], np.abs(L(q["lam"][me:])) + np.abs(inv), np.abs(L(q["ce"])),
           np.abs(L(q["ci"])) + np.abs(L(q["s"]))]
    T = [np.full(n, 1 + me + mi), np.full(mi, 2), np.full(me, 1), np.full(mi, 2)]
    return np.concatenate(val), np.concatenate(mag), np.concatenate(T)


class Worst(object):
    """Checks against the two rules and keeps the worst error / bound of the test."""

    def __init__(self):
        self.ratio = 0.0

    def judge(self, err, bound, what):
        err, bound = np.atleast_1d(err), np.atleast_1d(bound)
        ratio = float(np.max(err / np.maximum(bound, LD(1e-300)))) if err.size else 0.0
        print("%-28s worst error / bound: %.3f" % (what, ratio))
        assert np.all(err <= bound), (what, int(np.argmax(err - bound)), float(np.max(err - bound)))
        self.ratio = max(self.ratio, ratio)

    def product(self, got, val, mag, T, what):
        """|got - ref| <= T eps sum|a_i b_i| + ulp(ref), componentwise"""
        got = np.asarray(got, dtype=np.float64)
        assert got.shape == val.shape, (what, got.shape, val.shape)
        bound = T * LD(EPS) * mag + np.spacing(np.abs(val.astype(np.float64)))
        self.judge(np.abs(got.astype(LD) - val), bound, what)

    def total(self, got, terms, what, square=False):
        """|got - fsum(terms)| <= (T + 8) eps sum|term_i|; ``square``: got is a norm, its square is compared"""
        val, bnd = rows_fsum(np.asarray(terms, dtype=LD).astype(np.float64))
        g = LD(got) * LD(got) if square else LD(got)
        self.judge(np.abs(g - LD(val[0])), bnd[0] * (EPS / U), what)


# ---- 1., 2. products ---------------------------------------------------------------------------------------------------------------
def check_products(core, shape, shifts, w, every=True):
    n, me, mi = shape
    q, t = system(shape), block_terms(shape)
    val, mag, T = ref_matvec(shape, *shifts)
    w.product(_np(core.matvec(q["v"])), val, mag, T, "matvec")
    got = core.block_products(q["vx"])
    for k, key, m in ((0, "S", n), (1, "JeT", me), (2, "JiT", mi)):
        if m == 0:
            assert got[k] is None
        else:
            w.product(_np(got[k]), t[key][0][:, 1], t[key][1][:, 1], n, "block_products[%d]" % k)
    if not every:
        return
    val, mag, T = ref_residual(shape)
    w.product(_np(core.residual()), val, mag, T, "residual")
    (ev, em), (iv, im) = t["Je"], t["Ji"]
    for le, li in ((True, True), (True, False), (False, True), (False, False)):
        out = _np(core.block_products_t(q["le"] if le else None, q["li"] if li else None))
        w.product(out, le * ev[:, 2] + li * iv[:, 2], le * em[:, 2] + li * im[:, 2], le * me + li * mi,
                  "block_products_t(%s, %s)" % ("le" if le else None, "li" if li else None))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_products_past_one_column_segment(shape, kind):
    core, shifts = handle(shape, kind)
    w = Worst()
    check_products(core, shape, shifts, w)
    core.close()
    assert w.ratio > 0.0
    print("%s %s: worst error / bound %.3f" % (_ids(shape), kind, w.ratio))


def test_products_with_128_row_chunks():
    """More than 8192 rows: symv_dev and kkt_matvec_dev hand rowcol_tiles chunks of 128 rows (eight 16-row groups)."""
    core, shifts = handle(BIG, "full")
    w = Worst()
    check_products(core, BIG, shifts, w, every=False)
    core.close()
    assert w.ratio > 0.0
    print("%s full: worst error / bound %.3f" % (_ids(BIG), w.ratio))


def test_shared_scratch_keeps_the_product():
    """ctx->partial (products, step_lengths) and the merit buffer are shared between the entries: kkt_matvec gives the same
    bits after the others have run in between."""
    import torch
    shape = SHAPES[4]
    n, me, mi = shape
    q = system(shape)
    core, _ = handle(shape, "full")
    rng = np.random.default_rng(5)
    dz = torch.from_numpy(rng.standard_normal(n + 2 * mi + me)).cuda()
    first = _np(core.matvec(q["v"]))
    prods = core.block_products(q["vx"])
    core.step_lengths(0.995, dz=dz)
    core.merit_info(dz=dz)
    core.dots([(prods[0], prods[0]), (dz, dz)])
    assert same(_np(core.matvec(q["v"])), first)
    core.close()


# ---- 3. merit_info -----------------------------------------------------------------------------------------------------------------
def mixed(rng, k, lo, hi):
    """k numbers of random sign with magnitudes spread over [10^lo, 10^hi]"""
    return rng.standard_normal(k) * 10.0 ** rng.uniform(lo, hi, k)


def merit_vectors(shape, seed):
    n, me, mi = shape
    rng = np.random.default_rng(seed)
    s = 10.0 ** rng.uniform(-6, 3, mi)
    v = dict(df=mixed(rng, n, -3, 3), ce=mixed(rng, me, -3, 3), s=s, ci=s + mixed(rng, mi, -4, 2),
             lam=np.concatenate([mixed(rng, me, -2, 2), 10.0 ** rng.uniform(-3, 3, mi)]))
    dz = np.concatenate([mixed(rng, n, -3, 3), s * mixed(rng, mi, -3, 1), mixed(rng, me + mi, -2, 2)])
    return v, dz


def check_merit_info(got, shape, v, dz, g, w, tag):
    """All thirteen entries.  g: the residual the handle holds (None: none formed, the two entries from it are NaN)."""
    n, me, mi = shape
    L = lambda a: np.asarray(a, dtype=np.float64).astype(LD)             # noqa: E731
    df, ce, ci, s, li = L(v["df"]), L(v["ce"]), L(v["ci"]), L(v["s"]), L(v["lam"][me:])
    dx, ds, r = L(dz[:n]), L(dz[n:n + mi]), L(v["ci"]) - L(v["s"])
    sums = dict(ce_l1=np.abs(ce), cis_l1=np.abs(r), df_dx=df * dx, ds_over_s=ds / (s + LD(EPS)), sum_log_s=np.log(s), comp_sum=s * li)
    norms = dict(kkt_ce=ce * ce, kkt_ci=r * r, dx_norm=dx * dx, ds_norm=ds * ds)
    if g is None:
        assert np.isnan(got["kkt_x"]) and np.isnan(got["kkt_s"])
    else:
        gs = L(g[n:n + mi]) * s
        norms.update(kkt_x=L(g[:n]) ** 2, kkt_s=gs * gs)
    for key, terms in sums.items():
        w.total(got[key], terms, tag + " " + key)
    for key, terms in norms.items():
        w.total(got[key], terms, tag + " " + key, square=True)
    if mi:
        assert got["comp_min"] == np.min(v["s"] * v["lam"][me:]), tag
    else:
        assert np.isnan(got["comp_min"])
    assert len(sums) + len(norms) + (2 if g is None else 0) + 1 == 13 == len(got)


def min_positions(mi):
    """Where the smallest s lda_i is put.  Block b owns the per = ceil(mi / 64) elements from b per on and thread t takes
    offsets t and t + 256 of them, so at mi = 20000 (per = 313) the second trips are offsets 256 .. 312 of every block:
    the last element of the last block (a second trip), offset 256 of the first block (a second trip), the first element
    of the last block, and index 16384, the first element past one trip of every thread (block 52, a first trip)."""
    per = (mi + 63) // 64
    return sorted({p for p in (mi - 1, 16384, 256 if per > 256 else 0, 63 * per) if 0 <= p < mi})


@pytest.mark.parametrize("shape", [(16500, 1, 1), (8, 16500, 0), (8, 0, 20000)], ids=_ids)
def test_merit_info_past_one_element_per_thread(shape):
    import torch
    from pyipm_amd.newton import NewtonCore
    n, me, mi = shape
    v, dz = merit_vectors(shape, 11 + mi)
    dzd = torch.from_numpy(dz).cuda()
    core = NewtonCore(n, me, mi, device=0, provider_only=True)
    w = Worst()
    for p in (min_positions(mi) if mi else [None]):
        lam = v["lam"].copy()
        if p is not None:
            lam[me + p] = 1e-12 / v["s"][p]                                # the unique smallest product
            assert np.argmin(v["s"] * lam[me:]) == p
        vp = dict(v, lam=lam)
        core.stage_vectors(vp["df"], vp["ce"], vp["ci"], vp["s"], vp["lam"], mu=0.1)
        check_merit_info(core.merit_info(dz=dzd), shape, vp, dz, None, w, "min at %s:" % p)
    core.close()
    assert w.ratio > 0.0
    print("%s: worst error / bound %.3f" % (_ids(shape), w.ratio))


def test_merit_info_with_the_residual_of_a_full_handle():
    import torch
    from pyipm_amd.newton import NewtonCore
    shape = (700, 300, 1000)
    n, me, mi = shape
    qp = make_qp(n, me, mi, seed=17)
    v, dz = merit_vectors(shape, 23)
    core = NewtonCore(n, me, mi, device=0)
    core.stage_blocks(qp["d2L"], qp["Je"], qp["Ji"])
    core.stage_vectors(v["df"], v["ce"], v["ci"], v["s"], v["lam"], mu=0.1)
    g = _np(core.residual())
    w = Worst()
    check_merit_info(core.merit_info(dz=torch.from_numpy(dz).cuda()), shape, v, dz, g, w, "full:")
    core.close()
    print("%s full: worst error / bound %.3f" % (_ids(shape), w.ratio))


# ---- 4. merit_ray ------------------------------------------------------------------------------------------------------------------
RAY_N, NU, MU = 64, 10.0, 0.2
ALPHAS = [0.995 ** k for k in range(1020)] + [1e-3, 1e-6, 1e-9, 1e-12]   # a0 = 1; 1024: all the entry takes in one call


@functools.lru_cache(maxsize=None)
def ray_case(me, mi):
    """A QP, a direction and a staged point at which every second constraint changes the sign of ce + a dce (of r + a dr,
    r = ci - s) at some a inside the candidates' range, so that both branches of abs_change are summed in every wave."""
    n = RAY_N
    qp = make_qp(n, me, mi, seed=7 + me + mi)
    rng = np.random.default_rng(me + 2 * mi)
    s = 10.0 ** rng.uniform(-2, 2, mi)
    dx, ds = rng.standard_normal(n), s * rng.uniform(-0.9, 2.0, mi)      # 1 + a ds / s >= 0.1
    dz = np.concatenate([dx, ds, rng.standard_normal(me + mi)])

    def zero_at(m):
        """the a at which c + a dc = 0: inside the candidates' range for every second element, outside [0, 1] for the rest"""
        a = rng.uniform(1.5, 3.0, m) * rng.choice([-1.0, 1.0], m)
        a[::2] = rng.uniform(0.02, 0.9, len(a[::2]))
        return a

    dce, dr = qp["A"] @ dx, qp["G"] @ dx - ds
    ce = -zero_at(me) * dce
    ci = s - zero_at(mi) * dr
    want, scale = _qp_numpy_ray(qp, qp["df"], ce, ci, s, dz, NU, MU, ALPHAS)
    dxl = dx.astype(LD)
    quad = float(dxl @ (qp["Q"].astype(LD) @ dxl))
    for c0, dc in ((ce, dce), (ci - s, dr)):                             # the arrangement is what it says, in every wave
        for lo in range(0, len(c0) - 1, 64):
            flips = np.sign(c0[lo:lo + 64] + ALPHAS[0] * dc[lo:lo + 64]) != np.sign(c0[lo:lo + 64])
            assert flips.any() and not flips.all()
    return dict(qp=qp, s=s, ce=ce, ci=ci, dz=dz, quad=quad, want=want, scale=scale)


@pytest.mark.parametrize("me,mi,kind", [(300, 0, "provider"), (0, 1000, "provider"), (257, 513, "provider"), (257, 513, "full")])
def test_merit_ray_past_one_wave_and_one_stride(me, mi, kind):
    import torch
    from pyipm_amd.newton import NewtonCore
    n = RAY_N
    c = ray_case(me, mi)
    qp = c["qp"]
    core = NewtonCore(n, me, mi, device=0, provider_only=(kind == "provider"))
    core.stage_blocks(None if kind == "provider" else qp["Q"], qp["Je"] if me else None, qp["Ji"] if mi else None)
    core.stage_vectors(qp["df"], c["ce"], c["ci"], c["s"], qp["lam"], mu=MU)
    dzd = torch.from_numpy(c["dz"]).cuda()
    got = np.array(core.merit_ray(ALPHAS, NU, MU, dz=dzd, quad=c["quad"] if kind == "provider" else None))
    core.close()
    bound = (n + me + mi + 8) * EPS * c["scale"]
    w = Worst()
    w.judge(np.abs(got - c["want"]), bound, "merit_ray, 1024 candidates")
    assert w.ratio > 0.0 and np.all(np.isfinite(got))
    print("n%d me%d mi%d %s: worst error / bound %.3f" % (n, me, mi, kind, w.ratio))


# ---- 5. step_lengths ---------------------------------------------------------------------------------------------------------------
TAU = 0.995


def want_length(v, dv):
    """the kernel's min(1, (-tau v_i) / dv_i over dv_i < 0), in its order of operations"""
    neg = dv < 0.0
    return float(np.min((-TAU * v[neg]) / dv[neg], initial=1.0))


@pytest.mark.parametrize("mi", [1, 63, 64, 65, 255, 256, 257, 700])
def test_step_lengths_are_numpys_minima_bit_for_bit(mi):
    import torch
    from pyipm_amd.newton import NewtonCore
    n, me = 4, 3
    rng = np.random.default_rng(100 + mi)
    s, li = 10.0 ** rng.uniform(-6, 3, mi), 10.0 ** rng.uniform(-3, 3, mi)
    core = NewtonCore(n, me, mi, device=0, provider_only=True)
    core.stage_vectors(rng.standard_normal(n), rng.standard_normal(me), s + 0.1, s, np.concatenate([rng.standard_normal(me), li]), mu=0.1)

    def lengths(ds, dl):
        dz = np.concatenate([rng.standard_normal(n), ds, rng.standard_normal(me), dl])
        return core.step_lengths(TAU, dz=torch.from_numpy(dz).cuda())

    def toward(v, lo, hi):
        """steps that reach the boundary at a fraction in [lo, hi] of the full step (half of them), or move away from it"""
        return np.where(rng.random(mi) < 0.5, -TAU * v / rng.uniform(lo, hi, mi), v * rng.uniform(0.1, 3.0, mi))

    ds, dl = toward(s, 0.3, 0.95), toward(li, 0.3, 0.95)
    ds[-1], dl[0] = -TAU * s[-1] / 0.5, -TAU * li[0] / 0.5               # (mi = 1: a negative entry in both)
    assert lengths(ds, dl) == (want_length(s, ds), want_length(li, dl)) and want_length(s, ds) < 1.0 > want_length(li, dl)
    assert lengths(np.abs(ds), np.abs(dl)) == (1.0, 1.0)                  # no negative entry
    far_s, far_l = toward(s, 1.5, 3.0), toward(li, 1.5, 3.0)              # the binding ratio exceeds 1
    far_s[-1], far_l[0] = -TAU * s[-1] / 1.5, -TAU * li[0] / 1.5
    assert want_length(s, far_s) == 1.0 == want_length(li, far_l) and lengths(far_s, far_l) == (1.0, 1.0)
    if mi in (257, 700):                                                  # the binding element through every position
        for p in range(mi):
            q = (p + mi // 2 + 1) % mi                                    # ... and another one for lda
            ds2, dl2 = ds.copy(), dl.copy()
            ds2[p], dl2[q] = -TAU * s[p] / (0.05 + 0.1 * p / mi), -TAU * li[q] / (0.02 + 0.1 * q / mi)
            ws, wl = want_length(s, ds2), want_length(li, dl2)
            assert ws == (-TAU * s[p]) / ds2[p] and wl == (-TAU * li[q]) / dl2[q] and p != q
            assert lengths(ds2, dl2) == (ws, wl), (p, q)
    core.close()


# ---- 6. dots -----------------------------------------------------------------------------------------------------------------------
def test_dots_of_eight_lengths_in_both_orders():
    import torch
    from pyipm_amd.newton import NewtonCore
    rng = np.random.default_rng(6)
    lens = [1, 63, 64, 1023, 1024, 1025, 5000, 40000]
    host = [(mixed(rng, k, -3, 3), mixed(rng, k, -3, 3)) for k in lens]
    pairs = [(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()) for a, b in host]
    core = NewtonCore(8, 2, 3, device=0, provider_only=True)
    out = core.dots(pairs)
    back = core.dots(pairs[::-1])
    core.close()
    w = Worst()
    for k, got, (a, b) in zip(lens, out, host):
        w.total(got, a.astype(LD) * b.astype(LD), "dot of %d" % k)
    assert same(np.array(back[::-1]), np.array(out))                      # a pair's bits do not depend on its block
    print("dots: worst error / bound %.3f" % w.ratio)
