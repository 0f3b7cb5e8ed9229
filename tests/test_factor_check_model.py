"""tests/factor_check.py on factors of the NumPy twin of the device algorithm (oracle/block_ldl_model.py, tb = 64): a clean
factor stays within the bound the GPU tests use (tests/test_gpu_factor_entrywise.py), the inertia read off the reconstructed
block pivots is the model's, and a factor that is subtly wrong in ONE tile is flagged.

Measured here (ratio = max |R| / (eps B), factor_check.py):

    matrix                                             block_refine 0 / 1 / 2
    make_qp (130, 63, 1)                               2.8 / 1.9 / 1.8
    make_qp (203, 37, 61)                              2.9 / 2.3 / 2.0
    make_qp (320, 128, 256)                            3.3 / 2.5 / 2.5
    _graded_qp (520, 130, 0), 3 decades                3.8 / 2.5 / 2.8
    _graded_qp (300, 40, 100), 7 decades               4.2 / 2.5 / 2.7
    Manufactured(300, 60, 140, "Q", n_neg=100)         5.8 / 5.2 / 4.4      (22 2x2 pivots, max B / max |K| = 8e4)

The third sabotage -- one tile of Lb built WITHOUT the refinement of the block solve -- needs the right matrix.  The grading of
_graded_qp does not show it (whole factors without any refinement: 3.8 against 2.5 and 4.2 against 2.5 above; the pivoted
inverse of a diagonally graded tile is componentwise accurate).  An ill-conditioned DENSE tile does: on make_qp (256, 256, 1024),
whose lambda_e Schur complement -Je' inv(H) Je has a square Je (me = n), the model gives 42.1 / 2.44 / 2.52 with 0 / 1 / 2
steps, and ONE tile of the unrefined run, (35, 23), in the refined factor gives 42.4 against a bound of 10.1
(test_one_unrefined_tile_is_flagged).  That is the defect the GPU tests found on the device."""
import numpy as np
import pytest

from factor_check import MARGIN, bound, check_factor, model_factor
from kkt_manufactured import Manufactured
from oracle import newton_oracle as orc
from oracle.block_ldl_model import sweep_invert
from pyipm_amd.problems import make_qp

TB = 64


def _graded_qp(n, me, mi, seed, decades):
    from test_gpu_tile_blocked import _graded_qp as graded
    return graded(n, me, mi, seed, decades)


def _kkt(qp, n, me, mi):
    return orc.kkt_matrix(qp["d2L"], qp["Je"], qp["Ji"], qp["s"], qp["lam"], n, me, mi)


def _matrix(kind, n, me, mi, arg):
    if kind == "qp":
        return _kkt(make_qp(n, me, mi, arg), n, me, mi)
    if kind == "graded":
        return _kkt(_graded_qp(n, me, mi, arg[0], arg[1]), n, me, mi)
    return Manufactured(n, me, mi, mixer="Q", n_neg=n // 3, seed=arg).kkt_matrix()


CASES = [("qp", 130, 63, 1, 0), ("qp", 203, 37, 61, 1), ("qp", 320, 128, 256, 2), ("graded", 520, 130, 0, (3, 3.0)),
         ("graded", 300, 40, 100, (1, 7.0)), ("manufactured", 300, 60, 140, 5)]
_memo = {}


def _clean(case, refine):
    """(H, K, Lb, model, FactorCheck) of a case, computed once."""
    if (case, refine) not in _memo:
        kind, n, me, mi, arg = case
        H = _matrix(kind, n, me, mi, arg)
        K, Lb, f = model_factor(H, refine=refine, neg_from=n + mi, sigma_from=n)
        _memo[(case, refine)] = (H, K, Lb, f, check_factor(K, Lb))
    return _memo[(case, refine)]


@pytest.mark.parametrize("refine", [0, 1, 2])
@pytest.mark.parametrize("case", CASES, ids=["%s-%d-%d-%d" % c[:4] for c in CASES])
def test_clean_model_factor_is_within_the_ceiling_and_gives_the_inertia(case, refine):
    """Ratio O(1) (the table above; asserted: below 8, far under the a-priori ceiling Npad + 64), whatever the growth; inertia
    from the eigenvalues of the reconstructed T_k = the model's pivot counts = (n + mi, me + mi) for the convex systems and
    Manufactured.inertia() for the indefinite one."""
    kind, n, me, mi, arg = case
    H, K, Lb, f, r = _clean(case, refine)
    print("%s refine %d: ratio %.2f at %s, growth %.1e, 2x2 %d, %.2f s" % (case, refine, r.ratio, r.where, r.growth,
                                                                        f.stats["n2x2"], r.seconds))
    assert f.stats["zero"] == 0
    assert r.ratio <= 8.0 < f.Np + 64, r
    pad = f.Np - f.N
    assert (r.n_pos - pad, r.n_neg) == (f.N - f.stats["neg"], f.stats["neg"]), (r, f.stats)
    if kind == "manufactured":
        neg, zero, pos = Manufactured(n, me, mi, mixer="Q", n_neg=n // 3, seed=arg).inertia()
        assert zero == 0 and (r.n_pos - pad, r.n_neg) == (pos, neg) and f.stats["n2x2"] >= 1
    else:
        assert (r.n_pos - pad, r.n_neg) == (n + mi, me + mi)


@pytest.mark.parametrize("case", CASES, ids=["%s-%d-%d-%d" % c[:4] for c in CASES])
def test_structural_zeros_are_exact(case):
    """Entries that neither K nor any product reaches (the slack rows of x columns, the padding) have B = 0, and a clean
    factor has such entries in every KKT system with a slack block or padding; a finite ratio says R = 0 there.  B counts
    |Lb| |T_k| too, so B = 0 needs the entry of Lb itself to be an exact zero: one of them set to 1e-300 has R = -Lb T_k
    against B = |Lb| |T_k|, a ratio of 1 / eps whatever its size."""
    H, K, Lb, f, r = _clean(case, 1)
    assert np.isfinite(r.ratio) and r.exact_zeros > 0, r
    if f.Np > f.N:                                   # a padding row of the first tile column: nothing reaches it
        assert not Lb[f.Np - 1, :TB].any()
        bad = Lb.copy()
        bad[f.Np - 1, 0] = 1e-300
        rb = check_factor(K, bad)
        assert rb.ratio >= 0.5 / np.finfo(float).eps and rb.where[:2] == (0, f.Np - 1), rb
        assert rb.exact_zeros < r.exact_zeros


def _largest_entry(Lb, tile):
    """The entry of largest magnitude of tile (ti, tj) of Lb, or None where the tile is zero."""
    blk = np.abs(Lb[tile[0] * TB:(tile[0] + 1) * TB, tile[1] * TB:(tile[1] + 1) * TB])
    if not blk.any():
        return None
    i, j = np.unravel_index(int(np.argmax(blk)), blk.shape)
    return tile[0] * TB + int(i), tile[1] * TB + int(j)


@pytest.mark.parametrize("case", CASES, ids=["%s-%d-%d-%d" % c[:4] for c in CASES])
def test_one_entry_off_by_1e_11_is_flagged(case):
    """One non-zero entry of Lb scaled by 1 + 1e-11 (4.5e4 eps): the ratio leaves the bound of the GPU tests as computed for
    this matrix, min(MARGIN x the clean model's ratio, Npad + 64).  The entry is the largest one of a tile: the first and the
    last tile below the diagonal tiles and one in the middle.  (B bounds the SUM an entry of R is made of, so an entry of Lb
    whose own term is a thousandth of that sum can be off by 1e-11 unseen -- measured on the indefinite matrix: a random entry
    gave 19.4 against a bound of 20.7 -- and is then also a thousand times less harmful.  The same perturbation on a
    structural zero changes nothing, so it is aimed at non-zero entries.)  On the indefinite matrix the tiles are those of the
    first tile column: behind it B carries the growth of the 2 x 2 pivots (max B / max |K| = 8e4), and 1e-11 of the largest
    entry of tile (6, 4) is within it (measured: 10.9 against 20.7)."""
    H, K, Lb, f, r = _clean(case, 1)
    lim = bound(r.ratio, f.Np, MARGIN)
    nt = f.Np // TB
    done = 0
    tiles = ((1, 0), (3, 0), (4, 0)) if case[0] == "manufactured" else \
        ((1, 0), (nt // 2 + 1, nt // 2 - 1), (nt - 1, nt - 2), (nt - 1, 0), (2, 1))
    for tile in tiles:
        ij = _largest_entry(Lb, tile)
        if ij is None or done == 3:
            continue
        bad = Lb.copy()
        bad[ij] *= 1.0 + 1e-11
        rb = check_factor(K, bad)
        print(case, ij, "clean %.2f sabotaged %.3g bound %.1f" % (r.ratio, rb.ratio, lim))
        assert rb.ratio > lim, (case, ij, rb, lim)
        done += 1
    assert done == 3


def _block_ldl(H, n, me, mi, refine, skip=None):
    """The loop of oracle.block_ldl_model.BlockLDL with one hook: skip = (i, c, j) leaves the rank-64 update of tile
    (i, c) by tile column j out (a stale update tile).  Returns the storage M."""
    N = H.shape[0]
    Np = (N + TB - 1) // TB * TB
    A = np.abs(H).copy()
    idx = np.arange(n, n + mi)
    A[idx, idx] = 0.0
    anorm = float(A.max())
    M = np.eye(Np)
    M[:N, :N] = np.tril(H) + np.tril(H, -1).T
    for k in range(Np // TB):
        k0, k1 = k * TB, (k + 1) * TB
        T = np.tril(M[k0:k1, k0:k1]) + np.tril(M[k0:k1, k0:k1], -1).T
        Ti, st = sweep_invert(T, anorm=anorm, neg_lim=n + mi - k0)
        if k1 < Np:
            W = M[k1:, k0:k1].copy()
            L = W @ Ti
            for _ in range(refine if st["zero"] == 0 else 0):
                L = L + (W - L @ T) @ Ti
            keep = None
            if skip is not None and skip[2] == k:
                i0, c0 = skip[0] * TB, skip[1] * TB
                keep = M[i0:i0 + TB, c0:c0 + TB].copy()
            M[k1:, k1:] -= L @ W.T
            if keep is not None:
                M[i0:i0 + TB, c0:c0 + TB] = keep
            M[k1:, k0:k1] = L
    return M


@pytest.mark.parametrize("case", [CASES[2], CASES[3], CASES[5]], ids=["%s-%d-%d-%d" % c[:4] for c in (CASES[2], CASES[3], CASES[5])])
def test_a_stale_update_tile_is_flagged(case):
    """One 64 x 64 tile of Lb taken from a model run in which one rank-64 update of that tile was skipped (what a tile list
    that misses a tile, or a launch that reads W before it is written, leaves behind); every other tile is the clean run's.
    The hook's loop is the model's: without a skip it gives the model's bits."""
    kind, n, me, mi, arg = case
    H, K, Lb, f, r = _clean(case, 1)
    assert np.array_equal(_block_ldl(H, n, me, mi, 1), f.M)
    lim = bound(r.ratio, f.Np, MARGIN)
    nt = f.Np // TB
    for (i, c, j) in ((2, 1, 0), (nt - 1, 2, 1)):
        i0, c0 = i * TB, c * TB
        stale = _block_ldl(H, n, me, mi, 1, skip=(i, c, j))
        bad = Lb.copy()
        bad[i0:i0 + TB, c0:c0 + TB] = stale[i0:i0 + TB, c0:c0 + TB]
        if np.array_equal(bad, Lb):                    # (the skipped product was structurally zero: nothing stale)
            continue
        rb = check_factor(K, bad)
        print(case, (i, c, j), "clean %.2f stale %.3g bound %.1f" % (r.ratio, rb.ratio, lim))
        assert rb.ratio > lim, (case, (i, c, j), rb, lim)
        break
    else:
        pytest.fail("no tile of %s with a non-zero update to skip" % (case,))


def test_one_unrefined_tile_is_flagged():
    """make_qp (256, 256, 1024): the last tile column of the lambda_e block (23) is dense and ill-conditioned (me = n).  The
    refined factor (block_refine = 2, the device's default) with ONE tile taken from the run without refinement, (35, 23) --
    where the unrefined run's own worst entry lies (row 2297) -- leaves the bound of the GPU tests for this matrix; the whole
    unrefined factor does too (measured: 42.1 / 2.44 / 2.52 with 0 / 1 / 2 steps, the one tile 42.4, bound 10.1)."""
    n, me, mi, seed = 256, 256, 1024, 5
    H = _kkt(make_qp(n, me, mi, seed), n, me, mi)
    out = {}
    for refine in (0, 2):
        K, Lb, f = model_factor(H, refine=refine, neg_from=n + mi, sigma_from=n)
        out[refine] = (Lb, check_factor(K, Lb))
    r0, r2 = out[0][1], out[2][1]
    lim = bound(r2.ratio, f.Np, MARGIN)
    print("refine 0 / 2: %.2f at %s / %.2f, bound %.1f" % (r0.ratio, r0.where, r2.ratio, lim))
    assert r2.ratio <= 8.0 and r0.ratio > lim and r0.where[0] == 23, (r0, r2)
    i, c = r0.where[1] // TB, r0.where[0]
    assert (i, c) == (35, 23)
    bad = out[2][0].copy()
    bad[i * TB:(i + 1) * TB, c * TB:(c + 1) * TB] = out[0][0][i * TB:(i + 1) * TB, c * TB:(c + 1) * TB]
    rb = check_factor(K, bad)
    print("one unrefined tile %s: %.2f" % ((i, c), rb.ratio))
    assert rb.ratio > lim and rb.where[0] == c and rb.where[1] // TB == i, (rb, lim)


def test_grading_alone_does_not_show_a_missing_refinement():
    """The whole factor of a diagonally graded matrix (pivot spread 1e7) built without the refinement of the block solves is
    within MARGIN of the refined one, in both directions: why the sabotage above is made on an ill-conditioned dense tile."""
    a, b = _clean(CASES[4], 0)[4], _clean(CASES[4], 1)[4]
    assert a.ratio <= MARGIN * b.ratio and b.ratio <= MARGIN * a.ratio, (a, b)
