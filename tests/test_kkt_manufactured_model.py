"""CPU self-check of the manufactured-KKT generator (tests/kkt_manufactured.py): before its predictions judge the GPU
factorisation at sizes no eigensolver reaches, they are held against dense LAPACK at small ragged sizes.

* the predicted inertia equals the eigenvalue count reghess makes (``inertia_from_eig``, pyipm.py:1381), unshifted and
  after the shifts reghess applies (delta0 * 10^k on the x block, delta_c on the equality block);
* x_true is the solution of K x = b;
* the blockwise host matvec is ``kkt_matrix(...) @ v``;
* with the orthogonal mixer the spectrum of d2L is D: the exact rcond is min|D| / max|D|."""
import numpy as np
import pytest

from kkt_manufactured import EPS, NN, PAIR, Z, Manufactured, blas_threads
from oracle.newton_oracle import inertia_from_eig

DELTA0 = np.sqrt(EPS)
DELTA_C = np.sqrt(EPS) * 1e-4 * 0.1 ** 0.4          # reg_coef * eta * mu_host^beta at mu_host = 0.1

SHAPES = [(300, 0, 0), (301, 37, 0), (257, 0, 61), (600, 70, 150), (450, 11, 141)]
VARIANTS = {
    "neg": dict(n_neg=None),
    "pairs": dict(n_pairs=5, n_neg=None),
    "zero": dict(zero_tile=True, n_zero=2),
    "dependent": dict(dependent_eq=3),
    "sigma": dict(sigma_decades=12.0, n_neg=None),
}


def _make(shape, variant, mixer, **extra):
    n, me, mi = shape
    kw = dict(VARIANTS[variant])
    if kw.get("n_neg", 0) is None:
        kw["n_neg"] = n // 3 if variant == "neg" else n // 6
    kw.update(extra)
    return Manufactured(n, me, mi, mixer=mixer, seed=n + me + mi, keep_mixer=True, **kw)


def _cases():
    for shape in SHAPES:
        n, me, mi = shape
        for variant in VARIANTS:
            if variant == "zero" and mi < 2 * 66:
                continue                                   # Ai needs full row rank on the 66 zero rows
            if variant == "dependent" and me < 6:
                continue
            for mixer in ("Q", "T"):
                yield pytest.param(shape, variant, mixer, id="%d-%d-%d-%s-%s" % (n, me, mi, variant, mixer))


@pytest.fixture(autouse=True)
def _blas16():
    with blas_threads():
        yield


@pytest.mark.parametrize("shape,variant,mixer", list(_cases()))
def test_predictions_hold(shape, variant, mixer):
    m = _make(shape, variant, mixer)
    n, me, mi, N = m.n, m.me, m.mi, m.N
    K = m.kkt_matrix()
    assert np.array_equal(K, K.T)
    # placement: the special coordinates sit on the tile / panel edges
    if variant == "pairs":
        assert (63, 64) in m.pairs and (255, 256) in m.pairs and (n - 2, n - 1) in m.pairs
        assert all(m.h["d2L"][i, i] == 0.0 and m.h["d2L"][j, j] == 0.0 for i, j in m.pairs) or mixer == "Q"
    if variant == "zero":
        z = np.flatnonzero(m.role == Z)
        t = (n // 2) // 64 * 64
        assert set(range(t, t + 64)) <= set(z) and {n - 2, n - 1} <= set(z)
        if mixer == "T":                                   # the zero rows are exact zeros of d2L
            assert not m.h["d2L"][z].any()
    if variant in ("neg", "sigma"):
        assert m.role[n - 1] == NN and m.role[n - 2] == NN
    # matvec from the blocks
    rng = np.random.default_rng(1)
    for _ in range(3):
        v = rng.standard_normal(N)
        want = K @ v
        assert np.linalg.norm(m.matvec(v) - want) <= 1e-14 * np.linalg.norm(np.abs(K) @ np.abs(v))
        Ks = K.copy()
        Ks[np.arange(n), np.arange(n)] += 0.37
        Ks[np.arange(n + mi, n + mi + me), np.arange(n + mi, n + mi + me)] -= 0.011
        assert np.linalg.norm(m.matvec(v, 0.37, 0.011) - Ks @ v) <= 1e-14 * np.linalg.norm(np.abs(Ks) @ np.abs(v))
    # inertia, unshifted
    neg, zero, pos = m.inertia()
    w = np.linalg.eigvalsh(K)
    if variant == "dependent":
        # the k exact zero eigenvalues come out at rounding level, which inertia_from_eig's |w| <= eps may count on either
        # side: count them against a bar far above rounding and far below every other |eigenvalue|
        assert zero == 3 and int(np.sum(np.abs(w) <= 1e-10)) == 3
        assert int(np.sum(w < -1e-10)) == neg and int(np.sum(w > 1e-10)) == pos
    else:
        assert zero == 0 and inertia_from_eig(K) == (neg, 0, pos)
        assert neg == m.counts()["Nn"] + m.counts()["pairs"] + me + mi
    # inertia after reghess' shifts (the orthogonal mixer keeps the spectrum of d2L + delta I at D + delta)
    shifts = [(0.0, DELTA_C)] if mixer == "T" else [(DELTA0 * 10.0 ** k, dc) for k in (0, 4, 7, 8, 9) for dc in (0.0, DELTA_C)]
    for delta, dc in shifts:
        if variant == "dependent" and dc == 0.0:
            continue
        if mixer == "T" and me == 0:
            continue
        Ks = K.copy()
        Ks[np.arange(n), np.arange(n)] += delta
        Ks[np.arange(n + mi, n + mi + me), np.arange(n + mi, n + mi + me)] -= dc
        assert inertia_from_eig(Ks) == m.inertia(delta, dc), (delta, dc)
    if variant == "dependent":
        assert m.inertia(0.0, DELTA_C)[0] == me + mi + m.counts()["Nn"] + m.counts()["pairs"]
    # the manufactured solution
    if variant != "dependent":
        x = np.linalg.solve(K, m.b)
        err = np.linalg.norm(x - m.x_true) / np.linalg.norm(m.x_true)
        if variant == "sigma":
            # Sigma over 12 decades: cond(K) ~ 1e12, no solver recovers x_true to 1e-12 -- LU's own error is the bar
            assert err <= 1e3 * EPS * np.linalg.cond(K), err
        else:
            assert err <= 1e-12, err
    # the mixer
    M = m.M
    if mixer == "Q":
        assert np.linalg.norm(M.T @ M - np.eye(n), 2) <= 1e-13
        assert np.array_equal(M, M.T)
        if me == mi == 0:
            dspec = np.abs(m.spectrum())
            exact = np.min(np.abs(w)) / np.max(np.abs(w))
            assert abs(exact / (dspec.min() / dspec.max()) - 1.0) <= 1e-12
            np.testing.assert_allclose(np.sort(w), m.spectrum(), rtol=0, atol=1e-13)
    else:
        keep = np.flatnonzero((m.role == PAIR) | (m.role == Z))
        assert np.array_equal(M[keep], np.eye(n)[keep])
        assert np.linalg.cond(M) <= 8.0


def test_rcond_spectrum_is_pinned():
    """The rcond cases of the GPU module: an isolated largest and smallest |D| give the exact rcond min|D| / max|D|, also
    at 1e-13 * max (450 eps), where the rounding of the assembled matrix (~1e-16 absolute) moves it by a few 1e-3."""
    for dmin in (1e-3, 4e-13):
        m = Manufactured(320, 0, 0, mixer="Q", n_neg=100, d_set={5: 4.0, 300: dmin}, seed=3, keep_mixer=True)
        assert m.role[5] == 0 and m.role[300] == 0
        w = np.linalg.eigvalsh(m.kkt_matrix())
        exact = np.min(np.abs(w)) / np.max(np.abs(w))
        assert abs(exact / (dmin / 4.0) - 1.0) <= (1e-12 if dmin > 1e-6 else 1e-2)
        assert sorted(np.abs(w))[1] >= 0.25 and sorted(np.abs(w))[-2] <= 2.0


def test_exact_zero_row_is_singular_in_floating_point():
    """T mixer, one Z coordinate, no constraints: a row of d2L is exactly zero."""
    m = Manufactured(300, 0, 0, mixer="T", n_zero=1, n_neg=50, seed=9)
    z = np.flatnonzero(m.role == Z)
    assert len(z) == 1 and not m.h["d2L"][z[0]].any()
