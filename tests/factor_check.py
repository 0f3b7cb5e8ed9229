"""The block LDL' factor itself, entrywise, against extended precision (test helper; imported by tests, not a conftest).

The library keeps K = Lb * blockdiag(T_k) * Lb' with Lb unit BLOCK lower triangular and 64 x 64 block pivots T_k.  From the
assembled matrix K and Lb alone the pivots follow by recursion; for tile column k (k0 = 64 k, k1 = k0 + 64):

    S_k = K[k0:, k0:k1] - sum_{j<k} Lb[k0:, j] T_j Lb[k, j]'          (numpy.longdouble)
    T_k = the first 64 rows of S_k, symmetrised
    R_k = S_k[64:, :] - Lb[k1:, k] T_k                                 (zero for an exact factor)

and the same sums of absolute values bound what rounding may leave in R_k:

    B_k = |K[k1:, k0:k1]| + sum_{j<k} |Lb[k1:, j]| |T_j| |Lb[k, j]|' + |Lb[k1:, k]| |T_k|          (float64, BLAS)

``check_factor`` returns max |R| / (eps B): O(1) whatever the growth and the grading of the matrix, so an error of 1e-11 in
one entry of Lb shows.  B counts |Lb| |T_k| too, so B = 0 only where Lb itself is an exact zero, and there R = 0; a structural
zero of Lb that holds anything else has R = -Lb T_k against B = |Lb| |T_k|: a ratio of 1 / eps.  The eigenvalues
of the T_k give the inertia (Sylvester), independent of every pivot kernel's counters.

Only entries of Lb strictly below the diagonal tiles are read (i // 64 > j // 64): the diagonal tiles and the upper part of
the storage hold pivot-kernel state or NaN poison and are not part of the factor as the substitutions read it
(csrc/kernels_solve.hpp, header comment)."""
from __future__ import annotations

import hashlib
import time
from collections import namedtuple

import numpy as np

EPS = float(np.finfo(np.float64).eps)
LD = np.longdouble
MARGIN = 4.0          # a device factor may exceed the model's ratio on the same matrix by this factor (see bound()): MFMA sums
                      # products in groups of 4 and in another order than NumPy.  Measured on an MI355X: 1.2 .. 3.0 times the model
                      # (tests/test_gpu_factor_entrywise.py), so the largest margin the bound allows is kept, not a tighter one
                      # fitted to those runs

FactorCheck = namedtuple("FactorCheck", "ratio where growth n_pos n_neg exact_zeros seconds")
FactorCheck.__doc__ = """ratio: max |R| / (eps B) (inf where B = 0 and R != 0); where: (tile column, row, column) of it;
growth: max B / max |K|; (n_pos, n_neg): signs of the eigenvalues of the T_k (identity padding included);
exact_zeros: entries with B = 0 (all of them had R = 0 unless ratio is inf); seconds: CPU time of the reconstruction
(0 when the result came out of the cache)."""

_cache = {}


def _lower_tiles_mask(Np, tb):
    t = np.arange(Np) // tb
    return t[:, None] > t[None, :]


def check_factor(K, Lb, tb=64):
    """K: (Npad, Npad), lower triangle of the assembled matrix (identity-padded); Lb: (Npad, Npad), read strictly below the
    diagonal tiles only.  Returns a FactorCheck.  Results are cached on the bits of what is read."""
    K = np.asarray(K, dtype=np.float64)
    Lb = np.asarray(Lb, dtype=np.float64)
    Np = K.shape[0]
    assert K.shape == (Np, Np) and Lb.shape == (Np, Np) and Np % tb == 0, (K.shape, Lb.shape, tb)
    mask = _lower_tiles_mask(Np, tb)
    assert np.isfinite(Lb[mask]).all(), "non-finite entry of Lb below the diagonal tiles"
    Kt = np.tril(K)
    assert np.isfinite(Kt).all(), "non-finite entry in the lower triangle of K"
    L = np.where(mask, Lb, 0.0)
    key = hashlib.sha256(Kt.tobytes() + L.tobytes() + bytes([tb])).hexdigest()
    if key in _cache:
        return _cache[key]._replace(seconds=0.0)
    t0 = time.perf_counter()
    nt = Np // tb
    Ksym = Kt + np.tril(Kt, -1).T
    Ll, aL, aK = L.astype(LD), np.abs(L), np.abs(Ksym)
    V = np.zeros((Np, tb), dtype=LD)             # rows of tile j: T_j Lb[k, j]'  (rebuilt per k)
    aV = np.zeros((Np, tb))
    T, aT = [], []
    worst, where, bmax, nz = 0.0, (0, 0, 0), 0.0, 0
    n_pos = n_neg = 0
    for k in range(nt):
        k0, k1 = k * tb, (k + 1) * tb
        S = Ksym[k0:, k0:k1].astype(LD)
        if k:
            for j in range(k):
                j0, j1 = j * tb, (j + 1) * tb
                V[j0:j1] = T[j] @ Ll[k0:k1, j0:j1].T
                aV[j0:j1] = aT[j] @ aL[k0:k1, j0:j1].T
            # (the extended-precision product has no BLAS: leave out what the KKT block structure makes exact zeros -- columns
            #  whose row of V is zero, rows of Lb that are zero in what is left)
            cols = np.flatnonzero(aV[:k0].any(axis=1))
            if cols.size:
                rows = np.flatnonzero(aL[k0:, cols].any(axis=1))
                if rows.size:
                    S[rows] -= Ll[k0:, :k0][np.ix_(rows, cols)] @ V[cols]
        Tk = np.tril(S[:tb]) + np.tril(S[:tb], -1).T
        T.append(Tk)
        aT.append(np.abs(Tk).astype(np.float64))
        w = np.linalg.eigvalsh(Tk.astype(np.float64))
        n_pos += int(np.sum(w > 0))
        n_neg += int(np.sum(w < 0))
        if k1 == Np:
            break
        R = np.abs(S[tb:] - Ll[k1:, k0:k1] @ Tk).astype(np.float64)
        B = aK[k1:, k0:k1] + aL[k1:, k0:k1] @ aT[k]
        if k:
            B += aL[k1:, :k0] @ aV[:k0]
        bmax = max(bmax, float(B.max()))
        zero = B == 0.0
        nz += int(zero.sum())
        ratio = np.where(zero, np.where(R == 0.0, 0.0, np.inf), R / (EPS * np.where(zero, 1.0, B)))
        i, c = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        if ratio[i, c] > worst:
            worst, where = float(ratio[i, c]), (k, int(k1 + i), int(k0 + c))
    res = FactorCheck(worst, where, bmax / float(aK.max()), n_pos, n_neg, nz, time.perf_counter() - t0)
    _cache[key] = res
    return res


def model_factor(A, tb=64, **kw):
    """(K, Lb, BlockLDL) of the NumPy twin of the device algorithm (oracle/block_ldl_model.py) in the checker's layout: K the
    identity-padded lower triangle, Lb the model's storage (its diagonal tiles hold Schur complements: not read)."""
    from oracle.block_ldl_model import BlockLDL
    f = BlockLDL(A, tb=tb, **kw)
    K = np.eye(f.Np)
    K[:f.N, :f.N] = f.A0
    return np.tril(K), f.M, f


def bound(model_ratio, Npad, margin):
    """What a device factor may reach: `margin` times the model's ratio on the same matrix, and never more than the a-priori
    ceiling Npad + 64 (products accumulated per entry)."""
    return min(margin * model_ratio, float(Npad + 64))


# ---- reading a NewtonCore ---------------------------------------------------------------------------------------------------
def storage_to_lower(S):
    """kkt_storage() is the (ncols, ld) row-major view of column-major lower storage: row j is column j.  Returns the
    (ld, ld) array A with A[i, j] = S[j, i] (columns the handle does not store stay zero)."""
    S = np.asarray(S)
    nc, ld = S.shape
    A = np.zeros((ld, ld))
    A[:, :nc] = S.T
    return A


def factor_of(core, factor=None, delta=0.0, delta_c=0.0):
    """(K, Lb, stats) of a staged handle.  The order matters: the view is taken FIRST (handing the pointer out makes every
    following assemble() store every entry and turns the reuse of kept factors off), then assemble, clone K, factor (``factor``:
    a callable taking the handle, default ``core.factor()``), clone Lb."""
    view = core.kkt_storage()
    core.assemble(delta, delta_c)
    view = core.kkt_storage()                     # (the condensed form has its own ld and ncols, known after assemble)
    K = view.clone()
    st = factor(core) if factor is not None else core.factor()
    core.torch.cuda.synchronize()
    Lb = view.clone()
    K, Lb = K.cpu().numpy(), Lb.cpu().numpy()
    assert K.shape[0] == K.shape[1], K.shape      # (single rank: every column is stored)
    return storage_to_lower(np.triu(K)), storage_to_lower(Lb), st      # (triu of the view: the lower triangle; the rest may be NaN)
