"""Manufactured KKT systems of known inertia and known solution (test helper; imported by tests, not a conftest).

The blocks follow the library's convention (d2L n x n, Je n x me, Ji n x mi, Sigma = lam_i / (s + eps)) and the layout of
``oracle.newton_oracle.kkt_matrix``.  They are built in y-coordinates, x = M y, with M a dense nonsingular mixer:

    d2L = M D M',  Je = M Ae,  Ji = M Ai,

so the KKT matrix is congruent to the y-coordinate one (Sylvester) and its inertia can be read off the roles of the y
coordinates:

* P     D in [0.5, 2]
* Nn    D in [-1.2, -0.25]                  (negative curvature)
* pairs [[0, b], [b, 0]] with b in [0.5, 2]  (one + and one - each; zero diagonals)
* Z     D = 0                                (zero Hessian rows: the LP / linear-variable case)

Ae lives on P only (full column rank), Ai on P and Z (full row rank on Z).  Nn and the pairs are then decoupled from the
convex remainder, and

    n_pos = |P| + |Z| + n_pairs + mi,   n_neg = |Nn| + n_pairs + me + mi,   n_zero = 0.

Mixers: ``"Q"`` = I - 2 W W' (W n x r orthonormal, r ~ n/8): orthogonal and symmetric, so the spectrum of d2L + delta I is
exactly D + delta.  ``"T"`` = I + 0.3 G / sqrt(n) with the rows of pair and Z coordinates replaced by identity rows: d2L
keeps the pairs' zero diagonals and the exact zero rows of Z while they stay densely coupled to everything else.

Every reference quantity is an O(N n) host computation in float64 (``matvec``), so the checks run at any size."""
from __future__ import annotations

import contextlib

import numpy as np

EPS = float(np.finfo(np.float64).eps)
P, NN, PAIR, Z = 0, 1, 2, 3


def blas_threads(limit=16):
    """Hold host BLAS to ``limit`` threads (a machine-wide pool is several times slower on the O(N n) products), never
    more than the pool the process started with (OpenBLAS cannot grow it and crashes when asked to)."""
    try:
        from threadpoolctl import threadpool_info, threadpool_limits
    except ImportError:
        return contextlib.nullcontext()
    pool = max([int(i.get("num_threads") or 1) for i in threadpool_info() if i.get("user_api") == "blas"] or [1])
    return threadpool_limits(limits=min(limit, pool), user_api="blas")


def _roles(n, rng, n_neg, n_pairs, zero_tile, n_zero):
    """Role of every y coordinate and the list of pairs.  The special coordinates sit where the kernels split work first:
    pairs straddle a 64-tile boundary (63|64) and a panel boundary (255|256), a zero block fills one whole 64-row tile,
    the last two coordinates carry the first special role asked for; the rest is spread at random."""
    role = np.full(n, P, dtype=np.int64)
    pairs = []

    def free(idx):
        return all(0 <= i < n and role[i] == P for i in idx)

    def draw(k):
        cand = np.flatnonzero(role == P)
        return list(rng.choice(cand, size=k, replace=False)) if k else []

    for i, j in ((63, 64), (255, 256), (n - 2, n - 1)):
        if len(pairs) < n_pairs and free((i, j)):
            role[[i, j]] = PAIR
            pairs.append((i, j))
    while len(pairs) < n_pairs:
        i, j = draw(2)
        role[[i, j]] = PAIR
        pairs.append((int(i), int(j)))
    if zero_tile:
        t = (n // 2) // 64 * 64                                   # a whole 64-row tile in the middle of the x block
        assert t + 64 <= n - 2 and free(range(t, t + 64)), "no free 64-row tile for the zero block"
        role[t:t + 64] = Z
    left = n_zero
    for i in (n - 2, n - 1):
        if left and free((i,)):
            role[i] = Z
            left -= 1
    role[draw(left)] = Z
    left = n_neg
    for i in (n - 2, n - 1):
        if left and free((i,)):
            role[i] = NN
            left -= 1
    role[draw(left)] = NN
    return role, pairs


class Manufactured(object):
    """One manufactured system.  Device tensors (``d2L``, ``Je``, ``Ji``, ``df``, ``ce``, ``ci``, ``s``, ``lam``) for the
    handle, float64 NumPy twins (``h``) for the host reference, the roles, ``x_true`` and ``b = K x_true``."""

    def __init__(self, n, me, mi, mixer="Q", n_neg=0, n_pairs=0, zero_tile=False, n_zero=0, dependent_eq=0,
                 sigma_decades=0.0, d_set=None, pin=None, seed=0, device="cpu", keep_mixer=False):
        import torch
        self.n, self.me, self.mi, self.mixer = int(n), int(me), int(mi), mixer
        self.N = self.n + self.me + 2 * self.mi
        self.dependent_eq = int(dependent_eq)
        rng = np.random.default_rng(seed)
        role, pairs = _roles(self.n, rng, int(n_neg), int(n_pairs), bool(zero_tile), int(n_zero))
        self.role, self.pairs = role, pairs
        d = np.zeros(n)
        d[role == P] = rng.uniform(0.5, 2.0, int(np.sum(role == P)))
        d[role == NN] = rng.uniform(-1.2, -0.25, int(np.sum(role == NN)))
        d_set = dict(d_set or {})
        if pin:                                                   # (largest, smallest) |D| on two random P coordinates
            d_set.update(zip(rng.choice(np.flatnonzero(role == P), size=2, replace=False).tolist(), pin))
        for i, v in d_set.items():                                # pinned spectrum entries (rcond tests); roles stay
            assert role[i] in (P, NN) and (v > 0) == (role[i] == P)
            d[i] = v
        beta = rng.uniform(0.5, 2.0, len(pairs))
        self.d, self.beta = d, beta
        nP, nZ = int(np.sum(role == P)), int(np.sum(role == Z))
        assert nZ == 0 or mi == 0 or mi >= 2 * nZ, "Ai needs full row rank on the zero rows (mi = 0: singular on purpose)"
        assert me == 0 or 4 * me <= 3 * nP                          # Ae full column rank, smallest singular value >~ 0.1
        assert self.dependent_eq <= me // 2

        dev = torch.device(device)
        f64 = dict(dtype=torch.float64, device=dev)
        gen = torch.Generator(device=dev)
        gen.manual_seed(int(seed) * 7919 + 17)

        def randn(*shape):
            return torch.randn(*shape, generator=gen, **f64)

        Dm = torch.diag(torch.from_numpy(d).to(dev))
        if pairs:
            pi = torch.tensor([p[0] for p in pairs], device=dev)
            pj = torch.tensor([p[1] for p in pairs], device=dev)
            bt = torch.from_numpy(beta).to(dev)
            Dm[pi, pj] = bt
            Dm[pj, pi] = bt
        if mixer == "Q":
            r = max(1, n // 8)
            W, _ = torch.linalg.qr(randn(n, r))
            M = torch.eye(n, **f64) - 2.0 * (W @ W.T)
            del W
        elif mixer == "T":
            M = randn(n, n).mul_(0.3 / np.sqrt(n))
            M.diagonal().add_(1.0)
            keep = torch.from_numpy(np.flatnonzero((role == PAIR) | (role == Z))).to(dev)
            M[keep] = 0.0
            M[keep, keep] = 1.0
        else:
            raise ValueError(mixer)
        A = (M @ Dm) @ M.T
        del Dm
        self.d2L = (A + A.T).mul_(0.5)                            # exactly symmetric (triu is what the library reads)
        del A
        iP = torch.from_numpy(np.flatnonzero(role == P)).to(dev)
        iZ = torch.from_numpy(np.flatnonzero(role == Z)).to(dev)
        if me:
            Ae = torch.zeros(n, me, **f64)
            Ae[iP] = randn(len(iP), me) / np.sqrt(n)
            Je = M @ Ae
            k = self.dependent_eq
            if k:                                                  # exact copies AFTER mixing: singular in floating point too
                Je[:, me - k:] = Je[:, :k]
            self.Je = Je
        else:
            self.Je = torch.zeros(n, 0, **f64)
        if mi:
            Ai = torch.zeros(n, mi, **f64)
            Ai[iP] = randn(len(iP), mi) / np.sqrt(n)
            if nZ:
                Ai[iZ] = randn(nZ, mi) / np.sqrt(mi)
            self.Ji = M @ Ai
        else:
            self.Ji = torch.zeros(n, 0, **f64)
        self.M = M.cpu().numpy() if keep_mixer else None
        del M
        # vectors: Sigma = lam_i / (s + eps) uniform in [0.5, 2], or spread over sigma_decades decades
        s = rng.uniform(0.5, 2.0, mi)
        sig = 10.0 ** rng.uniform(-sigma_decades / 2, sigma_decades / 2, mi) if sigma_decades else rng.uniform(0.5, 2.0, mi)
        lam = np.concatenate([rng.standard_normal(me), sig * s])
        vec = dict(df=rng.standard_normal(n), ce=rng.standard_normal(me), ci=rng.standard_normal(mi), s=s, lam=lam)
        if self.dependent_eq:                                     # duplicated constraints with the same right-hand side:
            vec["ce"][me - self.dependent_eq:] = vec["ce"][:self.dependent_eq]    # consistent, as in a real problem
        self.mu = 0.1
        for k_, v in vec.items():
            setattr(self, k_, torch.from_numpy(v).to(dev))
        self.h = dict(vec, d2L=self.d2L.cpu().numpy(), Je=self.Je.cpu().numpy(), Ji=self.Ji.cpu().numpy())
        self.sigma = lam[me:] / (s + EPS)
        self.x_true = rng.standard_normal(self.N)
        with blas_threads():
            self.b = self.matvec(self.x_true)

    # -- reference quantities ------------------------------------------------------------------------------------------
    def counts(self):
        role = self.role
        return dict(P=int(np.sum(role == P)), Nn=int(np.sum(role == NN)), Z=int(np.sum(role == Z)), pairs=len(self.pairs))

    def spectrum(self):
        """Eigenvalues of D: those of d2L itself with the orthogonal mixer."""
        single = self.d[self.role != PAIR]
        return np.sort(np.concatenate([single, self.beta, -self.beta]))

    def inertia(self, delta=0.0, delta_c=0.0):
        """(n_neg, n_zero, n_pos) of K + delta I_x - delta_c I_e (the order of ``newton_oracle.inertia_from_eig``).
        A shift of the x block is read off D only with the orthogonal mixer (then d2L + delta I = M (D + delta I) M')."""
        assert delta == 0.0 or self.mixer == "Q"
        dn = self.d[self.role == NN] + delta
        neg = int(np.sum(dn < 0)) + int(np.sum(np.abs(self.beta) > delta)) + self.me + self.mi
        zero = self.dependent_eq if delta_c == 0.0 else 0
        neg -= zero
        return neg, zero, self.N - neg - zero

    def matvec(self, v, delta=0.0, delta_c=0.0):
        """(K + delta I_x - delta_c I_e) v from the blocks in float64 (the signs of ``kkt_matrix``), no N x N matrix."""
        n, me, mi, h = self.n, self.me, self.mi, self.h
        v = np.asarray(v, dtype=np.float64)
        vx, vs, ve, vi = v[:n], v[n:n + mi], v[n + mi:n + mi + me], v[n + mi + me:]
        y = np.empty(self.N)
        y[:n] = h["d2L"] @ vx + delta * vx
        if me:
            y[:n] += h["Je"] @ ve
            y[n + mi:n + mi + me] = h["Je"].T @ vx - delta_c * ve
        if mi:
            y[:n] += h["Ji"] @ vi
            y[n:n + mi] = self.sigma * vs - vi
            y[n + mi + me:] = h["Ji"].T @ vx - vs
        return y

    def residual(self):
        """g = -grad, the right-hand side of the Newton step (``oracle.newton_oracle.kkt_residual``)."""
        from oracle import newton_oracle as orc
        h = self.h
        return -orc.kkt_residual(h["df"], h["Je"], h["Ji"], h["ce"], h["ci"], h["s"], h["lam"], self.mu,
                                 self.n, self.me, self.mi)

    def backward_error(self, raw, g, delta=0.0, delta_c=0.0):
        """|K raw - g| / |g| with K applied from the blocks (raw: the direction WITHOUT the multiplier sign flip)."""
        with blas_threads():
            return float(np.linalg.norm(self.matvec(raw, delta, delta_c) - g) / np.linalg.norm(g))

    def unflip(self, dz):
        raw = np.array(dz, dtype=np.float64)
        raw[self.n + self.mi:] *= -1.0
        return raw

    def kkt_matrix(self):
        """The dense N x N matrix (small sizes only: the CPU self-check)."""
        from oracle import newton_oracle as orc
        h = self.h
        return orc.kkt_matrix(h["d2L"], h["Je"], h["Ji"], h["s"], h["lam"], self.n, self.me, self.mi)

    def stage(self, core):
        core.stage_blocks(self.d2L, self.Je, self.Ji)
        core.stage_vectors(self.df, self.ce, self.ci, self.s, self.lam, mu=self.mu)

    def direction_args(self):
        """Positional arguments of ``HipNewtonBackend.direction`` after the blocks and vectors, for delta = 0 and the
        reference's constants (pyipm.py: reg_coef = delta0 = sqrt(eps), eta = 1e-4, beta = 0.4)."""
        return (self.d2L, self.Je, self.Ji, self.df, self.ce, self.ci, self.s, self.lam, self.mu, 0.0, self.mu,
                1e-4, 0.4, np.sqrt(EPS), np.sqrt(EPS), EPS)

    def free_device(self):
        for k in ("d2L", "Je", "Ji", "df", "ce", "ci", "s", "lam"):
            setattr(self, k, None)
