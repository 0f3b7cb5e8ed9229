"""L-BFGS direction (include/pyipm_lbfgs.h) at every memory depth the kernels branch on and past the fixed row strides,
against the CPU oracle (oracle/lbfgs_oracle.py).

tests/test_gpu_lbfgs.py pins the reference's recorded directions and a ragged sweep over (n, me, mi); this module moves
the two other quantities the kernels of csrc/kernels_lbfgs.hpp branch on:

* the depth m (r = 2m, rr = 2m + 1): the column passes of k_tall_tn (LB_CC = 17: rr = 19, 33, 35, 51, 53, 65), the
  64-lane k_small_solve and the r * ne = 64 * 65 outputs of k_small_gram at the cap m = 32, one handle at a shrinking m;
* the row count n against LB_KPAD = 8192 (n_pad), the 256 blocks x 32 rows of k_small_gram (second trip past 8192 rows),
  the 16384 blocks x 16 rows of k_jvec (second trip past 262144 rows), and the 1 .. 8 rows around the 4-row unroll and
  prefetch of tall_tn_body;
* and the one shape-dependent branch of the host side, the unsplit Gram launch of lb_factor_G (lb_ksplit == 1).

Every case is built as test_direction_matches_oracle_at_larger_sizes builds its own (make_qp(n, me, mi, 3), storage from
_storage, g standard normal, reg = 1e-12) and checked with that file's bounds: 1e-9 relative in the 2-norm where
4 (me + mi) <= n, 1e-6 otherwise (the Gram system squares J's condition), 1e-10 for the matrix-free residual.  Each case
prints its measured error."""
import functools

import numpy as np
import pytest

from test_gpu_lbfgs import EPS, _core, _rel, _storage

pytestmark = pytest.mark.gpu


def _tol(n, me, mi):
    return 1e-9 if 4 * (me + mi) <= n else 1e-6


def _qp_constraints(n, me, mi, seed=3):
    """Je, Ji, s and lambda of make_qp(n, me, mi, seed), bit for bit, without its Hessian: make_qp draws the n x n factor
    of Q first and forms Q = M M'/n + I, an n^3 product (13 of 19 s at n = 16400) that no direction reads.  The same draws in
    the same order, M's discarded in pieces."""
    rng = np.random.default_rng(seed)
    left = n * n
    while left:
        k = min(left, 1 << 22)
        rng.standard_normal(k)
        left -= k
    A = rng.standard_normal((me, n)) / np.sqrt(n)
    G = rng.standard_normal((mi, n)) / np.sqrt(n)
    rng.standard_normal(n)                                # c
    s = rng.uniform(0.5, 2.0, mi)
    lam_i = rng.uniform(0.5, 2.0, mi)
    lam_e = rng.standard_normal(me)
    return np.ascontiguousarray(A.T), np.ascontiguousarray(G.T), s, np.concatenate([lam_e, lam_i])


@functools.lru_cache(maxsize=None)
def _shape(n, me, mi):
    """Jacobians, s and lambda of make_qp(n, me, mi, 3), once per shape."""
    from pyipm_amd.problems import make_qp
    if me + mi == 0:
        return {"Je": None, "Ji": None, "s": np.zeros(0), "lda": np.zeros(0)}
    if n <= 2100:
        qp = make_qp(n, me, mi, 3)
        Je, Ji, s, lda = qp["Je"], qp["Ji"], qp["s"], qp["lam"]
    else:
        Je, Ji, s, lda = _qp_constraints(n, me, mi)
        small = make_qp(2100, me, mi, 3)                  # (2100^2 > one piece of the discarded draws)
        for got, want in zip(_qp_constraints(2100, me, mi), (small["Je"], small["Ji"], small["s"], small["lam"])):
            assert np.array_equal(got, want)              # make_qp changed its draws: restate them above
    return {"Je": Je if me else None, "Ji": Ji if mi else None, "s": s if mi else np.zeros(0), "lda": lda}


@functools.lru_cache(maxsize=None)
def _case(n, me, mi, m):
    """One direction's inputs and the oracle's answer, computed once and shared by the tests that need it (read only)."""
    from oracle import lbfgs_oracle as lo
    rng = np.random.default_rng(n + 7 * me + 13 * mi + m)
    c = dict(_shape(n, me, mi))
    zeta, S, Y, SS, L, D = _storage(n, m, rng, bool(me or mi), max(m, 1))
    assert S.shape[1] == m                    # lbfgs_update kept every pair: the depth under test is the depth run
    c.update(zeta=zeta, S=S, Y=Y, SS=SS, L=L, D=D, g=rng.standard_normal(n + 2 * mi + me))
    c["ref"] = lo.direction(c["g"], zeta, S, Y, SS, L, D, Je=c["Je"], Ji=c["Ji"], s=c["s"], lda=c["lda"], reg=1e-12)
    return c


def _run(core, c, **kw):
    dz, st = core.direction(c["g"], c["s"], c["lda"], c["zeta"], c["S"], c["Y"], c["SS"], c["L"], c["D"], reg=1e-12, **kw)
    return dz.cpu().numpy(), st


def _check_stats(st, m):
    assert st["m"] == m
    assert st["regularised"] == 0 and st["n_neg"] == 0 and st["n_zero"] == 0
    if m > 0:
        assert np.isfinite(st["small_pivot_min"]) and st["small_pivot_min"] > 0.0


def _vs_oracle(tag, n, me, mi, m, nb=128):
    c = _case(n, me, mi, m)
    core = _core(n, me, mi, max(m, 1), nb=nb)
    core.stage_jacobian(c["Je"], c["Ji"])
    dz, st = _run(core, c)
    core.close()
    _check_stats(st, m)
    err = _rel(dz, c["ref"])
    print("%s n=%d me=%d mi=%d m=%d: rel.err vs oracle %.3e (bound %.0e)" % (tag, n, me, mi, m, err, _tol(n, me, mi)))
    assert err <= _tol(n, me, mi), st


# ------------------------------------------------------------------------------------------- 1. depth sweep
DEPTHS = (1, 8, 9, 16, 17, 24, 25, 26, 31, 32)
SWEEP = [(300, 20, 44), (300, 30, 0), (300, 0, 70), (300, 0, 0)]


@pytest.mark.parametrize("m", DEPTHS)
@pytest.mark.parametrize("n,me,mi", SWEEP)
def test_depth_sweep_vs_oracle(n, me, mi, m):
    """rr = 2m + 1 on both sides of every split of k_tall_tn's passes of 17 columns (19: a second pass of 2; 33 / 35;
    51: three full passes and no partial one; 53; 63; 65: a last pass of 14), and at the cap m = 32 all 64 lanes of
    k_small_solve and the 64 * 65 outputs of k_small_gram.  flip=True negates exactly the multiplier rows."""
    _depth_case(n, me, mi, m)


@pytest.mark.parametrize("n,me,mi,m", [(40, 0, 0, 32), (70, 10, 20, 32)])
def test_depth_close_to_n_vs_oracle(n, me, mi, m):
    """The cap m = 32 with n barely above it: 2m = 64 columns of W over 40 and 70 rows."""
    _depth_case(n, me, mi, m)


def _depth_case(n, me, mi, m):
    c = _case(n, me, mi, m)
    core = _core(n, me, mi, m, nb=128)
    core.stage_jacobian(c["Je"], c["Ji"])
    dz, st = _run(core, c)
    flipped, _ = _run(core, c, flip=True)
    core.close()
    _check_stats(st, m)
    err = _rel(dz, c["ref"])
    print("depth n=%d me=%d mi=%d m=%d: rel.err vs oracle %.3e (bound %.0e)" % (n, me, mi, m, err, _tol(n, me, mi)))
    assert err <= _tol(n, me, mi), st
    np.testing.assert_array_equal(flipped[:n + mi], dz[:n + mi])
    np.testing.assert_array_equal(flipped[n + mi:], -dz[n + mi:])


# ------------------------------------------------------------------------------------------- 2. one handle, shrinking depth
@pytest.mark.parametrize("n,me,mi", [(300, 20, 44), (300, 0, 0)])
def test_one_handle_at_shrinking_depth(n, me, mi):
    """lbfgs_update grows the storage from 0 and drops it back to 0 after a failed update: one handle of max_pairs = 32
    is called at m = 32, 3, 17, 0, 32 on the same staged Jacobians, so V, Hs, Ha, Hb, M2, v11 and gpart are reused at a
    smaller rr.  Every result matches the oracle AND, bit for bit, a fresh handle of max_pairs = max(m, 1) whose
    (NaN-poisoned) workspace never held a deeper call: the kernels take rr = 2m + 1, never the cap."""
    order = (32, 3, 17, 0, 32)
    shared = _core(n, me, mi, 32, nb=128)
    shape = _shape(n, me, mi)
    shared.stage_jacobian(shape["Je"], shape["Ji"])
    got = []
    for m in order:
        c = _case(n, me, mi, m)
        dz, st = _run(shared, c)
        _check_stats(st, m)
        err = _rel(dz, c["ref"])
        print("shrinking n=%d me=%d mi=%d m=%d on the shared handle: rel.err vs oracle %.3e" % (n, me, mi, m, err))
        assert err <= _tol(n, me, mi), (m, st)
        assert shared.last_timings()["gram_launches"] == (1 if me + mi else 0)
        fresh = _core(n, me, mi, max(m, 1), nb=128)
        fresh.stage_jacobian(shape["Je"], shape["Ji"])
        dz_fresh, st_fresh = _run(fresh, c)
        fresh.close()
        assert np.array_equal(dz, dz_fresh), (m, float(np.max(np.abs(dz - dz_fresh))))
        assert st["small_pivot_min"] == st_fresh["small_pivot_min"]
        got.append(dz)
    shared.close()
    assert np.array_equal(got[0], got[-1])


# ------------------------------------------------------------------------------------------- 3. tiny n
@pytest.mark.parametrize("n,me,mi,m", [(1, 0, 0, 1), (2, 0, 1, 2), (3, 0, 0, 3), (4, 1, 2, 4), (7, 2, 3, 3), (8, 3, 0, 5),
                                       (6, 0, 2, 0)])
def test_tiny_n_vs_oracle(n, me, mi, m):
    """The rows one split of tall_tn_body can hold around its 4-row unroll: 1 - 3 never enter it, 4 - 7 enter once and
    take the "re-read the current four" branch of the prefetch, 8 prefetches a real second four; (6, 0, 2, 0) is the
    empty storage."""
    _vs_oracle("tiny", n, me, mi, m)


# ------------------------------------------------------------------------------------------- 4. past one n_pad
@pytest.mark.parametrize("n,me,mi,m", [(8193, 5, 9, 9), (8300, 40, 88, 32), (8193, 0, 0, 32), (16400, 3, 6, 17)])
def test_past_one_row_pad_vs_oracle(n, me, mi, m):
    """n > LB_KPAD = 8192: n_pad = 16384 (24576 for n = 16400, no power-of-two multiple), and k_small_gram's 256 blocks
    of 32-row chunks take a second (third) trip of their grid-stride loop."""
    _vs_oracle("rows", n, me, mi, m, nb=256)


def test_single_split_gram_vs_oracle():
    """The ksplit == 1 branch of lb_factor_G (the Gram launch straight into Gc, no partial matrices): lb_ksplit's cost
    model returns 1 where the tile count T = nt (nt + 1) / 2 sits just under a multiple of the 512 block slots, first at
    p_pad = 3584 (nt = 28, T = 406: one round unsplit, two rounds of half the depth plus the sums when split in two) for
    n_pad = 8192 and 16384.  p = 3540 constraints over n = 600 rows; 4 p > n, so the 1e-6 bound.  Nothing here reads the
    split factor back: if lb_ksplit's model changes, evaluate it again to keep this case on the branch."""
    _vs_oracle("ksplit1", 600, 40, 3500, 2, nb=256)


# ------------------------------------------------------------------------------------------- 5. past one k_jvec trip
@pytest.mark.parametrize("n,me,mi,m", [(262144 + 21, 30, 70, 9)])
def test_past_one_jvec_trip_matrix_free(n, me, mi, m):
    """n > 16384 blocks x 16 rows: k_jvec's stride loop takes a second trip (the last block of it on a partial four);
    the J'V pass runs 1025 splits of 256 rows and a partial second column pass.  No oracle at this size: the direction
    must solve H dz = g for H = Z - U inv(M) U', applied matrix-free with torch as in
    test_large_direction_satisfies_the_quasi_newton_system; the second direction runs on the cached J'J."""
    import torch
    p, N = me + mi, n + 2 * mi + me
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev); gen.manual_seed(3)
    J = torch.randn((n, p), generator=gen, dtype=torch.float64, device=dev) / np.sqrt(n)
    rng = np.random.default_rng(4)
    S = rng.standard_normal((n, m)) / np.sqrt(n)
    Mq = rng.standard_normal((n, 8)) / 3.0
    Y = Mq @ (Mq.T @ S) + 0.5 * S
    SY = S.T @ Y
    SS, L, D = S.T @ S, np.tril(SY, -1), np.diag(np.diag(SY))
    zeta = float(SY[-1, -1] / SS[-1, -1])
    td = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)       # noqa: E731
    Sd, Yd = td(S), td(Y)
    core = _core(n, me, mi, m)
    core.stage_jacobian(J[:, :me], J[:, me:])
    for trial in range(2):                                  # second pass: other Sigma / zeta on the cached J'J
        s = td(rng.uniform(0.5, 2.0, mi))
        lda = td(np.concatenate([rng.standard_normal(me), rng.uniform(0.5, 2.0, mi)]))
        g = td(rng.standard_normal(N))
        z = zeta * (1.0 + trial)
        dz, st = core.direction(g, s, lda, z, Sd, Yd, SS, L, D, reg=1e-12)
        _check_stats(st, m)
        x, ds, dl = dz[:n], dz[n:n + mi], dz[n + mi:]
        W = torch.cat([z * Sd, Yd], dim=1)
        Minv = td(np.block([[z * SS, L], [L.T, -D]]))
        res = torch.empty_like(dz)
        res[:n] = z * x - W @ torch.linalg.solve(Minv, W.T @ x) + J @ dl
        res[n:n + mi] = lda[me:] / (s + EPS) * ds - dl[me:]
        low = J.t() @ x
        low[me:] -= ds
        res[n + mi:] = low
        err = float((res - g).norm() / g.norm())
        print("jvec n=%d me=%d mi=%d m=%d trial %d: |H dz - g| / |g| = %.3e (bound 1e-10)" % (n, me, mi, m, trial, err))
        assert err <= 1e-10
        assert core.last_timings()["gram_launches"] == 1
    core.close()


# ------------------------------------------------------------------------------------------- 6. determinism
@pytest.mark.parametrize("n,me,mi,m,nb", [(300, 20, 44, 32, 128), (8193, 5, 9, 9, 256)])
def test_same_direction_twice_is_bit_equal(n, me, mi, m, nb):
    """Fixed partitions and a fixed summation order (the split-K Gram launch, J'V, the skinny reductions): the same
    direction twice on one handle gives the same bits, the second time on the cached J'J."""
    c = _case(n, me, mi, m)
    core = _core(n, me, mi, m, nb=nb)
    core.stage_jacobian(c["Je"], c["Ji"])
    first, st = _run(core, c)
    second, st2 = _run(core, c)
    assert core.last_timings()["gram_launches"] == 1
    core.close()
    _check_stats(st, m)
    assert np.array_equal(first, second), float(np.max(np.abs(first - second)))
    assert st == st2
