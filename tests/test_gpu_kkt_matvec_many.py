"""kkt_matvec_many: Y = Hc V for k columns in one pass over the staged blocks (pyipm_newton_kkt_matvec_many; the matrix of
pyipm.py:824-842 applied to a matrix), on the manufactured systems of tests/kkt_manufactured.py at the smallest shapes at
which the tiling can go wrong: N never a multiple of 128, n never a multiple of 4.

Values are judged against Hc V in extended precision with the a-priori bound of tests/test_gpu_strided_blocks.py for
kkt_matvec: a row of Hc has at most N terms, so |Y - Y_ref| <= N eps (|Hc| |V|) + one ulp of Y_ref whatever the summation
order -- no measured tolerance."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from kkt_manufactured import EPS, Manufactured

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [
    (200, 37, 59),       # several row tiles, ragged everywhere
    (130, 0, 70),        # no equalities, x block just over one tile
    (97, 40, 0),         # no inequalities: no slack rows
    (300, 130, 141),     # the multiplier rows span a tile border
    (61, 0, 0),          # nothing but the x block and the pad
]
IDS = ["%dx%dx%d" % s for s in SHAPES]
KS = (1, 3, 16, 17, 70)
DELTA, DELTA_C = 1e-3, 1e-7
NAN = float("nan")
BADARG = -1
LD = np.longdouble


@functools.lru_cache(maxsize=None)
def system(shape):
    n, me, mi = shape
    m = Manufactured(n, me, mi, seed=n + 3 * me + 5 * mi)
    m.V = np.random.default_rng(n + me + mi).standard_normal((m.N, max(KS)))
    return m


@functools.lru_cache(maxsize=None)
def reference(shape, delta, delta_c):
    """(Y_ref rounded to double, the componentwise bound) for all max(KS) columns: the dense Hc in np.longdouble from the
    blocks (the upper triangle of d2L mirrored, as the library reads it), Sigma = lam_i / (s + eps), delta, delta_c."""
    n, me, mi = shape
    m = system(shape)
    h, N = m.h, m.N
    H = np.zeros((N, N), dtype=LD)
    U = np.triu(h["d2L"]).astype(LD)
    H[:n, :n] = U + np.triu(U, 1).T
    H[np.arange(n), np.arange(n)] += LD(delta)
    s0, e0, i0 = n, n + mi, n + mi + me
    if me:
        H[:n, e0:i0] = h["Je"]
        H[e0:i0, :n] = h["Je"].T
        H[np.arange(e0, i0), np.arange(e0, i0)] = -LD(delta_c)
    if mi:
        H[:n, i0:] = h["Ji"]
        H[i0:, :n] = h["Ji"].T
        H[np.arange(s0, e0), np.arange(s0, e0)] = h["lam"][me:].astype(LD) / (h["s"].astype(LD) + LD(EPS))
        H[np.arange(s0, e0), np.arange(i0, N)] = -1.0
        H[np.arange(i0, N), np.arange(s0, e0)] = -1.0
    V = m.V.astype(LD)
    Y = H @ V
    Y64 = Y.astype(np.float64)
    bound = (LD(N) * LD(EPS) * (np.abs(H) @ np.abs(V))).astype(np.float64) + np.spacing(np.abs(Y64))
    return Y64, bound, Y


def handle(shape, kind="full", blocks=None):
    """A handle on the system of ``shape`` with blocks and vectors staged and the shifts (delta, delta_c) it applies:
    'full' / 'condensed' have been assembled with (DELTA, DELTA_C), a provider-only handle has no assembly and keeps (0, 0)."""
    from pyipm_amd.newton import NewtonCore
    n, me, mi = shape
    m = system(shape)
    core = NewtonCore(n, me, mi, device=0, provider_only=(kind == "provider"))
    if kind == "condensed":
        core.set_option("condensed", 1)
    if blocks is None:
        core.stage_blocks(m.d2L, m.Je, m.Ji)
    else:
        core.stage_blocks(*blocks)
    core.stage_vectors(m.df, m.ce, m.ci, m.s, m.lam, mu=m.mu)
    if kind == "provider":
        return core, (0.0, 0.0)
    core.residual()
    core.assemble(DELTA, DELTA_C)
    return core, (DELTA, DELTA_C)


def bits(t):
    a = t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


def raw_call(core, k, v, ld_v, y, ld_y, memkind=0):
    p = lambda t: ctypes.c_void_p(t.data_ptr() if hasattr(t, "data_ptr") else t.ctypes.data)      # noqa: E731
    return core.lib.pyipm_newton_kkt_matvec_many(core.h, k, p(v), ld_v, p(y), ld_y, memkind)


KINDS = [(s, "full") for s in SHAPES] + [(s, "provider") for s in SHAPES] + [(s, "condensed") for s in SHAPES if s[2]]


# ---- 1. values ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,kind", KINDS, ids=["%dx%dx%d-%s" % (s + (k,)) for s, k in KINDS])
def test_values_meet_the_a_priori_bound(shape, kind):
    import torch
    m = system(shape)
    core, (delta, delta_c) = handle(shape, kind)
    Yref, bound, _ = reference(shape, delta, delta_c)
    Vd = torch.from_numpy(m.V).cuda()
    for k in KS:
        Y = core.kkt_matvec_many(Vd[:, :k])
        assert tuple(Y.shape) == (m.N, k)
        Y = Y.cpu().numpy()
        err = np.abs(Y - Yref[:, :k])
        print("k = %d: worst error / bound = %.3f" % (k, float((err / bound[:, :k]).max())))
        assert np.all(err <= bound[:, :k]), (k, float(err.max()), np.unravel_index(np.argmax(err / bound[:, :k]), err.shape))
    # the one-vector entry computes the same matrix (to rounding)
    y1 = core.matvec(Vd[:, 0].contiguous()).cpu().numpy()
    assert np.all(np.abs(y1 - Yref[:, 0]) <= bound[:, 0])
    core.close()


# ---- 2. bitwise independence -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[3]], ids=[IDS[0], IDS[3]])
def test_a_column_keeps_its_bits_wherever_it_stands(shape):
    import torch
    m = system(shape)
    core, _ = handle(shape)
    rng = np.random.default_rng(9)
    vj = m.V[:, 7:8]
    one = core.kkt_matvec_many(torch.from_numpy(vj).cuda())
    assert bits(core.kkt_matvec_many(torch.from_numpy(vj).cuda())) == bits(one)         # two identical calls
    V17 = rng.standard_normal((m.N, 17)); V17[:, 5] = vj[:, 0]
    V70 = rng.standard_normal((m.N, 70)); V70[:, 69] = vj[:, 0]
    Y17 = core.kkt_matvec_many(torch.from_numpy(V17).cuda())
    Y70 = core.kkt_matvec_many(torch.from_numpy(V70).cuda())
    assert torch.equal(Y17[:, 5], one[:, 0]) and torch.equal(Y70[:, 69], one[:, 0])
    assert bits(core.kkt_matvec_many(torch.from_numpy(V70).cuda())) == bits(Y70)
    # NaN neighbours: whole columns, and single entries in every block of rows
    Vn = V17.copy()
    Vn[:, 4] = NAN
    Vn[[0, m.n - 1, m.N - 1], 6] = NAN
    Yn = core.kkt_matvec_many(torch.from_numpy(Vn).cuda())
    assert bool(torch.isnan(Yn[:, 4]).all()) and bool(torch.isnan(Yn[:, 6]).any())
    keep = [j for j in range(17) if j not in (4, 6)]
    assert torch.equal(Yn[:, keep], Y17[:, keep])
    core.close()


# ---- 3. layout ---------------------------------------------------------------------------------------------------------------------
def test_leading_dimensions_and_memory_kinds():
    import torch
    from pyipm_amd.newton import MEM_DEVICE, MEM_HOST
    shape = SHAPES[0]
    m = system(shape)
    core, _ = handle(shape)
    N, k, ld_v, ld_y = m.N, 17, m.N + 3, m.N + 5
    ref = core.kkt_matvec_many(torch.from_numpy(m.V[:, :k]).cuda()).cpu().numpy()
    got = core.kkt_matvec_many(m.V[:, :k])                                           # NumPy in, NumPy out: the host entry
    assert isinstance(got, np.ndarray) and got.shape == (N, k) and bits(got) == bits(ref)
    vh = np.full((k, ld_v), NAN)
    vh[:, :N] = m.V[:, :k].T
    yh = np.full((k, ld_y), 7.0)
    assert raw_call(core, k, vh, ld_v, yh, ld_y, MEM_HOST) == 0
    assert bits(yh[:, :N].T) == bits(ref) and np.all(yh[:, N:] == 7.0)
    vd = torch.from_numpy(vh).cuda()
    yd = torch.full((k, ld_y), 7.0, dtype=torch.float64, device="cuda")
    assert raw_call(core, k, vd, ld_v, yd, ld_y, MEM_DEVICE) == 0
    torch.cuda.synchronize()
    y = yd.cpu().numpy()
    assert bits(y[:, :N].T) == bits(ref) and np.all(y[:, N:] == 7.0)
    core.close()


def _padded(block, ld, off, triu_only=False):
    """``block`` as a row-strided view (row r at off + r * ld) of a NaN-filled device buffer; d2L with NaN below its diagonal."""
    import torch
    rows, width = block.shape
    if width == 0:
        return None
    buf = torch.full((off + rows * ld + 8,), NAN, dtype=torch.float64, device="cuda")
    view = buf.as_strided((rows, width), (ld, 1), off)
    view.copy_(block.cuda())
    if triu_only:
        r, c = np.tril_indices(rows, -1)
        view[torch.from_numpy(r).cuda(), torch.from_numpy(c).cuda()] = NAN
    return view


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[3]], ids=[IDS[0], IDS[3]])
def test_strided_blocks_give_the_bits_of_packed_ones(shape):
    import torch
    m = system(shape)
    n, me, mi = shape
    odd = lambda w: (w + 1) | 1                                                      # noqa: E731  (an odd ld > width)
    blocks = (_padded(m.d2L, odd(n), 1, triu_only=True), _padded(m.Je, odd(me), 3), _padded(m.Ji, odd(mi), 5))
    a, _ = handle(shape, blocks=blocks)
    for key, t in zip(("d2L", "Je", "Ji"), blocks):                                  # the views went through as they are
        assert t is None or (a._keep[key].data_ptr() == t.data_ptr() and a._keep[key].stride() == t.stride())
    b, _ = handle(shape)
    Vd = torch.from_numpy(m.V).cuda()
    Ya, Yb = a.kkt_matvec_many(Vd), b.kkt_matvec_many(Vd)
    assert bool(torch.isfinite(Ya).all()) and torch.equal(Ya, Yb)
    a.close(); b.close()


# ---- 4. state ----------------------------------------------------------------------------------------------------------------------
def test_state_is_left_alone():
    import torch
    shape = SHAPES[0]
    m = system(shape)
    Vd = torch.from_numpy(m.V).cuda()
    a, _ = handle(shape)
    b, _ = handle(shape)
    a.factor(); b.factor()                                 # (a residual is pending: the forward pass runs under the factorisation)
    a.kkt_matvec_many(Vd)
    assert torch.equal(a.solve(), b.solve())               # consumes the fused forward pass
    a.kkt_matvec_many(Vd)
    assert torch.equal(a.solve(), b.solve())               # the kept residual, solved again without the fused pass
    b.step(DELTA, DELTA_C)
    la, ma = b.step_lengths(0.99), b.merit_info()
    b.kkt_matvec_many(Vd)
    assert b.step_lengths(0.99) == la and b.merit_info() == ma
    a.close(); b.close()


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_and_the_empty_call():
    import torch
    from pyipm_amd.batched import BatchedNewton
    from pyipm_amd.newton import NewtonCore
    shape = SHAPES[0]
    m = system(shape)
    N = m.N
    vd = torch.from_numpy(np.ascontiguousarray(m.V[:, :3].T)).cuda()
    yd = torch.full((3, N), 5.0, dtype=torch.float64, device="cuda")

    def refused(core, k, v, ld_v, y, ld_y):
        assert raw_call(core, k, v, ld_v, y, ld_y) == BADARG
        assert len(core.lib.pyipm_newton_last_error(core.h)) > 0

    bn = BatchedNewton(70, 10, 30, batch=2)
    refused(bn, 1, vd, 140, yd, 140)
    bn.close()
    bare = NewtonCore(*shape, device=0)
    refused(bare, 3, vd, N, yd, N)                         # nothing staged
    bare.close()
    core, _ = handle(shape)
    refused(core, 3, vd, N - 1, yd, N)
    refused(core, 3, vd, N, yd, N - 1)
    refused(core, -1, vd, N, yd, N)
    refused(core, 3, vd, N, vd, N)                         # y is v
    both = torch.zeros(4 * N, dtype=torch.float64, device="cuda")
    refused(core, 3, both, N, both[N:], N)                 # y starts inside v
    assert raw_call(core, 0, vd, N, yd, N) == 0
    torch.cuda.synchronize()
    assert bool((yd == 5.0).all())
    core.close()


# ---- 6. the switch of solve_many ---------------------------------------------------------------------------------------------------
CHILD = """
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import numpy as np, torch
from kkt_manufactured import Manufactured
from pyipm_amd.newton import NewtonCore
m = Manufactured(200, 37, 59, seed=61)
X = np.random.default_rng(1).standard_normal((m.N, 20))
B = np.stack([m.matvec(X[:, j]) for j in range(20)], axis=1)
core = NewtonCore(m.n, m.me, m.mi, device=0)
m.stage(core)
core.residual(); core.assemble(0.0, 0.0); core.factor()
Xs = core.solve_many(B, flip=False, refine=2).cpu().numpy()
torch.cuda.synchronize()
np.savez(sys.argv[1], X=X, Xs=Xs)
core.close()
"""


def test_solve_many_refines_through_it_when_asked(tmp_path):
    out = {}
    for name, value in (("unset", None), ("set", "1")):
        env = dict(os.environ)
        env.pop("PYIPM_MS_MATVEC_MANY", None)
        if value is not None:
            env["PYIPM_MS_MATVEC_MANY"] = value
        path = str(tmp_path / (name + ".npz"))
        code = CHILD % dict(root=ROOT, tests=os.path.join(ROOT, "tests"))
        p = subprocess.run([sys.executable, "-c", code, path], env=env, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        out[name] = np.load(path)
    colerr = lambda A, B: np.linalg.norm(A - B, axis=0) / np.linalg.norm(B, axis=0)      # noqa: E731
    for name in out:
        assert colerr(out[name]["Xs"], out[name]["X"]).max() <= 1e-10, name
    assert colerr(out["set"]["Xs"], out["unset"]["Xs"]).max() <= 1e-12
