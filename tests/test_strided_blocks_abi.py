"""What the three bindings hand to the C-ABI for a caller-owned block: a row-strided view (dense rows, stride(-2) >= width, for the
batch a stride >= rows * stride(-2)) arrives as (data_ptr of the view, its strides) and is the SAME storage -- the library retains
device pointers, the binding may not copy behind the caller's back -- while every other layout arrives packed.  No GPU: the
handles are built without their constructors around a ``lib`` that records its arguments, on CPU tensors with ``device`` = cpu
(the bindings compare the tensor's device with the handle's, whichever it is)."""
import types

import numpy as np
import torch

F64 = torch.float64


class Recorder(object):
    """Every pyipm_* call returns 0 and is kept as (name, args)."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("pyipm_"):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn

    def last(self, name):
        return [a for k, a in self.calls if k == name][-1]


class NoStreams(object):
    """torch, but for the current stream (the bindings pass its handle on and wait for it)."""

    def __init__(self):
        st = types.SimpleNamespace(cuda_stream=0, synchronize=lambda: None)
        self.cuda = types.SimpleNamespace(current_stream=lambda device=None: st)

    def __getattr__(self, name):
        return getattr(torch, name)


def val(p):
    """ctypes pointer argument -> address (None: null)."""
    return getattr(p, "value", p)


def padded(rows, width, ld, off, batch=None, batch_stride=None, seed=0):
    """A (rows, width) / (batch, rows, width) view into a flat buffer: row r at off + [b * batch_stride +] r * ld."""
    g = torch.Generator().manual_seed(seed)
    if batch is None:
        buf = torch.full((off + rows * ld,), float("nan"), dtype=F64)
        v = buf.as_strided((rows, width), (ld, 1), off)
        v.copy_(torch.randn((rows, width), dtype=F64, generator=g))
    else:
        buf = torch.full((off + batch * batch_stride,), float("nan"), dtype=F64)
        v = buf.as_strided((batch, rows, width), (batch_stride, ld, 1), off)
        v.copy_(torch.randn((batch, rows, width), dtype=F64, generator=g))
    return buf, v


def same_storage(t, view):
    return t.data_ptr() == view.data_ptr() and t.untyped_storage().data_ptr() == view.untyped_storage().data_ptr()


def is_packed_copy(t, view):
    return t.is_contiguous() and t.untyped_storage().data_ptr() != view.untyped_storage().data_ptr() and torch.equal(t, view)


def newton_core(n, me, mi):
    from pyipm_amd.newton import NewtonCore
    c = object.__new__(NewtonCore)
    c.torch, c.lib, c.device = NoStreams(), Recorder(), torch.device("cpu")
    c.n, c.me, c.mi, c.N = n, me, mi, n + 2 * mi + me
    c.provider_only, c._keep = False, {}
    c.h = None                                       # (close() at collection: nothing to destroy)
    c._use_current_stream = lambda: None
    return c


def test_newton_stage_blocks_passes_row_strided_views_through():
    n, me, mi = 6, 2, 3
    c = newton_core(n, me, mi)
    (_, H), (_, E), (_, I) = padded(n, n, n + 1, 0), padded(n, me, me + 2, 1, seed=1), padded(n, mi, 64 + 64, 2, seed=2)
    c.stage_blocks(H, E, I)
    _, pH, ldH, pE, ldE, pI, ldI, memkind = c.lib.last("pyipm_newton_stage_blocks")
    assert (val(pH), ldH) == (H.data_ptr(), n + 1)
    assert (val(pE), ldE) == (E.data_ptr(), me + 2)
    assert (val(pI), ldI) == (I.data_ptr(), 128)
    assert memkind == 0
    for k, v in (("d2L", H), ("Je", E), ("Ji", I)):
        assert same_storage(c._keep[k], v), k          # kept alive: the very tensor, not a copy
    # the row-sharded staging shares the helper
    c.owned_rows = lambda: np.arange(4)
    c.stage_blocks_owned(H[:4], E[:4], I[:4])
    _, pH, ldH, pE, ldE, pI, ldI, _ = c.lib.last("pyipm_newton_stage_blocks_owned")
    assert (val(pH), ldH, val(pE), ldE, val(pI), ldI) == (H.data_ptr(), n + 1, E.data_ptr(), me + 2, I.data_ptr(), 128)


def test_newton_stage_blocks_packs_every_other_layout():
    n, me, mi = 6, 2, 3
    c = newton_core(n, me, mi)
    Ht = torch.randn((n, n), dtype=F64).t()                           # transposed: stride (1, n)
    Et = torch.randn((me, n), dtype=F64).t()
    I2 = torch.randn((n, 2 * mi), dtype=F64)[:, ::2]                  # every other column: stride(1) == 2
    c.stage_blocks(Ht, Et, I2)
    _, pH, ldH, pE, ldE, pI, ldI, _ = c.lib.last("pyipm_newton_stage_blocks")
    assert (ldH, ldE, ldI) == (n, me, mi)
    for k, v, p in (("d2L", Ht, pH), ("Je", Et, pE), ("Ji", I2, pI)):
        assert is_packed_copy(c._keep[k], v) and val(p) == c._keep[k].data_ptr(), k
    # rows that overlap (stride(0) < width), a reversed copy's negative-stride stand-in (flip makes a copy in torch: a zero
    # stride is the layout a view CAN have), another dtype, a NumPy array
    ov = torch.randn(64, dtype=F64).as_strided((n, n), (n - 1, 1))
    ex = torch.randn((1, n), dtype=F64).expand(n, n)
    f32 = torch.randn((n, n), dtype=torch.float32)
    host = np.random.default_rng(0).standard_normal((n, n))
    for bad in (ov, ex, f32, host):
        c.stage_blocks(bad, Et, I2)
        _, pH, ldH = c.lib.last("pyipm_newton_stage_blocks")[:3]
        kept = c._keep["d2L"]
        assert ldH == n and kept.is_contiguous() and kept.dtype == F64 and val(pH) == kept.data_ptr()
        assert np.array_equal(kept.numpy(), np.asarray(bad, dtype=np.float64) if isinstance(bad, np.ndarray) else bad.double().numpy())
    # a packed tensor goes through as it is, as it always did
    Hc = torch.randn((n, n), dtype=F64)
    c.stage_blocks(Hc, Et, I2)
    assert same_storage(c._keep["d2L"], Hc) and c.lib.last("pyipm_newton_stage_blocks")[2] == n
    # absent blocks: null pointers, a leading dimension of at least 1 (what the binding has always passed)
    c0 = newton_core(n, 0, 0)
    c0.stage_blocks(Hc)
    _, pH, ldH, pE, ldE, pI, ldI, _ = c0.lib.last("pyipm_newton_stage_blocks")
    assert (val(pH), ldH, val(pE), ldE, val(pI), ldI) == (Hc.data_ptr(), n, None, 1, None, 1)


def batched(n, me, mi, B):
    from pyipm_amd.batched import BatchedNewton
    bn = object.__new__(BatchedNewton)
    bn.torch, bn.lib, bn.device = NoStreams(), Recorder(), torch.device("cpu")
    bn.n, bn.me, bn.mi, bn.N = n, me, mi, n + 2 * mi + me
    bn.h, bn.batch, bn._keep = 1, B, None               # (a handle of this batch size exists: stage() creates none)
    bn.close = lambda: None
    return bn


def _vectors(n, me, mi, B):
    z = lambda k: torch.zeros((B, k), dtype=F64)        # noqa: E731
    return dict(df=z(n), ce=z(me), ci=z(mi), s=z(mi), lda=z(me + mi))


def test_batched_stage_passes_row_and_batch_strides_through():
    n, me, mi, B = 5, 2, 3, 4
    bn = batched(n, me, mi, B)
    ldh, lde, ldi = n + 1, me + 2, 128
    (_, H), (_, E), (_, I) = (padded(n, n, ldh, 0, B, n * ldh + 3), padded(n, me, lde, 1, B, n * lde + 3, seed=1),
                              padded(n, mi, ldi, 2, B, n * ldi + 3, seed=2))
    bn.stage(H, E, I, **_vectors(n, me, mi, B))
    _, pH, lH, sH, pE, lE, sE, pI, lI, sI = bn.lib.last("pyipm_newton_stage_blocks_batched")
    assert (val(pH), lH, sH) == (H.data_ptr(), ldh, n * ldh + 3)
    assert (val(pE), lE, sE) == (E.data_ptr(), lde, n * lde + 3)
    assert (val(pI), lI, sI) == (I.data_ptr(), ldi, n * ldi + 3)
    for kept, v in zip(bn._keep[0], (H, E, I)):
        assert same_storage(kept, v)
    # a batch cut out of a bigger tensor (every other member): only the batch stride differs from the packed one
    big = torch.randn((2 * B, n, n), dtype=F64)
    bn.stage(big[::2], E, I, **_vectors(n, me, mi, B))
    _, pH, lH, sH = bn.lib.last("pyipm_newton_stage_blocks_batched")[:4]
    assert (val(pH), lH, sH) == (big.data_ptr(), n, 2 * n * n) and same_storage(bn._keep[0][0], big[::2])


def test_batched_stage_packs_every_other_layout():
    n, me, mi, B = 5, 2, 3, 4
    bn = batched(n, me, mi, B)
    Ht = torch.randn((B, n, n), dtype=F64).transpose(1, 2)                        # rows transposed
    Eb = torch.randn((n, B, me), dtype=F64).transpose(0, 1)                       # members interleaved: stride(0) < rows * stride(1)
    Ix = torch.randn((1, n, mi), dtype=F64).expand(B, n, mi)                      # zero batch stride
    bn.stage(Ht, Eb, Ix, **_vectors(n, me, mi, B))
    _, pH, lH, sH, pE, lE, sE, pI, lI, sI = bn.lib.last("pyipm_newton_stage_blocks_batched")
    assert (lH, sH, lE, sE, lI, sI) == (n, n * n, me, n * me, mi, n * mi)
    for kept, v, p in zip(bn._keep[0], (Ht, Eb, Ix), (pH, pE, pI)):
        assert is_packed_copy(kept, v) and val(p) == kept.data_ptr()
    # absent blocks as before: null, 0, 0
    b0 = batched(n, 0, 0, B)
    Hc = torch.randn((B, n, n), dtype=F64)
    b0.stage(Hc, None, None, **_vectors(n, 0, 0, B))
    _, pH, lH, sH, pE, lE, sE, pI, lI, sI = b0.lib.last("pyipm_newton_stage_blocks_batched")
    assert (val(pH), lH, sH, val(pE), lE, sE, val(pI), lI, sI) == (Hc.data_ptr(), n, n * n, None, 0, 0, None, 0, 0)


def lbfgs_core(n, me, mi, cap):
    from pyipm_amd.lbfgs import LbfgsCore
    c = object.__new__(LbfgsCore)
    c.torch, c.lib, c.device = NoStreams(), Recorder(), torch.device("cpu")
    c.n, c.me, c.mi, c.cap, c.N = n, me, mi, cap, n + 2 * mi + me
    c.h = None
    return c


def test_lbfgs_passes_row_strided_views_through_and_packs_the_rest():
    n, me, mi, m = 7, 2, 3, 4
    c = lbfgs_core(n, me, mi, m)
    (_, E), (_, I) = padded(n, me, me + 1, 0), padded(n, mi, mi + 2, 1, seed=1)
    c.stage_jacobian(E, I)
    _, pE, ldE, pI, ldI, memkind = c.lib.last("pyipm_lbfgs_stage_jacobian")
    assert (val(pE), ldE, val(pI), ldI, memkind) == (E.data_ptr(), me + 1, I.data_ptr(), mi + 2, 0)
    Et = torch.randn((me, n), dtype=F64).t()
    c.stage_jacobian(Et, I)
    _, pE, ldE, pI, ldI, _ = c.lib.last("pyipm_lbfgs_stage_jacobian")
    assert ldE == me and val(pE) != Et.data_ptr() and (val(pI), ldI) == (I.data_ptr(), mi + 2)
    (_, S), (_, Y) = padded(n, m, m + 1, 0, seed=2), padded(n, m, 128, 2, seed=3)
    z = torch.zeros
    small = [np.eye(m)] * 3
    c.direction(z(c.N, dtype=F64), z(mi, dtype=F64), z(me + mi, dtype=F64), 1.0, S, Y, *small)
    a = c.lib.last("pyipm_lbfgs_direction")
    assert (a[5], val(a[6]), a[7], val(a[8]), a[9]) == (m, S.data_ptr(), m + 1, Y.data_ptr(), 128)
    St = torch.randn((m, n), dtype=F64).t()
    c.direction(z(c.N, dtype=F64), z(mi, dtype=F64), z(me + mi, dtype=F64), 1.0, St, Y, *small)
    a = c.lib.last("pyipm_lbfgs_direction")
    assert a[7] == m and val(a[6]) != St.data_ptr() and (val(a[8]), a[9]) == (Y.data_ptr(), 128)
    # no pairs: null, 1 (as before)
    c.direction(z(c.N, dtype=F64), z(mi, dtype=F64), z(me + mi, dtype=F64), 1.0, None, None, None, None, None)
    a = c.lib.last("pyipm_lbfgs_direction")
    assert (a[5], val(a[6]), a[7], val(a[8]), a[9]) == (0, None, 1, None, 1)
