"""ctypes binding of ``include/pyipm_lbfgs.h`` — the L-BFGS search direction on the device.

Counterpart of the reference's compiled ``lbfgs_dir_func`` (``/root/reference/pyipm.py:872-875``, built by
``lbfgs_builder`` ``:1007-1182``, called from ``lbfgs_dir`` ``:1184-1246``).  Same shared object and the
same conventions as ``pyipm_amd.newton``; PyTorch owns tensors and the stream, every kernel is HIP.
No CPU fallback: without the library or a GPU the constructor raises.

``PairStore`` is the storage that feeds it: ``lbfgs_init`` / ``lbfgs_update`` (pyipm.py:993-1005, 1282-1371) behind the
``pyipm_pairs_*`` entry points, which ``include/pyipm_newton.h`` declares and ``pyipm_amd.newton`` binds, as they do the
later additions to the direction's own handle (``pyipm_qn_*``, ``pyipm_lbfgs_stage_jacobian_columns``,
``pyipm_lbfgs_bounded_*``).
"""
from __future__ import annotations

import ctypes
from ctypes import POINTER, c_char_p, c_double, c_int, c_int64, c_size_t, c_void_p

import numpy as np

from ._device import RawDeviceArray, ptr, rows_to_device, to_device
from .newton import ERRORS, MEM_DEVICE, MEM_HOST, NewtonError, load_library


class LbfgsStats(ctypes.Structure):
    """Mirror of ``pyipm_lbfgs_stats``."""
    _fields_ = [("m", c_int64), ("n_neg", c_int64), ("n_zero", c_int64), ("regularised", c_int64),
                ("n_factor", c_int64), ("d_min", c_double), ("d_max", c_double), ("small_pivot_min", c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


_SIG = {
    "pyipm_lbfgs_create": (c_int, [POINTER(c_void_p), c_int64, c_int64, c_int64, c_int, c_int, c_int, c_void_p]),
    "pyipm_lbfgs_destroy": (c_int, [c_void_p]),
    "pyipm_lbfgs_last_error": (c_char_p, [c_void_p]),
    "pyipm_lbfgs_set_stream": (c_int, [c_void_p, c_void_p]),
    "pyipm_lbfgs_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int64, c_int, c_int]),
    "pyipm_lbfgs_stage_jacobian": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int]),
    "pyipm_lbfgs_direction": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_double, c_int, c_void_p, c_int64,
                                      c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_double, c_double,
                                      c_void_p, c_int, c_int, POINTER(LbfgsStats)]),
    "pyipm_lbfgs_last_timings": (c_int, [c_void_p, POINTER(c_double)]),
    "pyipm_lbfgs_set_option": (c_int, [c_void_p, c_char_p, c_double]),
    "pyipm_lbfgs_set_allreduce": (c_int, [c_void_p, c_void_p, c_void_p]),
}
ALLREDUCE_FN = ctypes.CFUNCTYPE(c_int, c_void_p, c_void_p, c_int64, c_void_p)


_bound = None


def load():
    global _bound
    if _bound is None:
        lib = load_library()
        for name, (res, args) in _SIG.items():
            fn = getattr(lib, name)              # AttributeError here = header / library mismatch
            fn.restype = res
            fn.argtypes = args
        _bound = lib
    return _bound


def exported_symbols():
    """Names every entry point ``include/pyipm_lbfgs.h`` declares (used by the CPU tests)."""
    load()
    return tuple(_SIG)


class LbfgsCore(object):
    """One handle = one problem shape (n, me, mi) and a bound on the stored pairs.

    ::

        core.stage_jacobian(Je, Ji)                               # dce(x), dci(x); once if the constraints are linear
        dz, st = core.direction(g, s, lda, zeta, S, Y, SS, L, D, reg=reg)     # RAW direction (flip=False), :1713

    ``bounds=(var, sign)``: a bounded handle (``pyipm_lbfgs_bounded_*``).  ``mi`` then counts the general inequalities, the
    columns of Ji, alone; bound j is ``sign[j] * x[var[j]] + const >= 0`` (+1 lower, -1 upper) and is never a column.  Every
    vector of ``direction`` counts ``mi + len(var)`` inequalities, the bounds last.  The operator entries (``matvec``,
    ``solve``, ``refine``, ``*_many``) and ``shard=True`` raise the library's refusal.
    """

    mb = 0                                       # simple bounds behind the mi general inequalities (a bounded handle)

    def __init__(self, n, me, mi, max_pairs, device=None, nb=256, group=None, shard=False, bounds=None):
        """shard=True (or a process group): this handle holds ``n`` ROWS of a row-sharded problem; the three sums over
        the ranks (J'J, J'[g_x|W], W'[g_x|W]) go through ``torch.distributed.all_reduce`` on ``group`` — backend "nccl"
        (= RCCL) in place on the device buffers, "gloo" staged through the host (tests)."""
        import torch
        self.torch = torch
        self.lib = load()
        if not torch.cuda.is_available():
            raise NewtonError("no HIP device visible: the L-BFGS direction has no CPU fallback")
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else int(device))
        self.n, self.me, self.mi, self.cap = int(n), int(me), int(mi), int(max_pairs)
        self.bounded = bounds is not None
        self.mb = int(np.asarray(bounds[0]).shape[0]) if self.bounded else 0
        self.mi_all = self.mi + self.mb                      # inequalities in the vectors of a direction
        self.N = self.n + 2 * self.mi_all + self.me
        if self.lib.pyipm_lbfgs_bounded_workspace_bytes(self.n, self.me, self.mi, self.mb, self.cap, int(nb)) == 0:
            raise NewtonError("invalid L-BFGS geometry n=%d me=%d mi=%d max_pairs=%d nb=%d" % (n, me, mi, max_pairs, nb))
        h = c_void_p()
        with torch.cuda.device(self.device):
            stream = c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            if self.bounded:
                rc = self.lib.pyipm_lbfgs_bounded_create(ctypes.byref(h), self.n, self.me, self.mi, self.mb, self.cap,
                                                         int(nb), self.device.index, stream)
            else:
                rc = self.lib.pyipm_lbfgs_create(ctypes.byref(h), self.n, self.me, self.mi, self.cap, int(nb),
                                                 self.device.index, stream)
        if rc:
            raise NewtonError("pyipm_lbfgs_create failed: %s" % ERRORS.get(rc, rc))
        self.h = h
        self.group, self.bytes_reduced, self._cb = group, 0, None
        try:
            if self.bounded:
                self.stage_bounds(*bounds)
            if shard or group is not None:
                self._install_allreduce()
        except Exception:
            self.close()                                     # (a refusal here must not leave the handle to the finaliser)
            raise

    def _install_allreduce(self):
        import torch.distributed as dist
        torch = self.torch
        if not dist.is_initialized():
            raise NewtonError("row-sharded L-BFGS needs an initialised torch.distributed process group")
        staged = dist.get_backend(self.group) == "gloo"

        def cb(user, ptr, count, stream):
            try:
                t = torch.as_tensor(RawDeviceArray(ptr, count), device=self.device)
                if staged:
                    hbuf = t.cpu()                                   # synchronises the stream
                    dist.all_reduce(hbuf, op=dist.ReduceOp.SUM, group=self.group)
                    t.copy_(hbuf)
                else:
                    dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.group)     # ordered on the current stream
                self.bytes_reduced += 8 * int(count)
                return 0
            except Exception as e:                                   # nothing may propagate through the C frames
                self._cb_error = e
                return 1

        self._cb = ALLREDUCE_FN(cb)                                  # keep alive as long as the handle
        self._ck(self.lib.pyipm_lbfgs_set_allreduce(self.h, ctypes.cast(self._cb, c_void_p), None))

    def _ck(self, rc):
        if rc:
            msg = self.lib.pyipm_lbfgs_last_error(self.h)
            err = NewtonError("%s: %s" % (ERRORS.get(rc, rc), msg.decode() if msg else ""))
            cause = getattr(self, "_cb_error", None)          # what the all-reduce callback swallowed, if that was it
            self._cb_error = None
            if cause is not None:
                raise err from cause
            raise err

    def _dev(self, a, shape):
        return to_device(a, self.device, shape)

    def _rows(self, a, shape):
        """A 2-D operand and its leading dimension: a row-strided device view as it is (``_device.rows_to_device``)."""
        if a is None:
            return None, max(shape[1], 1)
        t, (ld,) = rows_to_device(a, self.device, shape)
        return t, ld

    _ptr = staticmethod(ptr)

    def set_option(self, name, value):
        self._ck(self.lib.pyipm_lbfgs_set_option(self.h, name.encode(), float(value)))

    def close(self):
        if getattr(self, "h", None):
            self.lib.pyipm_lbfgs_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def stage_jacobian(self, Je=None, Ji=None):
        """Je (n, me), Ji (n, mi): NumPy arrays or device tensors (copied into the padded operand buffer)."""
        n, me, mi = self.n, self.me, self.mi
        if me + mi == 0:
            return
        Je, lde = self._rows(Je if me else None, (n, me))
        Ji, ldi = self._rows(Ji if mi else None, (n, mi))
        self._ck(self.lib.pyipm_lbfgs_stage_jacobian(self.h, self._ptr(Je), lde, self._ptr(Ji), ldi, MEM_DEVICE))
        self.torch.cuda.current_stream(self.device).synchronize()      # Je / Ji temporaries may die now

    def stage_bounds(self, var, sign):
        """The simple bounds of a bounded handle: ``var`` (integers in 0 .. n-1) and ``sign`` (+1 lower, -1 upper), as many
        entries each as the handle was made for.  Host arrays; the library keeps a grouping by variable.  Again to change them."""
        var = np.ascontiguousarray(np.asarray(var), dtype=np.int64).reshape(-1)
        sign = np.ascontiguousarray(np.asarray(sign), dtype=np.float64).reshape(-1)
        if not self.bounded or var.shape[0] != self.mb or sign.shape[0] != self.mb:
            raise NewtonError("stage_bounds: the handle was made for %d bounds" % self.mb)
        self._ck(self.lib.pyipm_lbfgs_bounded_stage(self.h, c_void_p(var.ctypes.data), c_void_p(sign.ctypes.data)))

    def stage_jacobian_columns(self, c0, Jc):
        """Jc (n, count), a NumPy array or a device tensor, replaces columns c0 .. c0 + count - 1 of [Je | Ji] (global column
        indices); the next direction recomputes only the 128 x 128 tiles of J'J those columns reach.  After a full
        ``stage_jacobian`` only."""
        count = int(Jc.shape[1])
        Jd, ld = self._rows(Jc if count else None, (self.n, count))
        self._ck(self.lib.pyipm_lbfgs_stage_jacobian_columns(self.h, int(c0), count, self._ptr(Jd), ld, MEM_DEVICE))
        self.torch.cuda.current_stream(self.device).synchronize()      # a temporary of Jc may die now

    def direction(self, g, s, lda, zeta, S, Y, SS, L, D, reg=0.0, eps=float(np.finfo(np.float64).eps), flip=False,
                  refine=0):
        """Returns (dz device tensor of length n + 2 mi + me, with the bounds of a bounded handle counted in mi; stats dict).  ``refine`` != 0 (constrained problems): the
        direction is then refined against the quasi-Newton KKT operator (``refine``); ``refine_info()`` has the outcome."""
        dz, st = self._direction(g, s, lda, zeta, S, Y, SS, L, D, reg, eps, flip)
        if refine and (self.me or self.mi or self.mb):
            dz, _ = self.refine(dz, refine=refine, flip=flip)
        return dz, st

    # ---- the quasi-Newton KKT operator K of the last direction (include/pyipm_newton.h, pyipm_qn_*): K dz = g
    def _stream(self):
        torch = self.torch
        self._ck(self.lib.pyipm_lbfgs_set_stream(self.h, c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))

    def matvec(self, v, flip=False):
        """K v (device tensor of N); ``flip``: v has its multiplier rows negated."""
        v = self._dev(v, (self.N,))
        out = self.torch.empty(self.N, dtype=self.torch.float64, device=self.device)
        self._stream()
        self._ck(self.lib.pyipm_qn_matvec(self.h, self._ptr(v), 1 if flip else 0, MEM_DEVICE, self._ptr(out)))
        return out

    def solve(self, rhs, flip=False):
        """dz with K dz = rhs from the state the last direction kept (no Gram launch, no factorisation)."""
        rhs = self._dev(rhs, (self.N,))
        dz = self.torch.empty(self.N, dtype=self.torch.float64, device=self.device)
        self._stream()
        self._ck(self.lib.pyipm_qn_solve(self.h, self._ptr(rhs), self._ptr(dz), 1 if flip else 0, MEM_DEVICE))
        return dz

    def refine(self, dz, rhs=None, refine=-1, flip=False):
        """Refines ``dz`` as a solution of K dz = rhs (None: the g of the last direction).  refine > 0: that many steps;
        < 0: adaptive (options ``refine_target`` / ``refine_max``); 0: measures the backward error only.
        Returns (a new device tensor, info dict)."""
        dz = self._dev(dz, (self.N,)).clone()
        rhs = None if rhs is None else self._dev(rhs, (self.N,))
        self._stream()
        self._ck(self.lib.pyipm_qn_refine(self.h, self._ptr(rhs), self._ptr(dz), 1 if flip else 0, int(refine), MEM_DEVICE))
        return dz, self.refine_info()

    def refine_info(self):
        out = (c_double * 4)()
        self._ck(self.lib.pyipm_qn_info(self.h, out))
        return {"steps": int(out[0]), "berr0": out[1], "berr": out[2], "converged": bool(out[3])}

    def _columns(self, name, A):
        """An (N, k) NumPy array or tensor as a contiguous (k, N) device buffer: column j at base + j * N."""
        A = to_device(A, self.device, contiguous=False)
        if A.dim() != 2 or A.shape[0] != self.N:
            raise ValueError("%s: the block must have shape (N, k) with N = %d, got %s" % (name, self.N, tuple(A.shape)))
        return A.t().contiguous()

    def matvec_many(self, V, flip=False):
        """K V for V of shape (N, k) in two passes over J per 64 columns (pyipm_lbfgs_kkt_matvec_many).  Returns an (N, k)
        device tensor, the transposed view of a contiguous (k, N) buffer; column j is bitwise independent of the others."""
        vin = self._columns("matvec_many", V)
        k = int(vin.shape[0])
        out = self.torch.empty((k, self.N), dtype=self.torch.float64, device=self.device)
        self._stream()
        self._ck(self.lib.pyipm_lbfgs_kkt_matvec_many(self.h, k, self._ptr(vin), self.N, self._ptr(out), self.N,
                                                      1 if flip else 0, MEM_DEVICE))
        self._keep_many = vin                            # (the library reads it on the stream, after this returns)
        return out.t()

    def solve_many(self, B, flip=False, refine=0):
        """K dz_j = B[:, j] for B of shape (N, k) from the state the last direction kept (pyipm_lbfgs_kkt_solve_many);
        ``refine`` as in ``NewtonCore.solve_many`` -- after ``refine != 0``, ``refine_info()`` reports the worst column.
        Returns an (N, k) device tensor, the transposed view of a contiguous (k, N) buffer."""
        rhs = self._columns("solve_many", B)
        k = int(rhs.shape[0])
        dz = self.torch.empty((k, self.N), dtype=self.torch.float64, device=self.device)
        self._stream()
        self._ck(self.lib.pyipm_lbfgs_kkt_solve_many(self.h, k, self._ptr(rhs), self.N, self._ptr(dz), self.N,
                                                     1 if flip else 0, int(refine), MEM_DEVICE))
        self._keep_many = rhs
        return dz.t()

    def _direction(self, g, s, lda, zeta, S, Y, SS, L, D, reg, eps, flip):
        torch = self.torch
        n, me, mi, N = self.n, self.me, self.mi, self.N
        m = 0 if S is None else int(S.shape[1])
        g = self._dev(g, (N,))
        mi += self.mb                                        # the bounds of a bounded handle count in s and lda
        s = self._dev(s, (mi,)) if mi else None
        lda = self._dev(lda, (me + mi,)) if (me + mi) else None
        Sd, lds = self._rows(S if m else None, (n, m))
        Yd, ldy = self._rows(Y if m else None, (n, m))
        small = [np.ascontiguousarray(np.asarray(a, dtype=np.float64)).reshape(m, m) if m else None for a in (SS, L, D)]
        dz = torch.empty(N, dtype=torch.float64, device=self.device)
        st = LbfgsStats()
        hp = lambda a: c_void_p(0) if a is None else a.ctypes.data_as(c_void_p)     # noqa: E731
        self._ck(self.lib.pyipm_lbfgs_set_stream(self.h, c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))
        self._ck(self.lib.pyipm_lbfgs_direction(self.h, self._ptr(g), self._ptr(s), self._ptr(lda), float(zeta), m,
                                                self._ptr(Sd), lds, self._ptr(Yd), ldy, hp(small[0]),
                                                hp(small[1]), hp(small[2]), float(reg), float(eps), self._ptr(dz),
                                                1 if flip else 0, MEM_DEVICE, ctypes.byref(st)))
        return dz, st.as_dict()

    def last_timings(self):
        out = (c_double * 8)()
        self._ck(self.lib.pyipm_lbfgs_last_timings(self.h, out))
        keys = ("total_ms", "gram_ms", "factor_ms", "solves_ms", "jacobian_passes_ms", "small_ms", "gram_flops",
                "gram_launches")
        return {k: out[i] for i, k in enumerate(keys)}


class PairsView(ctypes.Structure):
    """Mirror of ``pyipm_pairs_view`` (``include/pyipm_newton.h``)."""
    _fields_ = [("m", c_int64), ("ld", c_int64), ("S", c_void_p), ("Y", c_void_p), ("SS", POINTER(c_double)),
                ("L", POINTER(c_double)), ("D", POINTER(c_double)), ("zeta", c_double), ("fail", c_int64)]


ACCEPTED, SKIPPED, RESET = 1, 0, 2          # outcomes of an offer


class PairStore(object):
    """The L-BFGS storage where the pairs live: ``lbfgs_init`` / ``lbfgs_update`` of the reference (pyipm.py:993-1005,
    1282-1371) behind ``pyipm_pairs_*`` of ``include/pyipm_newton.h``.  S and Y stay on the device, SS / L / D, zeta and
    the skip counter on the host inside the library.  No CPU fallback.

    ::

        store = PairStore(n, memory, constrained)
        outcome = store.offer(x_old, x_new, g_old, g_new, eps)          # 1 accepted, 0 skipped, 2 reset
        zeta, S, Y, SS, L, D, fail = store.view()                       # straight into LbfgsCore.direction
    """

    def __init__(self, n, memory, constrained, zeta0=1.0, device=None):
        import torch
        self.torch = torch
        self.lib = load_library()
        if not torch.cuda.is_available():
            raise NewtonError("no HIP device visible: the L-BFGS pair store has no CPU fallback")
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else int(device))
        self.n, self.memory, self.constrained = int(n), int(memory), bool(constrained)
        if self.lib.pyipm_pairs_workspace_bytes(self.n, self.memory) == 0:
            raise NewtonError("invalid pair-store geometry n=%d memory=%d (1 <= memory <= 31)" % (n, memory))
        h = c_void_p()
        with torch.cuda.device(self.device):
            rc = self.lib.pyipm_pairs_create(ctypes.byref(h), self.n, self.memory, int(self.constrained), float(zeta0),
                                             self.device.index, c_void_p(torch.cuda.current_stream(self.device).cuda_stream))
        if rc:
            raise NewtonError("pyipm_pairs_create failed: %s" % ERRORS.get(rc, rc))
        self.h = h
        self.n_offers = 0

    def _ck(self, rc):
        if rc:
            msg = self.lib.pyipm_pairs_last_error(self.h)
            err = NewtonError("%s: %s" % (ERRORS.get(rc, rc), msg.decode() if msg else ""))
            err.code = rc
            raise err

    def close(self):
        if getattr(self, "h", None):
            self.lib.pyipm_pairs_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        """lbfgs_init: the empty storage with zeta0."""
        self._ck(self.lib.pyipm_pairs_reset(self.h))

    def offer(self, x_old, x_new, g_old, g_new, eps=float(np.finfo(np.float64).eps)):
        """lbfgs_update.  Four NumPy arrays (staged by the library) or four device tensors (read where they are);
        ``g_old`` / ``g_new`` may be longer than n.  Returns ACCEPTED, SKIPPED or RESET."""
        torch, n = self.torch, self.n
        args = (x_old, x_new, g_old, g_new)
        if all(isinstance(a, torch.Tensor) for a in args):
            keep = [to_device(a.reshape(-1), self.device) for a in args]         # (no copy for a contiguous fp64 device tensor)
            ptrs, kind = [ptr(t) for t in keep], MEM_DEVICE
        else:
            keep = [np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float64),
                                         dtype=np.float64).reshape(-1) for a in args]
            ptrs, kind = [c_void_p(a.ctypes.data) for a in keep], MEM_HOST
        if any(a.shape[0] < n for a in keep):
            raise NewtonError("offer: x and g need at least n = %d entries" % n)
        out = c_int(0)
        self._ck(self.lib.pyipm_pairs_set_stream(self.h, c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))
        self._ck(self.lib.pyipm_pairs_offer(self.h, ptrs[0], ptrs[1], ptrs[2], ptrs[3], float(eps), kind, ctypes.byref(out)))
        self.n_offers += 1
        return out.value

    def view(self):
        """(zeta, S, Y, SS, L, D, fail): S and Y are (n, m) device tensors that ALIAS the store's memory, rows ``ld`` doubles
        apart -- valid until the next offer or reset; SS, L, D are NumPy copies."""
        torch, n = self.torch, self.n
        v = PairsView()
        self._ck(self.lib.pyipm_pairs_view_get(self.h, ctypes.byref(v)))
        m, ld = int(v.m), int(v.ld)
        if m:
            span = (n - 1) * ld + m
            S, Y = (torch.as_tensor(RawDeviceArray(p, span), device=self.device).as_strided((n, m), (ld, 1)) for p in (v.S, v.Y))
            SS, L, D = (np.ctypeslib.as_array(p, shape=(m, m)).copy() for p in (v.SS, v.L, v.D))
        else:
            S, Y = (torch.zeros((n, 0), dtype=torch.float64, device=self.device) for _ in range(2))
            SS, L, D = (np.zeros((0, 0)) for _ in range(3))
        return float(v.zeta), S, Y, SS, L, D, int(v.fail)


__all__ = ["LbfgsCore", "LbfgsStats", "PairStore", "PairsView", "MEM_DEVICE", "MEM_HOST", "exported_symbols"]
