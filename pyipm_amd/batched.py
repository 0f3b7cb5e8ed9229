"""Batched independent Newton steps (BASELINE.json configs[4]: 512 independent n=256 QPs, multi-start).

Independent problems shard with no exchange at all ("replicas only"), and a system
this small (Npad <= 1024) fits one workgroup: the library's batched handle
(``pyipm_newton_create_batched`` / ``stage_blocks_batched`` / ``step_batched``, ``csrc/kernels_batched.hpp``)
runs the whole batch with four launches -- residuals, assembly, ONE factorisation launch with a workgroup per
problem (2 resident per CU: 512 problems in flight on an MI355X), substitutions.  Across GPUs the batch is
simply split by rank.  Same algorithm and tile-inversion code as the single-system path; no CPU fallback."""
from __future__ import annotations

import ctypes
from ctypes import c_void_p

import numpy as np

from . import reghess
from ._device import alloc_workspace, ptr, rows_to_device, to_device
from .newton import ERRORS, MEM_DEVICE, FactorStats, NewtonError, load_library


class LazyStats(object):
    """The per-problem factor statistics of one ``step_all`` -- a list of dicts, read from the device at first use (``len``,
    indexing, iteration).  Valid until the handle's next step."""

    def __init__(self, owner, step_id):
        self._owner, self._step_id, self._data = owner, step_id, None

    def _fetch(self):
        if self._data is None:
            self._data = self._owner._fetch_stats(self._step_id)
        return self._data

    def __len__(self):
        return len(self._fetch())

    def __getitem__(self, i):
        return self._fetch()[i]

    def __iter__(self):
        return iter(self._fetch())

    def __eq__(self, other):
        return list(self._fetch()) == list(other)

    def __repr__(self):
        return repr(self._fetch())


class BatchedNewton(object):
    condensed_tol = 1e-9                   # backward-error bar (against the FULL blocks) a condensed direction must meet

    def __init__(self, n, me, mi, batch=None, device=None, workers=None, nb=None, refine=0, condensed=False, guard=True):
        """``workers`` / ``nb`` are accepted and ignored (an earlier version drove one handle per host thread).
        ``condensed``: factor the condensed system of every problem (n + me + |active rows| columns instead of n + 2 mi + me:
        the (s, lambda_i) pairs eliminated analytically, SURVEY 8f rank 2 for the batched handle) -- same directions, inertia
        of the full matrix.  With ``guard`` every condensed step is checked on the device (inertia, static pivots, backward
        error against the full blocks: ``pyipm_newton_backward_error_batched``) and the batch is redone with the full form
        when a problem misses ``condensed_tol`` (counted in ``n_condensed_fallback``)."""
        import torch
        if refine:
            raise NotImplementedError("iterative refinement is not part of the batched path")
        self.condensed, self.guard = bool(condensed and mi), bool(guard)
        self.n_condensed_fallback, self.last_backward_errors = 0, None
        if self.condensed:
            self._opts = {"condensed": 1.0}
        self.torch = torch
        self.lib = load_library()
        if not torch.cuda.is_available():
            raise NewtonError("no HIP device visible: the Newton-step core has no CPU fallback")
        self.n, self.me, self.mi = int(n), int(me), int(mi)
        self.N = self.n + 2 * self.mi + self.me
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else int(device))
        self.h, self.batch, self.workspace = None, 0, None
        self._keep = None
        if batch:
            self._create(int(batch))

    def _create(self, batch):
        torch = self.torch
        self.close()
        need = self.lib.pyipm_newton_workspace_bytes_batched(self.n, self.me, self.mi, batch)
        if need == 0:
            raise NewtonError("batched handles need n + 2 mi + me <= 1024 (got %d)" % self.N)
        with torch.cuda.device(self.device):
            self.workspace = alloc_workspace(need, self.device)
            h = c_void_p()
            rc = self.lib.pyipm_newton_create_batched(ctypes.byref(h), self.n, self.me, self.mi, batch, self.device.index,
                                                      c_void_p(self.workspace.data_ptr()), need,
                                                      c_void_p(torch.cuda.current_stream(self.device).cuda_stream))
        if rc:
            raise NewtonError("pyipm_newton_create_batched failed: %s" % ERRORS.get(rc, rc))
        self.h, self.batch = h, batch
        self._step_id = getattr(self, "_step_id", 0) + 1    # (statistics of a step on the old handle are gone)
        for k, v in getattr(self, "_opts", {}).items():
            self._ck(self.lib.pyipm_newton_set_option(self.h, k.encode(), v))

    def set_option(self, name, value):
        """Same options as ``NewtonCore.set_option`` where they apply (e.g. ``tile_blocked``); kept for the handle that the
        first ``step_all`` creates (its size is the batch's)."""
        if not hasattr(self, "_opts"):
            self._opts = {}
        self._opts[name] = float(value)
        if getattr(self, "h", None):
            self._ck(self.lib.pyipm_newton_set_option(self.h, name.encode(), float(value)))

    def _ck(self, rc):
        if rc:
            msg = self.lib.pyipm_newton_last_error(self.h)
            raise NewtonError("%s: %s" % (ERRORS.get(rc, rc), msg.decode() if msg else ""))

    def step_all(self, d2L, Je=None, Ji=None, df=None, ce=None, ci=None, s=None, lda=None, mu=0.2,
                 delta=0.0, delta_c=0.0, eps=float(np.finfo(np.float64).eps)):
        """All arguments carry a leading batch dimension (torch device tensors or NumPy arrays):
        d2L (B,n,n), Je (B,n,me), Ji (B,n,mi), df (B,n), ce (B,me), ci (B,mi), s (B,mi), lda (B,me+mi).
        Returns (dz (B,N) device tensor, list of per-problem factor statistics)."""
        torch = self.torch
        me, mi = self.me, self.mi
        B = self.stage(d2L, Je, Ji, df, ce, ci, s, lda, mu=mu, eps=eps)
        out = self._last_out = torch.empty((B, self.N), dtype=torch.float64, device=self.device)
        # the step is five launches and returns once they are enqueued; the B statistics records stay on the device until somebody
        # looks at them (LazyStats: round 6 -- copying and unpacking 512 records per step was a third of the step's wall time)
        self._ck(self.lib.pyipm_newton_step_batched(self.h, float(delta), float(delta_c), ptr(out), None, MEM_DEVICE))
        self._step_id += 1
        stats = LazyStats(self, self._step_id)
        if self._opts_get("condensed") and self.guard and mi:
            # the condensed form's guard (as HipNewtonBackend's for a single system): right inertia, no static pivot, and a
            # direction that satisfies the FULL blocks; otherwise the batch is redone with the full 4-block system
            be = self.backward_errors(out)
            self.last_backward_errors = be
            bad = (be > self.condensed_tol) | ~torch.isfinite(be)
            ok = not bool(bad.any()) and all(x["n_neg"] == me + mi and x["n_zero"] == 0 and not x["nonfinite"] for x in stats)
            if not ok:
                self.n_condensed_fallback += 1
                self._ck(self.lib.pyipm_newton_set_option(self.h, b"condensed", 0.0))
                try:
                    self._ck(self.lib.pyipm_newton_step_batched(self.h, float(delta), float(delta_c), ptr(out), None, MEM_DEVICE))
                    self._step_id += 1
                    stats = LazyStats(self, self._step_id)
                    stats._fetch()                      # (read while the handle is in the full form)
                finally:
                    self._ck(self.lib.pyipm_newton_set_option(self.h, b"condensed", 1.0))
        return out, stats

    def stage(self, d2L, Je=None, Ji=None, df=None, ce=None, ci=None, s=None, lda=None, mu=0.2,
              eps=float(np.finfo(np.float64).eps)):
        """Stage the blocks and vectors of a batch (arguments as ``step_all``'s; the handle is created for the batch's size
        when there is none of that size).  ``mu`` is the one ``step_all`` steps with; ``step_each`` brings its own.
        Returns the batch size."""
        torch = self.torch
        n, me, mi = self.n, self.me, self.mi

        def dev(a, shape):
            return to_device(a, self.device, shape)

        B = int(d2L.shape[0])
        if self.h is None or B != self.batch:
            self._create(B)

        def rows(a, width):                    # a row- and batch-strided device view as it is: (tensor, batch stride, ld)
            if not width:
                return None, 0, 0
            t, (sb, ld) = rows_to_device(a, self.device, (B, n, width))
            return t, sb, ld

        (H, sH, ldh), (E, sE, lde), (I, sI, ldi) = rows(d2L, n), rows(Je, me), rows(Ji, mi)
        blocks = (H, E, I)
        vecs = (dev(df, (B, n)), dev(ce, (B, me)) if me else None, dev(ci, (B, mi)) if mi else None,
                dev(s, (B, mi)) if mi else None, dev(lda, (B, me + mi)) if (me + mi) else None)
        self._keep = (blocks, vecs)            # the library retains the block pointers

        self._ck(self.lib.pyipm_newton_set_stream(self.h, c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))
        self._ck(self.lib.pyipm_newton_stage_blocks_batched(self.h, ptr(H), ldh, sH, ptr(E), lde, sE, ptr(I), ldi, sI))
        self._ck(self.lib.pyipm_newton_stage_vectors(self.h, ptr(vecs[0]), ptr(vecs[1]), ptr(vecs[2]), ptr(vecs[3]),
                                                     ptr(vecs[4]), float(mu), float(eps), MEM_DEVICE))
        self._eps = float(eps)
        self._last_out = None                  # (directions of other vectors)
        return B

    def _per_problem(self, x, dtype):
        """A scalar or (B,) array / tensor as a contiguous device tensor of B entries."""
        torch = self.torch
        if isinstance(x, torch.Tensor):
            return x.to(device=self.device, dtype=dtype).expand(self.batch).contiguous()
        a = np.broadcast_to(np.asarray(x, dtype=np.float64 if dtype == torch.float64 else np.int32), (self.batch,)).copy()
        return torch.from_numpy(a).to(self.device)

    def step_each(self, mu, delta, delta_c, active=None, out=None):
        """One step on the blocks / vectors staged last (``stage`` or ``step_all``) with each problem's own ``mu``, ``delta``,
        ``delta_c`` (scalars or (B,)), for the problems ``active`` selects ((B,) flags; None = all): the thin call over
        ``pyipm_newton_step_batched_each``.  A problem that sits out keeps its row of ``out``, its statistics record and its
        parameters in the handle.  ``out``: the (B, N) device tensor to write into -- e.g. the one an earlier step returned;
        None = a new one, whose rows of inactive problems are NaN.  Returns (dz, LazyStats); no guard, no fallback here."""
        torch = self.torch
        if self.h is None:
            raise NewtonError("step_each: stage a batch first (stage / step_all)")
        f64 = torch.float64
        pm, pd, pc = (self._per_problem(x, f64) for x in (mu, delta, delta_c))
        pa = None if active is None else self._per_problem(active, torch.int32)
        if out is None:
            out = torch.empty((self.batch, self.N), dtype=f64, device=self.device)
            if pa is not None:
                out.fill_(float("nan"))
        elif tuple(out.shape) != (self.batch, self.N) or out.dtype != f64 or not out.is_contiguous() or out.device != self.device:
            raise NewtonError("step_each: out must be a contiguous float64 (B, N) tensor on the handle's device")
        self._ck(self.lib.pyipm_newton_set_stream(self.h, c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))
        self._ck(self.lib.pyipm_newton_step_batched_each(self.h, ptr(pm), ptr(pd), ptr(pc), ptr(pa), ptr(out), MEM_DEVICE))
        self._step_id += 1
        self._last_out = out
        return out, LazyStats(self, self._step_id)

    def step_lengths_all(self, tau, dz=None):
        """Fraction-to-the-boundary step lengths of every problem (pyipm.py:1408-1436) for the staged s, lda and the directions
        ``dz`` ((B, N) device tensor; None = what the last step returned): device tensor (B, 2) of (alpha_s, alpha_l)."""
        torch = self.torch
        if dz is None:
            dz = self._last_out
            if dz is None:
                raise NewtonError("step_lengths_all: no direction (step first, or pass dz)")
        dz = to_device(dz, self.device, (self.batch, self.N))
        al = torch.empty((self.batch, 2), dtype=torch.float64, device=self.device)
        self._ck(self.lib.pyipm_newton_set_stream(self.h, c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))
        self._ck(self.lib.pyipm_newton_step_lengths_batched(self.h, float(tau), ptr(dz), ptr(al), MEM_DEVICE))
        return al

    # -- the provider's products and the merit pieces of every problem (pyipm_newton_*_batched; device tensors in and out) -----
    def _staged_handle(self, who):
        if self.h is None:
            raise NewtonError("%s: stage a batch first (stage / step_all)" % who)
        self._ck(self.lib.pyipm_newton_set_stream(self.h, c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)))

    def _direction(self, dz, who):
        if dz is None:
            dz = self._last_out
            if dz is None:
                raise NewtonError("%s: no direction (step first, or pass dz)" % who)
        return to_device(dz, self.device, (self.batch, self.N))

    def products_all(self, v, want=(True, True, True)):
        """(Q_b v_b, Je_b' v_b, Ji_b' v_b) of every problem for v (B, n), from the staged blocks in one launch
        (``pyipm_newton_block_products_batched``): device tensors (B, n), (B, me), (B, mi); entries not wanted (or of an empty
        block) are None."""
        self._staged_handle("products_all")
        t, B = self.torch, self.batch
        v = to_device(v, self.device, (B, self.n))
        mk = lambda k, on: t.empty((B, k), dtype=t.float64, device=self.device) if (on and k) else None    # noqa: E731
        q, e, i = mk(self.n, want[0]), mk(self.me, want[1]), mk(self.mi, want[2])
        self._ck(self.lib.pyipm_newton_block_products_batched(self.h, ptr(v), ptr(q), ptr(e), ptr(i)))
        return q, e, i

    def products_t_all(self, le=None, li=None):
        """Je_b le_b + Ji_b li_b (B, n) of every problem (``pyipm_newton_block_products_t_batched``); le (B, me) / li (B, mi),
        either may be None."""
        self._staged_handle("products_t_all")
        t, B = self.torch, self.batch
        le = to_device(le, self.device, (B, self.me)) if (le is not None and self.me) else None
        li = to_device(li, self.device, (B, self.mi)) if (li is not None and self.mi) else None
        out = t.empty((B, self.n), dtype=t.float64, device=self.device)
        self._ck(self.lib.pyipm_newton_block_products_t_batched(self.h, ptr(le), ptr(li), ptr(out)))
        return out

    MERIT_KEYS = ("ce_l1", "cis_l1", "df_dx", "ds_over_s", "sum_log_s", "kkt_x", "kkt_s", "kkt_ce", "kkt_ci", "comp_sum",
                  "comp_min", "dx_norm", "ds_norm")              # columns 0 .. 12 of merit_info_all (NewtonCore.MERIT_KEYS)

    def merit_info_all(self, dz=None, use_last=True):
        """The 16 quantities of ``NewtonCore.merit_info`` for every problem (``pyipm_newton_merit_info_batched``): device tensor
        (B, 16), columns as MERIT_KEYS.  ``dz`` (B, N): the directions; None = what the last step returned, or none at all
        (``use_last=False``, or no step yet): the direction columns are NaN."""
        self._staged_handle("merit_info_all")
        if dz is None and use_last:
            dz = self._last_out
        if dz is not None:
            dz = to_device(dz, self.device, (self.batch, self.N))
        out = self.torch.empty((self.batch, 16), dtype=self.torch.float64, device=self.device)
        self._ck(self.lib.pyipm_newton_merit_info_batched(self.h, ptr(dz), ptr(out), MEM_DEVICE))
        return out

    def merit_ray_all(self, alphas, nu, mu, dz=None, quad=None):
        """phi_b(x + a dx, s + a ds) - phi_b(x, s) for every a in ``alphas[b]`` ((B, K), K <= 1024) with each problem's own
        ``nu``, ``mu`` (scalars or (B,)): device tensor (B, K) (``pyipm_newton_merit_ray_batched``: one launch for every
        candidate of every problem).  ``dz``: None = what the last step returned; ``quad`` (B,): dx'Q dx given by the caller."""
        self._staged_handle("merit_ray_all")
        t, B = self.torch, self.batch
        dz = self._direction(dz, "merit_ray_all")
        alphas = to_device(alphas, self.device)
        if alphas.dim() != 2 or alphas.shape[0] != B:
            raise NewtonError("merit_ray_all: alphas must be (B, K)")
        alphas = alphas.to(t.float64).contiguous()
        K = int(alphas.shape[1])
        pn, pm = self._per_problem(nu, t.float64), self._per_problem(mu, t.float64)
        pq = None if quad is None else self._per_problem(quad, t.float64)
        out = t.empty((B, K), dtype=t.float64, device=self.device)
        self._ck(self.lib.pyipm_newton_merit_ray_batched(self.h, ptr(dz), ptr(pn), ptr(pm), ptr(pq), ptr(alphas), K, ptr(out),
                                                         MEM_DEVICE))
        return out

    # -- the kept factors as a solver (pyipm_newton_solve_batched / kkt_matvec_batched / rcond_batched) ----------------------
    def _columns(self, a, who):
        """(B, N) or (B, k, N) as a contiguous float64 device tensor (B, k, N), and whether it came without the k axis."""
        t = to_device(a, self.device)
        flat = t.dim() == 2
        if flat:
            t = t.unsqueeze(1)
        if t.dim() != 3 or t.shape[0] != self.batch or t.shape[2] != self.N:
            raise NewtonError("%s: expected (B, N) or (B, k, N) with B = %d, N = %d" % (who, self.batch, self.N))
        return t.to(self.torch.float64).contiguous(), flat

    def solve_all(self, rhs, flip=True, refine=0, active=None, out=None):
        """``inv(Hc_b) rhs_b`` for every problem against the factor its last step left -- the matrix with that problem's own
        shifts, full or condensed as that step was.  ``rhs``: (B, N) or (B, k, N); returns a device tensor of the same shape
        (``out``: a contiguous float64 tensor of that shape to write into; it may be ``rhs`` itself: solved in place).  ``flip``: rows n + mi .. negated, as the steps
        return directions.  ``refine``: that many steps ``R = B - Hc X; X += solve(R)`` against the blocks (>= 0).
        ``active`` ((B,) flags; None = all): the rows of the other problems are not written (NaN in a new tensor)."""
        self._staged_handle("solve_all")
        t = self.torch
        r, flat = self._columns(rhs, "solve_all")
        k = int(r.shape[1])
        pa = None if active is None else self._per_problem(active, t.int32)
        if out is None:
            x = t.empty_like(r)
            if pa is not None:
                x.fill_(float("nan"))
        else:
            if tuple(out.shape) != tuple(rhs.shape) or out.dtype != t.float64 or not out.is_contiguous() or out.device != self.device:
                raise NewtonError("solve_all: out must be a contiguous float64 device tensor of rhs' shape")
            x = out.unsqueeze(1) if flat else out
        N = self.N
        self._ck(self.lib.pyipm_newton_solve_batched(self.h, k, ptr(r), N, k * N, ptr(x), N, k * N, ptr(pa), int(bool(flip)),
                                                     int(refine), MEM_DEVICE))
        return out if out is not None else (x.squeeze(1) if flat else x)

    def kkt_matvec_all(self, v):
        """``Hc_b v_b`` for every problem from the staged blocks (never the factor), with each problem's own shifts of its last
        step and Sigma of the staged vectors; raw sign.  ``v``: (B, N) or (B, k, N); a device tensor of the same shape."""
        self._staged_handle("kkt_matvec_all")
        vv, flat = self._columns(v, "kkt_matvec_all")
        k, N = int(vv.shape[1]), self.N
        y = self.torch.empty_like(vv)
        self._ck(self.lib.pyipm_newton_kkt_matvec_batched(self.h, k, ptr(vv), N, k * N, ptr(y), N, k * N, MEM_DEVICE))
        return y.squeeze(1) if flat else y

    RCOND_KEYS = ("w_min", "w_max", "rcond", "static_pivot")     # columns of rcond_all (NewtonCore.rcond's four)

    def rcond_all(self, it_inv=0, it_pow=0, active=None):
        """The condition estimate of every problem (``pyipm_newton_rcond_batched``): device tensor (B, 4), columns as
        RCOND_KEYS -- min|w| from ``it_inv`` inverse iterations with the kept factor, max|w| from ``it_pow`` power iterations
        with the blocks (0 = 3 / 6), their ratio, and the magnitude of a static pivot.  Where a factor holds static pivots
        the min|w| estimate is corrected against the unperturbed blocks, so a singular member reads as singular.  Full form
        only.  ``active``: the rows of the other problems are NaN."""
        self._staged_handle("rcond_all")
        t = self.torch
        pa = None if active is None else self._per_problem(active, t.int32)
        out = t.full((self.batch, 4), float("nan"), dtype=t.float64, device=self.device)
        self._ck(self.lib.pyipm_newton_rcond_batched(self.h, int(it_inv), int(it_pow), ptr(pa), ptr(out), MEM_DEVICE))
        return out

    REFINE_KEYS = ("steps", "backward_error0", "backward_error", "converged")     # columns of refine_all (NewtonCore.solve_info's four)

    def refine_all(self, dz, active=None, flip=True, target=None, max_steps=None):
        """Adaptive refinement of the directions ``dz`` IN PLACE, every problem by itself (``pyipm_newton_refine_batched``):
        ``dz`` (B, ld >= N) float64 on the handle's device, rows of unit stride -- e.g. what the last step returned -- each a
        solution of its problem's kept system (the residual of the last step, the blocks with that problem's own shifts and
        Sigma); ``flip``: rows n + mi .. are negated, as the steps write them.  Per problem: the backward error against the
        blocks is measured before every step, and the problem stops converged at ``target``, after ``max_steps`` steps or
        when a step gained less than 4x; a step that made it worse is taken back (None: the handle's ``refine_target`` /
        ``refine_max``, 1e-14 / 8).  Returns a device tensor (B, 4), columns as REFINE_KEYS; ``active`` ((B,) flags; None =
        all): the rows of the other problems are NaN there and untouched in ``dz``.  Nothing returns to the host on the way."""
        self._staged_handle("refine_all")
        t = self.torch
        if not isinstance(dz, t.Tensor) or dz.dim() != 2 or dz.shape[0] != self.batch or dz.dtype != t.float64 \
                or dz.device != self.device or (dz.shape[1] > 1 and dz.stride(1) != 1):
            raise NewtonError("refine_all: dz must be a float64 (B, ld) tensor on the handle's device with rows of unit stride")
        pa = None if active is None else self._per_problem(active, t.int32)
        info = t.full((self.batch, 4), float("nan"), dtype=t.float64, device=self.device)
        self._ck(self.lib.pyipm_newton_refine_batched(self.h, ptr(dz), int(dz.shape[1]), int(dz.stride(0)), ptr(pa), int(bool(flip)),
                                                      0.0 if target is None else float(target),
                                                      -1 if max_steps is None else int(max_steps), ptr(info), MEM_DEVICE))
        return info

    n_factor = 0                           # passes over the batch (direction_all)
    n_inertia_retries = 0                  # problem x shifted pass whose inertia was still wrong (delta *= 10, pyipm.py:1399-1403)
    # direction_all(refine=True): HipNewtonBackend's counters per problem, and the bars of the rule (reghess.py), which is
    # given this instance's values
    suspect_spread, berr_tol, berr_fallback = reghess.SUSPECT_SPREAD, reghess.BERR_TOL, reghess.BERR_FALLBACK
    n_rcond = 0                            # problems a condition estimate was taken for
    n_refined = 0                          # problems whose direction went through refine_all
    n_static = 0                           # directions recovered from a statically pivoted factor
    n_unconverged = 0                      # refined directions that missed berr_tol and were sent to the shift loop
    n_inexact = 0                          # directions returned on berr_fallback
    _shift_info = None

    def shift_info(self):
        """What the last ``direction_all`` decided, per problem: ``failed`` (entered the shift loop), ``suspect`` (the
        pivot-level ``rcond <= eps`` trigger fired on pass 1), ``delta_c`` (what its retry passes were given), ``delta`` (the
        shift its last pass ran with; 0 where none), ``passes`` (retry passes it took part in).  After
        ``direction_all(refine=True)`` also ``singular`` (the condition estimate, or a refinement that stalled, said so),
        ``refined`` (its direction went through ``refine_all``) and ``backward_error`` (of the direction returned, against
        the blocks; NaN where none was measured)."""
        return self._shift_info

    def direction_all(self, d2L, Je, Ji, df, ce, ci, s, lda, mu, delta=0.0, eta=1e-4, beta=0.4, reg_coef=None, delta0=None,
                      max_shift_tries=60, active=None, refine=False):
        """``reghess`` + solve (pyipm.py:1373-1406, 1717-1725) per problem of the batch: the rule of ``pyipm_amd/reghess.py``,
        which ``HipNewtonBackend.direction`` follows too, with each launch serving all problems that need it.  ``mu`` and
        ``delta`` (the delta each problem persists from its last call) are scalars or (B,).
        Pass 1: no shifts, every problem.  ``refine=False``: a problem fails when it is ``wrong`` or ``suspect`` at the bar eps
        -- the pivot-level trigger for the reference's rcond <= eps; there is no condition estimate and no refinement on this
        path, suspect means singular, and members with static pivots (LPs) are shifted.  Failing problems are stepped again
        ALONE (``reghess.first_shift``, ``reghess.delta_c``, then delta *= 10) until their inertia is right; the others keep
        the bits of pass 1.  With ``condensed`` pass 1 is condensed, a problem that misses the guard fails too, and the retry
        passes run in the full form.
        ``refine=True``: the decisions of ``HipNewtonBackend.direction`` per problem.  ONE ``rcond_all`` over the suspect
        (``suspect_spread``), ``reghess.singular`` on each estimate; ONE ``refine_all`` over those ``at_risk`` and not singular,
        and a problem that misses ``berr_tol`` enters the loop as a singular one.  In the loop a problem whose inertia has come
        right is refined again if it is at risk, and its ``reghess.ShiftLoop`` says whether it is shifted further, settles on
        its best direction (``n_inexact``) or is lost (a ``RuntimeError`` names the problems).  With ``condensed``, problems that
        fail pass 1, are suspect, at risk or miss the guard are first re-stepped in the full form WITHOUT shifts and judged
        there (the condition estimate is the full form's).
        ``active`` ((B,) flags; None = all): only these problems take part -- the others sit every pass out (their rows of dz
        are NaN, their statistics those of their last step, their delta unchanged).
        Returns (dz, delta (B,) float64, list of statistics): delta as the reference persists it, unchanged without a shift."""
        torch = self.torch
        me, mi, need = self.me, self.mi, self.me + self.mi
        eps = float(np.finfo(np.float64).eps)
        reg_coef = float(np.sqrt(eps)) if reg_coef is None else float(reg_coef)      # pyipm.py:353
        delta0 = reg_coef if delta0 is None else float(delta0)                       # pyipm.py:372
        B = self.stage(d2L, Je, Ji, df, ce, ci, s, lda, mu=float(np.asarray(mu, dtype=np.float64).reshape(-1)[0]), eps=eps)
        mu_v = np.broadcast_to(np.asarray(mu, dtype=np.float64), (B,)).copy()
        delta_v = np.broadcast_to(np.asarray(delta, dtype=np.float64), (B,)).copy()
        dc_v, zero = np.zeros(B), np.zeros(B)
        part = np.ones(B, dtype=bool) if active is None else np.asarray(active).astype(bool).reshape(B)
        out, st = self.step_each(mu_v, zero, zero, None if active is None else part.astype(np.int32))
        self.n_factor += 1
        stats = list(st)

        def flags(pred, *args):
            return np.array([bool(pred(x, *args)) for x in stats])

        def mask(idx):
            a = np.zeros(B, dtype=np.int32)
            a[idx] = 1
            return a

        passes = np.zeros(B, dtype=np.int64)
        berr = np.full(B, np.nan)
        refined, guard_miss = np.zeros(B, dtype=bool), np.zeros(B, dtype=bool)
        loops = {}                             # b -> the reghess.ShiftLoop of a problem that missed berr_tol or is being shifted
        cond = bool(self._opts_get("condensed")) and mi > 0
        full = False                           # the handle has been switched to the full form for the rest of this call

        def go_full():
            nonlocal full
            if cond and not full:
                self.n_condensed_fallback += 1
                self._ck(self.lib.pyipm_newton_set_option(self.h, b"condensed", 0.0))
                full = True

        def loop_of(b):
            if b not in loops:
                loops[b] = reghess.ShiftLoop(max_shift_tries, self.berr_fallback)
            return loops[b]

        def refine_group(idx):
            """ONE refine_all over ``idx``; returns those that missed berr_tol."""
            info = self.refine_all(out, active=mask(idx)).cpu().numpy()
            self.n_refined += int(idx.size)
            missed = []
            for b in idx:
                refined[b], berr[b] = True, info[b, 2]
                if info[b, 2] >= 0.0 and info[b, 2] <= self.berr_tol:
                    if stats[b]["n_zero"] > 0:     # reference: LU over the whole matrix, no shift (pyipm.py:1381 not taken);
                        self.n_static += 1         # counted for a shifted solve too, which HipNewtonBackend does not do
                    continue
                self.n_unconverged += 1
                missed.append(b)
            return missed

        try:
            if cond and self.guard:
                be = self.last_backward_errors = self.backward_errors(out)
                guard_miss = ((be > self.condensed_tol) | ~torch.isfinite(be)).cpu().numpy()
            judged = part
            if cond and refine:
                judged = (flags(reghess.wrong, need) | flags(reghess.suspect, self.suspect_spread) | flags(reghess.at_risk)
                          | guard_miss) & part
                if judged.any():
                    go_full()
                    _, st = self.step_each(mu_v, zero, zero, mask(np.flatnonzero(judged)), out=out)
                    self.n_factor += 1
                    stats = list(st)
            bad = flags(reghess.wrong, need) & judged
            nonfinite = flags(lambda x: x["nonfinite"])
            if refine:
                sus = flags(reghess.suspect, self.suspect_spread) & judged
                singular = nonfinite & judged
                ask = np.flatnonzero(sus & ~singular)      # (whatever the inertia says: the estimate decides on delta_c)
                if ask.size:
                    rc = self.rcond_all(active=mask(ask)).cpu().numpy()
                    self.n_rcond += int(ask.size)
                    for b in ask:
                        singular[b] = reghess.singular(rc[b], stats[b], eps, nan_singular=True)
                risk = np.flatnonzero(flags(reghess.at_risk) & judged & ~bad & ~singular)
                for b in (refine_group(risk) if risk.size else ()):
                    loop_of(b).remember(float(berr[b]), out[b].clone, 0.0, stats[b])
                    singular[b] = True
                failed = bad | singular
            else:
                sus = singular = nonfinite | flags(reghess.suspect, eps)
                failed = (bad | sus | guard_miss) & part
            pending = np.flatnonzero(failed)
            for b in pending:
                dc_v[b] = reghess.delta_c(singular[b], me, reg_coef, eta, mu_v[b], beta)
                delta_v[b] = reghess.first_shift(delta_v[b], delta0)
            if pending.size:
                go_full()
            while pending.size:
                act = mask(pending)
                _, st = self.step_each(mu_v, np.where(act, delta_v, 0.0), np.where(act, dc_v, 0.0), act, out=out)
                self.n_factor += 1
                passes[pending] += 1
                new = list(st)
                verdict = {}
                for b in pending:
                    stats[b] = new[b]
                    if reghess.wrong(stats[b], need):  # an inertia retry, not an unconverged solve: no part in the stall count
                        self.n_inertia_retries += 1
                        verdict[b] = loop_of(b).inertia_retry()
                lost = [b for b in verdict if verdict[b] != reghess.AGAIN]
                if lost:
                    raise RuntimeError("inertia not corrected after %d diagonal shifts: problems %s"
                                       % (max_shift_tries + 1, lost if refine else [int(b) for b in lost]))
                ok = np.array([b for b in pending if b not in verdict], dtype=np.int64)
                berr[ok] = np.nan
                rk = np.array([b for b in ok if refine and reghess.at_risk(stats[b])], dtype=np.int64)
                for b in (refine_group(rk) if rk.size else ()):
                    verdict[b] = loop_of(b).miss(float(berr[b]), out[b].clone, delta_v[b], stats[b])
                    if verdict[b] == reghess.SETTLE:       # the best direction seen, in place of the last solve
                        self.n_inexact += 1
                        berr[b], best, delta_v[b], stats[b] = loops[b].best
                        out[b].copy_(best)
                lost = [b for b in ok if verdict.get(b) == reghess.LOST_SOLVE]
                if lost:
                    raise RuntimeError("refined solve did not reach backward error %.1e after %d diagonal shifts: problems %s"
                                       % (self.berr_tol, max_shift_tries + 1, lost))
                pending = np.array([b for b in pending if verdict.get(b) == reghess.AGAIN], dtype=np.int64)
                delta_v[pending] *= 10.0
        finally:
            if full:
                self._ck(self.lib.pyipm_newton_set_option(self.h, b"condensed", 1.0))
        self._shift_info = {"failed": failed.copy(), "suspect": sus, "delta_c": dc_v, "delta": np.where(failed, delta_v, 0.0),
                            "passes": passes}
        if refine:
            self._shift_info.update(singular=singular, refined=refined, backward_error=berr)
        return out, delta_v, stats

    def _fetch_stats(self, step_id):
        if step_id != self._step_id:
            raise NewtonError("the statistics of an earlier step_all are gone: the handle keeps the last step's only -- read them "
                              "(len / index / iterate) before the next step")
        st = (FactorStats * self.batch)()
        rc = self.lib.pyipm_newton_stats_batched(self.h, st)
        if rc and rc != -4:                                   # (-4 = PYIPM_E_NONFINITE: the records say which problems)
            self._ck(rc)
        return [x.as_dict() for x in st]

    def _opts_get(self, name):
        return getattr(self, "_opts", {}).get(name, 0.0)

    def backward_errors(self, dz):
        """|g - Hc raw| / |g| per problem for the directions ``dz`` (B, N) of the last step, Hc from the staged blocks (device
        tensor of B doubles)."""
        torch = self.torch
        be = torch.empty(self.batch, dtype=torch.float64, device=self.device)
        self._ck(self.lib.pyipm_newton_backward_error_batched(self.h, c_void_p(dz.data_ptr()), c_void_p(be.data_ptr()), MEM_DEVICE))
        return be

    def last_ms(self):
        """HIP-event times of the last step (ms): residual + assembly, factorisation, substitutions, the whole step."""
        from ctypes import c_double
        t = (c_double * 8)()
        self._ck(self.lib.pyipm_newton_last_timings(self.h, t))
        return {"assemble_ms": t[0], "factor_ms": t[6], "solve_ms": t[3], "step_ms": t[1]}

    def close(self):
        if getattr(self, "h", None):
            self.lib.pyipm_newton_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
