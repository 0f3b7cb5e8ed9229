"""A whole batch of QPs of one shape from their starts to their KKT points, in lockstep, on the batched handle.

    min 1/2 x'Q_b x + c_b'x    s.t.  A_b x = b_b ,  G_b x - h_b >= 0            b = 0 .. B-1

``BatchedQPIPM`` runs the barrier loop of ``pyipm_amd.loop.BarrierLoop`` (``/root/reference/pyipm.py:1567-1863``) for every
problem at once: one lockstep iteration is ONE batched direction (``BatchedNewton.direction_all``: per-problem ``mu`` and
shifts, the ``active`` mask), ONE ``step_lengths_all``, ONE ``merit_info_all`` (KKT norms, the ``nu`` update, the barrier
update, ``phi0`` and ``dphi0``) and one ``merit_ray_all`` per ``RAY_BATCH`` backtracking candidates ``alpha tau^k`` of every
problem (the sequence of roundings ``alpha *= tau`` of ``QPDeviceIPM.search``); ``f, df, ce, ci`` come from ``products_all``.
Every problem carries its own ``mu``, ``nu``, ``delta``, ``signal`` and iteration counters; a problem that has met its stopping
test sits out through ``active`` and keeps its iterate bit for bit.  Iterates and directions never leave the device; per phase
one small device-to-host copy serves the whole batch (never one per problem).  Multi-start is the same blocks with different
starts.

Scope: the plain backtracking Armijo search only -- no second-order correction, no ``Ftol`` test, no ``lbfgs`` mode;
``signal = -2`` per problem on a dead direction (1: converged to ``Ktol``, -1: out of outer iterations).

The KKT norms of a point are those of the residual the step at that point forms, so a problem whose barrier parameter changes
(or that stops) at a point has taken part in one step there whose direction is not used: per problem one such step per barrier
update.  No CPU fallback.
"""
from __future__ import annotations

import time

import numpy as np

from ._device import to_device
from .batched import BatchedNewton


class BatchedQPIPM(object):
    RAY_BATCH = 64                       # backtracking candidates alpha tau^k of every problem per launch of k_b_merit_ray

    def __init__(self, Q, c, A=None, b=None, G=None, h=None, x0=None, s0=None, lda0=None, mu=0.2, nu=10.0, rho=0.1, tau=0.995,
                 eta=1.0E-4, beta=0.4, miter=20, niter=10, Ktol=1.0E-4, device=None, condensed=False, profile=False, refine=False):
        """Q (B, n, n), c (B, n), A (B, me, n), b (B, me), G (B, mi, n), h (B, mi): NumPy arrays or torch tensors; a block
        without the batch dimension is shared by every problem.  Starts x0 (B, n; default 0), s0 (B, mi; default
        max(G x0 - h, Ktol)), lda0 (B, me + mi; default lda_e = 0, lda_i = mu / s0).  ``profile``: synchronise around the
        phases and keep their times in ``timings``.  ``refine``: ``direction_all(refine=True)`` -- a condition estimate
        and adaptive refinement per problem instead of a shift for every suspect one (an LP is then not shifted at all)."""
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("BatchedQPIPM needs a GPU: the Newton-step core has no CPU fallback")
        self.torch = torch
        dev = self.device = torch.device("cuda", torch.cuda.current_device() if device is None else int(device))
        f64 = torch.float64
        c = to_device(c, dev)
        B, n = self.batch, self.nvar = int(c.shape[0]), int(c.shape[1])

        def block(a, rows, trans):
            if a is None:
                return None
            a = to_device(a, dev, contiguous=False)
            if a.dim() == 2:
                a = a.expand(B, *a.shape)
            return (a.transpose(1, 2) if trans else a).contiguous()

        self.c = c
        self.Q = block(Q, n, False)
        # Jacobians in the reference's layout: Je = dce (n x me), Ji = dci (n x mi)  (pyipm.py:486-501)
        self.Je, self.Ji = block(A, None, True), block(G, None, True)
        me = self.neq = 0 if self.Je is None else int(self.Je.shape[2])
        mi = self.nineq = 0 if self.Ji is None else int(self.Ji.shape[2])
        if me == 0:
            self.Je = None
        if mi == 0:
            self.Ji = None
        assert self.Q.shape == (B, n, n)
        z = lambda k: torch.zeros((B, k), dtype=f64, device=dev)          # noqa: E731
        self.b = to_device(b, dev, (B, me)) if me else z(0)
        self.h = to_device(h, dev, (B, mi)) if mi else z(0)
        self.eps = float(np.finfo(np.float64).eps)
        self.mu, self.nu, self.rho, self.tau, self.eta, self.beta = mu, nu, rho, tau, eta, beta
        self.miter, self.niter, self.Ktol = int(miter), int(niter), Ktol
        self.profile, self.refine = bool(profile), bool(refine)
        self.core = BatchedNewton(n, me, mi, device=dev.index, condensed=condensed)
        # the constant blocks, and vectors of the right shapes so that the handle exists before the first product
        self.core.stage(self.Q, self.Je, self.Ji, self.c, z(me) if me else None, z(mi) + 1.0 if mi else None,
                        z(mi) + 1.0 if mi else None, z(me + mi) if (me + mi) else None, mu=mu, eps=self.eps)
        self.x0 = to_device(x0, dev, (B, n)) if x0 is not None else z(n)
        if mi:
            self.s0 = to_device(s0, dev, (B, mi)) if s0 is not None else torch.clamp(self._provider(self.x0)[3], min=Ktol)
        else:
            self.s0 = z(0)
        if lda0 is not None:
            self.lda0 = to_device(lda0, dev, (B, me + mi))
        else:
            self.lda0 = torch.cat([z(me), mu / self.s0], dim=1) if mi else z(me)
        self.timings = {"direction_s": 0.0, "search_s": 0.0, "n_ray": 0}
        self.n_lockstep = 0
        self.x_at_exit, self.exit_iteration = [None] * B, np.full(B, -1, dtype=np.int64)
        self.on_iteration = None             # callable(solver, lockstep index, active (B,) bool, x device tensor): a test's view

    # ------------------------------------------------------------------ provider (pyipm.py:855-954 for every problem)
    def _provider(self, x):
        """(f (B,), df, ce, ci) at x from ONE products_all."""
        Qx, Ax, Gx = self.core.products_all(x)
        f = (x * (0.5 * Qx + self.c)).sum(dim=1)
        return f, Qx + self.c, (Ax - self.b) if self.neq else None, (Gx - self.h) if self.nineq else None

    def _tick(self):
        if self.profile:
            self.torch.cuda.synchronize(self.device)
        return time.perf_counter()

    # ------------------------------------------------------------------ the control flow of BarrierLoop._barrier_loop, per problem
    def _small(self, kkt, tol):
        return all(k <= tol for k in kkt)

    def _advance(self, b, kkt, q, st):
        """Problem b stands at a point whose KKT norms ``kkt`` are known (the place of ``kkt = self.KKT(x, s, lda)`` in
        ``_barrier_loop``): run its loop forward to the next direction.  False: it stopped (``signal`` set).  The barrier
        update (pyipm.py:1804-1814) on the way changes ``st['mu'][b]``."""
        me, mi = self.neq, self.nineq
        while True:
            if st["at_outer"][b]:
                if self._small(kkt, self.Ktol):
                    st["signal"][b] = 1
                    return False
                st["at_outer"][b], st["inner"][b] = False, 0
            tol = max(self.Ktol, st["mu"][b])
            if st["inner"][b] < self.miter and not self._small(kkt, tol):
                return True
            if self._small(kkt, tol) and not me and not mi:
                st["signal"][b] = 1
            if st["outer"][b] >= self.niter - 1:
                st["signal"][b] = -1
                return False
            if mi:
                comp, mn = q[9], q[10]
                xi = mi * mn / (comp + self.eps)
                mu_new = 0.1 * min(0.05 * (1.0 - xi) / (xi + self.eps), 2.0) ** 3 * comp / mi
                st["mu"][b] = max(float(mu_new), 0.0)
            st["outer"][b] += 1
            st["at_outer"][b] = True

    def solve(self):
        """Returns a dict: ``x, s, lda`` (device tensors (B, .)), ``fval, signal, iter_count, mu`` (NumPy (B,)).  ``mu`` is the
        barrier parameter of each problem's last KKT report -- the one its returned point satisfies the perturbed KKT
        conditions for; ``self.kkt`` holds those four norms per problem."""
        torch, core = self.torch, self.core
        B, n, me, mi = self.batch, self.nvar, self.neq, self.nineq
        dev, eps, K = self.device, self.eps, self.RAY_BATCH
        x, s, lda = self.x0.clone(), self.s0.clone(), self.lda0.clone()
        st = {"mu": np.full(B, self.mu if mi else self.Ktol, dtype=np.float64), "signal": np.zeros(B, dtype=np.int64),
              "outer": np.zeros(B, dtype=np.int64), "inner": np.zeros(B, dtype=np.int64), "at_outer": np.ones(B, dtype=bool)}
        mu, signal = st["mu"], st["signal"]
        nu, delta = np.full(B, float(self.nu)), np.zeros(B)
        iters = np.zeros(B, dtype=np.int64)
        done, pending = np.zeros(B, dtype=bool), np.zeros(B, dtype=bool)
        mu_kkt, self.kkt = mu.copy(), np.full((B, 4), np.nan)
        self.n_lockstep = 0

        def stop(b):
            done[b] = True
            self.x_at_exit[b], self.exit_iteration[b] = x[b].clone(), self.n_lockstep

        while not done.all():
            act = ~done
            if self.on_iteration is not None:
                self.on_iteration(self, self.n_lockstep, act.copy(), x)
            t0 = self._tick()
            f, df, ce, ci = self._provider(x)
            dz, delta_new, _ = core.direction_all(self.Q, self.Je, self.Ji, df, ce, ci, s if mi else None,
                                                  lda if (me or mi) else None, mu, delta, self.eta, self.beta, active=act,
                                                  refine=self.refine)
            delta[act] = delta_new[act]
            info = core.merit_info_all(dz)
            al = core.step_lengths_all(self.tau, dz)
            host = torch.cat([info, al, f[:, None]], dim=1).cpu().numpy()        # the iteration's ONE report: (B, 19)
            t1 = self._tick()
            take = np.zeros(B, dtype=bool)
            for b in np.flatnonzero(act):
                q = host[b]
                if not pending[b]:
                    kkt = (q[5], q[6] if mi else 0.0, q[7] if me else 0.0, q[8] if mi else 0.0)
                    self.kkt[b], mu_kkt[b] = kkt, mu[b]
                    mu_was = mu[b]
                    if not self._advance(b, kkt, q, st):
                        stop(b)
                        continue
                    if mu[b] != mu_was:                      # the direction in hand belongs to the old barrier parameter
                        pending[b] = True
                        continue
                pending[b] = False
                if not np.isfinite(q[2]) or not np.isfinite(q[11]):          # no usable direction
                    signal[b] = -2
                    stop(b)
                    continue
                take[b] = True
            # merit parameter (pyipm.py:1727-1735), phi0 and its slope (:670-721) from the report
            con_l1 = (host[:, 0] if me else 0.0) + (host[:, 1] if mi else 0.0) + np.zeros(B)
            with np.errstate(divide='ignore', invalid='ignore'):
                if me or mi:
                    thres = (host[:, 2] - (mu * host[:, 3] if mi else 0.0)) / ((1 - self.rho) * con_l1)
                    up = take & (nu < thres)
                    nu[up] = thres[up]
                phi0 = host[:, 18] + (nu * con_l1 if (me or mi) else 0.0) - (mu * host[:, 4] if mi else 0.0)
                dphi0 = host[:, 2] - (nu * con_l1 if (me or mi) else 0.0) - (mu * host[:, 3] if mi else 0.0)
            ndx, nds = host[:, 11], (host[:, 12] if mi else np.zeros(B))
            cur_s = np.where(take, host[:, 16], 0.0)
            cur_l = np.where(take, host[:, 17], 0.0) if (me or mi) else np.zeros(B)
            acc_s, acc_l = np.zeros(B), np.zeros(B)
            searching, first = take.copy(), True
            nu_d, mu_d = torch.from_numpy(nu).to(dev), torch.from_numpy(mu).to(dev)
            while searching.any():
                cand, cand_l = np.zeros((B, K)), np.zeros((B, K))
                cand[:, 0], cand_l[:, 0] = (cur_s, cur_l) if first else (cur_s * self.tau, cur_l * self.tau)
                for k in range(1, K):                        # alpha *= tau, the reference's sequence of roundings
                    cand[:, k], cand_l[:, k] = cand[:, k - 1] * self.tau, cand_l[:, k - 1] * self.tau
                cand[~searching], cand_l[~searching] = 0.0, 0.0
                d = core.merit_ray_all(torch.from_numpy(cand).to(dev), nu_d, mu_d, dz).cpu().numpy()
                self.timings["n_ray"] += 1
                with np.errstate(invalid='ignore'):
                    tr = (phi0[:, None] + d) - (phi0[:, None] + (cand * self.eta) * dphi0[:, None])   # > 0: rejected
                for b in np.flatnonzero(searching):
                    for k in range(K):
                        if not tr[b, k] > 0.0:
                            acc_s[b], acc_l[b], searching[b] = cand[b, k], cand_l[b, k], False
                            break
                        if first and k == 0:
                            continue
                        size = np.sqrt((cand[b, k] * ndx[b]) ** 2 + (cand_l[b, k] * nds[b]) ** 2) if mi else cand[b, k] * ndx[b]
                        if size < eps:                       # search direction unreliable to machine precision
                            signal[b], searching[b], take[b] = -2, False, False
                            iters[b] += 1
                            stop(b)
                            break
                    else:
                        cur_s[b], cur_l[b] = cand[b, -1], cand_l[b, -1]
                first = False
            if take.any():
                step = torch.from_numpy(np.stack([np.where(take, acc_s, 0.0), np.where(take, acc_l, 0.0)], axis=1)).to(dev)
                m = torch.from_numpy(take).to(dev)[:, None]
                x = torch.where(m, x + step[:, 0:1] * dz[:, :n], x)
                if mi:
                    s = torch.where(m, s + step[:, 0:1] * dz[:, n:n + mi], s)
                if me or mi:
                    lda = torch.where(m, lda + step[:, 1:2] * dz[:, n + mi:], lda)
                iters[take] += 1
                st["inner"][take] += 1
            t2 = self._tick()
            self.timings["direction_s"] += t1 - t0
            self.timings["search_s"] += t2 - t1
            self.n_lockstep += 1

        fval = self._provider(x)[0].cpu().numpy()
        self.x, self.s, self.lda = x, s, lda
        self.signal, self.iter_count, self.mu_next = signal.copy(), iters.copy(), mu.copy()
        return {"x": x, "s": s, "lda": lda, "fval": fval, "signal": signal.copy(), "iter_count": iters.copy(),
                "mu": mu_kkt.copy()}
