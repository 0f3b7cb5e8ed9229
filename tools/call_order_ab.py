#!/usr/bin/env python
"""A/B helper for the C-ABI's bookkeeping of what a handle holds (csrc/ctx.hpp: Held): a fixed list of legal and illegal
call sequences on small systems.  Every call prints its return code, last_error when it was refused, and a sha1 of every
vector it returned.  Run it with two libraries (PYIPM_NEWTON_LIB) and diff the outputs: a change that is meant to keep
the entry points' behaviour prints the same lines.  The illegal orders are the ones the library refuses with a code;
nothing here reaches the device with bad arguments."""
import ctypes, hashlib, os, sys
os.environ.setdefault("PYIPM_EXPERT", "1")     # tools use expert switches (include/pyipm_newton.h)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from pyipm_amd import newton
from pyipm_amd.newton import NewtonCore, NewtonError, FactorStats
from pyipm_amd.batched import BatchedNewton
from pyipm_amd.problems import make_qp

HOST, DEV = newton.MEM_HOST, newton.MEM_DEVICE
ALPHAS = (1.0, 0.5, 0.25, 0.01)


def fp(x):
    if isinstance(x, torch.Tensor):
        return hashlib.sha1(x.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]
    if isinstance(x, np.ndarray):
        return hashlib.sha1(np.ascontiguousarray(x).tobytes()).hexdigest()[:16]
    if isinstance(x, dict):
        return "{" + " ".join("%s=%s" % (k, fp(v)) for k, v in sorted(x.items()) if not k.endswith("_ms")) + "}"
    if isinstance(x, (list, tuple)):
        return "[" + " ".join(fp(v) for v in x) + "]"
    if isinstance(x, float):
        return "%.17g" % x
    return repr(x)


def call(tag, fn, *a, **kw):
    """one line per call: tag, code, fingerprints or the refusal's text"""
    try:
        out = fn(*a, **kw)
        print("  %-34s rc=0 %s" % (tag, fp(out)))
        return out
    except NewtonError as e:
        print("  %-34s rc=%s %s" % (tag, getattr(e, "code", "?"), e))
        return None


def raw(tag, lib, h, rc, *outs):
    msg = lib.pyipm_newton_last_error(h).decode() if rc else ""
    print("  %-34s rc=%d %s %s" % (tag, rc, msg, " ".join(fp(o) for o in outs) if not rc else ""))


def staged(n, me, mi, seed, cond=0, **kw):
    qp = make_qp(n, me, mi, seed)
    c = NewtonCore(n, me, mi, device=0, **kw)
    c.set_option("condensed", cond)
    c.stage_blocks(qp["d2L"], qp["Je"], qp["Ji"])
    c.stage_vectors(qp["df"], qp["ce"], qp["ci"], qp["s"], qp["lam"], mu=qp["mu"])
    return c, qp


def after_solve(c):
    call("step_lengths", c.step_lengths, 0.995)
    call("merit_info", c.merit_info)
    call("merit_ray", c.merit_ray, ALPHAS, 10.0, 0.1)
    call("merit_ray again", c.merit_ray, ALPHAS, 10.0, 0.1)


# what may come between a factorisation with a fused forward pass and solve(rhs = NULL)
def between(c, qp, what):
    N = c.N
    v = torch.linspace(-1.0, 1.0, N, dtype=torch.float64, device=c.device)
    if what == "kkt_matvec":
        call("kkt_matvec", c.matvec, v)
    elif what == "rcond_adaptive":
        call("rcond(-1,-1)", c.rcond, -1, -1); call("rcond(-1,-1) warm", c.rcond, -1, -1)
    elif what == "rcond_fixed":
        call("rcond(2,3)", c.rcond, 2, 3)
    elif what == "solve_many":
        call("solve_many k=3", c.solve_many, torch.stack([v, v * v, 1.0 - v], dim=1), True, 1)
    elif what == "merit":
        call("merit_info", c.merit_info); call("merit_ray", c.merit_ray, ALPHAS, 10.0, 0.1)
    elif what == "stage_vectors":
        call("stage_vectors", c.stage_vectors, qp["df"] * 1.5, qp["ce"], qp["ci"], qp["s"], qp["lam"], mu=qp["mu"])
    elif what == "residual":
        call("residual", c.residual)
    elif what == "solve_rhs":
        call("solve(rhs)", c.solve, v, True, 0)
    elif what == "step_lengths":
        call("step_lengths", c.step_lengths, 0.995)


BETWEEN = ("nothing", "kkt_matvec", "rcond_adaptive", "rcond_fixed", "solve_many", "merit", "stage_vectors", "residual",
           "solve_rhs", "step_lengths")

for shape in [(96, 32, 48, 4), (300, 100, 150, 7)]:
    n, me, mi, seed = shape
    for cond in (0, 1):
        for what in BETWEEN:
            print("== fused factor, %s, solve(NULL): qp %s cond %d" % (what, shape, cond))
            c, qp = staged(n, me, mi, seed, cond)
            call("residual", c.residual); call("assemble", c.assemble, 0.0, 0.0); call("factor", c.factor)
            between(c, qp, what)
            call("solve(NULL)", c.solve)           # (after stage_vectors: refused, no right-hand side)
            after_solve(c)
            call("solve(NULL) refine=-1", c.solve, None, True, -1); call("solve_info", c.solve_info)
            between(c, qp, what)
            after_solve(c)
            call("step", c.step, 0.0, 0.0, 1)
            after_solve(c)
            call("solve(NULL) flip=0", c.solve, None, False, 0)
            call("step_lengths (no direction)", c.step_lengths, 0.995)
            c.close()

print("== condensed switched on and off on one handle")
c, qp = staged(300, 100, 150, 7, 0)
for cond in (1, 0, 1, 1, 0):
    c.set_option("condensed", cond)
    call("step cond=%d" % cond, c.step, 1e-8, 1e-8, 2)
    if cond == 0:
        call("kkt_storage", lambda: tuple(c.kkt_storage().shape))     # (its upper triangle is never written: no hash)
    call("rcond(-1,-1)", c.rcond, -1, -1)
    call("solve(NULL)", c.solve)
    after_solve(c)
c.close()

print("== kkt_storage followed by assemble (keep_zeros)")
c, qp = staged(300, 100, 150, 7, 0)
call("step", c.step, 0.0, 0.0)
call("step (zeros in place)", c.step, 0.0, 0.0)
call("kkt_storage", lambda: tuple(c.kkt_storage().shape))
call("step (after export)", c.step, 0.0, 0.0)
call("set keep_zeros", c.set_option, "keep_zeros", 1)
call("step", c.step, 0.0, 0.0); call("step", c.step, 0.0, 0.0)
c.close()

print("== per-panel phases followed by solve")
c, qp = staged(700, 200, 300, 8, 0, nb=128)
call("factor_begin (not assembled)", c.factor_begin)
call("residual", c.residual); call("assemble", c.assemble, 0.0, 0.0); call("factor_begin", c.factor_begin)
for p in range(c.npanels):
    call("factor_panel %d" % p, c.factor_panel, p); call("trailing_update %d" % p, c.trailing_update, p)
call("factor_end", c.factor_end)
call("solve(NULL)", c.solve); after_solve(c)
call("step (group schedule again)", c.step, 0.0, 0.0); after_solve(c)
c.set_option("condensed", 1)
call("assemble cond", c.assemble, 0.0, 0.0); call("factor_begin (condensed)", c.factor_begin)
c.close()

print("== nonfinite factorisation, then a shifted retry")
n = 96
c, qp = staged(n, 32, 48, 4, 0)
bad = np.array(qp["d2L"], dtype=np.float64, copy=True); bad[3, 5] = bad[5, 3] = np.nan
call("stage_blocks (NaN)", c.stage_blocks, bad, qp["Je"], qp["Ji"])
call("residual", c.residual); call("assemble", c.assemble, 0.0, 0.0); call("factor", c.factor)
call("step", c.step, 0.0, 0.0)                         # (refused again; no substitution is run on the NaN factor)
call("stage_blocks", c.stage_blocks, qp["d2L"], qp["Je"], qp["Ji"])
call("residual", c.residual); call("assemble shifted", c.assemble, 1e-4, 1e-8); call("factor", c.factor)
call("solve(NULL)", c.solve); after_solve(c)
c.close()

print("== wrong orders on a fresh handle")
lib = newton.load_library()
h = ctypes.c_void_p()
for args in [(0, 0, 0, 256, 0, 1, 0), (8, 0, 0, 96, 0, 1, 0), (8, 0, 0, 256, 99, 1, 0)]:
    print("  create%s rc=%d" % (args, lib.pyipm_newton_create(ctypes.byref(h), *args, None, 0, None)))
print("  create rc=%d" % lib.pyipm_newton_create(ctypes.byref(h), 8, 2, 3, 256, 0, 1, 0, None, 0, None))
st = FactorStats(); x = np.zeros(8 + 6 + 2); o4 = (ctypes.c_double * 4)(); a = ctypes.c_double(); b = ctypes.c_double()
P = lambda v: v.ctypes.data_as(ctypes.c_void_p)
raw("assemble", lib, h, lib.pyipm_newton_assemble(h, 0.0, 0.0))
raw("residual", lib, h, lib.pyipm_newton_residual(h, P(x), HOST))
raw("factor", lib, h, lib.pyipm_newton_factor(h, ctypes.byref(st)))
raw("solve", lib, h, lib.pyipm_newton_solve(h, None, P(x), 1, 0, HOST))
raw("solve null output", lib, h, lib.pyipm_newton_solve(h, None, None, 1, 0, HOST))
raw("solve_many", lib, h, lib.pyipm_newton_solve_many(h, 2, P(x), 16, P(x), 16, 1, 0, HOST))
raw("solve_many k=0", lib, h, lib.pyipm_newton_solve_many(h, 0, None, 16, None, 16, 1, 0, HOST))
raw("solve_many k<0", lib, h, lib.pyipm_newton_solve_many(h, -1, None, 16, None, 16, 1, 0, HOST))
raw("rcond", lib, h, lib.pyipm_newton_rcond(h, 0, 0, o4))
raw("step", lib, h, lib.pyipm_newton_step(h, 0.0, 0.0, 0, P(x), ctypes.byref(st), HOST))
raw("step_lengths", lib, h, lib.pyipm_newton_step_lengths(h, 0.9, None, ctypes.byref(a), ctypes.byref(b)))
raw("merit_info", lib, h, lib.pyipm_newton_merit_info(h, None, (ctypes.c_double * 16)()))
raw("factor_begin", lib, h, lib.pyipm_newton_factor_begin(h))
raw("step_batched", lib, h, lib.pyipm_newton_step_batched(h, 0.0, 0.0, P(x), None, HOST))
raw("stats_batched", lib, h, lib.pyipm_newton_stats_batched(h, ctypes.byref(st)))
raw("solve_dist", lib, h, lib.pyipm_newton_solve_dist(h, None, P(x), 1, 0, HOST))
raw("set_option unknown", lib, h, lib.pyipm_newton_set_option(h, b"no_such_option", 1.0))
raw("set_option group 99", lib, h, lib.pyipm_newton_set_option(h, b"group", 99.0))
print("  null handle: assemble rc=%d solve rc=%d last_error=%s" % (
    lib.pyipm_newton_assemble(None, 0.0, 0.0), lib.pyipm_newton_solve(None, None, P(x), 1, 0, HOST), lib.pyipm_newton_last_error(None)))
print("  destroy rc=%d" % lib.pyipm_newton_destroy(h))

print("== provider-only handle")
c = NewtonCore(96, 32, 48, device=0, provider_only=True)
qp = make_qp(96, 32, 48, 4)
call("stage_blocks", c.stage_blocks, qp["d2L"], qp["Je"], qp["Ji"])
call("stage_vectors", c.stage_vectors, qp["df"], qp["ce"], qp["ci"], qp["s"], qp["lam"], mu=qp["mu"])
call("residual", c.residual); call("assemble", c.assemble, 0.0, 0.0)
call("solve_many", c.solve_many, torch.ones(c.N, 2, dtype=torch.float64, device=c.device))
call("matvec", c.matvec, torch.ones(c.N, dtype=torch.float64, device=c.device))
c.close()

print("== batched handle")
B, n, me, mi = 6, 64, 16, 32
qps = [make_qp(n, me, mi, 20 + k) for k in range(B)]
stack = lambda key: np.stack([np.asarray(q[key], dtype=np.float64) for q in qps])
for cond in (0, 1):
    bn = BatchedNewton(n, me, mi, batch=B, device=0, condensed=bool(cond), guard=False)
    lib, h = bn.lib, bn.h
    sts = (FactorStats * B)(); out = torch.empty((B, bn.N), dtype=torch.float64, device=bn.device)
    be = torch.empty(B, dtype=torch.float64, device=bn.device)
    op, bp = ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(be.data_ptr())
    raw("stats_batched first", lib, h, lib.pyipm_newton_stats_batched(h, sts))
    raw("backward_error first", lib, h, lib.pyipm_newton_backward_error_batched(h, op, bp, DEV))
    raw("step_batched unstaged", lib, h, lib.pyipm_newton_step_batched(h, 0.0, 0.0, op, None, DEV))
    raw("residual (single-system)", lib, h, lib.pyipm_newton_residual(h, op, DEV))
    raw("factor (single-system)", lib, h, lib.pyipm_newton_factor(h, ctypes.byref(st)))
    raw("solve (single-system)", lib, h, lib.pyipm_newton_solve(h, None, op, 1, 0, DEV))
    raw("rcond (single-system)", lib, h, lib.pyipm_newton_rcond(h, 0, 0, o4))
    raw("kkt_matvec (single-system)", lib, h, lib.pyipm_newton_kkt_matvec(h, op, op, DEV))
    for rep in range(2):
        dz, stats = bn.step_all(stack("d2L"), stack("Je"), stack("Ji"), stack("df"), stack("ce"), stack("ci"), stack("s"),
                                stack("lam"), mu=qps[0]["mu"])
        print("  step_all cond=%d %s %s" % (cond, fp(dz), fp([(s["n_neg"], s["n_zero"], s["d_min"], s["d_max"]) for s in stats])))
        raw("backward_error", lib, h, lib.pyipm_newton_backward_error_batched(h, ctypes.c_void_p(dz.data_ptr()), bp, DEV), be)
        raw("stats_batched", lib, h, lib.pyipm_newton_stats_batched(h, sts), [(s.n_neg, s.n_zero, s.d_min) for s in sts])
        raw("stats_batched null", lib, h, lib.pyipm_newton_stats_batched(h, None))
    bn.close()

print("== distributed entries on a single-rank handle")
for cond in (0, 1):
    c, qp = staged(300, 100, 150, 7, cond, nb=128)
    v = torch.linspace(-1.0, 1.0, c.N, dtype=torch.float64, device=c.device)
    call("solve_dist (not factored)", c.solve_dist)
    call("step_dist", c.step_dist, 0.0, 0.0, 1); after_solve(c)
    call("matvec_dist", c.matvec_dist, v)
    call("solve_dist(rhs)", c.solve_dist, v, True, -1); call("solve_info", c.solve_info); after_solve(c)
    call("residual_dist", c.residual_dist); call("assemble", c.assemble, 1e-8, 1e-8); call("factor_dist", c.factor_dist)
    call("solve_dist(NULL)", c.solve_dist); after_solve(c)
    call("solve(NULL) after dist", c.solve); after_solve(c)
    call("step", c.step, 0.0, 0.0); call("merit_ray", c.merit_ray, ALPHAS, 10.0, 0.1)
    call("solve_dist(rhs) after merit_ray", c.solve_dist, v); call("merit_ray", c.merit_ray, ALPHAS, 10.0, 0.1)
    c.close()

print("== L-BFGS direction twice, with and without restaged Jacobians")
from pyipm_amd.lbfgs import LbfgsCore
n, me, mi, m = 96, 32, 48, 4
qp = make_qp(n, me, mi, 4)
rng = np.random.default_rng(0)
S = rng.standard_normal((n, m)) / np.sqrt(n)
Y = 0.5 * S + 0.1 * rng.standard_normal((n, 3)) @ (rng.standard_normal((3, n)) @ S) / n
SY = S.T @ Y
SS, L, D = S.T @ S, np.tril(SY, -1), np.diag(np.diag(SY))
zeta = float(SY[-1, -1] / SS[-1, -1])
g = rng.standard_normal(n + 2 * mi + me)
lb = LbfgsCore(n, me, mi, m, device=0)
lb.stage_jacobian(qp["Je"], qp["Ji"])
for rep, restage in enumerate((False, False, True, False)):
    if restage:
        lb.stage_jacobian(qp["Je"] * 1.25, qp["Ji"])
    dz, st = lb.direction(g * (1.0 + rep), qp["s"], qp["lam"], zeta, S, Y, SS, L, D, reg=1e-12)
    print("  direction %d restaged=%d %s" % (rep, restage, fp(dz)))
