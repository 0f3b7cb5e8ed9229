#!/usr/bin/env python
"""Device-event timings of the batched handle's solve against the kept factors (pyipm_newton_solve_batched) on the config-5
shape (512 x (n, me, mi) = (256, 0, 256)), both forms, warmed, the variants alternating in one process:

  solve_all with k = 1, 16, 64 right-hand sides per problem (ms per call and per column), kkt_matvec_all with k = 16 and
  rcond_all (full form), next to the step's own substitution time -- ``solve_ms`` of ``last_ms()``, the existing k_b_solve on
  ONE column -- sampled in the same windows.

Prints one JSON line.  Every figure is the median over --rounds windows of --steps calls, with the min and max window beside
it (the spread of that same run).  ``k16_per_column_below_step_solve``: the per-column time at k = 16 is below the step's
one-column solve_ms beyond the spread of both (max of the one below min of the other).

    python tools/bench_solve_batched.py [--batch 512] [--rounds 9] [--steps 20]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def summary(ms, per=1):
    ms = np.asarray(ms) / per
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    import torch
    from pyipm_amd.batched import BatchedNewton
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    n, me, mi, B = 256, 0, 256, a.batch
    N = n + 2 * mi + me
    gen = torch.Generator(device="cuda").manual_seed(5)
    f64, dev = torch.float64, "cuda"
    M = torch.randn(B, n, n, dtype=f64, device=dev, generator=gen)
    Q = M @ M.transpose(1, 2) / n + torch.eye(n, dtype=f64, device=dev)
    Ji = (torch.randn(B, mi, n, dtype=f64, device=dev, generator=gen) / np.sqrt(n)).transpose(1, 2).contiguous()
    c = torch.randn(B, n, dtype=f64, device=dev, generator=gen)
    s = torch.rand(B, mi, dtype=f64, device=dev, generator=gen) * 1.5 + 0.5
    lam = torch.rand(B, mi, dtype=f64, device=dev, generator=gen) * 1.5 + 0.5
    ci = s + 0.1 * torch.randn(B, mi, dtype=f64, device=dev, generator=gen)
    out = {"shape": [n, me, mi], "batch": B, "rounds": a.rounds, "steps": a.steps}
    for form, condensed in (("full", False), ("condensed", True)):
        bn = BatchedNewton(n, me, mi, condensed=condensed, guard=False)
        bn.stage(Q, None, Ji, c, None, ci, s, lam, mu=0.2)
        mu = torch.full((B,), 0.2, dtype=f64, device=dev)
        zero = torch.zeros(B, dtype=f64, device=dev)
        dz, _ = bn.step_each(mu, zero, zero)
        rhs = {k: torch.randn(B, k, N, dtype=f64, device=dev, generator=gen) for k in (1, 16, 64)}
        xs = {k: torch.empty_like(v) for k, v in rhs.items()}
        fns = {"solve_k%d" % k: (lambda k=k: bn.solve_all(rhs[k], out=xs[k])) for k in rhs}
        fns["solve_k16_refine1"] = lambda: bn.solve_all(rhs[16], refine=1, out=xs[16])
        fns["matvec_k16"] = lambda: bn.kkt_matvec_all(rhs[16])
        if not condensed:
            fns["rcond"] = lambda: bn.rcond_all()
        res = {k: [] for k in fns}
        step_solve, step_total = [], []
        for f in fns.values():                         # warm-up
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for name, f in fns.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.steps):
                    f()
                e1.record()
                e1.synchronize()
                res[name].append(e0.elapsed_time(e1) / a.steps)
            w = []
            for _ in range(a.steps):                   # the step's own phases, one call at a time (its events are the handle's)
                bn.step_each(mu, zero, zero, None, out=dz)
                torch.cuda.synchronize()
                w.append(bn.last_ms())
            step_solve.append(float(np.mean([x["solve_ms"] for x in w])))
            step_total.append(float(np.mean([x["step_ms"] for x in w])))
        r = {"step_solve_ms_one_column": summary(step_solve), "step_ms": summary(step_total)}
        for k in (1, 16, 64):
            r["solve_k%d" % k] = {"per_call": summary(res["solve_k%d" % k]), "per_column": summary(res["solve_k%d" % k], k)}
        r["solve_k16_refine1_per_call"] = summary(res["solve_k16_refine1"])
        r["matvec_k16_per_call"] = summary(res["matvec_k16"])
        if not condensed:
            r["rcond_per_call"] = summary(res["rcond"])
        r["k16_per_column_below_step_solve"] = bool(r["solve_k16"]["per_column"]["max_ms"] < r["step_solve_ms_one_column"]["min_ms"])
        bn.close()
        out[form] = r
    print(json.dumps(out))


if __name__ == "__main__":
    main()
