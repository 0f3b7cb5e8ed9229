#!/usr/bin/env python
"""Device-event timings of the per-problem adaptive refinement of the batched handle (pyipm_newton_refine_batched) on the
config-5 shape (512 x (n, me, mi) = (256, 0, 256)), full form, warmed, the variants alternating in one process:

  look       refine_all on a batch of QPs: no member needs a step -- one residual and the decision per member
  few        8 of the 512 members are LPs (d2L = 0: static pivots) and take steps, the others stop at the first look
  all        every member is an LP, max_steps = 1: every member takes max_steps steps
  step_each  one unshifted step of the QP batch, on the same build
  solve_k1_refine1   solve_all(k = 1, refine = 1): the fixed-count refinement every member pays for
  copy       restoring the direction before a call (part of the three refine_all figures: the call works in place)

Prints one JSON line.  Every figure is the median over --rounds windows of --steps calls, with the min and max window beside
it (the spread of that same run).  ``--root DIR`` measures the package of another checkout of this repository -- the parent
commit's -- which has no refine_all: only step_each and solve_k1_refine1 are timed there.

    python tools/bench_refine_batched.py [--batch 512] [--rounds 9] [--steps 20] [--root DIR]"""
import argparse
import json
import os
import sys

import numpy as np


def summary(ms):
    ms = np.asarray(ms)
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import torch
    from pyipm_amd.batched import BatchedNewton
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    have = hasattr(BatchedNewton, "refine_all")
    n, me, mi, B = 256, 0, 256, a.batch
    N = n + 2 * mi + me
    gen = torch.Generator(device="cuda").manual_seed(5)
    f64, dev = torch.float64, "cuda"
    M = torch.randn(B, n, n, dtype=f64, device=dev, generator=gen)
    Q = M @ M.transpose(1, 2) / n + torch.eye(n, dtype=f64, device=dev)
    del M
    Ji = (torch.randn(B, mi, n, dtype=f64, device=dev, generator=gen) / np.sqrt(n)).transpose(1, 2).contiguous()
    c = torch.randn(B, n, dtype=f64, device=dev, generator=gen)
    s = torch.rand(B, mi, dtype=f64, device=dev, generator=gen) * 1.5 + 0.5
    lam = torch.rand(B, mi, dtype=f64, device=dev, generator=gen) * 1.5 + 0.5
    ci = s + 0.1 * torch.randn(B, mi, dtype=f64, device=dev, generator=gen)
    mu = torch.full((B,), 0.2, dtype=f64, device=dev)
    zero = torch.zeros(B, dtype=f64, device=dev)
    out = {"shape": [n, me, mi], "batch": B, "rounds": a.rounds, "steps": a.steps, "refine_all": have}

    def handle(lp_members):
        q = Q.clone()
        q[lp_members] = 0.0
        bn = BatchedNewton(n, me, mi, guard=False)
        bn.stage(q, None, Ji, c, None, ci, s, lam, mu=0.2)
        dz, _ = bn.step_each(mu, zero, zero)
        return bn, q, dz.clone(), dz

    bn, _, dz0, dz = handle([])
    rhs = torch.randn(B, 1, N, dtype=f64, device=dev, generator=gen)
    x = torch.empty_like(rhs)
    fns = {"step_each": lambda: bn.step_each(mu, zero, zero, None, out=dz),
           "solve_k1_refine1": lambda: bn.solve_all(rhs, refine=1, out=x)}
    keep = [bn]
    if have:
        few = list(range(0, B, max(B // 8, 1)))[:8]
        bf, _, df0, df = handle(few)
        ba, _, da0, da = handle(list(range(B)))
        keep += [bf, ba]
        work = dz0.clone()

        def refine(h, d0, d, **kw):
            d.copy_(d0)
            return h.refine_all(d, **kw)

        fns["look"] = lambda: refine(bn, dz0, work)
        fns["few"] = lambda: refine(bf, df0, df)
        fns["all"] = lambda: refine(ba, da0, da, max_steps=1)
        fns["copy"] = lambda: work.copy_(dz0)
        for name, who in (("look", "look"), ("few", "few"), ("all", "all")):
            info = fns[name]().cpu().numpy()
            out[who + "_members_by_steps"] = {str(int(k)): int(v) for k, v in zip(*np.unique(info[:, 0], return_counts=True))}
            out[who + "_converged"] = int(info[:, 3].sum())
    res = {k: [] for k in fns}
    for name, f in fns.items():                        # warm-up
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
    for name in fns:
        out[name] = summary(res[name])
    for h in keep:
        h.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
