#!/usr/bin/env python
"""Time pyipm_newton_solve_many (k right-hand sides against one factor) against k sequential solve() calls.

    python tools/bench_solve_many.py [--n 16384 --me 4096 --mi 6144] [--ks 1,8,64,256]

The bench shape of bench.py (N = 32768), its generator and default options, one factorisation.  For every k one JSON
line: ms per solve_many (HIP events, one warm-up call, median of 5), ms of k sequential solve() calls (k <= 64 timed;
beyond, extrapolated from k = 64 and labelled so), executed fp64 TF/s on the flops the kernels run (structural zeros
skipped, k padded to the column block) and the dense-equivalent rate 2 N^2 k / t, and the worst column backward error
|b - Hc x| / |b| with Hc applied by kkt_matvec.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MS_KB, TB, PAD = 64, 64, 128          # kernels_msolve.hpp column block, tile, Npad granularity


def executed_flops(n, me, mi, nb, kpad, wide_sub=256, skip_zeros=True):
    """Flops of the substitution kernels as launched (active_ranges / 64-row tiles as the driver skips them)."""
    N = n + me + 2 * mi
    Npad = (N + PAD - 1) // PAD * PAD

    def ranges(cA, cB):
        if not skip_zeros or mi == 0:
            return (0, Npad), (0, 0)
        s0, s1, i0 = n, n + mi, n + mi + me
        if cB <= s0:
            return (0, s0), (s1, Npad)
        if cA >= s0 and cB <= s1:
            return (i0 + (cA - s0), i0 + (cB - s0)), (0, 0)
        return (0, Npad), (0, 0)

    tot = 0.0
    for c in range(0, Npad, nb):
        pw = min(nb, Npad - c)
        sw = wide_sub if (wide_sub >= TB and wide_sub % TB == 0 and pw > wide_sub) else pw
        for off in range(0, pw, sw):
            c0, nbw = c + off, min(sw, pw - off)
            nt = nbw // TB
            tot += 2 * (2.0 * TB * TB * nt * (nt - 1) / 2) * kpad                # in-panel, forward and backward
            (a0, a1), (b0, b1) = ranges(c0, c0 + nbw)
            rows = sum(TB for r in range(c0 + nbw, Npad, TB) if (r + TB > a0 and r < a1) or (r + TB > b0 and r < b1))
            tot += 2 * (2.0 * rows * nbw) * kpad                                   # below the panel, forward and backward
    tot += 2.0 * TB * Npad * kpad                                                  # inv(T) y
    return tot


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--me", type=int, default=4096)
    ap.add_argument("--mi", type=int, default=6144)
    ap.add_argument("--ks", default="1,8,64,256")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-seq", action="store_true", help="skip the sequential solve() baseline and the backward-error "
                    "check (a kernel trace of the solve_many calls alone)")
    a = ap.parse_args()
    import numpy as np
    import torch
    from bench import default_panel_width, make_qp_device
    from pyipm_amd.newton import NewtonCore
    dev = torch.device("cuda", 0)
    n, me, mi = a.n, a.me, a.mi
    N = n + me + 2 * mi
    qp = make_qp_device(n, me, mi, a.seed, dev)
    nb = default_panel_width(1, N)
    core = NewtonCore(n, me, mi, device=0, nb=nb)
    core.stage_blocks(qp["d2L"], qp["Je"], qp["Ji"])
    core.stage_vectors(qp["df"], qp["ce"], qp["ci"], qp["s"], qp["lam"], mu=qp["mu"])
    core.residual()
    core.assemble(0.0, 0.0)
    core.factor()
    torch.cuda.synchronize()
    gen = torch.Generator(device=dev).manual_seed(1)
    ks = [int(x) for x in a.ks.split(",")]
    B_all = torch.randn(N, max(ks), dtype=torch.float64, device=dev, generator=gen)

    def timed(fn, reps):
        out = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1))
        return float(np.median(out))

    seq64 = None
    for k in ks:
        B = B_all[:, :k].contiguous()
        core.solve_many(B)                                                        # warm-up (allocates its buffer)
        torch.cuda.synchronize()
        t_many = timed(lambda: core.solve_many(B), 5)
        cols = [B[:, j].contiguous() for j in range(k)]
        if a.no_seq:
            t_seq, seq_label = float("nan"), "not run"
        elif k <= 64:
            core.solve(cols[0])
            t_seq = timed(lambda: [core.solve(c) for c in cols], 3 if k == 64 else 5)
            seq_label = "measured"
            if k == 64:
                seq64 = t_seq
        else:
            t_seq = seq64 * k / 64.0 if seq64 else float("nan")
            seq_label = "extrapolated from k = 64"
        X = core.solve_many(B, flip=False)
        berr = float("nan") if a.no_seq else 0.0
        for j in (range(0) if a.no_seq else range(k)):
            r = core.matvec(X[:, j].contiguous()) - B[:, j]
            berr = max(berr, float(r.norm() / B[:, j].norm()))
        kpad = (k + MS_KB - 1) // MS_KB * MS_KB
        fl = executed_flops(n, me, mi, nb, kpad)
        print(json.dumps({
            "metric": "solve_many", "N": N, "n": n, "me": me, "mi": mi, "nb": nb, "k": k,
            "ms_solve_many": round(t_many, 3), "ms_sequential_solve": round(t_seq, 3), "sequential": seq_label,
            "speedup": round(t_seq / t_many, 2),
            "executed_tflops": round(fl / (t_many * 1e-3) / 1e12, 2),
            "executed_flops_note": "flops the kernels run: structural zeros skipped, k padded to %d" % MS_KB,
            "dense_equivalent_tflops": round(2.0 * N * N * k / (t_many * 1e-3) / 1e12, 2),
            "worst_backward_error": berr}), flush=True)
    core.close()


if __name__ == "__main__":
    main()
