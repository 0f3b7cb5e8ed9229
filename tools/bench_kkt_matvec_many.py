#!/usr/bin/env python
"""Device-event timings of pyipm_newton_kkt_matvec_many (Y = Hc V for k columns in one launch) on the benchmark shape
(n, me, mi) = (16384, 4096, 6144), bench.py's generator, warmed, the variants alternating in one process:

  one kkt_matvec call (the yardstick: its code path is the parent commit's), kkt_matvec_many with k = 1, 16, 64 (ms per
  call and per column), and -- in two fresh processes, PYIPM_MS_MATVEC_MANY unset and set to 1, the switch being read at
  create time -- solve_many(k = 64, refine = 1).

Prints one JSON line (and writes it to --out).  Every figure is the median over --rounds windows of --steps calls, with
the min and max window beside it (the spread of that same run).  ``k16_per_column_below_one_matvec``: the per-column time at
k = 16 is below one kkt_matvec call beyond the spread of both (max of the one below min of the other).  For every k the
achieved TF/s on the flops the kernel executes (tiles and the column block padded to 64) and the TB/s on the bytes that
must move (every block once, V and Y once), next to the fp64 MFMA peak and the HBM rate DESIGN section 4 works with.

    python tools/bench_kkt_matvec_many.py [--rounds 9] [--steps 20] [--out profiles/kkt_matvec_many_ab.json]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KM = 64                                  # kernels_kmany.hpp: rows per workgroup, column block, K step


def summary(ms, per=1):
    ms = np.asarray(ms) / per
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms))}


def up(x):
    return (x + KM - 1) // KM * KM


def executed_flops(n, me, mi, k):
    kpad = up(k)
    rows_k = up(n) * (up(n) + up(me) + up(mi)) + (up(me) + up(mi)) * up(n)      # (tile rows) x (K walked), summed over the tiles
    return 2.0 * rows_k * kpad


def min_bytes(n, me, mi, k):
    N = n + me + 2 * mi
    return 8.0 * (n * (n + 1) / 2 + n * (me + mi) + 2 * N * k)


def windows(fns, rounds, steps):
    import torch
    res = {k: [] for k in fns}
    for f in fns.values():                             # warm-up
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for name, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                f()
            e1.record()
            e1.synchronize()
            res[name].append(e0.elapsed_time(e1) / steps)
    return res


def staged(a, factor):
    import torch
    from bench import default_panel_width, make_qp_device
    from pyipm_amd.newton import NewtonCore
    dev = torch.device("cuda", 0)
    qp = make_qp_device(a.n, a.me, a.mi, 0, dev)
    core = NewtonCore(a.n, a.me, a.mi, device=0, nb=default_panel_width(1, a.n + a.me + 2 * a.mi))
    core.stage_blocks(qp["d2L"], qp["Je"], qp["Ji"])
    core.stage_vectors(qp["df"], qp["ce"], qp["ci"], qp["s"], qp["lam"], mu=qp["mu"])
    core.residual()
    core.assemble(0.0, 0.0)
    if factor:
        core.factor()
    torch.cuda.synchronize()
    return core, dev


def child_solve_many(a):
    import torch
    core, dev = staged(a, True)
    N = core.N
    B = torch.randn(N, 64, dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    res = windows({"solve_many_k64_refine1": lambda: core.solve_many(B, refine=1)}, a.rounds, a.steps)
    print(json.dumps({"switch": os.environ.get("PYIPM_MS_MATVEC_MANY"), "per_call": summary(res["solve_many_k64_refine1"])}))
    core.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--me", type=int, default=4096)
    ap.add_argument("--mi", type=int, default=6144)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-solve-many", action="store_true", help="skip the two solve_many processes")
    ap.add_argument("--child-solve-many", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    if a.child_solve_many:
        return child_solve_many(a)
    n, me, mi = a.n, a.me, a.mi
    core, dev = staged(a, False)
    N = core.N
    gen = torch.Generator(device=dev).manual_seed(1)
    V = {k: torch.randn(N, k, dtype=torch.float64, device=dev, generator=gen) for k in (1, 16, 64)}
    v1 = V[1][:, 0].contiguous()
    fns = {"kkt_matvec": lambda: core.matvec(v1)}
    for k in V:
        fns["many_k%d" % k] = lambda k=k: core.kkt_matvec_many(V[k])
    res = windows(fns, a.rounds, a.steps)
    # the same matrix: worst column difference between the two routines, relative to the column
    Y = core.kkt_matvec_many(V[16])
    diff = max(float((core.matvec(V[16][:, j].contiguous()) - Y[:, j]).norm() / Y[:, j].norm()) for j in range(16))
    core.close()
    out = {"shape": [n, me, mi], "N": N, "rounds": a.rounds, "steps": a.steps, "kkt_matvec_per_call": summary(res["kkt_matvec"]),
           "column_block": KM, "many_vs_matvec_worst_column_difference": diff,
           "peaks": {"fp64_mfma_tflops": 78.6, "hbm_tbs": 8.0, "note": "vendor peaks of the MI355X"}}
    for k in V:
        t = summary(res["many_k%d" % k])
        sec = t["median_ms"] * 1e-3
        out["many_k%d" % k] = {"per_call": t, "per_column": summary(res["many_k%d" % k], k),
                               "executed_tflops": executed_flops(n, me, mi, k) / sec / 1e12,
                               "min_bytes_tbs": min_bytes(n, me, mi, k) / sec / 1e12}
    out["k16_per_column_below_one_matvec"] = bool(out["many_k16"]["per_column"]["max_ms"] < out["kkt_matvec_per_call"]["min_ms"])
    out["k1_slower_than_matvec"] = bool(out["many_k1"]["per_call"]["min_ms"] > out["kkt_matvec_per_call"]["max_ms"])
    if not a.no_solve_many:
        torch.cuda.empty_cache()
        for name, value in (("switch_unset", None), ("switch_set", "1")):
            env = dict(os.environ)
            env.pop("PYIPM_MS_MATVEC_MANY", None)
            if value is not None:
                env["PYIPM_MS_MATVEC_MANY"] = value
            cmd = [sys.executable, os.path.abspath(__file__), "--child-solve-many", "--n", str(n), "--me", str(me), "--mi", str(mi),
                   "--rounds", str(a.rounds), "--steps", str(max(1, a.steps // 4))]
            p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                raise SystemExit("solve_many process (%s) failed: %s" % (name, p.stderr[-2000:]))
            out.setdefault("solve_many_k64_refine1", {})[name] = json.loads(p.stdout.strip().splitlines()[-1])["per_call"]
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
