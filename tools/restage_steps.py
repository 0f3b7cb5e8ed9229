"""The path of an NLP loop: blocks restaged before EVERY fused step, as pyipm_amd/ipm.py does (the x-block factorisation is
never reused there; the first step of a handle records a snapshot, the others must cost what a plain step costs).
Usage: python tools/restage_steps.py [--nvar N --neq ME --nineq MI --steps K]; prints one JSON line: the first step of the
handle (the recording step where the library has one) and the K restaged steps that follow, ms each (wall, synchronised)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nvar", type=int, default=16384)
    ap.add_argument("--neq", type=int, default=4096)
    ap.add_argument("--nineq", type=int, default=6144)
    ap.add_argument("--steps", type=int, default=10)
    args = ap.parse_args()
    import torch
    from bench import make_qp_device
    from pyipm_amd.newton import NewtonCore
    dev = torch.device("cuda", 0)
    n, me, mi = args.nvar, args.neq, args.nineq
    qp = make_qp_device(n, me, mi, 0, dev)

    def one(core):
        core.stage_blocks(qp["d2L"], qp["Je"], qp["Ji"])
        core.stage_vectors(qp["df"], qp["ce"], qp["ci"], qp["s"], qp["lam"], mu=qp["mu"])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        core.step(0.0, 0.0)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    warm = NewtonCore(n, me, mi, device=0)           # tile lists, streams, the clocks: not what is measured
    for _ in range(2):
        one(warm)
    warm.close()
    core = NewtonCore(n, me, mi, device=0)
    first = one(core)
    ms = [one(core) for _ in range(args.steps)]
    out = {"workload": "restaged fused steps n=%d me=%d mi=%d" % (n, me, mi), "first_step_ms": first, "ms": ms,
           "median_ms": sorted(ms)[len(ms) // 2], "spread_ms": max(ms) - min(ms)}
    if hasattr(core, "reuse_info"):
        out["reuse_info"] = core.reuse_info()
    core.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
