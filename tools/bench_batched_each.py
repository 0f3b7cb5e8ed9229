#!/usr/bin/env python
"""Device-event timings of the batched handle's per-problem step on the config-5 shape (512 x (n, me, mi) = (256, 0, 256)),
both forms, warmed, the variants alternating in one process:

  (a) the scalar step (pyipm_newton_step_batched) of this library -- and, with --baseline-lib, of another build of it
      (an older one: only entry points both have are called), alternating with it;
  (b) a retry pass of pyipm_newton_step_batched_each with --active of the problems active, against the full step;
  (c) pyipm_newton_step_lengths_batched alone.

Prints one JSON line.  Every figure is the median over --rounds windows of --steps calls, with the min and max window
beside it (the spread of that same run).

    python tools/bench_batched_each.py [--baseline-lib PATH] [--batch 512] [--rounds 9] [--steps 20]"""
import argparse
import ctypes
import json
import os
import sys
from ctypes import POINTER, c_double, c_int, c_int64, c_size_t, c_void_p

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


class RawBatched(object):
    """A batched handle through plain ctypes, on the entry points every build of the library has."""

    def __init__(self, path, n, me, mi, B, torch, condensed):
        self.torch, self.B, self.N = torch, B, n + 2 * mi + me
        lib = self.lib = ctypes.CDLL(path)
        lib.pyipm_newton_workspace_bytes_batched.restype = c_size_t
        lib.pyipm_newton_workspace_bytes_batched.argtypes = [c_int64, c_int64, c_int64, c_int]
        lib.pyipm_newton_create_batched.argtypes = [POINTER(c_void_p), c_int64, c_int64, c_int64, c_int, c_int, c_void_p, c_size_t, c_void_p]
        lib.pyipm_newton_stage_blocks_batched.argtypes = [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64]
        lib.pyipm_newton_stage_vectors.argtypes = [c_void_p] + [c_void_p] * 5 + [c_double, c_double, c_int]
        lib.pyipm_newton_step_batched.argtypes = [c_void_p, c_double, c_double, c_void_p, c_void_p, c_int]
        lib.pyipm_newton_set_option.argtypes = [c_void_p, ctypes.c_char_p, c_double]
        lib.pyipm_newton_destroy.argtypes = [c_void_p]
        need = lib.pyipm_newton_workspace_bytes_batched(n, me, mi, B)
        self.ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        self.h = c_void_p()
        self.ck(lib.pyipm_newton_create_batched(ctypes.byref(self.h), n, me, mi, B, torch.cuda.current_device(),
                                                c_void_p(self.ws.data_ptr()), need, c_void_p(torch.cuda.current_stream().cuda_stream)))
        if condensed:
            self.ck(lib.pyipm_newton_set_option(self.h, b"condensed", 1.0))
        self.out = torch.empty((B, self.N), dtype=torch.float64, device="cuda")

    def ck(self, rc):
        if rc:
            raise RuntimeError("library call failed: %d" % rc)

    def stage(self, Q, Ji, c, ci, s, lam, n, mi):
        p = lambda t: c_void_p(t.data_ptr())           # noqa: E731
        self.ck(self.lib.pyipm_newton_stage_blocks_batched(self.h, p(Q), n, n * n, None, 0, 0, p(Ji), mi, n * mi))
        self.ck(self.lib.pyipm_newton_stage_vectors(self.h, p(c), None, p(ci), p(s), p(lam), 0.2, float(np.finfo(float).eps), 0))

    def step(self):
        self.ck(self.lib.pyipm_newton_step_batched(self.h, 0.0, 0.0, c_void_p(self.out.data_ptr()), None, 0))

    def close(self):
        self.lib.pyipm_newton_destroy(self.h)


def windows(torch, fns, rounds, steps):
    """ms per call of every function of `fns`, alternating between them window by window: {name: [ms per round]}."""
    res = {k: [] for k in fns}
    for k, f in fns.items():                           # warm-up
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                f()
            e1.record()
            e1.synchronize()
            res[k].append(e0.elapsed_time(e1) / steps)
    return res


def summary(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--active", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    import torch
    from pyipm_amd import newton
    from pyipm_amd.batched import BatchedNewton
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    n, me, mi, B = 256, 0, 256, a.batch
    gen = torch.Generator(device="cuda").manual_seed(5)
    f64, dev = torch.float64, "cuda"
    M = torch.randn(B, n, n, dtype=f64, device=dev, generator=gen)
    Q = M @ M.transpose(1, 2) / n + torch.eye(n, dtype=f64, device=dev)
    Ji = (torch.randn(B, mi, n, dtype=f64, device=dev, generator=gen) / np.sqrt(n)).transpose(1, 2).contiguous()
    c = torch.randn(B, n, dtype=f64, device=dev, generator=gen)
    s = torch.rand(B, mi, dtype=f64, device=dev, generator=gen) * 1.5 + 0.5
    lam = torch.rand(B, mi, dtype=f64, device=dev, generator=gen) * 1.5 + 0.5
    ci = s + 0.1 * torch.randn(B, mi, dtype=f64, device=dev, generator=gen)
    out = {"shape": [n, me, mi], "batch": B, "rounds": a.rounds, "steps": a.steps, "active": a.active}
    for form, condensed in (("full", False), ("condensed", True)):
        r = {}
        # (a) the scalar entry, this build against the baseline build
        libs = {"this": newton.LIB_PATH}
        if a.baseline_lib:
            libs = {"baseline": a.baseline_lib, "this": newton.LIB_PATH}
        hs = {k: RawBatched(p, n, me, mi, B, torch, condensed) for k, p in libs.items()}
        for h in hs.values():
            h.stage(Q, Ji, c, ci, s, lam, n, mi)
        res = windows(torch, {k: h.step for k, h in hs.items()}, a.rounds, a.steps)
        r["a_step_batched"] = {k: summary(v) for k, v in res.items()}
        if a.baseline_lib:
            r["a_same_bits"] = bool(torch.equal(hs["baseline"].out, hs["this"].out))
        for h in hs.values():
            h.close()
        # (b) a retry pass of few problems against the full step; (c) the step lengths
        bn = BatchedNewton(n, me, mi, condensed=condensed, guard=False)
        bn.stage(Q, None, Ji, c, None, ci, s, lam, mu=0.2)
        mu = torch.full((B,), 0.2, dtype=f64, device=dev)
        zero = torch.zeros(B, dtype=f64, device=dev)
        act = torch.zeros(B, dtype=torch.int32, device=dev)
        act[torch.arange(a.active, device=dev) * (B // a.active)] = 1
        dz, _ = bn.step_each(mu, zero, zero)
        res = windows(torch, {"all_active": lambda: bn.step_each(mu, zero, zero, None, out=dz),
                              "retry_pass": lambda: bn.step_each(mu, zero, zero, act, out=dz),
                              "step_lengths": lambda: bn.step_lengths_all(0.995, dz=dz)}, a.rounds, a.steps)
        r["b_step_each_all_active"] = summary(res["all_active"])
        r["b_retry_pass"] = summary(res["retry_pass"])
        r["c_step_lengths_all"] = summary(res["step_lengths"])
        bn.close()
        out[form] = r
    print(json.dumps(out))


if __name__ == "__main__":
    main()
