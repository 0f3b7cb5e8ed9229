#!/usr/bin/env python
"""Time one L-BFGS search direction (include/pyipm_lbfgs.h) on one MI355X and check it.

    python tools/bench_lbfgs.py --n 262144 --me 1024 --mi 3072 --m 8

Inputs are synthetic and generated on the device (J ~ N(0,1)/sqrt(n), storage from random displacement pairs
of positive curvature).  The check is size-independent: the direction must satisfy H dz = g for
H = Z - U inv(M) U' (the matrix of pyipm.py:1036-1052), applied matrix-free with torch as the checker.
The CPU comparison (the reference's arithmetic, oracle/lbfgs_oracle.py) lives in bench.py --extras: tools do not touch oracle/.
Prints one JSON line.

    python tools/bench_lbfgs.py --update --n 262144 --memories 8,31

times the OTHER half of the mode, lbfgs_update (pyipm.py:1282-1371), as one accepted offer to a FULL device-resident pair store
(pyipm_pairs_offer, include/pyipm_newton.h) and, in the same process on the same inputs, as the torch body of
QPDeviceIPM.lbfgs_update without the store (two torch.cat, the products through rocBLAS, two .contiguous()).

    python tools/bench_lbfgs.py --refine --n 262144 --me 1024 --mi 3072 --m 8 --reps 20

times what works from the state a direction keeps (pyipm_qn_*, include/pyipm_newton.h), Jacobians staged once: one direction, one
K v, one kept-state solve, one adaptive refinement -- and, in the same process on the same inputs, K v through the two kernels
the fused pass over J replaces (k_tall_tn with one column + k_jvec: a second handle created with PYIPM_QN_TWO_PASS set), the
two alternating.  Kernel times come from a kernel trace of this command in a run of its own.

    python tools/bench_lbfgs.py --columns --n 262144 --me 1024 --mi 3072 --m 8 --reps 20

times one direction after restaging 128, 512 and p/2 columns of [Je | Ji] (pyipm_lbfgs_stage_jacobian_columns; tile-aligned and
unaligned first columns, 128 columns once in Je and once in Ji), beside a direction after a full stage_jacobian, one that reuses
J'J and one after restaging every column; per leg the restaging copy, the direction, its Gram launch, the tiles it computed and
the launch's flop count.

    python tools/bench_lbfgs.py --many 8,64 --n 262144 --me 1024 --mi 3072 --m 8 --reps 10

times the many-column entries (pyipm_lbfgs_kkt_matvec_many / _solve_many) at each k against k calls of pyipm_qn_matvec /
pyipm_qn_solve on the same handle, the legs alternating; with the flops 4 n p k of the two products with J over the call time as a
share of the measured fp64 MFMA peak and the bytes of the staged J a call moves (profiles/qn_many_ab.json).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def storage(n, m, seed, constrained=True):
    """(zeta, S, Y, SS, L, D) with the invariants of lbfgs_update (pyipm.py:1282-1371): SS = S'S, L = strictly
    lower S'Y for constrained problems; SS = Y'Y, L = upper-triangular S'Y for unconstrained ones."""
    rng = np.random.default_rng(seed)
    S = rng.standard_normal((n, m)) / np.sqrt(n)
    Mq = rng.standard_normal((n, 16)) / 4.0
    Y = Mq @ (Mq.T @ S) + 0.5 * S                       # dg = Q dx, Q SPD
    SY = S.T @ Y
    D = np.diag(np.diag(SY))
    if constrained:
        SS, L = S.T @ S, np.tril(SY, -1)
        zeta = float(SY[-1, -1] / SS[-1, -1]) if m else 1.0
    else:
        SS, L = Y.T @ Y, np.triu(SY)
        zeta = float(SY[-1, -1] / SS[-1, -1]) if m else 1.0
    return zeta, S, Y, SS, L, D


HBM_PEAK_BPS = 8.0e12          # MI355X HBM3E, specification peak: what "fraction of the read floor" is taken against


def torch_update(torch, memory, con, eps, x_old, x_new, g_old, g_new, zeta, S, Y, SS, L, D, fail):
    """The body of QPDeviceIPM.lbfgs_update with the torch storage, as it stands (pyipm_amd/qp.py)."""
    from pyipm_amd.loop import lbfgs_pair_update
    t, n = torch, x_old.numel()
    dx = x_new - x_old
    dg = g_old[:n] - g_new[:n]
    drop = S.shape[1] > memory
    Sn = t.cat([S[:, 1:] if drop else S, dx[:, None]], dim=1)
    Yn = t.cat([Y[:, 1:] if drop else Y, dg[:, None]], dim=1)
    prods = t.cat([Sn.t() @ dx if con else Yn.t() @ dg, dx @ Yn if con else Sn.t() @ dg,
                   t.stack([t.dot(dg, dx), t.dot(dx, dx) if con else t.dot(dg, dg)])]).tolist()
    kk = Sn.shape[1]
    accepted, reset, zeta, SS, L, D, fail = lbfgs_pair_update(
        zeta, SS, L, D, fail, drop, np.array(prods[:kk]), np.array(prods[kk:2 * kk]), prods[-2], prods[-1], con, memory, eps)
    if accepted:
        S, Y = Sn.contiguous(), Yn.contiguous()
    assert accepted and not reset
    return zeta, S, Y, SS, L, D, fail


def update_leg(a):
    """One accepted offer on a full store, store against torch storage, per memory depth."""
    import torch
    from pyipm_amd.lbfgs import PairStore
    n, eps, con = a.n, float(np.finfo(np.float64).eps), True
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev); gen.manual_seed(3)
    rnd = lambda *shape: torch.randn(shape, generator=gen, dtype=torch.float64, device=dev)      # noqa: E731
    Mq = rnd(n, 16) / 4.0
    hv = lambda v: Mq @ (Mq.T @ v) + 0.5 * v                                                      # noqa: E731
    rows = []
    for memory in [int(k) for k in a.memories.split(",")]:
        xs = [rnd(n)]
        for _ in range(memory + 1 + a.reps + 1):
            xs.append(xs[-1] + rnd(n) / np.sqrt(n))
        gs = [torch.cat([-hv(x), rnd(5)]) for x in xs]                # g is longer than n, as the loop passes it
        store = PairStore(n, memory, con, device=0)
        state = (1.0, torch.zeros((n, 0), dtype=torch.float64, device=dev), torch.zeros((n, 0), dtype=torch.float64, device=dev),
                 np.zeros((0, 0)), np.zeros((0, 0)), np.zeros((0, 0)), 0)
        t_store, t_torch = [], []
        for k in range(len(xs) - 1):
            args = (xs[k], xs[k + 1], gs[k], gs[k + 1])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            assert store.offer(*args, eps) == 1
            torch.cuda.synchronize()                                 # (the append of the accepted pair is left in flight)
            t1 = time.perf_counter()
            state = torch_update(torch, memory, con, eps, *args, *state)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if k > memory + 1:                                       # full store, first full offer taken as warm-up
                t_store.append((t1 - t0) * 1e3); t_torch.append((t2 - t1) * 1e3)
        zeta, S, Y, SS, L, D, _ = store.view()
        assert S.shape[1] == state[1].shape[1] == memory + 1 and torch.equal(S, state[1]) and torch.equal(Y, state[2])
        floor_bytes = (2 * n * memory + 4 * n) * 8                   # the kept columns (the oldest one leaves) + x_old, x_new, g_old, g_new
        ms = float(np.median(t_store))
        rows.append({"memory": memory, "stored_pairs": memory + 1, "offer_ms": ms, "torch_update_ms": float(np.median(t_torch)),
                     "offer_ms_all": t_store, "torch_update_ms_all": t_torch, "read_floor_bytes": floor_bytes,
                     "fraction_of_read_floor": floor_bytes / HBM_PEAK_BPS / (ms * 1e-3),
                     "zeta_rel_diff": abs(zeta - state[0]) / abs(state[0]),
                     "SS_rel_diff": float(np.abs(SS - state[3]).max() / np.abs(state[3]).max())})
        store.close()
    print(json.dumps({"workload": "L-BFGS update (pyipm.py:1282-1371): one accepted offer on a full store, constrained", "n": n,
                      "dtype": "f64", "hbm_peak_Bps": HBM_PEAK_BPS, "timing": "wall, device synchronised before and after, median of %d" % a.reps,
                      "update": rows}))


def refine_leg(a):
    import torch
    from pyipm_amd.lbfgs import LbfgsCore
    n, me, mi, m = a.n, a.me, a.mi, a.m
    p, N = me + mi, n + 2 * mi + me
    p_pad = (p + 127) // 128 * 128
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev); gen.manual_seed(0)
    J = torch.randn((n, p), generator=gen, dtype=torch.float64, device=dev) / np.sqrt(n)
    zeta, S, Y, SS, L, D = storage(n, m, 1, True)
    rng = np.random.default_rng(2)
    s = rng.uniform(0.5, 2.0, mi)
    sig = np.exp(rng.uniform(np.log(10.0 ** -a.sigma_decades), np.log(10.0 ** a.sigma_decades), mi))   # the late-iteration spread
    lda = np.concatenate([rng.standard_normal(me), sig * s])
    td = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)          # noqa: E731
    gd, sd, ld, Sd, Yd, vd = td(rng.standard_normal(N)), td(s), td(lda), td(S), td(Y), td(rng.standard_normal(N))
    cores = {}
    for name, env in (("fused", None), ("two_kernels", "1")):
        if env:
            os.environ["PYIPM_QN_TWO_PASS"] = env
        cores[name] = LbfgsCore(n, me, mi, max(m, 1), device=0)
        os.environ.pop("PYIPM_QN_TWO_PASS", None)
        cores[name].stage_jacobian(J[:, :me] if me else None, J[:, me:] if mi else None)
    direct = lambda c: c.direction(gd, sd, ld, zeta, Sd, Yd, SS, L, D, reg=1e-12)      # noqa: E731
    dz = {k: direct(c)[0] for k, c in cores.items()}
    assert torch.equal(dz["fused"], dz["two_kernels"])
    core = cores["fused"]

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    legs = {"direction_ms": lambda: direct(core), "matvec_ms": lambda: core.matvec(vd),
            "matvec_two_kernels_ms": lambda: cores["two_kernels"].matvec(vd), "solve_ms": lambda: core.solve(gd),
            "refine_adaptive_ms": lambda: core.refine(dz["fused"], refine=-1)}
    rec = {k: [] for k in legs}
    for it in range(a.reps + 2):                     # two warm-up rounds; the legs alternate inside a round
        for k, fn in legs.items():
            ms, out = wall(fn)
            if it >= 2:
                rec[k].append(ms)
    kv = {k: c.matvec(vd) for k, c in cores.items()}
    _, info = core.refine(dz["fused"], refine=-1)
    launches = core.last_timings()["gram_launches"]
    jbytes = n * p_pad * 8
    med = {k: float(np.median(v)) for k, v in rec.items()}
    print(json.dumps({"workload": "quasi-Newton KKT operator of an L-BFGS direction (pyipm_qn_*), QP-shaped synthetic, Jacobians staged once",
                      "n": n, "me": me, "mi": mi, "m": m, "sigma_decades": a.sigma_decades, "dtype": "f64",
                      "timing": "wall, device synchronised before and after, median of %d, legs alternating" % a.reps,
                      "ms": med, "ms_all": rec, "refine_info": info, "gram_launches": launches,
                      "matvec_fused_vs_two_kernels_rel_diff": float((kv["fused"] - kv["two_kernels"]).norm() / kv["fused"].norm()),
                      "jacobian_bytes_padded": jbytes, "hbm_peak_Bps": HBM_PEAK_BPS,
                      "matvec_call_fraction_of_one_read_floor": jbytes / HBM_PEAK_BPS / (med["matvec_ms"] * 1e-3),
                      "matvec_two_kernels_call_fraction_of_two_read_floor": 2 * jbytes / HBM_PEAK_BPS / (med["matvec_two_kernels_ms"] * 1e-3)}))


MFMA_F64_VENDOR_TFLOPS = 78.6   # MI355X fp64 matrix peak, specification


def many_leg(a):
    """pyipm_lbfgs_kkt_matvec_many / _solve_many at k columns against k calls of pyipm_qn_matvec / pyipm_qn_solve on the same
    handle (the yardstick: the single-column entries are what every earlier commit has), legs alternating inside a round."""
    import torch
    from pyipm_amd.lbfgs import LbfgsCore
    from pyipm_amd.newton import mfma_f64_peak
    n, me, mi, m = a.n, a.me, a.mi, a.m
    p, N = me + mi, n + 2 * mi + me
    p_pad = (p + 127) // 128 * 128
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev); gen.manual_seed(0)
    J = torch.randn((n, p), generator=gen, dtype=torch.float64, device=dev) / np.sqrt(n)
    zeta, S, Y, SS, L, D = storage(n, m, 1, True)
    rng = np.random.default_rng(2)
    s = rng.uniform(0.5, 2.0, mi)
    lda = np.concatenate([rng.standard_normal(me), rng.uniform(0.5, 2.0, mi)])
    td = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)          # noqa: E731
    gd, sd, ld, Sd, Yd = td(rng.standard_normal(N)), td(s), td(lda), td(S), td(Y)
    core = LbfgsCore(n, me, mi, max(m, 1), device=0)
    core.stage_jacobian(J[:, :me] if me else None, J[:, me:] if mi else None)
    del J
    core.direction(gd, sd, ld, zeta, Sd, Yd, SS, L, D, reg=1e-12)
    peak = mfma_f64_peak(0)
    rows = []
    for k in [int(x) for x in a.many.split(",")]:
        V = torch.randn((k, N), generator=gen, dtype=torch.float64, device=dev)          # (k, N): column j at V[j]
        legs = {"matvec_many_ms": lambda: core.matvec_many(V.t()), "matvec_k_calls_ms": lambda: [core.matvec(V[j]) for j in range(k)],
                "solve_many_ms": lambda: core.solve_many(V.t()), "solve_k_calls_ms": lambda: [core.solve(V[j]) for j in range(k)]}
        rec = {name: [] for name in legs}
        for it in range(a.reps + 2):                 # two warm-up rounds; the legs alternate inside a round
            for name, fn in legs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if it >= 2:
                    rec[name].append((time.perf_counter() - t0) * 1e3)
        diff = {"matvec": float(max((core.matvec_many(V.t())[:, j] - core.matvec(V[j])).norm() / core.matvec(V[j]).norm() for j in (0, k - 1))),
                "solve": float(max((core.solve_many(V.t())[:, j] - core.solve(V[j])).norm() / core.solve(V[j]).norm() for j in (0, k - 1)))}
        med = {name: float(np.median(v)) for name, v in rec.items()}
        spread = {name: float(max(v) - min(v)) for name, v in rec.items()}
        flops = 4.0 * n * p * k                      # the two products with J
        blocks = (k + 63) // 64
        rows.append({"k": k, "ms": med, "ms_spread_max_minus_min": spread, "ms_all": rec,
                     "matvec_speedup": med["matvec_k_calls_ms"] / med["matvec_many_ms"],
                     "solve_speedup": med["solve_k_calls_ms"] / med["solve_many_ms"],
                     "faster_by_more_than_the_yardsticks_spread": {
                         "matvec": med["matvec_k_calls_ms"] - med["matvec_many_ms"] > spread["matvec_k_calls_ms"],
                         "solve": med["solve_k_calls_ms"] - med["solve_many_ms"] > spread["solve_k_calls_ms"]},
                     "many_vs_single_rel_diff_first_and_last_column": diff,
                     "product_flops_4npk": flops, "jacobian_bytes_moved_per_call": 2 * 8 * n * p_pad * blocks,
                     "matvec_many_call_tflops_on_4npk": flops / (med["matvec_many_ms"] * 1e-3) / 1e12,
                     "matvec_many_call_share_of_measured_mfma_peak": flops / (med["matvec_many_ms"] * 1e-3) / 1e12 / peak,
                     "solve_many_call_share_of_measured_mfma_peak": flops / (med["solve_many_ms"] * 1e-3) / 1e12 / peak,
                     "matvec_many_call_jacobian_TBps": 2 * 8 * n * p_pad * blocks / (med["matvec_many_ms"] * 1e-3) / 1e12})
    print(json.dumps({"workload": "quasi-Newton KKT operator for k columns per call (pyipm_lbfgs_kkt_*_many) against k single-column "
                                  "calls (pyipm_qn_matvec / pyipm_qn_solve), QP-shaped synthetic, Jacobians staged once",
                      "n": n, "me": me, "mi": mi, "m": m, "dtype": "f64",
                      "timing": "wall, device synchronised before and after, median of %d, legs alternating; whole-call rates, not "
                                "kernel rates" % a.reps,
                      "mfma_f64_peak_measured_tflops": peak, "mfma_f64_peak_vendor_tflops": MFMA_F64_VENDOR_TFLOPS,
                      "hbm_peak_Bps": HBM_PEAK_BPS, "gram_launches": core.last_timings()["gram_launches"], "many": rows}))


def columns_leg(a):
    """One direction after restaging a run of columns (pyipm_lbfgs_stage_jacobian_columns), beside one after a full
    stage_jacobian (the yardstick: that path is the one every earlier commit has) and one that reuses J'J."""
    import torch
    from pyipm_amd.lbfgs import LbfgsCore
    n, me, mi, m = a.n, a.me, a.mi, a.m
    p, N = me + mi, n + 2 * mi + me
    p_pad = (p + 127) // 128 * 128
    nt = p_pad // 128
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev); gen.manual_seed(0)
    J = torch.randn((n, p), generator=gen, dtype=torch.float64, device=dev) / np.sqrt(n)
    zeta, S, Y, SS, L, D = storage(n, m, 1, True)
    rng = np.random.default_rng(2)
    s = rng.uniform(0.5, 2.0, mi)
    lda = np.concatenate([rng.standard_normal(me), rng.uniform(0.5, 2.0, mi)])
    td = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)          # noqa: E731
    gd, sd, ld, Sd, Yd = td(rng.standard_normal(N)), td(s), td(lda), td(S), td(Y)
    core = LbfgsCore(n, me, mi, max(m, 1), device=0)
    full = lambda: core.stage_jacobian(J[:, :me] if me else None, J[:, me:] if mi else None)      # noqa: E731
    full()
    half = p_pad // 2
    # (name, c0, count): c0 = None -> a full stage_jacobian, count = 0 -> nothing staged.  The sizes are for p = 4096, me = 1024.
    legs = [("full_stage", None, p), ("reuse", 0, 0),
            ("c128_aligned_Je", 128, 128), ("c128_aligned_Ji", (me + 127) // 128 * 128 + 128, 128), ("c128_unaligned", 200, 128),
            ("c512_aligned", 1024, 512), ("c512_unaligned", 1100, 512),
            ("c%d_aligned" % half, 1024, half), ("c%d_unaligned" % half, 1100, half),
            ("all_columns", 0, p)]
    legs = [g for g in legs if g[1] is None or g[1] + g[2] <= p]

    def dirty_tiles(c0, count):
        if c0 is None:
            return nt * (nt + 1) // 2
        if count == 0:
            return 0
        clean = nt - ((c0 + count - 1) // 128 - c0 // 128 + 1)
        return nt * (nt + 1) // 2 - clean * (clean + 1) // 2

    rec = {g[0]: [] for g in legs}
    for it in range(a.reps + 2):                     # two warm-up rounds; the legs alternate inside a round
        for name, c0, count in legs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if c0 is None:
                full()
            elif count:
                core.stage_jacobian_columns(c0, J[:, c0:c0 + count])         # a row-strided view: copied as it is
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            core.direction(gd, sd, ld, zeta, Sd, Yd, SS, L, D, reg=1e-12)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if it >= 2:
                tm = core.last_timings()
                tm["stage_ms"], tm["wall_ms"] = (t1 - t0) * 1e3, (t2 - t1) * 1e3
                rec[name].append(tm)
    out = []
    for name, c0, count in legs:
        r = rec[name]
        med = {k: float(np.median([x[k] for x in r])) for k in ("stage_ms", "wall_ms", "total_ms", "gram_ms", "factor_ms")}
        launched = name != "reuse"
        med.update(leg=name, c0=c0, columns=count, dirty_tiles=dirty_tiles(c0, count), tiles=nt * (nt + 1) // 2,
                   gram_flops=r[-1]["gram_flops"] if launched else 0.0,
                   gram_tflops=r[-1]["gram_flops"] / (med["gram_ms"] * 1e-3) / 1e12 if launched and med["gram_ms"] > 0 else None,
                   wall_ms_all=[x["wall_ms"] for x in r], gram_ms_all=[x["gram_ms"] for x in r])
        if launched:
            assert r[-1]["gram_flops"] == 2.0 * 128 * 128 * ((n + 8191) // 8192 * 8192) * med["dirty_tiles"], name
        out.append(med)
    print(json.dumps({"workload": "L-BFGS direction after a partial restaging of the Jacobians, QP-shaped synthetic", "n": n, "me": me,
                      "mi": mi, "m": m, "dtype": "f64", "jacobian_bytes_padded": n * p_pad * 8, "hbm_peak_Bps": HBM_PEAK_BPS,
                      "timing": "wall, device synchronised before and after, median of %d, legs alternating; gram_ms from the "
                                "library's events" % a.reps,
                      "gram_launches": core.last_timings()["gram_launches"], "legs": out}))


def bounds_leg(a):
    """A direction on a bounded handle (simple bounds eliminated in closed form, pyipm_lbfgs_bounded_*): a box on every variable,
    mb = 2 n, beside the yardstick in the same process -- the plain handle's direction right after a full staging of the same J
    without bounds -- and the bounds-only handle (me = mg = 0: no Gram launch at all) against the read floor of V."""
    import torch
    from pyipm_amd.lbfgs import LbfgsCore
    n, me, mg, m = a.n, a.me, a.mi, a.m
    p, mb = me + mg, 2 * a.n
    mi = mg + mb
    N = n + 2 * mi + me
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev); gen.manual_seed(0)
    J = torch.randn((n, p), generator=gen, dtype=torch.float64, device=dev) / np.sqrt(n)
    zeta, S, Y, SS, L, D = storage(n, m, 1, True)
    rng = np.random.default_rng(2)
    s = rng.uniform(0.5, 2.0, mi)
    lda = np.concatenate([rng.standard_normal(me), rng.uniform(0.5, 2.0, mi)])
    g = rng.standard_normal(N)
    var = np.concatenate([np.arange(n), np.arange(n)])
    sign = np.concatenate([np.ones(n), -np.ones(n)])
    td = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)          # noqa: E731
    Sd, Yd = td(S), td(Y)
    gen_rows = np.concatenate([np.arange(n + mg), n + mi + np.arange(me + mg)])                 # the rows without the bounds
    only_rows = np.concatenate([np.arange(n), n + mg + np.arange(mb), n + mi + me + mg + np.arange(mb)])

    def run(core, gv, sv, lv, restage):
        gd, sd, ld = td(gv), td(sv), td(lv)
        rec = []
        for it in range(a.reps + 2):
            if restage:
                core.stage_jacobian(J[:, :me] if me else None, J[:, me:] if mg else None)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = core.direction(gd, sd, ld, zeta, Sd, Yd, SS, L, D, reg=1e-12)
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) * 1e3
            if it >= 2:
                tm = core.last_timings(); tm["wall_ms"] = wall
                rec.append(tm)
        med = {k: float(np.median([r[k] for r in rec])) for k in rec[0]}
        med["wall_ms_all"] = [r["wall_ms"] for r in rec]
        return out[0], med

    legs = {}
    plain = LbfgsCore(n, me, mg, max(m, 1), device=0)
    _, legs["plain_full_stage"] = run(plain, g[gen_rows], s[:mg], lda[:p], True)
    plain.close()
    bounded = LbfgsCore(n, me, mg, max(m, 1), device=0, bounds=(var, sign))
    bounded.stage_jacobian(J[:, :me] if me else None, J[:, me:] if mg else None)
    dz, legs["bounded"] = run(bounded, g, s, lda, False)
    bounded.close()
    # ---- checker: K dz = g with the bound columns applied by index, matrix-free
    gd, sd, ld, vd, sgd = td(g), td(s), td(lda), td(var), td(sign)
    x, ds, dl = dz[:n], dz[n:n + mi], dz[n + mi:]
    W = torch.cat([zeta * Sd, Yd], dim=1)
    Minv = td(np.block([[zeta * SS, L], [L.T, -D]]))
    top = zeta * x - W @ torch.linalg.solve(Minv, W.T @ x) if m else zeta * x
    top = top + J @ dl[:p]
    top.index_add_(0, vd, sgd * dl[p:])
    res = torch.empty_like(dz)
    res[:n] = top
    res[n:n + mi] = ld[me:] / (sd + np.finfo(float).eps) * ds - dl[me:]
    low = torch.cat([J.T @ x, sgd * x[vd]])
    low[me:] -= ds
    res[n + mi:] = low
    check = float((res - gd).norm() / gd.norm())
    del J
    only = LbfgsCore(n, 0, 0, max(m, 1), device=0, bounds=(var, sign))
    _, legs["bounds_only"] = run(only, g[only_rows], s[mg:], lda[p:], False)
    only.close()
    p_pad = (p + 127) // 128 * 128
    print(json.dumps({"workload": "L-BFGS direction with a box on every variable as structure, QP-shaped synthetic", "n": n, "me": me,
                      "mg": mg, "mb": mb, "m": m, "dtype": "f64", "explicit_order_would_be": p + mb,
                      "scale_pass_bytes": 2 * n * p_pad * 8, "v_bytes": n * (2 * m + 1) * 8, "hbm_peak_Bps": HBM_PEAK_BPS,
                      "timing": "wall, device synchronised before and after, median of %d; gram_ms from the library's events" % a.reps,
                      "residual_K_dz_minus_g_rel": check, "legs": legs}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=262144)
    ap.add_argument("--me", type=int, default=1024)
    ap.add_argument("--mi", type=int, default=3072)
    ap.add_argument("--m", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu-n", type=int, default=0, help="ignored (kept for old command lines): the CPU leg is bench.py --extras")
    ap.add_argument("--update", action="store_true", help="time lbfgs_update (pair store against torch storage) instead of the direction")
    ap.add_argument("--memories", default="8,31", help="--update: memory depths, comma-separated")
    ap.add_argument("--refine", action="store_true", help="time K v, the kept-state solve and the refinement of a direction (pyipm_qn_*)")
    ap.add_argument("--sigma-decades", type=float, default=6.0, help="--refine: Sigma spread, decades either side of 1")
    ap.add_argument("--columns", action="store_true", help="time a direction after restaging 128, 512 and p/2 columns (stage_jacobian_columns)")
    ap.add_argument("--many", default="", metavar="K", help="time pyipm_lbfgs_kkt_matvec_many / _solve_many at k = K (a comma-separated "
                    "list: one handle, one process) against K calls of the single-column entries")
    ap.add_argument("--bounds", action="store_true", help="time a direction with a box on every variable on a bounded handle "
                    "(pyipm_lbfgs_bounded_*), the plain handle after a full staging beside it, and the bounds-only handle")
    a = ap.parse_args()
    if a.bounds:
        return bounds_leg(a)
    if a.many:
        return many_leg(a)
    if a.columns:
        return columns_leg(a)
    if a.update:
        return update_leg(a)
    if a.refine:
        return refine_leg(a)
    import torch
    from pyipm_amd.lbfgs import LbfgsCore
    n, me, mi, m = a.n, a.me, a.mi, a.m
    p, N = me + mi, n + 2 * mi + me
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev); gen.manual_seed(0)
    J = torch.randn((n, p), generator=gen, dtype=torch.float64, device=dev) / np.sqrt(n) if p else None
    zeta, S, Y, SS, L, D = storage(n, m, 1, bool(p))
    rng = np.random.default_rng(2)
    s = rng.uniform(0.5, 2.0, mi)
    lda = np.concatenate([rng.standard_normal(me), rng.uniform(0.5, 2.0, mi)])
    g = rng.standard_normal(N)
    core = LbfgsCore(n, me, mi, max(m, 1), device=0)
    t0 = time.perf_counter()
    if p:
        core.stage_jacobian(J[:, :me] if me else None, J[:, me:] if mi else None)
    torch.cuda.synchronize()
    t_stage = time.perf_counter() - t0
    td = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)          # noqa: E731
    gd, sd, ld, Sd, Yd = td(g), td(s), td(lda), td(S), td(Y)
    def timed(restage):
        rec = []
        for it in range(a.reps + 1):
            if restage and p:                        # a changed Jacobian: J'J is recomputed by the next direction
                core.stage_jacobian(J[:, :me] if me else None, J[:, me:] if mi else None)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = core.direction(gd, sd, ld, zeta, Sd, Yd, SS, L, D, reg=1e-12)
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) * 1e3
            if it:
                tm = core.last_timings(); tm["wall_ms"] = wall
                rec.append(tm)
        return out, {k: float(np.median([r[k] for r in rec])) for k in rec[0]}

    (dz, st), med = timed(True)
    reuse = timed(False)[1] if p else None           # linear constraints: J'J of the staged Jacobians is reused
    # ---- checker: H dz = g, matrix-free (constrained); dz = Hinv g recomputed with torch (unconstrained)
    x, ds, dl = dz[:n], dz[n:n + mi], dz[n + mi:]
    res = torch.empty_like(dz)
    if not p:
        W = torch.cat([Sd, zeta * Yd], dim=1)
        Ld, DS = td(L), td(D + zeta * SS)
        t = W.T @ gd
        Bc = -torch.linalg.solve(Ld, t[:m])
        Ac = -torch.linalg.solve(Ld.T, DS @ Bc) - torch.linalg.solve(Ld.T, t[m:])
        ref = zeta * gd + W @ torch.cat([Ac, Bc]) if m else zeta * gd
        top = gd + (ref - dz)                       # so that res - g = ref - dz
    else:
        W = torch.cat([zeta * Sd, Yd], dim=1)
        Minv = td(np.block([[zeta * SS, L], [L.T, -D]]))
        top = zeta * x - W @ torch.linalg.solve(Minv, W.T @ x) if m else zeta * x
    if p:
        top = top + J @ dl
        sig = ld[me:] / (sd + np.finfo(float).eps)
        res[n:n + mi] = sig * ds - dl[me:]
        low = J.T @ x
        low[me:] -= ds
        res[n + mi:] = low
    res[:n] = top
    check = float((res - gd).norm() / gd.norm())
    rr = 2 * m + 1
    chunks = (rr + 16) // 17
    out = {"workload": "L-BFGS direction (pyipm.py:1184-1246), QP-shaped synthetic", "n": n, "me": me, "mi": mi,
           "m": m, "dtype": "f64", "ms": med, "ms_reusing_gram": reuse, "stage_jacobian_ms": t_stage * 1e3, "stats": st,
           "residual_H_dz_minus_g_rel": check}
    if p:
        out["gram_tflops"] = med["gram_flops"] / (med["gram_ms"] * 1e-3) / 1e12 if med["gram_ms"] > 0 else None
        out["jacobian_pass_GBps"] = (chunks + 1) * n * ((p + 127) // 128 * 128) * 8 / (med["jacobian_passes_ms"] * 1e-3) / 1e9
        out["jacobian_bytes"] = n * p * 8
    print(json.dumps(out))


if __name__ == "__main__":
    main()
