#!/usr/bin/env python
"""Which HIP resources one handle creates, when, and whether each one is released (profiles/owned_resources_ab.json).

  rocprofv3 --hip-trace --memory-allocation-trace --output-format csv -d DIR -- python tools/resource_trace.py run
  python tools/resource_trace.py summarise DIR [OTHER_DIR]

`run` drives the C-ABI with HOST pointers and a library-owned workspace, so every device allocation, event and stream of
the process is the library's own (torch is loaded for its HIP runtime and never touches the device): create, a
host-pointer step, factor + solve, solve_many, a condensed step, the merit and ray calls, rcond twice (cold, warm), destroy.
`summarise` prints, per trace, the ordered creations (memory, events, streams) up to the last release, the ordered sizes
of the allocation trace and the create / release balance; with two directories it also says whether the two agree."""
import csv, ctypes, glob, json, os, sys
from ctypes import c_double, c_void_p

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CREATE = ("hipMalloc", "hipHostMalloc", "hipEventCreate", "hipEventCreateWithFlags", "hipStreamCreateWithFlags",
          "hipStreamCreateWithPriority", "hipStreamCreate")
RELEASE = {"hipFree": "memory", "hipHostFree": "pinned", "hipEventDestroy": "event", "hipStreamDestroy": "stream"}
KIND = {"hipMalloc": "memory", "hipHostMalloc": "pinned", "hipEventCreate": "event", "hipEventCreateWithFlags": "event",
        "hipStreamCreateWithFlags": "stream", "hipStreamCreateWithPriority": "stream", "hipStreamCreate": "stream"}


def run():
    import numpy as np
    from pyipm_amd.newton import load_library, FactorStats, MEM_HOST
    from pyipm_amd.problems import make_qp
    lib = load_library()
    n, me, mi = 700, 200, 300
    N = n + 2 * mi + me
    qp = make_qp(n, me, mi, 8)
    f64 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float64))
    P = lambda a: c_void_p(a.ctypes.data)
    h = c_void_p()

    def ck(rc):
        if rc:
            raise RuntimeError("%d: %s" % (rc, lib.pyipm_newton_last_error(h).decode()))

    ck(lib.pyipm_newton_create(ctypes.byref(h), n, me, mi, 256, 0, 1, 0, None, 0, None))
    d2L, Je, Ji = f64(qp["d2L"]), f64(qp["Je"]), f64(qp["Ji"])
    vec = [f64(qp[k]) for k in ("df", "ce", "ci", "s", "lam")]
    ck(lib.pyipm_newton_stage_blocks(h, P(d2L), n, P(Je), me, P(Ji), mi, MEM_HOST))
    ck(lib.pyipm_newton_stage_vectors(h, *[P(v) for v in vec], float(qp["mu"]), float(np.finfo(np.float64).eps), MEM_HOST))
    dz, st = np.empty(N), FactorStats()
    ck(lib.pyipm_newton_step(h, 0.0, 0.0, 0, P(dz), ctypes.byref(st), MEM_HOST))            # host-pointer step
    g = np.empty(N)
    ck(lib.pyipm_newton_residual(h, P(g), MEM_HOST))
    ck(lib.pyipm_newton_assemble(h, 0.0, 0.0))
    ck(lib.pyipm_newton_factor(h, ctypes.byref(st)))
    ck(lib.pyipm_newton_solve(h, None, P(dz), 1, -1, MEM_HOST))                              # adaptive refinement
    B = f64(np.random.default_rng(0).standard_normal((5, N))); X = np.empty((5, N))
    ck(lib.pyipm_newton_solve_many(h, 5, P(B), N, P(X), N, 1, 1, MEM_HOST))
    out4 = (c_double * 4)()
    ck(lib.pyipm_newton_rcond(h, 0, 0, out4)); ck(lib.pyipm_newton_rcond(h, 0, 0, out4))     # cold, then warm
    out16 = (c_double * 16)()
    ck(lib.pyipm_newton_merit_info(h, None, out16))
    al, ray = (c_double * 3)(1.0, 0.5, 0.25), (c_double * 3)()
    ck(lib.pyipm_newton_merit_ray(h, None, 10.0, float(qp["mu"]), None, al, 3, ray))
    ck(lib.pyipm_newton_set_option(h, b"condensed", 1.0))
    ck(lib.pyipm_newton_step(h, 0.0, 0.0, 2, P(dz), ctypes.byref(st), MEM_HOST))            # condensed step
    ck(lib.pyipm_newton_destroy(h))
    print("resource_trace: ok, n_neg", st.n_neg, "checksum %.17g" % float(np.abs(dz).sum()))


def rows_of(d, pattern):
    """The rows of the rocprofv3 CSV files under d whose name ends in `pattern`, in start order."""
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*" + pattern), recursive=True):
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r.get("Start_Timestamp") or 0))
    return rows


def summarise(d):
    api = [r["Function"] for r in rows_of(d, "hip_api_trace.csv")]
    made, freed = {}, {}
    last_release = max([i for i, nm in enumerate(api) if nm in RELEASE], default=-1)
    for nm in api:
        if nm in CREATE:
            made[KIND[nm]] = made.get(KIND[nm], 0) + 1
        elif nm in RELEASE:
            freed[RELEASE[nm]] = freed.get(RELEASE[nm], 0) + 1
    # the allocation trace carries the sizes (the HIP API trace has no arguments); frees are its rows of size 0
    sizes = [int(r["Allocation_Size"]) for r in rows_of(d, "memory_allocation_trace.csv")
             if "ALLOC" in r.get("Operation", "").upper() and "FREE" not in r.get("Operation", "").upper()]
    return {"hip_api_records": len(api), "created": made, "released": freed,
            "balanced": all(made.get(k, 0) == freed.get(k, 0) for k in set(made) | set(freed)),
            "creation_order": [nm for nm in api[:last_release + 1] if nm in CREATE], "allocation_sizes": sizes}


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "run":
        run()
    elif len(sys.argv) >= 3 and sys.argv[1] == "summarise":
        res = [summarise(d) for d in sys.argv[2:]]
        if len(res) == 2:
            print(json.dumps({"same_creation_order": res[0]["creation_order"] == res[1]["creation_order"],
                              "same_allocation_sizes": res[0]["allocation_sizes"] == res[1]["allocation_sizes"]}))
        for d, r in zip(sys.argv[2:], res):
            print(d, json.dumps(r))
    else:
        sys.exit(__doc__)
