#!/usr/bin/env python
"""A/B helper for the distributed driver (csrc/dist_impl.hpp): per case and rank one line with a fingerprint of the Newton
direction, the factor statistics to 17 digits, the wire counters of pyipm_newton_dist_wire (all but the milliseconds), the bytes
and messages of dist_timings and comm_bcast_mode.  Gloo ranks sharing device 0, as tests/test_gpu_dist.py::_run_world starts
them.  Run it with two libraries (PYIPM_NEWTON_LIB) and diff the outputs: a change of the host driver that is meant to keep every
launch and every message where it was leaves them identical byte for byte.

usage: python tools/dist_ab.py [--only forms0,forms1,forms2,forms3,condensed,wide,world1]"""
import argparse
import ctypes
import hashlib
import os
import socket
import sys
os.environ.setdefault("PYIPM_EXPERT", "1")     # tools use expert switches (include/pyipm_newton.h)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FORM_SHAPES = [(2, (900, 200, 300, 8), 256), (3, (700, 150, 260, 9), 128), (4, (1500, 300, 500, 10), 256), (3, (2000, 400, 600, 12), 1024)]
P2P, NOP2P = {"p2p": True, "serialize": True, "selftest": True}, {"p2p": False}
FORMS = [("A", {"dist_sag_min_bytes": 8}, P2P), ("B", None, NOP2P),
         ("C", {"dist_slices": 0, "dist_sag_min_bytes": 8}, {"p2p": True, "serialize": False, "selftest": True}),
         ("D", {"dist_slices": 0}, NOP2P), ("E", {"dist_slices": 1}, NOP2P)]
COND_SHAPES = [(2, (900, 200, 300, 8), 256), (3, (700, 150, 260, 9), 128), (2, (1400, 0, 400, 10), 128)]
WIDE_SHAPES = [(2, (1300, 300, 450, 11), 512), (3, (4480, 920, 1344, 12), 1024)]       # one message per panel: the wide classic head


def cases(only):
    out = []
    for i, (world, shape, nb) in enumerate(FORM_SHAPES):
        if "forms%d" % i in only:
            out += [("form %s" % name, world, shape, nb, opts, kw, "native-sharded") for name, opts, kw in FORMS]
    if "condensed" in only:
        out += [("condensed", world, shape, nb, {"condensed": 1}, None, "native") for world, shape, nb in COND_SHAPES]
    if "wide" in only:
        out += [("wide head", world, shape, nb, {"dist_slices": 0}, None, "native") for world, shape, nb in WIDE_SHAPES]
    if "world1" in only:
        out.append(("selfmsg", 1, (700, 200, 300, 8), 256, {"dist_selfmsg": 1}, None, "native"))
    return out


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, shape, nb, opts, drv_kw, mode, out):
    import torch.distributed as dist
    from pyipm_amd.dist import DistNewton
    from pyipm_amd.newton import NewtonCore
    from pyipm_amd.problems import make_qp
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        n, me, mi, seed = shape
        qp = make_qp(n, me, mi, seed)
        core = NewtonCore(n, me, mi, device=0, nb=nb, world=world, rank=rank)
        for k, v in (opts or {}).items():
            core.set_option(k, v)
        if mode == "native-sharded":                    # a rank stages only the rows of the x-columns it owns
            rows = core.owned_rows()
            core.stage_blocks_owned(qp["d2L"][rows], qp["Je"][rows] if me else None, qp["Ji"][rows] if mi else None)
        else:
            core.stage_blocks(qp["d2L"], qp["Je"], qp["Ji"])
        core.stage_vectors(qp["df"], qp["ce"], qp["ci"], qp["s"], qp["lam"], mu=qp["mu"])
        dz, st = DistNewton(core, native=True, **(drv_kw or {})).step(0.0, 0.0)
        wire = (ctypes.c_double * 12)()
        core.lib.pyipm_newton_dist_wire(core.h, wire)
        tm = core.dist_timings()
        out[rank] = "%s | %d %d %d %d %d %.17g %.17g %.17g | wire %s | %d bytes %d messages | bcast_mode %d" % (
            hashlib.sha1(dz.cpu().numpy().tobytes()).hexdigest(), st["n_neg"], st["n_zero"], st["n_2x2"], st["n_pos"], st["nonfinite"],
            st["d_min"], st["d_max"], st["growth"], " ".join("%d" % wire[i] for i in range(12) if i != 10),      # ([10]: milliseconds)
            tm["bytes"], tm["messages"], core.comm_bcast_mode())
        core.close()
    finally:
        if world > 1:
            dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="forms0,forms1,forms2,forms3,condensed,wide,world1")
    args = ap.parse_args()
    import torch.multiprocessing as mp
    for name, world, shape, nb, opts, kw, mode in cases(args.only.split(",")):
        out = mp.Manager().dict()
        mp.spawn(_worker, args=(world, _free_port(), shape, nb, opts, kw, mode, out), nprocs=world, join=True)
        for r in range(world):
            print("%s world %d shape %s nb %d rank %d | %s" % (name, world, shape, nb, r, out[r]), flush=True)


if __name__ == "__main__":
    main()
