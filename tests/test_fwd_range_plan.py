"""The no-hang argument of k_fwd_range and k_fwd_prefix on the CPU.

pyipm_amd/csrc/fwd_range_plan.hpp is k_fwd_range's one statement of what the chain of the launch waits for, which visit of a
row owner is final and which chunks have an owner.  tests/fwd_range_replay.cpp includes it, rebuilds every workgroup's visits and
replays the protocol: every (word, value) the chain waits for is stored by exactly one owner visit, every flag an owner waits for
is raised by the chain, a round-robin execution of all workgroups ends with every chunk complete in memory, the updates are those
of the per-panel kernels' active launch blocks.  k_fwd_prefix keeps its own text; the replay restates its numbering (the slack
hole), visits and rule (prog[c] >= s, final at s + 1 == c / cpp), runs them through the same checks for Pa = 0 inside the x block,
and asserts that the header gives that rule there.  The program is built by the host compiler with the address and undefined-behaviour
sanitizers and run on its own: nothing is loaded into Python.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRIDS = (2, 3, 5, 97)
# (n, me, mi), nb: the shapes of tests/test_gpu_fwd_range.py, those of tests/test_gpu_fwd_prefix.py, the benchmark's
RANGE_SHAPES = [((256, 256, 256), 128), ((384, 512, 384), 128), ((256, 384, 256), 128), ((256, 256, 192), 128), ((256, 128, 256), 128),
                ((256, 0, 256), 128), ((1024, 512, 512), 256), ((256, 256, 1024), 128)]
PREFIX_SHAPES = [((512, 128, 256), 128), ((384, 128, 192), 128), ((1024, 256, 512), 256), ((512, 128, 0), 128), ((512, 0, 256), 128)]
BENCH_SHAPE = ((16384, 4096, 6144), 256)


def _cases():
    lines = []
    for shape, nb in RANGE_SHAPES + PREFIX_SHAPES:
        for grid in GRIDS:
            lines.append((shape, nb, grid, 0))                 # every range [Pa, Pb) of the geometry
    for grid in GRIDS:
        lines.append((BENCH_SHAPE[0], BENCH_SHAPE[1], grid, 1))  # the ranges a handle can launch
    for nb in (128, 256):                                       # a sweep of small multiples of 128, every range, every grid
        for n in (128, 256, 384):
            for me in (0, 128, 256, 384):
                for mi in (0, 128, 320, 512):
                    for grid in GRIDS:
                        lines.append(((n, me, mi), nb, grid, 0))
    return "".join("%d %d %d %d %d %d\n" % (s[0], s[1], s[2], nb, grid, mode) for s, nb, grid, mode in lines), len(lines)


def test_the_protocol_of_the_range_sweeps_cannot_hang(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "clang++", "c++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "fwd_range_replay")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "pyipm_amd", "csrc"), os.path.join(ROOT, "tests", "fwd_range_replay.cpp"),
                           "-o", exe])
    text, count = _cases()
    res = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    replayed = int(res.stdout.split()[0])
    assert replayed >= count, (replayed, count)
