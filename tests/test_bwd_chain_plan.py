"""The chain order of k_bwd_sweep without the closed-form slack panels, on the CPU.

pyipm_amd/csrc/bwd_chain_plan.hpp is the kernel's one statement of which panels workgroup 0 leaves out, of pred(t) -- whose columns
the near specialists take at step t -- and of the chain-step numbers the progress words count.  tests/bwd_chain_replay.cpp includes
it, rebuilds the walk, the specialists' steps and every owner wave's visits and replays the protocol: every awaited (word, value) is
stored by exactly one visit, a round-robin execution ends, every block of a chain step is visited exactly once (by the specialists
if its group lies in pred(t), otherwise by its owner), per column the order of subtraction is descending t with the near one last,
and with skip == 0, or with no panel wholly inside the slack block, walk, visits and numbers are those of the walk over all
panels.  The program is built by the host compiler with the address and undefined-behaviour sanitizers and run on its own: nothing
is loaded into Python.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OWNERS = (1, 2, 5, 61)      # workgroups of column owners, 16 waves each: several groups per wave ... more waves than groups
# (n, me, mi), nb: the shapes of tests/test_gpu_bwd_slack.py and the panel structures they stand for at half the width
GPU_SHAPES = [((128, 64, 128), 128), ((128, 0, 192), 128), ((100, 40, 150), 128), ((64, 64, 128), 128), ((192, 64, 32), 128),
              ((256, 128, 256), 128), ((256, 0, 384), 128), ((200, 80, 300), 128), ((128, 128, 256), 128), ((384, 128, 64), 128),
              ((512, 256, 512), 256)]
HALF_WIDTH = [((128, 64, 128), 64), ((128, 0, 192), 64), ((100, 40, 150), 64), ((64, 64, 128), 64), ((192, 64, 32), 64)]
BENCH_SHAPES = [((16384, 4096, 6144), 256), ((2048, 0, 2048), 256)]


def _cases():
    lines = []
    for shape, nb in GPU_SHAPES + HALF_WIDTH:
        for ow in OWNERS:
            lines.append((shape, nb, ow))
    for shape, nb in BENCH_SHAPES:
        for ow in (5, 254):
            lines.append((shape, nb, ow))
    for nb in (64, 128, 256):       # me = 0, n or n + mi no multiple of nb, mi < nb, n < nb
        for n in (40, 64, 100, 256, 300):
            for me in (0, 40, 128):
                for mi in (0, 32, 100, 192, 256, 448, 700):
                    for ow in (1, 3):
                        lines.append(((n, me, mi), nb, ow))
    return "".join("%d %d %d %d %d\n" % (s[0], s[1], s[2], nb, ow) for s, nb, ow in lines), len(lines)


def test_the_chain_without_the_slack_panels_cannot_hang_and_keeps_the_order(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "clang++", "c++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "bwd_chain_replay")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "pyipm_amd", "csrc"), os.path.join(ROOT, "tests", "bwd_chain_replay.cpp"),
                           "-o", exe])
    text, count = _cases()
    res = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    replayed = int(res.stdout.split()[0])
    assert replayed >= 2 * count, (replayed, count)      # skip in {0, 1} x the walk with and without the slack panels, but for one-panel systems
