"""The per-problem decision of pyipm_newton_refine_batched against the loop it restates, on the CPU.

pyipm_amd/csrc/refine_each_plan.hpp is the one statement of what a problem of a batch does after a measurement of its backward
error -- converged, take the last step back, stop, go on -- and of the record it leaves; k_b_ref_round (kernels_brefine.hpp)
compiles it.  tests/refine_each_replay.cpp includes it and moves one problem's state through the max_steps + 1 rounds the host
enqueues, on scripted sequences of measured errors.  ``refine_loop`` below restates drv::refine_loop with refine < 0
(pyipm_amd/csrc/driver.hpp), the single-system rule, line by line with callbacks on a numbered iterate; the four fields of the
record must EQUAL its info_steps / info_berr0 / info_berr / info_converged, the iterate kept must be the same one, and so must
the number of measurements.  The program is built by the host compiler with the address and undefined-behaviour sanitizers and
run on its own: nothing is loaded into Python.  No GPU."""
import math
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")


def refine_loop(errors, refine_max, refine_target):
    """drv::refine_loop(refine < 0): (info_steps, info_berr0, info_berr, info_converged, iterate kept, measurements)."""
    state = {"x": 0, "spare": None, "visits": 0}

    def berr_of():
        state["visits"] += 1
        return errors[state["visits"] - 1]

    def save():
        state["spare"] = state["x"]

    def restore():
        state["x"] = state["spare"]

    def correct():
        state["x"] += 1

    info_steps, info_converged, info_berr0, info_berr = 0, 0, -1.0, -1.0
    maxit = refine_max
    prev = -1.0
    for it in range(maxit + 1):
        berr = berr_of()
        if it == 0:
            info_berr0 = berr
        info_berr = berr
        if prev >= 0.0 and not (berr <= prev):
            restore()
            info_berr, info_steps = prev, it - 1
            break
        if not (berr <= 1.0e300):
            break
        if berr <= refine_target:
            info_converged = 1
            break
        if it == maxit or (prev >= 0.0 and berr > 0.25 * prev):
            break
        prev = berr
        save()
        correct()
        info_steps = it + 1
    return info_steps, info_berr0, info_berr, info_converged, state["x"], state["visits"]


TARGET = 1e-14
CASES = {                                   # name: (max_steps, target, the measurements)
    "immediate convergence": (8, TARGET, [3e-16]),
    "at the target exactly": (8, TARGET, [1e-14]),
    "steady 10x gains": (8, TARGET, [1e-8, 1e-9, 1e-10, 1e-11, 1e-12, 1e-13, 1e-14, 1e-15]),
    "one step is enough": (8, TARGET, [7.4e-8, 4.3e-16]),
    "a gain of 3x": (8, TARGET, [3e-8, 1e-8, 1e-9]),
    "a gain of 4x exactly goes on": (8, TARGET, [4e-8, 1e-8, 1e-15]),
    "a worse step (take back)": (8, TARGET, [1e-8, 1e-10, 5e-10, 1e-16]),
    "worse at once": (8, TARGET, [1e-8, 2e-8]),
    "NaN first": (8, TARGET, [NAN, 1e-16]),
    "Inf first": (8, TARGET, [INF, 1e-16]),
    "NaN later": (8, TARGET, [1e-6, 1e-8, NAN, 1e-16]),
    "Inf later": (8, TARGET, [1e-6, INF]),
    "budget spent": (3, TARGET, [1e-2, 1e-3, 1e-4, 1e-5, 1e-6]),
    "budget of two": (2, 1e-30, [1e-8, 1e-12, 1e-16, 1e-20]),
    "no budget": (0, TARGET, [1e-8, 1e-16]),
    "no budget, converged": (0, TARGET, [1e-15]),
    "converged on the last visit": (2, TARGET, [1e-4, 1e-9, 1e-15]),
    "worse on the last visit": (2, TARGET, [1e-4, 1e-9, 1e-8]),
    "zero error": (8, TARGET, [0.0]),
    "equal error counts as no gain": (8, TARGET, [1e-8, 1e-8]),
}


def same(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


def test_the_plan_is_refine_loop_for_one_problem(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "clang++", "c++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "refine_each_replay")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "pyipm_amd", "csrc"), os.path.join(ROOT, "tests", "refine_each_replay.cpp"),
                           "-o", exe])
    names = list(CASES)
    text = "".join("%d %r %d %s\n" % (CASES[k][0], CASES[k][1], len(CASES[k][2]), " ".join(repr(e) for e in CASES[k][2]))
                   for k in names)
    res = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = res.stdout.strip().splitlines()
    assert len(lines) == len(names)
    verdict_kinds = set()
    for name, line in zip(names, lines):
        max_steps, target, errors = CASES[name]
        got = line.split()
        steps, berr0, berr, conv = (float(v) for v in got[:4])
        iterate, visits = int(got[4]), int(got[5])
        w_steps, w_berr0, w_berr, w_conv, w_iter, w_visits = refine_loop(errors, max_steps, target)
        print(name, "->", line)
        assert steps == w_steps and same(berr0, w_berr0) and same(berr, w_berr) and conv == w_conv, (name, line)
        assert iterate == w_iter == w_steps, (name, line)         # the iterate kept is the one the step count names
        assert visits == w_visits <= max_steps + 1, (name, line)
        verdict_kinds.add((w_conv, w_steps < visits - 1))
    assert len(verdict_kinds) >= 3                                 # converged, stopped, taken back all occurred
