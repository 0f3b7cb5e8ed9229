"""The tail split of a reusing step on the CPU.

pyipm_amd/csrc/step_plan.hpp states where a hand-over between two chain groups is split (plan_tail_split), which enqueue items the
lookahead loop then consists of (tail_regions) and which item waits for which (TAIL_DEPS).  tests/step_plan_split_replay.cpp
includes it and checks, per geometry, that every (rows, columns) region of every group is written by exactly one item per stage,
that every item's writers are in its wait list, and that the split applies exactly where the stated conditions hold.  The shapes
are those of tests/test_gpu_tail_split.py, the benchmark's and config 2, the switch on and off, and a sweep of small ones.  The
program is built by the host compiler with the address and undefined-behaviour sanitizers and run on its own.  No GPU."""
import ast
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = ((16384, 4096, 6144), 256, 8, 0)       # (n, me, mi), nb, group, tail_group (0: the handle's default)
CONFIG2 = ((2048, 0, 2048), 256, 8, 0)
# the dependencies no shape here exercises: a source that is no chain group although it is not a slack group (more than 32 tiles);
# an unsplit hand-over behind a split one; a split hand-over behind an unsplit one with rows left behind the target (refused_once
# has such a hand-over, but its target is the last group)
RARE = {("TI_HEAD_OLD", "TI_CHAIN"), ("TI_BULK_REST", "TI_CHAIN"), ("TI_HEAD_OLD", "TI_BULK_NEXT"),
        ("TI_HEAD_REST", "TI_BULK_REST"), ("TI_HEAD_XROWS", "TI_BULK_REST")}


def _from_gpu_test(name):
    """A module-level literal of tests/test_gpu_tail_split.py, read from its source (that module needs a GPU to be of use)."""
    with open(os.path.join(ROOT, "tests", "test_gpu_tail_split.py")) as f:
        tree = ast.parse(f.read())
    for node in tree.body:
        if isinstance(node, ast.Assign) and any(getattr(t, "id", None) == name for t in node.targets):
            return ast.literal_eval(node.value)
    raise AssertionError("no %s in tests/test_gpu_tail_split.py" % name)


def _dep_names():
    """(reader, writer) of every TAIL_DEPS row, in order, read from the header."""
    rows, inside = [], False
    with open(os.path.join(ROOT, "pyipm_amd", "csrc", "step_plan.hpp")) as f:
        for ln in f:
            if "constexpr TailDep TAIL_DEPS[]" in ln:
                inside = True
            elif inside and ln.startswith("};"):
                break
            elif inside and ln.strip().startswith("{"):
                a, b = ln.strip()[1:].split(",")[:2]
                rows.append((a.strip(), b.strip()))
    return rows


def test_the_split_writes_every_region_once_and_every_reader_waits_for_its_writers(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "clang++", "c++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "step_plan_split_replay")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "pyipm_amd", "csrc"), os.path.join(ROOT, "tests", "step_plan_split_replay.cpp"),
                           "-o", exe])
    shapes, splits = _from_gpu_test("SHAPES"), _from_gpu_test("SPLITS")
    named = {name: (shape, nb, group, group) for name, (shape, nb, group) in shapes.items()}
    named["bench"], named["config2"] = BENCH, CONFIG2
    lines = [(s, nb, grp, tg, on) for s, nb, grp, tg in named.values() for on in (1, 0)]
    for n in (256, 512):
        for me in (0, 128, 256):
            for mi in (0, 320, 512, 1536):
                for nb in (128, 256):
                    for grp in (1, 2, 4, 8):
                        lines.append(((n, me, mi), nb, grp, grp, 1))
                        lines.append(((n, me, mi), nb, grp, 0, 1))
    text = "".join("%d %d %d %d %d %d %d\n" % (s[0], s[1], s[2], nb, grp, tg, on) for s, nb, grp, tg, on in lines)
    res = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    out = res.stdout.splitlines()
    assert int(out[-1].split()[0]) == len(lines), (out[-1], len(lines))
    got = {tuple(int(x) for x in ln.split()[:7]): tuple(int(x) for x in ln.split()[7:]) for ln in out[:-2]}

    def of(name, on):
        s, nb, grp, tg = named[name]
        return got[(s[0], s[1], s[2], nb, grp, tg, on)]          # g0, ngroups, nsplit, first split group
    # the benchmark: the five hand-overs between the six lambda_i groups g17 .. g22; config 2 has one lambda_i group
    assert of("bench", 1) == (17, 23, 5, 17), of("bench", 1)
    assert of("config2", 1)[2] == 0, of("config2", 1)
    # the GPU test's shapes split as often as that test asserts from the trace; refused_once: only the last hand-over
    for name, least in splits.items():
        g0, ng, nsplit, first = of(name, 1)
        assert nsplit >= least, (name, of(name, 1))
    g0, ng, nsplit, first = of("refused_once", 1)
    assert nsplit == 1 and first == ng - 2 and first > g0, of("refused_once", 1)
    for name in named:
        assert of(name, 0)[2] == 0, (name, of(name, 0))
    # every dependency stated is one some shape needs
    used = out[-2].split()[1]
    deps = _dep_names()
    assert len(deps) == len(used) and len(deps) >= 20, (len(deps), used)
    unused = {d for d, u in zip(deps, used) if u == "0"}
    assert unused <= RARE, unused
