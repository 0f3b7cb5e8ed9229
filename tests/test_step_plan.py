"""What a reusing or recording step keeps, copies and skips, on the CPU.

pyipm_amd/csrc/step_plan.hpp is the one statement of it: the group schedule, the prefix [0, gB), the kept lambda_e groups [gS, gE),
both snapshots' ranges and sizes, the first group of the lookahead loop and the owner of every panel's forward substitution.  The
assembly and the factorisation both call it.  tests/step_plan_replay.cpp includes it, builds the full, recording and reusing plans of
every geometry below -- with and without the lambda_e level, fuse_forward and the one-launch sweeps -- and checks them against the
geometry: one owner per panel for both outcomes of the range launch, the range launch's panels, the borders of the kept groups,
the snapshot's ranges and sizes, what each step kind may and may not do.  The program is built by the host compiler with the
address and undefined-behaviour sanitizers and run on its own: nothing is loaded into Python.  No GPU."""
import ast
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (n, me, mi), nb, group: tests/test_gpu_reuse_x.py, tests/test_gpu_fwd_prefix.py (group 2), tests/test_gpu_fwd_range.py
REUSE_X = [((512, 128, 256), 128, grp) for grp in (1, 2, 4)]
# test_boundary_shapes of tests/test_gpu_reuse_x.py: (n, me, mi), group, does the schedule have a prefix
REUSE_X_BOUNDARY = [((384, 128, 256), 2, True), ((320, 128, 256), 2, True), ((512, 0, 256), 2, True), ((512, 128, 0), 2, True),
                    ((128, 128, 256), 2, False), ((384, 128, 192), 2, True)]
FWD_PREFIX = [((512, 128, 256), 128, 2), ((384, 128, 192), 128, 2), ((1024, 256, 512), 256, 2), ((512, 128, 0), 128, 2), ((512, 0, 256), 128, 2)]
FWD_RANGE = [((256, 256, 256), 128, 1), ((384, 512, 384), 128, 2), ((256, 384, 256), 128, 2), ((256, 256, 192), 128, 1), ((256, 128, 256), 128, 2),
             ((256, 0, 256), 128, 1), ((1024, 512, 512), 256, 2), ((256, 256, 1024), 128, 1)]
BENCH = ((16384, 4096, 6144), 256, 8)


def _lam_e_shapes():
    """SHAPES of tests/test_gpu_reuse_lam_e.py, read from its source (that module needs the package and a GPU to import)."""
    with open(os.path.join(ROOT, "tests", "test_gpu_reuse_lam_e.py")) as f:
        tree = ast.parse(f.read())
    for node in tree.body:
        if isinstance(node, ast.Assign) and any(getattr(t, "id", None) == "SHAPES" for t in node.targets):
            return ast.literal_eval(node.value)
    raise AssertionError("no SHAPES in tests/test_gpu_reuse_lam_e.py")


def _cases():
    lam_e = _lam_e_shapes()
    assert len(lam_e) >= 4
    lines = [(shape, 128, group, 2, 1) for shape, group, _ in lam_e.values()]
    for shape, nb, group in REUSE_X + [(s, 128, grp) for s, grp, _ in REUSE_X_BOUNDARY] + FWD_PREFIX + FWD_RANGE + [BENCH]:
        for lookahead in (1, 2):
            lines.append((shape, nb, group, lookahead, 1))
    for n in (128, 256, 384):
        for me in (0, 128, 256, 384):
            for mi in (0, 128, 320, 512):
                for nb in (128, 256):
                    for group in (1, 2, 4, 8):
                        for lookahead in (1, 2):
                            for skip in (0, 1):
                                lines.append(((n, me, mi), nb, group, lookahead, skip))
    return lam_e, lines


def test_every_plan_is_consistent_with_its_geometry(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "clang++", "c++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "step_plan_replay")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "pyipm_amd", "csrc"), os.path.join(ROOT, "tests", "step_plan_replay.cpp"),
                           "-o", exe])
    lam_e, lines = _cases()
    text = "".join("%d %d %d %d %d %d %d\n" % (s[0], s[1], s[2], nb, group, la, skip) for s, nb, group, la, skip in lines)
    res = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    out = res.stdout.splitlines()
    assert int(out[-1].split()[0]) >= len(lines), (out[-1], len(lines))
    got = {tuple(int(x) for x in ln.split()[:7]): tuple(int(x) for x in ln.split()[7:]) for ln in out[:-1]}
    # the kept lambda_e groups of tests/test_gpu_reuse_lam_e.py: its table's third column, None where the level does not apply
    for name, (shape, group, kept) in lam_e.items():
        gB, gS, gE = got[(shape[0], shape[1], shape[2], 128, group, 2, 1)]
        assert gB > 0, name
        assert ((gS, gE) if gS >= 0 else None) == kept, (name, gS, gE, kept)
    # the boundary shapes of tests/test_gpu_reuse_x.py: a prefix everywhere but where the first group reaches beyond the x block
    for shape, group, applies in REUSE_X_BOUNDARY:
        for lookahead in (1, 2):
            gB = got[(shape[0], shape[1], shape[2], 128, group, lookahead, 1)][0]
            assert (gB > 0) == applies and (applies or gB == 0), (shape, lookahead, gB)
    # the benchmark keeps its x prefix and lambda_e groups (profiles/reuse_lam_e_ab.json)
    gB, gS, gE = got[(16384, 4096, 6144, 256, 8, 2, 1)]
    assert gB > 0 and gB < gS < gE, (gB, gS, gE)
