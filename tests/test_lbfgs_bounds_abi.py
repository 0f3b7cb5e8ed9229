"""CPU-side checks of the bounded L-BFGS handle's boundary (include/pyipm_newton.h, pyipm_lbfgs_bounded_*): the three entry
points are declared beside the other later additions to the L-BFGS handle, exported and bound; the interface version is
still 8; NULL pointers and bad geometry are error codes before any device is looked for; the workspace query answers
without a GPU and grows with the bounds by O(n + mb), never by mb^2.  And the host half behind bounded_stage,
pyipm_amd/csrc/bounds_csr.hpp (the stable grouping of the bounds by variable), replayed by tests/bounds_csr_replay.cpp
under the host compiler with the address and undefined-behaviour sanitizers."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["pyipm_lbfgs_bounded_create", "pyipm_lbfgs_bounded_stage", "pyipm_lbfgs_bounded_workspace_bytes"]
E_BADARG = -1


def _declared(name):
    txt = open(os.path.join(ROOT, "include", name)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(pyipm_[a-z0-9_]+)\s*\(", txt)))


def test_the_three_entry_points_are_declared_exported_and_bound():
    from pyipm_amd import lbfgs, newton
    assert [k for k in _declared("pyipm_newton.h") if k.startswith("pyipm_lbfgs_bounded_")] == NAMES
    assert not [k for k in _declared("pyipm_lbfgs.h") if "bounded" in k]
    assert len(_declared("pyipm_lbfgs.h")) == 10 and len(lbfgs.exported_symbols()) == 10
    lib = ctypes.CDLL(newton.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), "missing export: " + name
    assert [k for k in sorted(newton.exported_symbols()) if k.startswith("pyipm_lbfgs_bounded_")] == NAMES
    c = ctypes
    bound = lbfgs.load()                                      # the library object LbfgsCore calls through
    assert bound.pyipm_lbfgs_bounded_workspace_bytes.restype is c.c_size_t
    assert list(bound.pyipm_lbfgs_bounded_workspace_bytes.argtypes) == [c.c_int64] * 4 + [c.c_int, c.c_int]
    assert list(bound.pyipm_lbfgs_bounded_create.argtypes) == [c.POINTER(c.c_void_p)] + [c.c_int64] * 4 + [c.c_int] * 3 + [c.c_void_p]
    assert list(bound.pyipm_lbfgs_bounded_stage.argtypes) == [c.c_void_p] * 3
    assert newton.load_library().pyipm_newton_abi_version() == 8


def test_null_pointers_are_badarg():
    from pyipm_amd import newton
    lib = newton.load_library()
    null = ctypes.c_void_p(0)
    var = (ctypes.c_int64 * 2)(0, 1)
    sign = (ctypes.c_double * 2)(1.0, -1.0)
    assert lib.pyipm_lbfgs_bounded_create(None, 10, 1, 2, 3, 4, 0, 0, null) == E_BADARG
    assert lib.pyipm_lbfgs_bounded_stage(null, var, sign) == E_BADARG
    assert lib.pyipm_lbfgs_bounded_stage(null, None, None) == E_BADARG


@pytest.mark.parametrize("geo", [(0, 1, 2, 3, 4), (10, -1, 2, 3, 4), (10, 1, -2, 3, 4), (10, 1, 2, -3, 4), (10, 1, 2, 3, 0),
                                 (10, 1, 2, 3, 33), (-5, 0, 0, 1, 4)])
def test_bad_geometry_is_refused_before_any_device_is_looked_for(geo):
    """(n, me, mg, mb, max_pairs).  On a machine without a GPU a well-formed geometry gives PYIPM_E_NODEVICE (-5): the
    refusals here come first, and *out is left NULL."""
    from pyipm_amd import newton
    lib = newton.load_library()
    n, me, mg, mb, cap = geo
    h = ctypes.c_void_p(5)
    assert lib.pyipm_lbfgs_bounded_create(ctypes.byref(h), n, me, mg, mb, cap, 0, 0, ctypes.c_void_p(0)) == E_BADARG
    assert not h.value
    assert lib.pyipm_lbfgs_bounded_workspace_bytes(n, me, mg, mb, cap, 0) == 0
    h = ctypes.c_void_p(5)
    assert lib.pyipm_lbfgs_bounded_create(ctypes.byref(h), 10, 1, 2, 3, 4, 100, 0, ctypes.c_void_p(0)) == E_BADARG     # nb
    assert not h.value


def test_workspace_query_needs_no_gpu_and_grows_linearly_with_the_bounds():
    from pyipm_amd import newton
    lib = newton.load_library()
    n, me, mg, mb, cap = 262144, 1024, 3072, 524288, 9
    plain = lib.pyipm_lbfgs_workspace_bytes(n, me, mg, cap, 0)
    bounded = lib.pyipm_lbfgs_bounded_workspace_bytes(n, me, mg, mb, cap, 0)
    p_pad, n_pad = 4096, 262144
    assert plain > 0 and bounded > plain
    assert bounded - plain < p_pad * n_pad * 8 + 64 * (n + mb)
    assert bounded - plain >= p_pad * n_pad * 8                  # the scaled operand is in it
    # the explicit form of the same problem would be of order p = me + mg + mb: its Gram matrix alone is p^2 doubles
    assert bounded < 8 * (me + mg + mb) ** 2 // 50
    # bounds only: no operand at all, O(n + mb)
    only = lib.pyipm_lbfgs_bounded_workspace_bytes(n, 0, 0, mb, cap, 0)
    assert 0 < only - lib.pyipm_lbfgs_workspace_bytes(n, 0, 0, cap, 0) < 64 * (n + mb)
    for geo in ((262144, 1024, 3072), (96, 24, 40), (130, 0, 0), (1, 0, 0), (8300, 100, 200)):
        for nb in (0, 128):
            assert lib.pyipm_lbfgs_bounded_workspace_bytes(*geo, 0, cap, nb) == lib.pyipm_lbfgs_workspace_bytes(*geo, cap, nb) > 0


def test_bounded_core_has_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from pyipm_amd.lbfgs import LbfgsCore
    from pyipm_amd.newton import NewtonError
    with pytest.raises(NewtonError):
        LbfgsCore(10, 1, 2, 4, bounds=([0, 1], [1.0, -1.0]))


# (n, [(var, sign), ...]) -- empty, repeated, unsorted, everything on one variable, a bound on the last variable only
REPLAY = [(1, []), (1, [(0, 1)]), (5, [(0, 1), (4, 1), (0, -1), (4, 1)]), (4, [(3, -1), (2, 1), (1, -1), (0, 1)]),
          (3, [(1, 1), (1, -1), (1, 1), (1, -1), (1, 1)]), (7, [(6, -1)]), (6, []),
          (96, [(k, 1) for k in range(96)] + [(k, -1) for k in range(96)]),
          (50, [((7 * j) % 50, 1 if j % 3 else -1) for j in range(173)]), (3, [(1, 1)] * 64)]
# each refused for the reason named, and the structure keeps what the case before built
REFUSED = [(5, [(0, 1), (5, 1)], "index"), (5, [(-1, 1)], "index"), (5, [(2, 0)], "sign"), (5, [(2, 2)], "sign"),
           (0, [], "geometry"), (3, [(1, 1)] * 65, "more than 64")]


def _want(n, bounds):
    """CSR by variable through a stable sort: (start, [(j, sign)] in CSR order)."""
    order = sorted(range(len(bounds)), key=lambda j: bounds[j][0])          # (sorted is stable)
    start = [0] * (n + 1)
    for v, _ in bounds:
        start[v + 1] += 1
    for k in range(n):
        start[k + 1] += start[k]
    return start, [(j, bounds[j][1]) for j in order]


def test_stable_grouping_by_variable_replay(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "clang++", "c++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "bounds_csr_replay")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "pyipm_amd", "csrc"), os.path.join(ROOT, "tests", "bounds_csr_replay.cpp"),
                           "-o", exe])
    cases = []
    for case in REPLAY:
        cases.append(case + (None,))
        cases.extend(REFUSED[len(cases) % len(REFUSED):][:1])              # a refusal between two builds
    cases.extend(REFUSED)
    text = "".join("%d %d %s\n" % (n, len(b), " ".join("%d %d" % vs for vs in b)) for n, b, _ in cases)
    res = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert res.returncode == 0, (res.stdout[-500:], res.stderr[-2000:])
    lines = res.stdout.strip().splitlines()
    assert len(lines) == len(cases)
    for (n, bounds, why), line in zip(cases, lines):
        if why is not None:
            assert line.startswith("refused") and why in line, (n, bounds, line)
            continue
        assert line.startswith("ok "), (n, bounds, line)
        left, right = line[3:].split("|")
        start = [int(v) for v in left.split()]
        ent = [tuple(int(v) for v in e.split(":")) for e in right.split()]
        assert (start, ent) == _want(n, bounds), (n, bounds)
        for k in range(n):                                                  # a variable's bounds in the order given
            seg = [j for j, _ in ent[start[k]:start[k + 1]]]
            assert seg == sorted(seg) and all(bounds[j][0] == k for j in seg)
