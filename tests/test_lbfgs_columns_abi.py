"""CPU-side checks of the partial restaging entry point (pyipm_lbfgs_stage_jacobian_columns): declared in
pyipm_newton.h, beside the other later additions to the L-BFGS handle, with the argument list the binding gives it, exported,
bound; the interface version is still 8; a NULL handle is an error code, never a crash.  And the host half behind it, pyipm_amd/csrc/gram_tiles.hpp (the set of restaged tile indices
and the tile list of the restricted Gram launch), replayed by tests/gram_tiles_replay.cpp under the host compiler with the
address and undefined-behaviour sanitizers against the same rules stated here."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "pyipm_lbfgs_stage_jacobian_columns"
E_BADARG = -1


def _header(name):
    txt = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_the_entry_point_is_declared_exported_and_bound():
    """Declared where the later additions to the L-BFGS handle are (pyipm_qn_*): in pyipm_newton.h, bound by pyipm_amd.newton.
    pyipm_lbfgs.h and the table of pyipm_amd.lbfgs keep the ten entries tests/test_abi.py counts."""
    from pyipm_amd import lbfgs, newton
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^)]*)\)\s*;", _header("pyipm_newton.h"))
    assert m, "not declared in pyipm_newton.h"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["pyipm_lbfgs_ctx* h", "int64_t c0", "int64_t count", "const double* Jc", "int64_t ld", "int memkind"]
    assert not re.search(r"\b" + NAME + r"\s*\(", _header("pyipm_lbfgs.h"))
    assert hasattr(ctypes.CDLL(newton.LIB_PATH), NAME), "missing export"
    assert NAME in newton.exported_symbols() and NAME not in lbfgs.exported_symbols()
    fn = getattr(lbfgs.load(), NAME)                           # the library object LbfgsCore calls through
    c = ctypes
    assert fn.restype is c.c_int and list(fn.argtypes) == [c.c_void_p, c.c_int64, c.c_int64, c.c_void_p, c.c_int64, c.c_int]
    assert newton.load_library().pyipm_newton_abi_version() == 8


def test_null_handle_is_badarg():
    from pyipm_amd import lbfgs, newton
    lib = lbfgs.load()
    buf = (ctypes.c_double * 4)()
    assert lib.pyipm_lbfgs_stage_jacobian_columns(None, 0, 1, buf, 1, newton.MEM_HOST) == E_BADARG
    assert lib.pyipm_lbfgs_stage_jacobian_columns(None, 0, 0, None, 0, newton.MEM_HOST) == E_BADARG


def _want(p_pad, ranges):
    """(dirty tile indices, lower-triangle tiles with a dirty row or column index) by enumeration."""
    nt = p_pad // 128
    dirty = set()
    for c0, count in ranges:
        dirty.update(c // 128 for c in range(c0, c0 + count))
    tiles = {(i, j) for j in range(nt) for i in range(j, nt) if i in dirty or j in dirty}
    return dirty, tiles


REPLAY = [(384, [(130, 5)]), (384, [(120, 20)]), (384, [(95, 15)]), (384, [(299, 1)]), (384, [(128, 128)]), (384, [(0, 300)]),
          (384, [(3, 5), (260, 11)]), (128, [(1, 1)]), (3584, [(250, 10), (3000, 1)]), (4096, [(128, 128)]), (4096, [(100, 128)]),
          (4096, [(1000, 2048)]), (4096, [(0, 4096)]), (4096, [(4095, 1), (0, 1)]), (1152, [(0, 0)]), (16384, [(8000, 300)])]


def test_dirty_set_and_tile_list_replay(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "clang++", "c++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "gram_tiles_replay")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "pyipm_amd", "csrc"), os.path.join(ROOT, "tests", "gram_tiles_replay.cpp"),
                           "-o", exe])
    text = "".join("%d %d %s\n" % (p_pad, len(r), " ".join("%d %d" % cc for cc in r)) for p_pad, r in REPLAY)
    res = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = res.stdout.strip().splitlines()
    assert len(lines) == len(REPLAY)
    for (p_pad, ranges), line in zip(REPLAY, lines):
        got = [int(v) for v in line.split()]
        ndirty, is_all, count, capacity, length = got[:5]
        codes = got[5:]
        dirty, tiles = _want(p_pad, ranges)
        assert ndirty == len(dirty) and bool(is_all) == (len(dirty) == p_pad // 128) and count == len(tiles), (p_pad, ranges)
        assert length == len(codes) and length % 8 == 0 and length <= capacity and length < len(tiles) + 8
        real = [c for c in codes if c != 0xffffffff]
        assert len(real) == len(set(real)) == len(tiles)                       # every dirty tile once, nothing else
        assert {(c & 0xffff, c >> 16) for c in real} == tiles
        per_xcd = [sum(1 for c in codes[x::8] if c != 0xffffffff) for x in range(8)]
        assert max(per_xcd) == (len(tiles) + 7) // 8                          # no sequence longer than the even share
