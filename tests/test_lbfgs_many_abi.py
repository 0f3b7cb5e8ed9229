"""CPU-side checks of the many-column entries of the quasi-Newton KKT operator (pyipm_lbfgs_kkt_matvec_many,
pyipm_lbfgs_kkt_solve_many): declared in pyipm_newton.h beside pyipm_qn_* with exactly these argument lists, absent from
pyipm_lbfgs.h, exported, bound by pyipm_amd.newton with matching argtypes; the interface version is still 8; a NULL handle is
an error code from both and nothing is written; both headers still compile as C11 and C++17."""
import ctypes
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_BADARG = -1
C = ctypes
ENTRIES = {
    "pyipm_lbfgs_kkt_matvec_many": (
        ["pyipm_lbfgs_ctx* h", "int64_t k", "const double* v", "int64_t ld_v", "double* out", "int64_t ld_out", "int flip",
         "int memkind"],
        [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int]),
    "pyipm_lbfgs_kkt_solve_many": (
        ["pyipm_lbfgs_ctx* h", "int64_t k", "const double* rhs", "int64_t ld_rhs", "double* dz", "int64_t ld_dz", "int flip",
         "int refine", "int memkind"],
        [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int]),
}


def _header(name):
    txt = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_both_entries_are_declared_exported_and_bound():
    from pyipm_amd import lbfgs, newton
    raw = ctypes.CDLL(newton.LIB_PATH)
    for name, (want_args, want_types) in ENTRIES.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", _header("pyipm_newton.h"))
        assert m, name + " is not declared in pyipm_newton.h"
        assert [" ".join(a.split()) for a in m.group(1).split(",")] == want_args
        assert not re.search(r"\b" + name + r"\s*\(", _header("pyipm_lbfgs.h"))
        assert hasattr(raw, name), "missing export: " + name
        assert name in newton.exported_symbols() and name not in lbfgs.exported_symbols()
        fn = getattr(lbfgs.load(), name)                       # the library object LbfgsCore calls through
        assert fn.restype is C.c_int and list(fn.argtypes) == want_types
    assert newton.load_library().pyipm_newton_abi_version() == 8


def test_null_handle_is_badarg_and_writes_nothing():
    from pyipm_amd import newton
    lib = newton.load_library()
    a = (C.c_double * 8)(*([7.0] * 8))
    b = (C.c_double * 8)(*([5.0] * 8))
    for k in (1, 0):
        assert lib.pyipm_lbfgs_kkt_matvec_many(None, k, a, 8, b, 8, 0, newton.MEM_HOST) == E_BADARG
        assert lib.pyipm_lbfgs_kkt_solve_many(None, k, a, 8, b, 8, 0, -1, newton.MEM_HOST) == E_BADARG
    assert list(a) == [7.0] * 8 and list(b) == [5.0] * 8


def test_both_headers_still_compile_as_c_and_cxx(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    src = ('#include "pyipm_lbfgs.h"\n#include "pyipm_newton.h"\n'
           "int main(void) { return pyipm_lbfgs_kkt_matvec_many(0, 0, 0, 0, 0, 0, 0, 0) +\n"
           "                        pyipm_lbfgs_kkt_solve_many(0, 0, 0, 0, 0, 0, 0, 0, 0) == 0; }\n")
    ran = 0
    for comp, ext, std in ((cc, "c", "-std=c11"), (cxx, "cpp", "-std=c++17")):
        if not comp:
            continue
        f = tmp_path / ("t." + ext)
        f.write_text(src)
        subprocess.run([comp, std, "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(f)],
                       check=True)
        ran += 1
    assert ran, "no C or C++ compiler found"
