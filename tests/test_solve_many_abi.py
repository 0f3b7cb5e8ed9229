"""CPU check of the matrix right-hand-side entry point (pyipm_newton_solve_many): declared in the header, exported by
the library, bound in the ctypes table with the header's argument types."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_solve_many_is_declared_exported_and_bound():
    from pyipm_amd import newton
    txt = open(os.path.join(ROOT, "include", "pyipm_newton.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    decl = re.search(r"int\s+pyipm_newton_solve_many\s*\(([^;]*)\)\s*;", txt)
    assert decl, "pyipm_newton_solve_many is not declared"
    args = [re.sub(r"\s+", " ", a.strip()) for a in decl.group(1).split(",")]
    assert args == ["pyipm_newton_ctx* ctx", "int64_t k", "const double* rhs", "int64_t ld_rhs", "double* dz",
                    "int64_t ld_dz", "int flip", "int refine", "int memkind"], args
    lib = ctypes.CDLL(newton.LIB_PATH)
    assert hasattr(lib, "pyipm_newton_solve_many")
    bound = newton.load_library()
    assert "pyipm_newton_solve_many" in newton.exported_symbols()
    fn = bound.pyipm_newton_solve_many
    c = ctypes
    assert fn.restype is c.c_int
    assert list(fn.argtypes) == [c.c_void_p, c.c_int64, c.c_void_p, c.c_int64, c.c_void_p, c.c_int64, c.c_int, c.c_int,
                                 c.c_int]


def test_solve_many_has_a_python_method():
    from pyipm_amd.newton import NewtonCore
    assert callable(getattr(NewtonCore, "solve_many", None))
