"""CPU check of the k-column product entry point (pyipm_newton_kkt_matvec_many): declared in the header, exported by the
library, bound in the ctypes table with the header's argument types; the interface version stays 8 (an entry is added,
nothing is changed)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_kkt_matvec_many_is_declared_exported_and_bound():
    from pyipm_amd import newton
    txt = open(os.path.join(ROOT, "include", "pyipm_newton.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    decl = re.search(r"int\s+pyipm_newton_kkt_matvec_many\s*\(([^;]*)\)\s*;", txt)
    assert decl, "pyipm_newton_kkt_matvec_many is not declared"
    args = [re.sub(r"\s+", " ", a.strip()) for a in decl.group(1).split(",")]
    assert args == ["pyipm_newton_ctx* ctx", "int64_t k", "const double* v", "int64_t ld_v", "double* y", "int64_t ld_y",
                    "int memkind"], args
    lib = ctypes.CDLL(newton.LIB_PATH)
    assert hasattr(lib, "pyipm_newton_kkt_matvec_many")
    bound = newton.load_library()
    assert "pyipm_newton_kkt_matvec_many" in newton.exported_symbols()
    fn = bound.pyipm_newton_kkt_matvec_many
    c = ctypes
    assert fn.restype is c.c_int
    assert list(fn.argtypes) == [c.c_void_p, c.c_int64, c.c_void_p, c.c_int64, c.c_void_p, c.c_int64, c.c_int]


def test_interface_version_is_still_8():
    from pyipm_amd import newton
    assert newton.load_library().pyipm_newton_abi_version() == 8
    hdr = open(os.path.join(ROOT, "include", "pyipm_newton.h")).read()
    assert re.search(r"#define\s+PYIPM_NEWTON_ABI_VERSION\s+8\b", hdr)


def test_kkt_matvec_many_has_a_python_method():
    from pyipm_amd.newton import NewtonCore
    assert callable(getattr(NewtonCore, "kkt_matvec_many", None))
