"""The three entry points that work against the kept factors of a batched handle -- pyipm_newton_solve_batched,
pyipm_newton_kkt_matvec_batched, pyipm_newton_rcond_batched -- at the boundary, without a GPU: declared in
include/pyipm_newton.h, exported by the library, bound by pyipm_amd/newton.py with the header's argument counts, a NULL handle
refused, and the interface version still 8 in all three places."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pyipm_newton_solve_batched", "pyipm_newton_kkt_matvec_batched", "pyipm_newton_rcond_batched")


def _header():
    return open(os.path.join(ROOT, "include", "pyipm_newton.h")).read()


def _code():
    return re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)


def test_the_three_names_are_declared_exported_and_bound():
    from pyipm_amd import newton
    declared = set(re.findall(r"\b(pyipm_[a-z0-9_]+)\s*\(", _code()))
    raw = ctypes.CDLL(newton.LIB_PATH)
    bound = set(newton.exported_symbols())
    for name in NAMES:
        assert name in declared, "not declared: " + name
        assert hasattr(raw, name), "not exported: " + name
        assert name in bound, "not bound: " + name


def test_argument_counts_of_header_and_binding():
    from pyipm_amd import newton
    lib = newton.load_library()
    want = {"pyipm_newton_solve_batched": 12, "pyipm_newton_kkt_matvec_batched": 9, "pyipm_newton_rcond_batched": 6}
    code = _code()
    for name, count in want.items():
        assert len(getattr(lib, name).argtypes) == count, name
        args = re.search(r"\b%s\s*\((.*?)\);" % name, code, re.S).group(1)
        assert len(args.split(",")) == count, (name, args)


def test_a_null_handle_is_refused_without_a_gpu():
    from pyipm_amd import newton
    lib = newton.load_library()
    assert lib.pyipm_newton_solve_batched(None, 1, None, 0, 0, None, 0, 0, None, 1, 0, 0) == -1
    assert lib.pyipm_newton_kkt_matvec_batched(None, 1, None, 0, 0, None, 0, 0, 0) == -1
    assert lib.pyipm_newton_rcond_batched(None, 0, 0, None, None, 0) == -1


def test_interface_version_is_still_8():
    from pyipm_amd import newton
    m = re.search(r"#define\s+PYIPM_NEWTON_ABI_VERSION\s+(\d+)", _header())
    assert m and int(m.group(1)) == 8
    assert newton.ABI_VERSION == 8
    assert newton.load_library().pyipm_newton_abi_version() == 8


def test_python_surface():
    from pyipm_amd.batched import BatchedNewton
    for name in ("solve_all", "kkt_matvec_all", "rcond_all"):
        assert callable(getattr(BatchedNewton, name))
    assert BatchedNewton.RCOND_KEYS == ("w_min", "w_max", "rcond", "static_pivot")
