"""The four batched entry points behind ``BatchedQPIPM`` -- products, transposed products, merit reductions, merit ray --
at the boundary, without a GPU: declared in include/pyipm_newton.h, exported by the library, bound by pyipm_amd/newton.py, and
the three statements of the interface version (header, binding, library) agree on 8."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pyipm_newton_block_products_batched", "pyipm_newton_block_products_t_batched", "pyipm_newton_merit_info_batched",
         "pyipm_newton_merit_ray_batched")


def _header():
    return open(os.path.join(ROOT, "include", "pyipm_newton.h")).read()


def test_the_four_names_are_declared_exported_and_bound():
    from pyipm_amd import newton
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = set(re.findall(r"\b(pyipm_[a-z0-9_]+)\s*\(", code))
    lib = ctypes.CDLL(newton.LIB_PATH)
    bound = set(newton.exported_symbols())
    for name in NAMES:
        assert name in declared, "not declared: " + name
        assert hasattr(lib, name), "not exported: " + name
        assert name in bound, "not bound: " + name
    # the argument lists of the header, as the binding states them
    lib = newton.load_library()
    assert len(lib.pyipm_newton_block_products_batched.argtypes) == 5
    assert len(lib.pyipm_newton_block_products_t_batched.argtypes) == 4
    assert len(lib.pyipm_newton_merit_info_batched.argtypes) == 4
    assert len(lib.pyipm_newton_merit_ray_batched.argtypes) == 9
    assert re.search(r"pyipm_newton_merit_ray_batched\(pyipm_newton_ctx\* ctx, const double\* dz, const double\* nu, const double\* mu, "
                     r"const double\* quad,\s+const double\* alphas, int K, double\* out, int memkind\);", code)


def test_interface_version_is_8_everywhere():
    from pyipm_amd import newton
    m = re.search(r"#define\s+PYIPM_NEWTON_ABI_VERSION\s+(\d+)", _header())
    assert m and int(m.group(1)) == 8
    assert newton.ABI_VERSION == 8
    assert newton.load_library().pyipm_newton_abi_version() == 8


def test_a_null_handle_is_refused_without_a_gpu():
    from pyipm_amd import newton
    lib = newton.load_library()
    assert lib.pyipm_newton_block_products_batched(None, None, None, None, None) == -1
    assert lib.pyipm_newton_block_products_t_batched(None, None, None, None) == -1
    assert lib.pyipm_newton_merit_info_batched(None, None, None, 0) == -1
    assert lib.pyipm_newton_merit_ray_batched(None, None, None, None, None, None, 1, None, 0) == -1
