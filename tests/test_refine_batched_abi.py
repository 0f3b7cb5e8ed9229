"""pyipm_newton_refine_batched -- adaptive refinement of a batch of directions, every problem by itself -- at the boundary, without
a GPU: declared in include/pyipm_newton.h, exported by the library, bound by pyipm_amd/newton.py with the header's argument
count, a NULL handle refused, the interface version still 8 in all three places, and the Python surface that goes with it."""
import ctypes
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "pyipm_newton_refine_batched"


def _header():
    return open(os.path.join(ROOT, "include", "pyipm_newton.h")).read()


def _code():
    return re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)


def test_the_name_is_declared_exported_and_bound():
    from pyipm_amd import newton
    declared = set(re.findall(r"\b(pyipm_[a-z0-9_]+)\s*\(", _code()))
    raw = ctypes.CDLL(newton.LIB_PATH)
    assert NAME in declared, "not declared"
    assert hasattr(raw, NAME), "not exported"
    assert NAME in set(newton.exported_symbols()), "not bound"


def test_argument_count_of_header_and_binding():
    from pyipm_amd import newton
    lib = newton.load_library()
    assert len(getattr(lib, NAME).argtypes) == 10
    args = re.search(r"\b%s\s*\((.*?)\);" % NAME, _code(), re.S).group(1)
    assert len(args.split(",")) == 10, args


def test_a_null_handle_is_refused_without_a_gpu():
    from pyipm_amd import newton
    lib = newton.load_library()
    assert lib.pyipm_newton_refine_batched(None, None, 0, 0, None, 1, 0.0, -1, None, 0) == -1


def test_interface_version_is_still_8():
    from pyipm_amd import newton
    m = re.search(r"#define\s+PYIPM_NEWTON_ABI_VERSION\s+(\d+)", _header())
    assert m and int(m.group(1)) == 8
    assert newton.ABI_VERSION == 8
    assert newton.load_library().pyipm_newton_abi_version() == 8


def test_the_decision_is_stated_once():
    """The kernel compiles refine_each_plan.hpp and states no threshold of its own."""
    csrc = os.path.join(ROOT, "pyipm_amd", "csrc")
    kern = open(os.path.join(csrc, "kernels_brefine.hpp")).read()
    assert '#include "refine_each_plan.hpp"' in kern and "refine_each_verdict(" in kern
    assert "0.25" not in re.sub(r"//.*", "", kern)


def test_python_surface():
    from pyipm_amd.batched import BatchedNewton
    from pyipm_amd.batched_qp import BatchedQPIPM
    assert callable(BatchedNewton.refine_all)
    assert BatchedNewton.REFINE_KEYS == ("steps", "backward_error0", "backward_error", "converged")
    p = inspect.signature(BatchedNewton.refine_all).parameters
    assert list(p) == ["self", "dz", "active", "flip", "target", "max_steps"]
    assert p["active"].default is None and p["flip"].default is True and p["target"].default is None and p["max_steps"].default is None
    assert inspect.signature(BatchedNewton.direction_all).parameters["refine"].default is False
    assert inspect.signature(BatchedQPIPM.__init__).parameters["refine"].default is False
    # HipNewtonBackend's bars, per problem
    from pyipm_amd.ipm import HipNewtonBackend
    for name in ("suspect_spread", "berr_tol", "berr_fallback"):
        assert getattr(BatchedNewton, name) == getattr(HipNewtonBackend, name), name
    assert BatchedNewton.suspect_spread == 1e-10 and BatchedNewton.berr_tol == 1e-11
    for name in ("n_rcond", "n_refined", "n_static", "n_unconverged", "n_inexact"):
        assert getattr(BatchedNewton, name) == 0, name
