"""CPU-side checks of the L-BFGS pair store's boundary (include/pyipm_newton.h, "pair store"): the eight entry points are
declared, exported and bound; the workspace query answers without a GPU; a NULL handle is an error code, never a crash; the
Python store has no CPU fallback."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["pyipm_pairs_create", "pyipm_pairs_destroy", "pyipm_pairs_last_error", "pyipm_pairs_offer", "pyipm_pairs_reset",
         "pyipm_pairs_set_stream", "pyipm_pairs_view_get", "pyipm_pairs_workspace_bytes"]
E_BADARG = -1


def _declared(name):
    txt = open(os.path.join(ROOT, "include", name)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(pyipm_[a-z0-9_]+)\s*\(", txt)))


def test_the_eight_entry_points_are_declared_exported_and_bound():
    from pyipm_amd import newton
    declared = [k for k in _declared("pyipm_newton.h") if k.startswith("pyipm_pairs_")]
    assert declared == NAMES
    assert not [k for k in _declared("pyipm_lbfgs.h") if k.startswith("pyipm_pairs_")]
    lib = ctypes.CDLL(newton.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), "missing export: " + name
    assert [k for k in sorted(newton.exported_symbols()) if k.startswith("pyipm_pairs_")] == NAMES
    assert newton.load_library().pyipm_newton_abi_version() == 8


def test_exported_symbol_set_is_what_the_two_headers_declare():
    """Nothing else leaves the shared object: its dynamic pyipm_* symbols are the headers' declarations."""
    import subprocess
    import shutil
    from pyipm_amd import newton
    nm = shutil.which("nm") or shutil.which("llvm-nm") or (os.path.exists("/opt/rocm/llvm/bin/llvm-nm") and "/opt/rocm/llvm/bin/llvm-nm")
    if not nm:
        pytest.skip("no nm")
    out = subprocess.run([nm, "-D", "--defined-only", newton.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted({ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("pyipm_")
                       and ln.split()[-2] in "TtWw"})
    assert exported == sorted(_declared("pyipm_newton.h") + _declared("pyipm_lbfgs.h"))


def test_workspace_query_needs_no_gpu():
    from pyipm_amd import newton
    lib = newton.load_library()
    assert lib.pyipm_pairs_workspace_bytes(262144, 0) == 0
    assert lib.pyipm_pairs_workspace_bytes(262144, 32) == 0
    assert lib.pyipm_pairs_workspace_bytes(0, 4) == 0
    for n, memory in ((262144, 8), (262144, 31), (1, 1), (8193, 4)):
        assert lib.pyipm_pairs_workspace_bytes(n, memory) > 2 * n * (memory + 1) * 8


def test_null_handle_is_badarg_from_every_entry():
    from pyipm_amd import newton
    lib = newton.load_library()
    null = ctypes.c_void_p(0)
    out = ctypes.c_int(7)
    buf = (ctypes.c_double * 4)()
    assert lib.pyipm_pairs_create(None, 10, 4, 1, 1.0, 0, null) == E_BADARG
    assert lib.pyipm_pairs_destroy(null) == E_BADARG
    assert lib.pyipm_pairs_set_stream(null, null) == E_BADARG
    assert lib.pyipm_pairs_reset(null) == E_BADARG
    assert lib.pyipm_pairs_offer(null, buf, buf, buf, buf, 1e-16, newton.MEM_HOST, ctypes.byref(out)) == E_BADARG
    assert out.value == 7
    view = (ctypes.c_char * 128)()
    assert lib.pyipm_pairs_view_get(null, view) == E_BADARG
    assert lib.pyipm_pairs_last_error(null) == b"null handle"
    # bad geometry is refused before any device is looked for
    h = ctypes.c_void_p(5)
    for memory in (0, 32):
        assert lib.pyipm_pairs_create(ctypes.byref(h), 10, memory, 1, 1.0, 0, null) == E_BADARG
        assert not h.value


def test_pair_store_has_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from pyipm_amd.lbfgs import PairStore
    from pyipm_amd.newton import NewtonError
    with pytest.raises(NewtonError):
        PairStore(100, 4, True)
