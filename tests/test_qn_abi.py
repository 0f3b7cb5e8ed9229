"""CPU-side checks of the quasi-Newton KKT operator's boundary (include/pyipm_newton.h, pyipm_qn_*): the four entry points are
declared in pyipm_newton.h (not in pyipm_lbfgs.h), exported and bound; the interface version is still 8; a NULL handle is an
error code from each, never a crash; the workspace query still answers without a GPU."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["pyipm_qn_info", "pyipm_qn_matvec", "pyipm_qn_refine", "pyipm_qn_solve"]
E_BADARG = -1


def _declared(name):
    txt = open(os.path.join(ROOT, "include", name)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(pyipm_[a-z0-9_]+)\s*\(", txt)))


def test_the_four_entry_points_are_declared_exported_and_bound():
    from pyipm_amd import newton
    assert [k for k in _declared("pyipm_newton.h") if k.startswith("pyipm_qn_")] == NAMES
    assert not [k for k in _declared("pyipm_lbfgs.h") if k.startswith("pyipm_qn_")]
    lib = ctypes.CDLL(newton.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), "missing export: " + name
    assert [k for k in sorted(newton.exported_symbols()) if k.startswith("pyipm_qn_")] == NAMES
    assert newton.load_library().pyipm_newton_abi_version() == 8


def test_both_headers_compile_as_c_and_cxx(tmp_path):
    """pyipm_newton.h now names the L-BFGS handle type; pyipm_lbfgs.h, which includes it, repeats that typedef (legal in C11 and
    C++): both still compile in both languages."""
    import shutil
    import subprocess
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    src = '#include "pyipm_lbfgs.h"\n#include "pyipm_newton.h"\nint main(void) { return pyipm_qn_info(0, 0) == 0; }\n'
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


def test_null_handle_is_badarg_from_every_entry():
    from pyipm_amd import newton
    lib = newton.load_library()
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_double * 8)(*([7.0] * 8))
    assert lib.pyipm_qn_matvec(null, buf, 0, newton.MEM_HOST, buf) == E_BADARG
    assert lib.pyipm_qn_solve(null, buf, buf, 0, newton.MEM_HOST) == E_BADARG
    assert lib.pyipm_qn_refine(null, None, buf, 0, -1, newton.MEM_HOST) == E_BADARG
    assert lib.pyipm_qn_info(null, buf) == E_BADARG
    assert list(buf) == [7.0] * 8


def test_workspace_still_exceeds_the_padded_jacobian():
    from pyipm_amd import lbfgs
    lib = lbfgs.load()
    b = lib.pyipm_lbfgs_workspace_bytes(262144, 1024, 3072, 9, 256)
    assert b > 262144 * 4096 * 8
    # the work vectors of the new calls are part of the figure: five vectors of N, J v (n), J'v (p_pad) and the row partials of
    # the pass over J, (p_pad / 64) x n doubles
    n, p_pad, N = 262144, 4096, 262144 + 2 * 3072 + 1024
    assert b > 262144 * 4096 * 8 + 8 * (5 * N + n + p_pad + (p_pad // 64) * n)
    assert lib.pyipm_lbfgs_workspace_bytes(100, 0, 0, 4, 256) > 0          # (no constraints: nothing of the above, still a handle)
