"""The two batched entry points of interface version 7 at the C-ABI: pyipm_newton_step_batched_each and
pyipm_newton_step_lengths_batched.  What needs no handle runs without a GPU; a refusal with a text needs a handle to
carry the text, and a handle needs a device (pyipm_newton_create*: PYIPM_E_NODEVICE without one), so those are GPU tests."""
import ctypes
import os
import re
from ctypes import c_void_p

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pyipm_newton_step_batched_each", "pyipm_newton_step_lengths_batched")
BADARG = -1


def test_new_entries_are_declared_bound_and_versioned():
    from pyipm_amd import newton
    hdr = open(os.path.join(ROOT, "include", "pyipm_newton.h")).read()
    lib = newton.load_library()
    assert int(re.search(r"#define PYIPM_NEWTON_ABI_VERSION (\d+)", hdr).group(1)) == newton.ABI_VERSION == lib.pyipm_newton_abi_version()
    assert newton.ABI_VERSION >= 7
    for name in NEW:
        assert name in newton.exported_symbols()
        # the comment in front of the declaration says what of the reference it replaces
        doc = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int %s\(" % name, hdr, re.S).group(1)
        assert "pyipm.py:" in doc, name


def test_null_handle_is_refused_without_a_gpu():
    from pyipm_amd import newton
    lib = newton.load_library()
    x = (ctypes.c_double * 4)()
    assert lib.pyipm_newton_step_batched_each(None, x, x, x, None, x, newton.MEM_HOST) == BADARG
    assert lib.pyipm_newton_step_lengths_batched(None, 0.995, None, x, newton.MEM_HOST) == BADARG


@pytest.mark.gpu
def test_refusals_carry_a_text():
    import torch
    from pyipm_amd.batched import BatchedNewton
    from pyipm_amd.newton import MEM_DEVICE, NewtonCore
    from pyipm_amd.problems import make_qp
    n, me, mi, B = 6, 2, 3, 2
    N = n + 2 * mi + me
    buf = torch.zeros(B * N, dtype=torch.float64, device="cuda")
    p = c_void_p(buf.data_ptr())

    def refused(lib, h, rc, text):
        assert rc == BADARG
        msg = lib.pyipm_newton_last_error(h)
        assert msg and text in msg, (msg, text)

    # a single-system handle
    core = NewtonCore(n, me, mi)
    refused(core.lib, core.h, core.lib.pyipm_newton_step_batched_each(core.h, p, p, p, None, p, MEM_DEVICE), b"not a batched handle")
    refused(core.lib, core.h, core.lib.pyipm_newton_step_lengths_batched(core.h, 0.995, p, p, MEM_DEVICE), b"not a batched handle")
    core.close()
    # nothing staged
    bn = BatchedNewton(n, me, mi, batch=B)
    lib, h = bn.lib, bn.h
    refused(lib, h, lib.pyipm_newton_step_batched_each(h, p, p, p, None, p, MEM_DEVICE), b"stage blocks and vectors first")
    refused(lib, h, lib.pyipm_newton_step_lengths_batched(h, 0.995, p, p, MEM_DEVICE), b"stage vectors first")
    # null pointers
    qps = [make_qp(n, me, mi, seed=b) for b in range(B)]
    bn.stage(*[np.stack([q[k] for q in qps]) for k in ("d2L", "Je", "Ji", "df", "ce", "ci", "s", "lam")])
    assert bn.h.value == h.value
    for args in ((None, p, p), (p, None, p), (p, p, None)):
        refused(lib, h, lib.pyipm_newton_step_batched_each(h, *args, None, p, MEM_DEVICE), b"null mu / delta / delta_c")
    refused(lib, h, lib.pyipm_newton_step_batched_each(h, p, p, p, None, None, MEM_DEVICE), b"null output")
    refused(lib, h, lib.pyipm_newton_step_lengths_batched(h, 0.995, p, None, MEM_DEVICE), b"null output")
    # dz = NULL: only after a step whose output was host memory (the handle keeps no copy of a device output)
    refused(lib, h, lib.pyipm_newton_step_lengths_batched(h, 0.995, None, p, MEM_DEVICE), b"pass dz")
    bn.close()


@pytest.mark.gpu
def test_host_arrays_and_the_kept_direction():
    """memkind = host: the parameter arrays and the mask are copied from host memory, only the rows of the active problems are
    written, and step_lengths_batched(dz = NULL) reads the handle's copy of them."""
    import torch
    from pyipm_amd.batched import BatchedNewton
    from pyipm_amd.newton import MEM_HOST
    from pyipm_amd.problems import make_qp
    n, me, mi, B = 20, 4, 12, 3
    N = n + 2 * mi + me
    qps = [make_qp(n, me, mi, seed=40 + b) for b in range(B)]
    bn = BatchedNewton(n, me, mi)
    bn.stage(*[np.stack([q[k] for q in qps]) for k in ("d2L", "Je", "Ji", "df", "ce", "ci", "s", "lam")])
    mu, dl, dc = np.array([0.2, 0.1, 0.05]), np.array([0.0, 1e-3, 1e-5]), np.array([0.0, 1e-9, 0.0])
    want, _ = bn.step_each(mu, dl, dc)
    want_al = bn.step_lengths_all(0.995).cpu().numpy()
    want = want.cpu().numpy()
    dp = lambda a: a.ctypes.data_as(c_void_p)          # noqa: E731
    out = np.full((B, N), -7.0)
    bn._ck(bn.lib.pyipm_newton_step_batched_each(bn.h, dp(mu), dp(dl), dp(dc), None, dp(out), MEM_HOST))
    assert np.array_equal(out, want)
    al = np.zeros((B, 2))
    bn._ck(bn.lib.pyipm_newton_step_lengths_batched(bn.h, 0.995, None, dp(al), MEM_HOST))
    assert np.array_equal(al, want_al)
    act = np.array([0, 1, 0], dtype=np.int32)
    out2 = np.full((B, N), -7.0)
    bn._ck(bn.lib.pyipm_newton_step_batched_each(bn.h, dp(mu), dp(dl * 3.0), dp(dc), dp(act), dp(out2), MEM_HOST))
    assert (out2[[0, 2]] == -7.0).all() and not np.array_equal(out2[1], want[1]) and np.isfinite(out2[1]).all()
    bn.close()
