"""Tensor plumbing shared by the ctypes bindings (``newton``, ``lbfgs``, ``batched``) and ``qp``: PyTorch owns the device
memory, the library gets raw pointers."""
from __future__ import annotations

import os
from ctypes import c_void_p

import numpy as np


def to_device(a, device, shape=None, contiguous=True):
    """``a`` (NumPy / torch / None) as an fp64 tensor on ``device``, reshaped when ``shape`` is given; ``contiguous=False``
    keeps the strides of a torch input (the caller lays it out itself)."""
    import torch
    if a is None:
        return None
    if isinstance(a, torch.Tensor):
        t = a.to(device=device, dtype=torch.float64)
    else:
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64))).to(device)
    if shape is not None:
        t = t.reshape(shape)
    return t.contiguous() if contiguous else t


def rows_to_device(a, device, shape):
    """``a`` as an fp64 tensor of ``shape`` ((rows, width) or (batch, rows, width)) on ``device``, with its strides in doubles
    but the last: (ld,) or (batch stride, ld).  A torch tensor that already has that dtype, device and shape, dense rows
    (``stride(-1) == 1``) that do not overlap (``stride(-2) >= width``) and batch members that do not either
    (``stride(0) >= rows * stride(1)``) is handed on as it is, no copy: the library takes a leading dimension and a batch stride
    for the blocks it retains.  Every other layout is made contiguous as ``to_device`` does."""
    import torch
    shape = tuple(int(k) for k in shape)
    if isinstance(a, torch.Tensor) and a.dtype == torch.float64 and a.device == device and tuple(a.shape) == shape:
        st = tuple(int(k) for k in a.stride())
        if st[-1] == 1 and st[-2] >= shape[-1] and (len(shape) == 2 or st[0] >= shape[1] * st[1]):
            return a, st[:-1]
    t = to_device(a, device, shape)
    return t, ((shape[-1],) if len(shape) == 2 else (shape[1] * shape[2], shape[2]))


def ptr(t):
    return c_void_p(0) if t is None else c_void_p(t.data_ptr())


class RawDeviceArray(object):
    """fp64 device memory at a raw address, as torch.as_tensor understands it (no copy)."""

    def __init__(self, ptr, count):
        self.__cuda_array_interface__ = {"data": (int(ptr), False), "shape": (int(count),), "typestr": "<f8", "version": 2}


def alloc_workspace(nbytes, device):
    """The byte buffer a handle lives in; call it with ``device`` current."""
    import torch
    ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
    if os.environ.get("PYIPM_POISON_WORKSPACE"):     # test hook (tests/conftest.py): every byte the library does not write
        ws.fill_(255)                                # itself reads back as NaN -- zero pages of a fresh process hide such reads
    return ws
