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
