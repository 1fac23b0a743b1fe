"""What ``decomposition`` and ``neighbors`` share on the way to the float64 tile kernels: dense [n, d] inputs and workspace launches."""
import ctypes

import numpy as np
import torch

from . import _lib

DT = {torch.float32: 0, torch.float64: 1}       # BBBP_DTYPE_F32 / BBBP_DTYPE_F64


def stream():
    return torch.cuda.current_stream().cuda_stream


def ld(t):
    """Leading dimension of a [n, d] tensor with unit inner stride."""
    return max(t.stride(0), t.shape[1]) if t.shape[0] > 1 else t.shape[1]


def to_device_matrix(X, device, who, *, allow_row_stride):
    """(device tensor [n, d] float32 / float64 with unit inner stride, was_numpy).  A row / column slice of a larger matrix is used in
    place where ``allow_row_stride``; every other layout is copied to dense rows."""
    was_numpy = not isinstance(X, torch.Tensor)
    if was_numpy:
        X = np.asarray(X)
        if X.dtype not in (np.float32, np.float64):
            X = X.astype(np.float64)
        X = torch.from_numpy(np.ascontiguousarray(X))
    elif not X.is_cuda:
        raise RuntimeError(f"{who}: expected a CUDA (HIP) tensor or a numpy array, got a tensor on {X.device} (no CPU fallback)")
    if X.dim() != 2:
        raise ValueError(f"{who}: expected a 2-D [n, d] input, got shape {tuple(X.shape)}")
    X = (X if X.dtype in DT else X.to(torch.float64)).to(device)
    in_place = allow_row_stride and (X.shape[1] == 1 or X.stride(1) == 1) and (X.shape[0] <= 1 or X.stride(0) >= X.shape[1])
    return (X if in_place else X.contiguous()), was_numpy


def launch_with_workspace(query_fn, run_fn, desc, device, what):
    """Ask ``query_fn(desc)`` for the workspace bytes, allocate them on ``device``, ``run_fn(stream, desc, workspace, bytes)``, check."""
    nbytes = query_fn(ctypes.byref(desc))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=device) if nbytes else None
    _lib.check(run_fn(stream(), ctypes.byref(desc), None if ws is None else ws.data_ptr(), nbytes), what)
