"""What every front end does to hand a tensor to the C ABI, each stated once: pointers, stride arrays, the current stream and the
workspace check.  ``augment``, ``color``, ``render``, ``validation``, ``evaluation`` and ``voting`` take them from here."""
from __future__ import annotations

import ctypes as C


def ptr(t):
    """the data pointer of a tensor as ``c_void_p``; None stays None (an optional argument)"""
    return None if t is None else C.c_void_p(t.data_ptr())


def strides(t, dims):
    """the strides of the chosen dimensions (a tuple of them, or a count for the first ``dims``) as an int64 array"""
    dims = range(dims) if isinstance(dims, int) else dims
    return (C.c_int64 * len(dims))(*[int(t.stride(d)) for d in dims])


def opt_strides(t, dims):
    return None if t is None else strides(t, dims)


def stream(dev=None):
    """the current stream of a device as ``c_void_p``"""
    import torch
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def nbytes(t) -> int:
    return t.numel() * t.element_size()


def workspace(ws, need, dev, least=0, align=0, sized=False):
    """the caller's workspace checked, or a new one of ``max(need, least)`` bytes.  A caller's must be a contiguous CUDA tensor on
    ``dev``; with ``align`` also aligned to that many bytes, with ``sized`` also of at least ``need`` bytes (otherwise the library
    answers PVNET_E_WORKSPACE itself)."""
    import torch
    if ws is None:
        return torch.empty(max(need, least), dtype=torch.uint8, device=dev)
    if not (isinstance(ws, torch.Tensor) and ws.is_cuda and ws.device == dev and ws.is_contiguous() and
            (not align or ws.data_ptr() % align == 0)):
        raise RuntimeError(f"workspace must be a contiguous{f', {align}-byte aligned' if align else ''} CUDA tensor on {dev}")
    if sized and nbytes(ws) < need:
        raise RuntimeError(f"workspace too small: {nbytes(ws)} < {need} bytes")
    return ws
