"""Call plumbing shared by ops.py (the autograd hot path) and frame_ops.py (the operators around the network): the loaded
library, pointers, the current stream, the return-code check and the fp32-on-the-device requirement of a kernel operand."""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from . import _lib

_C = _lib.CONSTANTS       # the integer #define DCA_* of include/dca_hip.h
_vp = ctypes.c_void_p


def _L():
    return _lib.load()


def _ptr(t: Optional[torch.Tensor]):
    return _vp(t.data_ptr()) if t is not None else None


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_raw_device = getattr(torch._C, "_cuda_getDevice", None)


def _stream():
    """torch's CURRENT stream on the current device as a hipStream_t (every launch goes there).  The raw C accessors
    cost ~0.3 us against ~9 us for torch.cuda.current_stream() -- there are ~1000 launches per training step."""
    if _raw_stream is not None and _raw_device is not None:
        return _vp(_raw_stream(_raw_device()))
    return _vp(torch.cuda.current_stream().cuda_stream)


def _chk(rc: int, name: str):
    if rc != 0:
        raise RuntimeError(f"{name} failed with hipError_t {rc}")


def _req(t: torch.Tensor, name: str, packed_ok: bool = False) -> torch.Tensor:
    if getattr(t, "_dca_px2", None) is not None and not packed_ok:
        raise RuntimeError(f"{name}: got a tensor in the packed px2 operand format (only the f16x2 3x3x3 stride-1 convolution "
                           "reads it; ask the producer for an fp32 result)")
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(
            f"{name}: the DCANet hot path runs only as HIP kernels on a ROCm device (got "
            f"{'a ' + str(t.device) + ' tensor' if isinstance(t, torch.Tensor) else type(t)}); there is no CPU fallback")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name}: expected float32, got {t.dtype}")
    t = t.contiguous()
    if t.data_ptr() % 16:
        t = t.clone(memory_format=torch.contiguous_format)
    return t


def _req_no_grad(name, *tensors):
    if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in tensors):
        raise RuntimeError(f"{name} is inference only (no backward): call it under torch.no_grad() or detach its inputs")
