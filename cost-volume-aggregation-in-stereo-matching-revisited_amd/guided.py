"""Guided stereo around the network (Poggi et al., CVPR 2019): `hints_to_quarter`, the wrapper of the
downsample launch (ops.py re-exports it; it uses frame_ops.py's argument checks and lives here because the set of public
functions of frame_ops.py is pinned by its launch trace), the numpy restatements of csrc/guided.hip as include/dca_hip.h
defines them, and the one check of the guide parameters that the device operators share.

`hints_to_quarter_host` is bitwise what `ops.hints_to_quarter` gives (compares and one exact multiply);
`volume_modulate_host` evaluates the factor in np.float32 in the kernel's order (np.exp on float32 in place of expf: equal to
the last bits, not bitwise)."""
from __future__ import annotations

import math

import numpy as np
import torch

from ._call import _L, _chk, _ptr, _req_no_grad, _stream
from .frame_ops import _fit, _out, _req_dev

GUIDE = (10.0, 1.0)      # (k, c) in quarter-resolution bins: the paper's values


def guide_params(name, guide):
    """(k, c) -> (k, 1 / (2 c^2)) as the kernels take them: both positive and finite; 1 / (2 c^2) is formed in float64 and
    has to be a positive finite float32 too"""
    try:
        k, c = (float(v) for v in guide)
    except (TypeError, ValueError):
        raise RuntimeError(f"{name}: guide is (k, c), got {guide!r}") from None
    if not (0.0 < k < math.inf and 0.0 < c < math.inf):
        raise RuntimeError(f"{name}: guide (k, c) must be positive and finite, got {(k, c)}")
    i2c2 = 1.0 / (2.0 * c * c)
    with np.errstate(over="ignore", under="ignore"):
        fits = 0.0 < float(np.float32(i2c2)) < math.inf and float(np.float32(k)) < math.inf
    if not fits:
        raise RuntimeError(f"{name}: guide (k, c) = {(k, c)} does not fit float32")
    return k, i2c2


def _placement(name, hw, frame_hw, placement):
    """(h, w), (Hc, Wc), (src_y0, dst_y0, rows, cols) or None -> the four window numbers, checked"""
    (h, w), (Hc, Wc) = (int(hw[0]), int(hw[1])), (int(frame_hw[0]), int(frame_hw[1]))
    if Hc <= 0 or Wc <= 0 or Hc % 4 or Wc % 4:
        raise RuntimeError(f"{name}: the frame must be a positive multiple of 4 in both directions, got {Hc} x {Wc}")
    if placement is None:
        if (h, w) != (Hc, Wc):
            raise RuntimeError(f"{name}: without a placement the {h} x {w} map must have the frame's size {Hc} x {Wc}")
        return 0, 0, Hc, Wc
    try:
        src_y0, dst_y0, rows, cols = (int(v) for v in placement)
    except (TypeError, ValueError):
        raise RuntimeError(f"{name}: placement is (src_y0, dst_y0, rows, cols), got {placement!r}") from None
    if min(src_y0, dst_y0) < 0 or min(rows, cols) < 1 or src_y0 + rows > h or cols > w or dst_y0 + rows > Hc or cols > Wc:
        raise RuntimeError(f"{name}: the {rows} x {cols} window from source row {src_y0} to frame row {dst_y0} does not fit "
                           f"the {h} x {w} map and the {Hc} x {Wc} frame")
    return src_y0, dst_y0, rows, cols


def hints_to_quarter_host(hints, frame_hw, placement=None, maxdisp=192, count=False):
    """hints (B,h,w) or (h,w) float32, a disparity in pixels, +0.0 where nothing was measured -> hints4 (B,Hc/4,Wc/4) or
    (Hc/4,Wc/4): per 4 x 4 block of the frame, 0.25 * the largest valid hint (0 < h < maxdisp) of the block's pixels inside
    the image window, +0.0 if there is none.  count=True: (hints4, the number of cells that hold a hint)."""
    hints = np.asarray(hints)
    if hints.dtype != np.float32 or hints.ndim not in (2, 3):
        raise RuntimeError(f"hints_to_quarter_host: expected a float32 (B,h,w) or (h,w) map, got {hints.dtype} {hints.shape}")
    src = hints if hints.ndim == 3 else hints[None]
    B, h, w = src.shape
    Hc, Wc = int(frame_hw[0]), int(frame_hw[1])
    src_y0, dst_y0, rows, cols = _placement("hints_to_quarter_host", (h, w), frame_hw, placement)
    maxdisp = np.float32(maxdisp)
    if not maxdisp > 0:
        raise RuntimeError("hints_to_quarter_host: maxdisp must be positive")
    frame = np.zeros((B, Hc, Wc), np.float32)
    win = src[:, src_y0:src_y0 + rows, :cols]
    with np.errstate(invalid="ignore"):
        frame[:, dst_y0:dst_y0 + rows, :cols] = np.where((win > 0) & (win < maxdisp), win, np.float32(0))
    out = np.float32(0.25) * frame.reshape(B, Hc // 4, 4, Wc // 4, 4).max(axis=(2, 4))
    out = out if hints.ndim == 3 else out[0]
    return (out, int((out > 0).sum())) if count else out


def guide_factor_host(D, hints4, guide=GUIDE):
    """m(d, h4) for d = 0 .. D-1 over a (..., H, W) float32 hint map -> (..., D, H, W) float32, in the kernel's order:
    t = float(d) - h4;  e = (t * t) * i2c2;  m = h4 > 0 ? k * exp(-e) : 1"""
    k, i2c2 = guide_params("guide_factor_host", guide)
    h4 = np.asarray(hints4, np.float32)[..., None, :, :]
    d = np.arange(D, dtype=np.float32).reshape(D, 1, 1)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        t = d - h4
        e = (t * t) * np.float32(i2c2)
        m = np.float32(k) * np.exp(-e)
        return np.where(h4 > 0, m, np.float32(1)).astype(np.float32)


def volume_modulate_host(volume, hints4, guide=GUIDE):
    """volume (B,C,D,H,W) float32 times m(d, hints4[b,y,x]), hints4 (B,H,W) float32"""
    volume, hints4 = np.asarray(volume), np.asarray(hints4)
    if volume.dtype != np.float32 or volume.ndim != 5 or hints4.dtype != np.float32 or \
            hints4.shape != (volume.shape[0],) + volume.shape[3:]:
        raise RuntimeError(f"volume_modulate_host: expected a float32 (B,C,D,H,W) volume and (B,H,W) hints, got "
                           f"{volume.dtype} {volume.shape} and {hints4.dtype} {hints4.shape}")
    return volume * guide_factor_host(volume.shape[2], hints4, guide)[:, None]


# ---- the device operator (csrc/guided.hip); what multiplies the cost volume is on the hot path: ops.cost_volume(hints4=) -----
def hints_to_quarter(hints, frame_hw, placement=None, maxdisp=192, out=None, count=False):
    """hints (B,h,w) or (h,w) float32 on the device -- a disparity in pixels, +0.0 where nothing was measured -- through
    placement = (src_y0, dst_y0, rows, cols) (`inference.placement`; None: the map has the frame's size) -> hints4
    (B,Hc/4,Wc/4) or (Hc/4,Wc/4): per 4 x 4 block of the frame 0.25 * the largest valid hint (0 < h < maxdisp; a NaN or an
    infinity is none), +0.0 where the block holds none.  One launch; every cell is written (definitions: include/dca_hip.h,
    dca_hints_to_quarter; `guided.hints_to_quarter_host` is the numpy restatement, equal bit for bit).  count: True or a
    (1,) int64 buffer: returns (hints4, count), the number of cells that hold a hint, on the device (a second launch).
    With `out` (and a count buffer) given nothing is allocated: the launches can be captured into a hipGraph."""
    name = "hints_to_quarter"
    _req_no_grad(name, hints)
    _req_dev(hints, name, "hints", torch.float32)
    if hints.dim() not in (2, 3) or hints.numel() == 0:
        raise RuntimeError(f"{name}: expected a (B,h,w) or (h,w) map, got {tuple(hints.shape)}")
    B = int(hints.shape[0]) if hints.dim() == 3 else 1
    h, w = int(hints.shape[-2]), int(hints.shape[-1])
    Hc, Wc = int(frame_hw[0]), int(frame_hw[1])
    if Hc <= 0 or Wc <= 0 or Hc % 4 or Wc % 4:
        raise RuntimeError(f"{name}: the frame must be a positive multiple of 4 in both directions, got {Hc} x {Wc}")
    if placement is None:
        if (h, w) != (Hc, Wc):
            raise RuntimeError(f"{name}: without a placement the {h} x {w} map must have the frame's size {Hc} x {Wc}")
        placement = (0, 0, Hc, Wc)
    try:
        src_y0, dst_y0, rows, cols = placement
    except (TypeError, ValueError):
        raise RuntimeError(f"{name}: placement is (src_y0, dst_y0, rows, cols), got {placement!r}") from None
    src_y0, _, rows, cols = _fit(name, h, w, src_y0, 0, rows, cols, "source")
    dst_y0 = _fit(name, Hc, Wc, dst_y0, 0, rows, cols, "frame")[0]
    maxdisp = float(maxdisp)
    if not maxdisp > 0:
        raise RuntimeError(f"{name}: maxdisp must be positive, got {maxdisp}")
    shape = (B, Hc // 4, Wc // 4) if hints.dim() == 3 else (Hc // 4, Wc // 4)
    out = _out(name, "out", out, torch.float32, shape, hints, alias=(hints,))
    cnt = None
    if count is not False and count is not None:
        cnt = _out(name, "count", None if count is True else count, torch.int64, (1,), hints)
    with torch.cuda.device_of(hints):
        _chk(_L().dca_hints_to_quarter(_ptr(hints), _ptr(out), _ptr(cnt), B, h, w, Hc, Wc, src_y0, dst_y0, rows, cols, maxdisp,
                                       _stream()), "dca_hints_to_quarter")
    return out if cnt is None else (out, cnt)
