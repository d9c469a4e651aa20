"""High-resolution pairs (csrc/highres.hip): an integer-factor area downscale of the uint8 pair and of
a ground-truth disparity in front of the network -- the arithmetic of the reference's myImageFloder_middlebury_additional
(dataloader/datasets.py:547-673: cv2.INTER_AREA at fx = fy = 0.5, the disparity resized the same way and multiplied by
resize_scale) -- and joint bilateral upsampling (Kopf et al. 2007) of the network's disparity under the full-resolution left
image behind it, which the reference does not have.  A Middlebury-F pair (about 2000 x 2964, disparities up to ~800) fits
neither the frame nor maxdisp = 192 unless it is downscaled; with a factor s the disparity range becomes s * maxdisp.

`area_downscale_pair`, `area_downscale_disp` and `guided_upsample` are the device wrappers (ops.py re-exports them), after
the conventions of frame_ops.py: a refusal names the operator, a tensor that is not on a ROCm device is an error, nothing is
allocated with `out=` given, no launch synchronises.  `area_downscale_pair_host`, `area_downscale_disp_host` and
`guided_upsample_host` restate the definitions of include/dca_hip.h in numpy, one float32 operation at a time: the CPU path
and the yardstick the kernels equal bit for bit (tests/test_gpu_highres.py).  `jbu_tables` makes the two weight tables of the
upsampler on the host; the device evaluates no transcendental function."""
from __future__ import annotations

import numpy as np
import torch

from ._call import _C, _L, _chk, _ptr, _req_no_grad, _stream
from .frame_ops import _mask_min, _maps, _out, _out_dict, _overlap, _req_dev, _req_u8, _req_u8_pair, _window

HR_MAX_SCALE = _C["DCA_HR_MAX_SCALE"]
HR_MAX_RADIUS = _C["DCA_HR_MAX_RADIUS"]
HR_RANGE_LEN = _C["DCA_HR_RANGE_LEN"]
HR_TILE = (_C["DCA_HR_TILE_H"], _C["DCA_HR_TILE_W"])
UPSAMPLE_OUTPUTS = ("disp", "valid")
_UPSAMPLE_KINDS = dict.fromkeys(UPSAMPLE_OUTPUTS, torch.float32)


def _scale(name, scale, exc=RuntimeError):
    """the factor as an int in 2..HR_MAX_SCALE"""
    if isinstance(scale, bool) or not isinstance(scale, (int, np.integer)) or not 2 <= int(scale) <= HR_MAX_SCALE:
        raise exc(f"{name}: scale is an integer in 2..{HR_MAX_SCALE}, got {scale!r}")
    return int(scale)


def small_hw(H, W, scale):
    """(ceil(H / scale), ceil(W / scale)): the size of the downscaled image"""
    return -(-int(H) // scale), -(-int(W) // scale)


# ------------------------------------------------------------------------------------------------
# The weight tables
# ------------------------------------------------------------------------------------------------
def jbu_tables(scale, radius=2, sigma_s=1.0, sigma_r=24.0, floor=1e-4):
    """(ws (scale, 2 radius + 1), wr (HR_RANGE_LEN,)) float32, the tables `guided_upsample` takes:
      ws[p][t + r] = exp(-(t - ((p + 0.5) / s - 0.5))^2 / (2 sigma_s^2))     the spatial weight, along one axis, of the tap t
                     low-resolution pixels from the one under an output pixel of phase p = y % s: the distance between the
                     tap's centre and the output pixel's, in low-resolution pixels
      wr[k]        = max(exp(-k^2 / (2 sigma_r^2)), floor)                   the range weight of a colour difference
                     k = |dR| + |dG| + |dB|
    both computed in float64 and rounded once.  The offset is formed as (2 p + 1 - s) / (2 s), the same number with an
    integer numerator, so that ws[p][t + r] == ws[s - 1 - p][r - t] holds exactly.  The floor keeps a pixel whose colour
    matches none of its neighbours from becoming a hole while any tap is active.  The defaults are those of a synthetic
    two-surface experiment (tests/test_highres_cpu.py); they were NOT tuned on real data."""
    s = _scale("jbu_tables", scale, ValueError)
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 1 <= int(radius) <= HR_MAX_RADIUS:
        raise ValueError(f"jbu_tables: radius is an integer in 1..{HR_MAX_RADIUS}, got {radius!r}")
    r = int(radius)
    sigma_s, sigma_r, floor = float(sigma_s), float(sigma_r), float(floor)
    if not (0.0 < sigma_s < np.inf and 0.0 < sigma_r < np.inf and 0.0 <= floor <= 1.0):
        raise ValueError(f"jbu_tables: sigma_s and sigma_r positive and finite, 0 <= floor <= 1, got {sigma_s}, {sigma_r}, {floor}")
    p = np.arange(s, dtype=np.float64)[:, None]
    t = np.arange(-r, r + 1, dtype=np.float64)[None, :]
    ws = np.exp(-(t - (2.0 * p + 1.0 - s) / (2.0 * s)) ** 2 / (2.0 * sigma_s * sigma_s))
    k = np.arange(HR_RANGE_LEN, dtype=np.float64)
    wr = np.maximum(np.exp(-(k * k) / (2.0 * sigma_r * sigma_r)), floor)
    return ws.astype(np.float32), wr.astype(np.float32)


# ------------------------------------------------------------------------------------------------
# numpy restatements of include/dca_hip.h
# ------------------------------------------------------------------------------------------------
def _block_counts(n, s):
    """pixels per block along an axis of n pixels: s, fewer in the last partial block"""
    return np.minimum(n, (np.arange(-(-n // s)) + 1) * s) - np.arange(-(-n // s)) * s


def _u8_image(name, img):
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] not in (3, 4) or img.size == 0:
        raise ValueError(f"{name}: expected a non-empty (H,W,3) or (H,W,4) uint8 image, got {img.dtype} {img.shape}")
    return img


def area_downscale_pair_host(left, right, scale):
    """dca_area_downscale_u8: (H,W,C) uint8 x2 -> (2,h,w,C) uint8, every byte (sum + cnt // 2) // cnt over the pixels of its
    scale x scale block that exist.  A full 2x2 block gives (a + b + c + d + 2) >> 2, OpenCV's INTER_AREA for uint8."""
    name = "area_downscale_pair_host"
    s = _scale(name, scale, ValueError)
    left, right = _u8_image(name, left), _u8_image(name, right)
    if left.shape != right.shape:
        raise ValueError(f"{name}: expected two images of one shape, got {left.shape} and {right.shape}")
    H, W, C = left.shape
    h, w = small_hw(H, W, s)
    cnt = (_block_counts(H, s)[:, None] * _block_counts(W, s)[None, :]).astype(np.int64)[:, :, None]
    out = np.empty((2, h, w, C), np.uint8)
    for n, img in enumerate((left, right)):
        padded = np.zeros((h * s, w * s, C), np.int64)
        padded[:H, :W] = img
        total = padded.reshape(h, s, w, s, C).sum(axis=(1, 3))
        out[n] = ((total + cnt // 2) // cnt).astype(np.uint8)
    return out


def area_downscale_disp_host(disp, scale, inf_to_zero=True, flip_rows=False):
    """dca_area_downscale_f32: (H,W) float32 -> (h,w) float32 = (sum / float32(cnt)) / float32(scale), the sum over the
    block's existing pixels in row-major order in float32; inf_to_zero: a result that is not finite becomes 0 (the mean is
    taken with the infinities in it, datasets.py:593-604); flip_rows: a bottom-up PFM payload."""
    name = "area_downscale_disp_host"
    s = _scale(name, scale, ValueError)
    d = np.asarray(disp)
    if d.dtype != np.float32 or d.ndim != 2 or d.size == 0:
        raise ValueError(f"{name}: expected a non-empty (H,W) float32 disparity, got {d.dtype} {d.shape}")
    if flip_rows:
        d = d[::-1]
    H, W = d.shape
    with np.errstate(invalid="ignore", over="ignore"):
        acc = d[0::s, 0::s].copy()                               # every block has its first pixel
        for dy in range(s):
            for dx in range(s):
                if dy or dx:
                    part = d[dy::s, dx::s]
                    acc[:part.shape[0], :part.shape[1]] = acc[:part.shape[0], :part.shape[1]] + part
        cnt = (_block_counts(H, s)[:, None] * _block_counts(W, s)[None, :]).astype(np.float32)
        out = (acc / cnt) / np.float32(s)
        assert out.dtype == np.float32
        if inf_to_zero:
            out[~(np.abs(out) < np.inf)] = 0
    return out


def _tables(name, tables, s, exc):
    """(ws, wr, r) from tables = (ws (s, 2r+1), wr (HR_RANGE_LEN,)); the caller checks dtype and device"""
    try:
        ws, wr = tables
        ok = ws.ndim == 2 and wr.ndim == 1
    except (TypeError, ValueError, AttributeError):
        ok = False
    if not ok:
        raise exc(f"{name}: tables is the (ws, wr) pair of `highres.jbu_tables`")
    r = (ws.shape[1] - 1) // 2
    if ws.shape[0] != s or ws.shape[1] != 2 * r + 1 or not 1 <= r <= HR_MAX_RADIUS or wr.shape[0] != HR_RANGE_LEN:
        raise exc(f"{name}: tables must be ws ({s}, 2 r + 1) with a radius r in 1..{HR_MAX_RADIUS} and wr ({HR_RANGE_LEN},), "
                  f"got {tuple(ws.shape)} and {tuple(wr.shape)}")
    return ws, wr, r


def _fits(name, H, W, s, rows, cols, exc):
    if small_hw(H, W, s) != (rows, cols):
        raise exc(f"{name}: a {H} x {W} guide_hi has {small_hw(H, W, s)[0]} x {small_hw(H, W, s)[1]} blocks of {s} x {s}, "
                  f"the low-resolution window is {rows} x {cols}")


def guided_upsample_host(disp_lo, guide_lo, guide_hi, scale, tables, window=None, mask=None, mask_min=0.5,
                         outputs=UPSAMPLE_OUTPUTS, counts=False):
    """dca_guided_upsample: disp_lo (Hc,Wc) float32 with the window (y0, rows, cols) (default whole), guide_lo (rows,cols,C)
    and guide_hi (H,W,C) uint8, tables of `jbu_tables` -> {"disp": (H,W) float32, "valid": (H,W) float32 of 0 / 1}.  For the
    output pixel (y,x) the taps (y // s + a, x // s + b), a (outer) and b (inner) from -r to r, that are active -- inside the
    window, a finite disparity > 0, mask absent or >= mask_min -- are added in that order, in float32:
      wgt = (ws[y % s][a + r] * ws[x % s][b + r]) * wr[|dR| + |dG| + |dB|];  num += wgt * d;  den += wgt
    and disp = (num / den) * float32(s), valid = 1 where den > 0, both 0 elsewhere.  counts=True adds "taps": the number of
    active taps of every pixel (int32), for tests."""
    name = "guided_upsample_host"
    s = _scale(name, scale, ValueError)
    d = np.asarray(disp_lo)
    if d.ndim == 4 and d.shape[:2] == (1, 1):
        d = d[0, 0]
    if d.dtype != np.float32 or d.ndim != 2 or d.size == 0:
        raise ValueError(f"{name}: expected a non-empty (Hc,Wc) float32 disparity, got {d.dtype} {d.shape}")
    Hc, Wc = d.shape
    y0, rows, cols = (0, Hc, Wc) if window is None else (int(v) for v in window)
    if y0 < 0 or rows <= 0 or cols <= 0 or y0 + rows > Hc or cols > Wc:
        raise ValueError(f"{name}: the {rows} x {cols} window at row {y0} does not fit the {Hc} x {Wc} map")
    glo, ghi = _u8_image(name, guide_lo), _u8_image(name, guide_hi)
    H, W, C = ghi.shape
    if glo.shape != (rows, cols, C):
        raise ValueError(f"{name}: guide_lo must be ({rows},{cols},{C}), got {glo.shape}")
    _fits(name, H, W, s, rows, cols, ValueError)
    ws, wr, r = _tables(name, tuple(np.asarray(t) for t in tables), s, ValueError)
    if ws.dtype != np.float32 or wr.dtype != np.float32:
        raise ValueError(f"{name}: the tables are float32, got {ws.dtype} and {wr.dtype}")
    if any(k not in UPSAMPLE_OUTPUTS for k in outputs) or not outputs:
        raise ValueError(f"{name}: outputs are chosen from {UPSAMPLE_OUTPUTS}, got {tuple(outputs)}")
    win = d[y0:y0 + rows, :cols]
    with np.errstate(invalid="ignore"):
        active = (np.abs(win) < np.inf) & (win > 0)
        if mask is not None:
            m = np.asarray(mask)
            if m.dtype != np.float32 or m.size != d.size or m.shape[-2:] != d.shape or np.isnan(mask_min):
                raise ValueError(f"{name}: the mask must be float32 of the map's shape {d.shape} and mask_min no NaN")
            m = m.reshape(d.shape)
            active &= m[y0:y0 + rows, :cols] >= np.float32(mask_min)
    dz = np.where(active, win, np.float32(0))
    lo = glo[:, :, :3].astype(np.int32)
    hi = ghi[:, :, :3].astype(np.int32)
    ys, xs = np.arange(H), np.arange(W)
    J, I, py, px = ys // s, xs // s, ys % s, xs % s
    num = np.zeros((H, W), np.float32)
    den = np.zeros((H, W), np.float32)
    taps = np.zeros((H, W), np.int32)
    for a in range(-r, r + 1):
        ja = J + a
        for b in range(-r, r + 1):
            ib = I + b
            inside = ((ja >= 0) & (ja < rows))[:, None] & ((ib >= 0) & (ib < cols))[None, :]
            jc, ic = np.clip(ja, 0, rows - 1)[:, None], np.clip(ib, 0, cols - 1)[None, :]
            act = inside & active[jc, ic]
            k = np.abs(hi - lo[jc, ic]).sum(axis=2)
            wgt = (ws[py, a + r][:, None] * ws[px, b + r][None, :]) * wr[k]
            assert wgt.dtype == np.float32
            num = np.where(act, num + wgt * dz[jc, ic], num)
            den = np.where(act, den + wgt, den)
            taps += act
    ok = den > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        disp = np.where(ok, (num / den) * np.float32(s), np.float32(0)).astype(np.float32)
    res = {"disp": disp, "valid": ok.astype(np.float32)}
    res = {k: res[k] for k in UPSAMPLE_OUTPUTS if k in outputs}
    if counts:
        res["taps"] = taps
    return res


# ------------------------------------------------------------------------------------------------
# Device wrappers
# ------------------------------------------------------------------------------------------------
def _own(name, what, t, inputs):
    """t overlaps no tensor of `inputs` (the operator is not in place; two outputs may be parts of one buffer)"""
    if any(i is not None and _overlap(t, i) for i in inputs):
        raise RuntimeError(f"{name}: {what} must be a buffer of its own: it must not alias an input (the operator is not in place)")


def area_downscale_pair(left_u8, right_u8, scale, out=None):
    """Both (H,W,C) uint8 images of a pair, C = 3 or 4, through an area downscale by the integer `scale` in 2..4, ONE launch
    (definitions: include/dca_hip.h, dca_area_downscale_u8; `area_downscale_pair_host` is the numpy restatement, equal bit
    for bit).  Returns the (2,h,w,C) uint8 tensor (left, right), h = ceil(H / scale), w = ceil(W / scale); out: a buffer of
    that shape to write into, not an input."""
    name = "area_downscale_pair"
    s = _scale(name, scale)
    H, W, C = _req_u8_pair(left_u8, right_u8, name)
    if left_u8.device != right_u8.device:
        raise RuntimeError(f"{name}: the two images must be on one device")
    h, w = small_hw(H, W, s)
    out = _out(name, "out", out, torch.uint8, (2, h, w, C), left_u8, alias=(left_u8, right_u8))
    with torch.cuda.device_of(left_u8):
        _chk(_L().dca_area_downscale_u8(_ptr(left_u8), _ptr(right_u8), _ptr(out), H, W, C, s, _stream()),
             "dca_area_downscale_u8")
    return out


def area_downscale_disp(disp, scale, inf_to_zero=True, flip_rows=False, out=None):
    """A ground-truth disparity map (H,W) float32 through the same area downscale, in pixels of the small image: the mean of
    every block divided by `scale`, one launch (definitions: include/dca_hip.h, dca_area_downscale_f32;
    `area_downscale_disp_host` is the numpy restatement, equal bit for bit).  inf_to_zero: a result that is not finite becomes
    0 (the Middlebury loaders); flip_rows: the source is a bottom-up PFM payload.  Returns float32 (h,w); out: a buffer of
    that shape to write into, not the input."""
    name = "area_downscale_disp"
    s = _scale(name, scale)
    _req_no_grad(name, disp)
    _req_dev(disp, name, "the disparity", torch.float32)
    if disp.dim() != 2 or disp.numel() == 0 or disp.numel() >= 1 << 31:
        raise RuntimeError(f"{name}: expected a non-empty (H,W) disparity of fewer than 2^31 pixels, got {tuple(disp.shape)}")
    H, W = int(disp.shape[0]), int(disp.shape[1])
    out = _out(name, "out", out, torch.float32, small_hw(H, W, s), disp, alias=(disp,))
    with torch.cuda.device_of(disp):
        _chk(_L().dca_area_downscale_f32(_ptr(disp), _ptr(out), H, W, s, int(bool(inf_to_zero)), int(bool(flip_rows)),
                                         _stream()), "dca_area_downscale_f32")
    return out


def device_tables(tables, device):
    """the (ws, wr) pair of `jbu_tables` as contiguous float32 tensors on `device`"""
    ws, wr = tables
    return tuple(torch.from_numpy(np.array(t, dtype=np.float32)).to(device) for t in (ws, wr))


def guided_upsample(disp_lo, guide_lo, guide_hi, scale, tables, window=None, mask=None, mask_min=0.5, outputs=UPSAMPLE_OUTPUTS,
                    out=None):
    """Joint bilateral upsampling of ONE low-resolution disparity map by the integer `scale` in 2..4 under the full-resolution
    left image, one launch (definitions: include/dca_hip.h, dca_guided_upsample; `guided_upsample_host` is the numpy
    restatement, equal bit for bit).  disp_lo: (Hc,Wc) / (1,1,Hc,Wc) float32, the padded network frame; window = (y0, rows,
    cols): the image inside it (default whole) -- nothing outside is read as a tap; guide_lo (rows,cols,C) uint8, the
    downscaled left image (`area_downscale_pair(...)[0]`); guide_hi (H,W,C) uint8 with ceil(H / scale) == rows and
    ceil(W / scale) == cols; tables: `device_tables(jbu_tables(scale, radius, ...), device)`; mask: float32 shaped like
    disp_lo, taps below mask_min take no part.  Returns a dict with the keys of `outputs`:
      disp   (H,W) float32  the upsampled disparity in FULL-resolution pixels (values times scale), +0.0 without an active tap
      valid  (H,W) float32  1.0 where at least one tap was active, 0.0 elsewhere
    out: a dict of buffers for some or all of them, none of them an input.  With `out` given nothing is allocated and the
    host never waits: the launch can be captured into a hipGraph.  Bitwise reproducible."""
    name = "guided_upsample"
    s = _scale(name, scale)
    _, Hc, Wc = _maps(name, disp_lo, mask, False)
    y0, rows, cols = _window(name, Hc, Wc, window, "map")
    mask_min = _mask_min(name, mask_min, mask is not None)
    H, W, C = _req_u8(guide_hi, name, "guide_hi", like=disp_lo)
    _req_dev(guide_lo, name, "guide_lo", torch.uint8, (rows, cols, C), like=disp_lo)
    _fits(name, H, W, s, rows, cols, RuntimeError)
    ws, wr, r = _tables(name, tables, s, RuntimeError)
    _req_dev(ws, name, "tables[0] (ws)", torch.float32, like=disp_lo)
    _req_dev(wr, name, "tables[1] (wr)", torch.float32, like=disp_lo)
    if not outputs:
        raise RuntimeError(f"{name}: outputs are chosen from {UPSAMPLE_OUTPUTS}, got none")
    res = _out_dict(name, _UPSAMPLE_KINDS, (), outputs, out, lambda k: (H, W), disp_lo)
    for k, t in res.items():
        _own(name, f"out[{k!r}]", t, (disp_lo, mask, guide_lo, guide_hi, ws, wr) + tuple(o for j, o in res.items() if j != k))
    with torch.cuda.device_of(disp_lo):
        _chk(_L().dca_guided_upsample(_ptr(disp_lo), _ptr(mask), _ptr(guide_lo), _ptr(guide_hi), _ptr(ws), _ptr(wr),
                                      _ptr(res.get("disp")), _ptr(res.get("valid")), Hc, Wc, y0, rows, cols, H, W, C, s, r,
                                      mask_min, _stream()), "dca_guided_upsample")
    return res
