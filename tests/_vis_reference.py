"""numpy restatements of the three launchers of csrc/visualize.hip as include/dca_hip.h defines them, in fp32 with every
operation rounded on its own.  Nothing here imports the package: the kernels AND the package's own host restatement
(dcanet_amd/utils/visualization.py) are judged by this file.

  error_image   the reference's utils/visualization.py:31-55 (`disp_error_image_func.forward`) with the table of :13-22
  disp_range    (lo, hi) of the valid pixels of a window
  colorize      the KITTI devkit's disp_to_color pinned in fp32, and the grey map
  devkit_f64    the devkit formula itself in float64 (what the fp32 definition is compared with, within one byte)
"""
import numpy as np

F = np.float32

# visualization.py:13-22: the edges 0.1875 / 3 ... 48 / 3 are 2^-4 ... 2^4, exact in fp32; the colour bytes
ERR_EDGES = np.array([0, 1 / 16, 1 / 8, 1 / 4, 1 / 2, 1, 2, 4, 8, 16, np.inf], dtype=np.float32)
ERR_BYTES = np.array([[49, 54, 149], [69, 117, 180], [116, 173, 209], [171, 217, 233], [224, 243, 248], [254, 224, 144],
                      [253, 174, 97], [244, 109, 67], [215, 48, 39], [165, 0, 38]], dtype=np.uint8)
LEGEND_ROWS, LEGEND_STEP = 10, 20

# the devkit's map: cumulative edges (x 1000), widths and corner colours (r, g, b)
KITTI_C = np.array([0, 114, 299, 413, 587, 701, 886, 1000], dtype=np.float32)
KITTI_W = np.array([114, 185, 114, 174, 114, 185, 114], dtype=np.float32)
KITTI_CORNERS = np.array([[0, 0, 0], [0, 0, 1], [1, 0, 0], [1, 0, 1], [0, 1, 0], [0, 1, 1], [1, 1, 0], [1, 1, 1]], dtype=np.float32)


def error_bins(pred, gt, abs_thres=3.0, rel_thres=0.05, legend=True, top_pad=0):
    """bin index per pixel of gt (B,H,W), -1 = black; pred (B,H+top_pad,>=W): rows padded on top, columns on the right"""
    gt = np.asarray(gt, dtype=np.float32)
    B, H, W = gt.shape
    p = np.asarray(pred, dtype=np.float32)[:, top_pad:top_pad + H, :W]
    mask = gt > 0                                                            # :36
    with np.errstate(all="ignore"):
        e = np.abs(gt - p)                                                   # :38
        err = np.minimum(e / F(abs_thres), (e / gt) / F(rel_thres))          # :40 (np.minimum hands a NaN on)
    bins = np.full(gt.shape, -1, dtype=np.int64)
    for i in range(10):                                                      # :45-46; NaN and +inf fall in no bin
        bins[(err >= ERR_EDGES[i]) & (err < ERR_EDGES[i + 1])] = i
    bins[~mask] = -1                                                         # :49
    if legend:                                                               # :51-53, numpy slicing clips to H and W
        for i in range(10):
            bins[:, :LEGEND_ROWS, i * LEGEND_STEP:(i + 1) * LEGEND_STEP] = i
    return bins


def error_image(pred, gt, abs_thres=3.0, rel_thres=0.05, legend=True, top_pad=0):
    """(float32 planar (B,3,H,W) = float32(byte) / float32(255), uint8 interleaved (B,H,W,3))"""
    bins = error_bins(pred, gt, abs_thres, rel_thres, legend, top_pad)
    u8 = np.where((bins >= 0)[..., None], ERR_BYTES[np.maximum(bins, 0)], np.uint8(0)).astype(np.uint8)
    f32 = u8.astype(np.float32) / F(255)                                     # :23
    return np.ascontiguousarray(f32.transpose(0, 3, 1, 2)), u8


def valid_pixels(d, mask=None, mask_min=0.5):
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(d) & (d > 0)
        if mask is not None:
            ok &= mask >= F(mask_min)
    return ok


def _window(a, window):
    if window is None:
        return a
    y0, rows, cols = window
    return a[..., y0:y0 + rows, :cols]


def disp_range(disp, window=None, mask=None, mask_min=0.5):
    """disp (B,Hc,Wc) -> (B,2) float32 (lo, hi) over the valid pixels of the window (y0, rows, cols); (0, 0) without one"""
    d = _window(np.asarray(disp, dtype=np.float32), window)
    ok = valid_pixels(d, None if mask is None else _window(np.asarray(mask, dtype=np.float32), window), mask_min)
    out = np.zeros((d.shape[0], 2), dtype=np.float32)
    for b in range(d.shape[0]):
        if ok[b].any():
            out[b] = d[b][ok[b]].min(), d[b][ok[b]].max()
    return out


def byte(v):
    return np.rint(v * F(255)).astype(np.uint8)


def kitti_bytes(t):
    """t float32 in [0,1], any shape -> (...,3) uint8"""
    t = np.asarray(t, dtype=np.float32)
    s = t * F(1000)
    ind = (s[..., None] > KITTI_C[1:7]).sum(-1)
    w = (s - KITTI_C[ind]) / KITTI_W[ind]
    a, z = KITTI_CORNERS[ind], KITTI_CORNERS[ind + 1]
    v = np.where(a == z, a, np.where(z > a, w[..., None], F(1) - w[..., None])).astype(np.float32)
    return byte(v)


def gray_bytes(t):
    t = np.asarray(t, dtype=np.float32)
    return np.repeat(byte(t)[..., None], 3, axis=-1)


def colorize(disp, y0, rows, cols, lo, hi, cmap="kitti", mask=None, mask_min=0.5):
    """the rows x cols window at row y0, column 0 of disp (Hc,Wc) -> (rows,cols,3) uint8; (lo, hi) = (0, max_disp) for a
    fixed range"""
    d = np.asarray(disp, dtype=np.float32)[y0:y0 + rows, :cols]
    m = None if mask is None else np.asarray(mask, dtype=np.float32)[y0:y0 + rows, :cols]
    ok = valid_pixels(d, m, mask_min)
    lo, hi = F(lo), F(hi)
    with np.errstate(all="ignore"):
        t = np.minimum(np.maximum((d - lo) / np.maximum(hi - lo, F(1e-5)), F(0)), F(1))
    t = np.where(ok, t, F(0)).astype(np.float32)
    rgb = {"kitti": kitti_bytes, "gray": gray_bytes}[cmap](t)
    rgb[~ok] = 0
    return rgb


def devkit_f64(t):
    """The KITTI devkit's disp_to_color (devkit/matlab/disp_to_color.m) in float64 for I = t in [0,1]: the weights of the
    eight-entry map are normalised by their sum, `ind` counts the inner cumulative edges below I, and the colour is the
    linear blend of two neighbouring corners, clipped to [0,1].  Returns (...,3) float64."""
    t = np.asarray(t, dtype=np.float64)
    weights = np.array([114, 185, 114, 174, 114, 185, 114], dtype=np.float64)
    cum = np.cumsum(weights)
    bins = weights / cum[-1]
    cbins = cum[:-1] / cum[-1]
    ind = np.minimum((t[..., None] > cbins).sum(-1), 6)
    cb = np.concatenate([[0.0], cbins])
    x = (t - cb[ind]) * (1.0 / bins)[ind]
    corners = KITTI_CORNERS.astype(np.float64)
    return np.clip(corners[ind] * (1 - x[..., None]) + corners[ind + 1] * x[..., None], 0.0, 1.0)
