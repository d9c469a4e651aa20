"""Stixels -- per-column ground / object / sky segments from disparity -- on the host, numpy only: the restatement of
include/dca_hip.h (dca_stixels) that the kernels of csrc/stixel.hip equal bit for bit (tests/test_gpu_stixel.py), and the
documented CPU path for a user without a ROCm device; below it the operator itself, `stixels` (`ops.stixels`), which takes
device tensors and has no CPU fallback, and `stixels_metric`, which turns a read-back list into metres.  DESIGN.md section 6q.

The frame is that of ground.py: ONE map (Hc,Wc) or a batch (B,Hc,Wc) / (B,1,Hc,Wc) of independent float32 maps, an optional mask
of the same shape with `mask_min`, an optional window (y0, rows, cols), and the plane record(s) of `ground_plane`.  All of the
energy is integer arithmetic in units of 1/16 px and (1/16 px)^2; the one float32 formula, the road's disparity at a cell's
centre, is evaluated one numpy operation at a time."""
from __future__ import annotations

import math

import numpy as np
import torch

from . import ground as G
from ._call import _C, _L, _chk, _ptr, _stream
from .frame_ops import POSTFILTER_MAX_BATCH, _out_dict, _pf_frame, _req_dev

GROUND, OBJECT, SKY, NONE = 0, 1, 2, 3          # the classes; NONE: "no segment below" in a back-pointer
CLASSES = ("ground", "object", "sky")
MAX_WIDTH = 16                                 # DCA_STIXEL_MAX_WIDTH
MAX_ROW_STEP = 8                               # DCA_STIXEL_MAX_ROW_STEP
MAX_CELLS = 1024                               # DCA_STIXEL_MAX_CELLS: cells per column
MAX_SEGMENTS = 64                              # DCA_STIXEL_MAX_SEGMENTS: the longest list
MAX_CONST = 1 << 20                            # DCA_STIXEL_MAX_CONST: every constant of the energy (every total stays below 2^39)
NO_CLASS = 255                                 # DCA_STIXEL_NO_CLASS: seg_class without a segmentation
STIXEL_OUTPUTS = ("cells", "seg_class", "seg_disp", "count", "stixels", "energy")

# defaults, in sixteenths of a pixel and their squares
STIXEL_WIDTH = 5
STIXEL_ROW_STEP = 1
STIXEL_MIN_VALID = 1
STIXEL_MAX_SEGMENTS = 16
STIXEL_TG = 1024                               # the truncation of a ground cell's squared deviation: 2 px
STIXEL_TS = 1024                               # ... and of a sky cell's
STIXEL_EPS = 16                                # an object's foot may miss the road by 1 px
STIXEL_BELOW = 2048                            # an object whose foot would lie under the road
STIXEL_FLOAT = 512                             # an object that hangs in the air behind the road
STIXEL_SEG = (256, 384, 256)                   # per segment of every class
STIXEL_MU_MIN = 16                             # an object nearer to infinity than 1 px ...
STIXEL_FAR = 2048                              # ... pays this: without it a noisy sky is a far object, which fits its own mean
STIXEL_FIRST = (0, 0, 0)                       # the bottom segment of every class
STIXEL_T = ((-1, 0, 0), (0, 0, 0), (-1, -1, -1))       # T[cp][c]; -1 forbids: no ground on ground, nothing on sky
PARAM_KEYS = ("Tg", "Ts", "eps", "below", "float", "mu_min", "far", "seg", "first", "T")
_NO_KEY = np.iinfo(np.int64).max               # above every key: costs stay below 2^50


def default_params():
    return dict(Tg=STIXEL_TG, Ts=STIXEL_TS, eps=STIXEL_EPS, below=STIXEL_BELOW, float=STIXEL_FLOAT, mu_min=STIXEL_MU_MIN,
                far=STIXEL_FAR, seg=STIXEL_SEG, first=STIXEL_FIRST, T=STIXEL_T)


def energy_params(name, err, params=None):
    """the constants of the energy, the defaults updated by `params` -> a dict of ints (seg, first: 3-tuples, T: 3 x 3) within
    the ranges of include/dca_hip.h; `err`: the exception a refusal raises"""
    p = default_params()
    if params is not None:
        if not isinstance(params, dict) or set(params) - set(PARAM_KEYS):
            raise err(f"{name}: params is a dict with keys out of {PARAM_KEYS}, got {params!r}")
        p.update(params)
    try:
        flat = [p[k] for k in PARAM_KEYS[:7]] + list(p["seg"]) + list(p["first"]) + [v for row in p["T"] for v in row]
        whole = all(int(v) == v for v in flat)
        shapes = len(p["seg"]) == 3 and len(p["first"]) == 3 and len(p["T"]) == 3 and all(len(row) == 3 for row in p["T"])
    except (TypeError, ValueError):
        raise err(f"{name}: the constants are whole numbers, seg and first three of them and T three rows of three") from None
    if not whole or not shapes:
        raise err(f"{name}: the constants are whole numbers, seg and first three of them and T three rows of three")
    if not all(0 <= int(v) <= MAX_CONST for v in flat[:13]) or not all(-1 <= int(v) <= MAX_CONST for v in flat[13:]):
        raise err(f"{name}: every constant lies in [0, {MAX_CONST}] and every entry of T in [-1, {MAX_CONST}] (-1 forbids), got {p}")
    out = {k: int(p[k]) for k in PARAM_KEYS[:7]}
    out.update(seg=tuple(int(v) for v in p["seg"]), first=tuple(int(v) for v in p["first"]),
               T=tuple(tuple(int(v) for v in row) for row in p["T"]))
    return out


def _abi_params(p):
    """the 22 integers in the order of dca_stixels"""
    return [p[k] for k in PARAM_KEYS[:7]] + list(p["seg"]) + list(p["first"]) + [v for row in p["T"] for v in row]


def grid_scalars(name, err, rows, cols, max_disp, width, row_step, min_valid, max_segments, min_disp):
    """the scalars of the cell grid within the ranges of include/dca_hip.h -> (NB, width, row_step, min_valid, max_segments,
    min_disp, H, CS)"""
    try:
        vals = (max_disp, width, row_step, min_valid, max_segments)
        whole = all(int(v) == v for v in vals)
        NB, width, row_step, min_valid, max_segments = (int(v) for v in vals)
        min_disp = float(min_disp)
    except (TypeError, ValueError):
        raise err(f"{name}: max_disp, width, row_step, min_valid and max_segments are whole numbers and min_disp a number") from None
    if not whole:
        raise err(f"{name}: max_disp, width, row_step, min_valid and max_segments are whole numbers")
    if rows > G.MAX_DIM or cols > G.MAX_DIM:
        raise err(f"{name}: rows and cols are at most {G.MAX_DIM}, got {rows} x {cols}")
    if not 8 <= NB <= G.MAX_DISP:
        raise err(f"{name}: max_disp is an integer in [8, {G.MAX_DISP}], got {max_disp}")
    if not (1 <= width <= MAX_WIDTH and 1 <= row_step <= MAX_ROW_STEP):
        raise err(f"{name}: 1 <= width <= {MAX_WIDTH} and 1 <= row_step <= {MAX_ROW_STEP}, got {width} and {row_step}")
    H, CS = rows // row_step, cols // width
    if not 2 <= H <= MAX_CELLS or CS < 1:
        raise err(f"{name}: a column has 2 <= rows // row_step <= {MAX_CELLS} cells and there is at least one column, got {H} "
                  f"cells and {CS} columns")
    if not 1 <= min_valid <= width * row_step:
        raise err(f"{name}: 1 <= min_valid <= width * row_step = {width * row_step}, got {min_valid}")
    if not 1 <= max_segments <= MAX_SEGMENTS:
        raise err(f"{name}: 1 <= max_segments <= {MAX_SEGMENTS}, got {max_segments}")
    if not 0.0 <= min_disp < math.inf:
        raise err(f"{name}: min_disp must be finite and >= 0, got {min_disp}")
    return NB, width, row_step, min_valid, max_segments, min_disp, H, CS


def cell_rows(k, rows, row_step):
    """(first, last) window row of cell k (an integer or an array), cell 0 at the bottom"""
    first = rows - (k + 1) * row_step
    return first, first + row_step - 1


def cells_of(d, passes, rec, NB, min_disp, width, row_step, min_valid):
    """one window d (rows,cols) float32 with its mask passes and plane record -> (q, g) int64 (H,CS), cell row 0 at the bottom"""
    rows, cols = d.shape
    H, CS = rows // row_step, cols // width
    valid, qpix = G.quantise(d, passes, min_disp, NB)
    top = rows - H * row_step
    big = 16 * NB                                                       # above every valid q: sorts behind them
    v = np.where(valid, qpix, big)[top:, :CS * width].reshape(H, row_step, CS, width)[::-1]      # [k]: cell row k from the bottom
    v = np.sort(v.transpose(0, 2, 1, 3).reshape(H, CS, row_step * width), axis=2)
    n = (v < big).sum(axis=2)
    med = np.take_along_axis(v, (np.maximum(n, 1) - 1)[..., None] // 2, axis=2)[..., 0]
    q = np.where(n >= min_valid, med, -1).astype(np.int64)
    with np.errstate(over="ignore"):
        a, b, c = (np.float32(rec[k]) for k in range(3))
    k = np.arange(H, dtype=np.int64)[:, None]
    s = np.arange(CS, dtype=np.int64)[None, :]
    u = (s * width + width // 2 - cols // 2).astype(np.float32)
    w = (rows - (k + 1) * row_step + row_step // 2 - rows // 2).astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        p = (a * u + b * w) + c
        t = np.floor(p * np.float32(16.0) + np.float32(0.5))
        lim = np.float32(16 * NB)
        g = np.where(~(t > -lim), -16 * NB, np.where(t >= lim, 16 * NB, np.where(np.isfinite(t), t, 0))).astype(np.int64)
    return q, np.broadcast_to(g, q.shape).copy()


def mean16(n, s1):
    """the mean of n values with the sum s1, rounded to a whole number; -1 for n = 0 (integers or integer arrays)"""
    return np.where(n > 0, (2 * s1 + n) // np.maximum(2 * n, 1), -1)


def columns_dp(q, g, p):
    """The recursion on every column at once.  q, g int64 (H,CS), p of `energy_params` -> (cost (CS,H,3) int64, back (CS,H,3)
    int64 = kb << 2 | cp).  cost[s, kt, c]: the least energy of the cells [0, kt] whose top segment has class c."""
    H, CS = q.shape
    q, g = q.T, g.T
    v = q >= 0
    qq = np.where(v, q, 0)
    zero = np.zeros((CS, 1), np.int64)
    pre = lambda x: np.concatenate([zero, np.cumsum(x, axis=1, dtype=np.int64)], axis=1)
    N, S1, S2 = pre(v), pre(qq), pre(qq * qq)
    Gd = pre(np.where(v, np.minimum((q - g) ** 2, p["Tg"]), 0))
    Kd = pre(np.where(v, np.minimum(qq * qq, p["Ts"]), 0))
    cost = np.zeros((CS, H, 3), np.int64)
    back = np.zeros((CS, H, 3), np.int64)
    T, seg, first = p["T"], p["seg"], p["first"]
    for kt in range(H):
        kb = np.arange(kt + 1, dtype=np.int64)[None, :]
        n, s1, s2 = N[:, kt + 1:kt + 2] - N[:, :kt + 1], S1[:, kt + 1:kt + 2] - S1[:, :kt + 1], S2[:, kt + 1:kt + 2] - S2[:, :kt + 1]
        mu = mean16(n, s1)
        obj = np.where(n > 0, s2 - 2 * mu * s1 + n * mu * mu, 0) + np.where((mu >= 0) & (mu < p["mu_min"]), p["far"], 0)
        base = (Gd[:, kt + 1:kt + 2] - Gd[:, :kt + 1] + seg[0], obj + seg[1], Kd[:, kt + 1:kt + 2] - Kd[:, :kt + 1] + seg[2])
        gk = g[:, :kt + 1]
        contact = np.where(mu > gk + p["eps"], p["below"], np.where(mu < gk - p["eps"], p["float"], 0))
        for c in range(3):
            keys = np.full((CS, kt + 1), _NO_KEY, np.int64)
            keys[:, 0] = (base[c][:, 0] + first[c]) << 12 | NONE
            for cp in range(3):
                if T[cp][c] < 0 or kt == 0:
                    continue
                cand = cost[:, :kt, cp] + T[cp][c] + base[c][:, 1:] + (contact[:, 1:] if (c, cp) == (OBJECT, GROUND) else 0)
                keys[:, 1:] = np.minimum(keys[:, 1:], cand << 12 | kb[:, 1:] << 2 | cp)
            best = keys.min(axis=1)
            cost[:, kt, c], back[:, kt, c] = best >> 12, best & 0xfff
    return cost, back


def walk_back(cost, back):
    """one column's cost (H,3) and back (H,3) -> (energy, [(kb, kt, c), ...] bottom-up)"""
    H = cost.shape[0]
    c = int(np.argmin(cost[H - 1]))                # the first minimum: the smallest class
    energy, kt, segs = int(cost[H - 1, c]), H - 1, []
    while True:
        kb, cp = int(back[kt, c]) >> 2, int(back[kt, c]) & 3
        segs.append((kb, kt, c))
        if kb == 0:
            return energy, segs[::-1]
        kt, c = kb - 1, cp


def column_stixels(q, g, params=None):
    """ONE column: q, g integer sequences of H cells, bottom-up -> (energy, [(kb, kt, class, mu), ...] bottom-up); mu of an
    object, -1 for ground, sky and an object without a valid cell"""
    p = energy_params("column_stixels", ValueError, params)
    q, g = np.asarray(q, np.int64).reshape(-1, 1), np.asarray(g, np.int64).reshape(-1, 1)
    cost, back = columns_dp(q, g, p)
    energy, segs = walk_back(cost[0], back[0])
    out = []
    for kb, kt, c in segs:
        sel = q[kb:kt + 1, 0]
        sel = sel[sel >= 0]
        out.append((kb, kt, c, int(mean16(sel.size, int(sel.sum()))) if c == OBJECT else -1))
    return energy, out


def stixels_host(disp, plane, max_disp=G.GROUND_MAX_DISP, *, width=STIXEL_WIDTH, row_step=STIXEL_ROW_STEP, mask=None, mask_min=0.5,
                 window=None, min_valid=STIXEL_MIN_VALID, params=None, max_segments=STIXEL_MAX_SEGMENTS, min_disp=G.GROUND_MIN_DISP,
                 outputs=None):
    """The stixel world of every map under the plane record(s) `plane` of `ground_plane_host` (definitions: include/dca_hip.h,
    dca_stixels): CS = cols // width columns of H = rows // row_step cells, cell 0 at the bottom; per column the segmentation of
    least energy into ground (0), object (1) and sky (2) segments.  Returns a dict with the keys of `outputs` (default all of
    STIXEL_OUTPUTS):
      cells      int16   lead + (H, CS, 2)              q: the cell's median disparity in sixteenths, -1 none; g: the road's
      seg_class  uint8   lead + (H, CS)                 the class of every cell (NO_CLASS without a segmentation)
      seg_disp   float32 lead + (H, CS)                 mu / 16 in the cells of an object, +0.0 elsewhere
      count      int32   lead + (CS,)                   the number of segments, also beyond max_segments
      stixels    int32   lead + (CS, max_segments, 4)   bottom-up: first and last window row, class, mu (-1: none); zero beyond count
      energy     int64   lead + (CS,)                   the minimum
    params: a dict of constants of the energy (PARAM_KEYS) that replace the defaults."""
    name = "stixels_host"
    names = STIXEL_OUTPUTS if outputs is None else tuple(outputs)
    if not names or any(k not in STIXEL_OUTPUTS for k in names):
        raise ValueError(f"{name}: outputs are chosen from {STIXEL_OUTPUTS}, got {names}")
    w, passes, lead = G._frame(name, disp, mask, mask_min, window)
    B, rows, cols = w.shape
    NB, width, row_step, min_valid, MAXS, min_disp, H, CS = grid_scalars(name, ValueError, rows, cols, max_disp, width, row_step,
                                                                         min_valid, max_segments, min_disp)
    p = energy_params(name, ValueError, params)
    planes = np.asarray(plane, np.float64)
    if planes.shape != lead + (G.PLANE_LEN,):
        raise ValueError(f"{name}: plane must be float64 of shape {lead + (G.PLANE_LEN,)}, got {planes.shape}")
    planes = planes.reshape(B, G.PLANE_LEN)
    cells = np.zeros((B, H, CS, 2), np.int16)
    seg_class = np.full((B, H, CS), NO_CLASS, np.uint8)
    seg_disp = np.zeros((B, H, CS), np.float32)
    count = np.zeros((B, CS), np.int32)
    stix = np.zeros((B, CS, MAXS, 4), np.int32)
    energy = np.zeros((B, CS), np.int64)
    for i in range(B):
        rec = planes[i]
        q, g = cells_of(w[i], passes[i], rec, NB, min_disp, width, row_step, min_valid)
        cells[i, ..., 0], cells[i, ..., 1] = q, g
        if not (rec[5] != 1.0 and np.float32(rec[9]) > 0) or set(names) == {"cells"}:
            continue
        cost, back = columns_dp(q, g, p)
        N = np.concatenate([np.zeros((1, CS), np.int64), np.cumsum(q >= 0, axis=0)])
        S1 = np.concatenate([np.zeros((1, CS), np.int64), np.cumsum(np.where(q >= 0, q, 0), axis=0)])
        for s in range(CS):
            energy[i, s], segs = walk_back(cost[s], back[s])
            count[i, s] = len(segs)
            for j, (kb, kt, c) in enumerate(segs):
                mu = int(mean16(N[kt + 1, s] - N[kb, s], S1[kt + 1, s] - S1[kb, s])) if c == OBJECT else -1
                seg_class[i, kb:kt + 1, s] = c
                seg_disp[i, kb:kt + 1, s] = np.float32(mu) / np.float32(16.0) if mu >= 0 else np.float32(0)
                if j < MAXS:
                    stix[i, s, j] = cell_rows(kt, rows, row_step)[0], cell_rows(kb, rows, row_step)[1], c, mu
    res = {"cells": cells.reshape(lead + (H, CS, 2)), "seg_class": seg_class.reshape(lead + (H, CS)),
           "seg_disp": seg_disp.reshape(lead + (H, CS)), "count": count.reshape(lead + (CS,)),
           "stixels": stix.reshape(lead + (CS, MAXS, 4)), "energy": energy.reshape(lead + (CS,))}
    return {k: res[k] for k in STIXEL_OUTPUTS if k in names}


def stixels_metric(stixels, count, plane, calib, width=STIXEL_WIDTH):
    """The object stixels of ONE image in metres.  stixels (CS, max_segments, 4) and count (CS,) as read back, plane the image's
    record (computed under `calib`, a geometry.StereoCalib) -> a dict of equally long arrays, one entry per listed object stixel
    with a disparity (mu >= 0) in front of the camera, columns left to right and bottom-up within a column:
      column int64, index int64 (its place in the column's list), disp float64 (pixels),
      Z = f baseline / (d + doffs),  X = (u - cx) Z / f  at the stixel's middle u = column width + (width - 1) / 2,
      base, top: h = hs (d - p) / (d + doffs) at its last and its first window row, p the plane's disparity there -- the heights
      of its foot and its head above the road (section 6o's height).  float64 throughout, closed forms."""
    name = "stixels_metric"
    st, cnt = np.asarray(stixels), np.asarray(count)
    rec = np.asarray(plane, np.float64).reshape(-1)
    if st.ndim != 3 or st.shape[2] != 4 or cnt.shape != st.shape[:1] or rec.size != G.PLANE_LEN:
        raise ValueError(f"{name}: stixels (CS, max_segments, 4), count (CS,) and one plane record of {G.PLANE_LEN} doubles, got "
                         f"{st.shape}, {cnt.shape} and {np.shape(plane)}")
    if int(width) != width or not 1 <= int(width) <= MAX_WIDTH:
        raise ValueError(f"{name}: width is an integer in [1, {MAX_WIDTH}], got {width!r}")
    f, baseline, cx, _, doffs, _ = G.calib_scalars(name, ValueError, calib)
    a, b, c, hs, uc, vc = (float(rec[k]) for k in (0, 1, 2, 9, 13, 14))
    if not hs > 0.0:
        raise ValueError(f"{name}: the record has no camera height: it must be computed with calib=")
    listed = np.arange(st.shape[1])[None, :] < np.minimum(cnt, st.shape[1])[:, None]
    col, idx = np.nonzero(listed & (st[..., 2] == OBJECT) & (st[..., 3] >= 0) & (st[..., 3] / 16.0 + doffs > 0))
    first, last, mu = (st[col, idx, k].astype(np.float64) for k in (0, 1, 3))
    d = mu / 16.0
    den = d + doffs
    u = col * float(width) + (float(width) - 1.0) / 2.0
    Z = f * baseline / den
    height = lambda row: hs * (d - ((a * (u - uc) + b * (row - vc)) + c)) / den
    return {"column": col.astype(np.int64), "index": idx.astype(np.int64), "disp": d, "Z": Z, "X": (u - cx) * Z / f,
            "base": height(last), "top": height(first)}


# ------------------------------------------------------------------------------------------------
# The operator on the device (csrc/stixel.hip), by the conventions of frame_ops.py: arguments are validated once, here; a
# refusal names the operator; a tensor that is not on a ROCm device is an error; no launch synchronises; with `out` and
# `workspace` passed in nothing is allocated either (hipGraph capture).  ops.py re-exports it.
# ------------------------------------------------------------------------------------------------
_STIXEL_KINDS = {"cells": torch.int16, "seg_class": torch.uint8, "seg_disp": torch.float32, "count": torch.int32,
                 "stixels": torch.int32, "energy": torch.int64}
assert (MAX_WIDTH, MAX_ROW_STEP, MAX_CELLS, MAX_SEGMENTS, MAX_CONST, NO_CLASS) == tuple(
    _C[k] for k in ("DCA_STIXEL_MAX_WIDTH", "DCA_STIXEL_MAX_ROW_STEP", "DCA_STIXEL_MAX_CELLS", "DCA_STIXEL_MAX_SEGMENTS",
                    "DCA_STIXEL_MAX_CONST", "DCA_STIXEL_NO_CLASS")), "stixel.py restates other constants than include/dca_hip.h defines"


def stixel_workspace(rows, cols, device, width=STIXEL_WIDTH, row_step=STIXEL_ROW_STEP, batch=1):
    """the int16 (batch, H, CS, 2) workspace of `stixels(..., workspace=)` for windows up to rows x cols: the cells on their
    way from the first launch to the second, needed when `cells` is not among the outputs.  A call writes every word before
    it reads it; nothing has to be cleared."""
    rows, cols, width, row_step, batch = int(rows), int(cols), int(width), int(row_step), int(batch)
    if not (1 <= width <= MAX_WIDTH and 1 <= row_step <= MAX_ROW_STEP and 1 <= batch <= POSTFILTER_MAX_BATCH
            and 2 <= rows // row_step <= MAX_CELLS and width <= cols <= G.MAX_DIM):
        raise RuntimeError(f"stixel_workspace: 1 <= width <= {MAX_WIDTH}, 1 <= row_step <= {MAX_ROW_STEP}, 2 <= rows // row_step <= "
                           f"{MAX_CELLS}, width <= cols <= {G.MAX_DIM} and 1 <= batch <= {POSTFILTER_MAX_BATCH}, got "
                           f"{(rows, cols, width, row_step, batch)}")
    return torch.empty((batch, rows // row_step, cols // width, 2), device=device, dtype=torch.int16)


def stixels(disp, plane, max_disp=G.GROUND_MAX_DISP, *, width=STIXEL_WIDTH, row_step=STIXEL_ROW_STEP, mask=None, mask_min=0.5,
            window=None, min_valid=STIXEL_MIN_VALID, params=None, max_segments=STIXEL_MAX_SEGMENTS, min_disp=G.GROUND_MIN_DISP,
            outputs=None, workspace=None, out=None):
    """The stixel world of disparity maps (Hc,Wc) / (B,Hc,Wc) / (B,1,Hc,Wc), images independent, over the window (y0, rows, cols)
    of every map, under `plane`, the device record(s) (..., GROUND_PLANE_LEN) of `ground_plane(..., calib=)` on the same window
    (definitions: include/dca_hip.h, dca_stixels).  The window is cut into CS = cols // width stixel columns of
    H = rows // row_step cells, cell 0 at the bottom; a cell's disparity q is the lower median of its valid pixels (`min_disp`,
    `max_disp`, the mask; at least `min_valid` of them) in sixteenths of a pixel, its road disparity g the plane's at its centre.
    Every column is cut bottom-up into ground (0), object (1) and sky (2) segments by the dynamic programme that minimises
    the energy of `params` (the defaults are the STIXEL_* constants of stixel.py) exactly, ties to the lower cut.
    Returns a dict of device tensors, those named in `outputs` (default all of STIXEL_OUTPUTS; the others are neither computed
    nor written):
      cells      int16   (..., H, CS, 2)               q (-1: no measurement) and g
      seg_class  uint8   (..., H, CS)                  the class of every cell
      seg_disp   float32 (..., H, CS)                  an object's disparity in pixels in its cells, +0.0 elsewhere
      count      int32   (..., CS)                     the number of segments of every column, also beyond max_segments
      stixels    int32   (..., CS, max_segments, 4)    bottom-up: first and last window row, class, mu in sixteenths (-1: none)
      energy     int64   (..., CS)                     the column's least energy
    A record of status 1 or without a calibration gives count 0 everywhere.  out: a dict of buffers for some or all of them;
    workspace: `stixel_workspace(...)`, read only when `cells` is not asked for.  Two launches (one for cells alone), no host
    wait; with `out` and `workspace` nothing is allocated.  Bitwise reproducible: integers, and no atomic."""
    name = "stixels"
    B, Hc, Wc, y0, rows, cols, mask_min, shape = _pf_frame(name, disp, mask, mask_min, window)
    NB, width, row_step, min_valid, MAXS, min_disp, H, CS = grid_scalars(name, RuntimeError, rows, cols, max_disp, width, row_step,
                                                                         min_valid, max_segments, min_disp)
    p = energy_params(name, RuntimeError, params)
    lead = shape[:-2]
    _req_dev(plane, name, "plane", torch.float64, lead + (G.PLANE_LEN,), like=disp)
    shapes = {"cells": lead + (H, CS, 2), "seg_class": lead + (H, CS), "seg_disp": lead + (H, CS), "count": lead + (CS,),
              "stixels": lead + (CS, MAXS, 4), "energy": lead + (CS,)}
    names = STIXEL_OUTPUTS if outputs is None else tuple(outputs)
    if not names:
        raise RuntimeError(f"{name}: outputs must name at least one of {STIXEL_OUTPUTS}")
    res = _out_dict(name, _STIXEL_KINDS, (), names, out, shapes.__getitem__, disp)
    if "cells" not in res:
        if workspace is None:
            workspace = stixel_workspace(rows, cols, disp.device, width, row_step, B)
        _req_dev(workspace, name, "workspace", torch.int16, like=disp)
        if workspace.numel() < B * H * CS * 2:
            raise RuntimeError(f"{name}: workspace must hold at least {B * H * CS * 2} int16 (`stixel_workspace`), got "
                               f"{workspace.numel()}")
    else:
        workspace = None
    with torch.cuda.device_of(disp):
        _chk(_L().dca_stixels(_ptr(disp), _ptr(mask), _ptr(plane), _ptr(workspace), *(_ptr(res.get(k)) for k in STIXEL_OUTPUTS),
                              B, Hc, Wc, y0, rows, cols, NB, width, row_step, min_valid, MAXS, min_disp, mask_min,
                              *_abi_params(p), _stream()), "dca_stixels")
    return res
