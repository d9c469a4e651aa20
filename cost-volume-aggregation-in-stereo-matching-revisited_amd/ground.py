"""Ground plane, obstacles and free space from disparity on the host, numpy only: the restatement of include/dca_hip.h
(dca_ground_plane, dca_ground_segment) that the kernels of csrc/ground.hip equal bit for bit (tests/test_gpu_ground.py), and
the documented CPU path for a user without a ROCm device; below them the operators themselves, `ground_plane` /
`ground_segment` (`ops.ground_plane`, ...), which take device tensors and have no CPU fallback, as the other operators around
the network have none.  DESIGN.md section 6o.

Both take ONE map (Hc,Wc) or a batch (B,Hc,Wc) / (B,1,Hc,Wc) of independent float32 maps, an optional mask of the same shape
with `mask_min`, and an optional window (y0, rows, cols) at frame row y0, column 0.  Every float32 formula is evaluated one
numpy operation at a time (each rounded to float32), every float64 one as Python floats: IEEE, no fused multiply-add."""
from __future__ import annotations

import math

import numpy as np
import torch

from ._call import _C, _L, _chk, _ptr, _stream
from .frame_ops import POSTFILTER_MAX_BATCH, _geo_scalars, _out_dict, _pf_frame, _req_dev

PLANE_LEN = 16                     # DCA_GROUND_PLANE_LEN of include/dca_hip.h: doubles per plane record
WS_LEN = 48                        # DCA_GROUND_WS_LEN: int64 words of workspace per image
MAX_REFINE = 4                     # DCA_GROUND_MAX_REFINE
MAX_DISP = 1024                    # DCA_GROUND_MAX_DISP: the largest NB
MAX_DIM = 32768                    # DCA_GROUND_MAX_DIM: the largest rows and cols (every int64 sum stays below 2^59)
PLANE_FIELDS = ("a", "b", "c", "inliers", "rms", "status", "d_top", "d_bot", "vote", "hs", "nx", "ny", "nz", "uc", "vc", "rounds")
SEGMENT_OUTPUTS = ("label", "height", "free_row", "free_disp", "bev")
LABELS = {"none": 0, "ground": 1, "obstacle": 2, "overhang": 3, "below": 4}

# defaults
GROUND_MAX_DISP = 192              # the model's default maxdisp
GROUND_MIN_DISP = 0.0625           # one step of the quantisation: the project's "no measurement", +0.0, is never valid
GROUND_MIN_RISE = 2                # d_bot - d_top of a candidate line: a wall draws a vertical line
GROUND_REFINE = 2
GROUND_TOL = 1.5                   # pixels, inliers of a refinement round
GROUND_MIN_INLIERS = 16
GROUND_TOL_D = 1.0                 # pixels: |d - p| of a ground pixel
GROUND_H_GROUND = 0.15             # metres: |h| of a ground pixel
GROUND_H_MAX = 3.0                 # metres: above it an overhang (a bridge, a crown), not an obstacle
GROUND_MIN_RUN = 3                 # pixels of label 2 in a column that make an obstacle's base
GROUND_GRID = (0.2, 20.0, 60.0)    # (cell, x_half, z_max) in metres: cells of 0.2 m over |X| < 20 m, Z < 60 m


def fit_rows(rows, rows_range=None):
    """(r_lo, r_hi), default the lower half [rows // 2, rows)"""
    r_lo, r_hi = (rows // 2, rows) if rows_range is None else (int(v) for v in rows_range)
    return r_lo, r_hi


def plane_scalars(name, err, rows, cols, max_disp, rows_range, min_rise, min_votes, refine, min_inliers, min_disp, tol):
    """the scalars of dca_ground_plane within the ranges of include/dca_hip.h -> (NB, r_lo, r_hi, min_rise, min_votes, refine,
    min_inliers, min_disp, tol); `err`: the exception a refusal raises"""
    try:
        whole = all(int(v) == v for v in (max_disp, min_rise, refine, min_inliers) + (() if min_votes is None else (min_votes,)))
        r_lo, r_hi = fit_rows(rows, rows_range)
        NB, min_rise, refine, min_inliers = int(max_disp), int(min_rise), int(refine), int(min_inliers)
        min_votes = r_hi - r_lo if min_votes is None else int(min_votes)
        min_disp, tol = float(min_disp), float(tol)
    except (TypeError, ValueError):
        raise err(f"{name}: max_disp, fit_rows, min_rise, min_votes, refine and min_inliers are whole numbers, min_disp and "
                  "tol numbers") from None
    if not whole:
        raise err(f"{name}: max_disp, min_rise, min_votes, refine and min_inliers are whole numbers")
    if rows < 2 or rows > MAX_DIM or cols > MAX_DIM:
        raise err(f"{name}: the window needs 2 <= rows <= {MAX_DIM} and cols <= {MAX_DIM}, got {rows} x {cols}")
    if not 8 <= NB <= MAX_DISP:
        raise err(f"{name}: max_disp is an integer in [8, {MAX_DISP}], got {max_disp}")
    if not 0 <= r_lo < r_hi <= rows:
        raise err(f"{name}: fit_rows must satisfy 0 <= r_lo < r_hi <= rows = {rows}, got {(r_lo, r_hi)}")
    if not 1 <= min_rise <= NB or min_votes < 1:
        raise err(f"{name}: 1 <= min_rise <= max_disp and min_votes >= 1, got {min_rise} and {min_votes}")
    if not 0 <= refine <= MAX_REFINE or min_inliers < 3:
        raise err(f"{name}: 0 <= refine <= {MAX_REFINE} and min_inliers >= 3, got {refine} and {min_inliers}")
    if not (0.0 <= min_disp < math.inf and 0.0 <= tol < math.inf):
        raise err(f"{name}: min_disp and tol must be finite and >= 0, got {min_disp} and {tol}")
    return NB, r_lo, r_hi, min_rise, min_votes, refine, min_inliers, min_disp, tol


def calib_scalars(name, err, calib, v0=0):
    """(f, baseline, cx, cy, doffs, v0) as floats of a geometry.StereoCalib, finite with f, baseline > 0"""
    try:
        vals = tuple(float(getattr(calib, k)) for k in ("f", "baseline", "cx", "cy", "doffs")) + (float(v0),)
    except (AttributeError, TypeError, ValueError) as e:
        raise err(f"{name}: calib must be a geometry.StereoCalib (f, baseline, cx, cy, doffs) and v0 a number: {e}") from None
    if not all(math.isfinite(v) for v in vals) or vals[0] <= 0 or vals[1] <= 0:
        raise err(f"{name}: the calibration and v0 must be finite with f > 0 and baseline > 0")
    return vals


def segment_scalars(name, err, max_disp, min_disp, tol_d, h_ground, h_max, min_run, grid):
    """the scalars of dca_ground_segment -> (NB, min_disp, tol_d, h_ground, h_max, min_run, (x_min, inv_cell, max_depth, NX, NZ));
    grid = (cell, x_half, z_max) in metres: NX = ceil(2 x_half / cell), NZ = ceil(z_max / cell), inv_cell = float32(1 / cell)"""
    try:
        whole = int(max_disp) == max_disp and int(min_run) == min_run
        NB, min_run = int(max_disp), int(min_run)
        min_disp, tol_d, h_ground, h_max = float(min_disp), float(tol_d), float(h_ground), float(h_max)
        cell, x_half, z_max = (float(v) for v in grid)
    except (TypeError, ValueError):
        raise err(f"{name}: max_disp and min_run are whole numbers, min_disp, tol_d, h_ground, h_max numbers and grid = (cell, "
                  "x_half, z_max)") from None
    if not whole or not 8 <= NB <= MAX_DISP or min_run < 1:
        raise err(f"{name}: max_disp is an integer in [8, {MAX_DISP}] and min_run an integer >= 1, got {max_disp} and {min_run}")
    if not (0.0 <= min_disp < math.inf and 0.0 <= tol_d < math.inf and 0.0 <= h_ground < math.inf and math.isfinite(h_max)):
        raise err(f"{name}: min_disp, tol_d and h_ground must be finite and >= 0 and h_max finite")
    if not (0.0 < cell < math.inf and 0.0 < x_half < math.inf and 0.0 < z_max < math.inf):
        raise err(f"{name}: grid = (cell, x_half, z_max) must be positive and finite, got {grid!r}")
    NX, NZ = math.ceil(2.0 * x_half / cell), math.ceil(z_max / cell)
    inv_cell = float(np.float32(1.0 / cell))
    if not (NX >= 1 and NZ >= 1 and 2 * NX * NZ < 1 << 31 and 0.0 < inv_cell < math.inf):
        raise err(f"{name}: the grid {grid!r} has {NX} x {NZ} cells: 2 NX NZ must stay below 2^31")
    return NB, min_disp, tol_d, h_ground, h_max, min_run, (float(np.float32(-x_half)), inv_cell, float(np.float32(z_max)), NX, NZ)


def _frame(name, disp, mask, mask_min, window):
    """(maps (B,rows,cols) float32 -- the window, mask passes (B,rows,cols) bool, the leading shape of the outputs)"""
    d = np.asarray(disp)
    if d.dtype != np.float32 or d.ndim < 2 or d.size == 0:
        raise ValueError(f"{name}: expected a non-empty float32 (Hc,Wc), (B,Hc,Wc) or (B,1,Hc,Wc) map, got {d.dtype} {d.shape}")
    if d.ndim > 4 or (d.ndim == 4 and d.shape[1] != 1):
        raise ValueError(f"{name}: expected (Hc,Wc), (B,Hc,Wc) or (B,1,Hc,Wc), got {d.shape}")
    Hc, Wc = d.shape[-2:]
    try:
        y0, rows, cols = (0, Hc, Wc) if window is None else (int(v) for v in window)
    except (TypeError, ValueError):
        raise ValueError(f"{name}: window is (y0, rows, cols), got {window!r}") from None
    if y0 < 0 or rows <= 0 or cols <= 0 or y0 + rows > Hc or cols > Wc:
        raise ValueError(f"{name}: the {rows} x {cols} window at row {y0} does not fit the {Hc} x {Wc} map")
    w = d.reshape(-1, Hc, Wc)[:, y0:y0 + rows, :cols]
    passes = np.ones(w.shape, bool)
    if mask is not None:
        m = np.asarray(mask)
        if m.dtype != np.float32 or m.shape != d.shape:
            raise ValueError(f"{name}: the mask must be float32 of the map's shape {d.shape}, got {m.dtype} {m.shape}")
        if np.isnan(mask_min):
            raise ValueError(f"{name}: mask_min must not be NaN")
        with np.errstate(invalid="ignore"):
            passes = m.reshape(-1, Hc, Wc)[:, y0:y0 + rows, :cols] >= np.float32(mask_min)
    return w, passes, d.shape[:-2]


def quantise(d, passes, min_disp, NB):
    """(valid bool, q int64: the disparity in sixteenths, 0 where not valid) of float32 d, as gm_valid has it"""
    with np.errstate(invalid="ignore", over="ignore"):
        t = d * np.float32(16.0) + np.float32(0.5)
        valid = (d >= np.float32(min_disp)) & (t < np.float32(16 * NB)) & passes
    return valid, np.where(valid, t, np.float32(0)).astype(np.int64)         # truncation, t >= 0


def line_bins(d_top, d_bot, r, R):
    """the bin of the line (d_top, d_bot) at window row r of R (integers or integer arrays): a true floor division"""
    return (2 * (d_top * (R - 1 - r) + d_bot * r) + (R - 1)) // (2 * (R - 1))


def hough_votes(vdisp, r_lo, r_hi, min_rise):
    """vdisp (rows, NB) -> int64 (NB - 1, 2 NB): the vote of the candidate (d_bot = 1 + i, d_top = j - NB), -1 for the pairs
    with d_bot - d_top < min_rise"""
    R, NB = vdisp.shape
    d_top = np.arange(-NB, NB, dtype=np.int64)[None, :]
    d_bot = np.arange(1, NB, dtype=np.int64)[:, None]
    votes = np.zeros((NB - 1, 2 * NB), np.int64)
    for r in range(r_lo, r_hi):
        b = line_bins(d_top, d_bot, r, R)
        inside = (b >= 0) & (b < NB)
        votes += np.where(inside, vdisp[r][np.clip(b, 0, NB - 1)], 0)
    votes[np.broadcast_to(d_bot - d_top < min_rise, votes.shape)] = -1
    return votes


def hough_line(vdisp, r_lo, r_hi, min_rise):
    """vdisp (rows, NB) -> (d_top, d_bot, vote) of the best candidate: the largest vote, then the smallest d_bot, then the
    smallest d_top"""
    NB = vdisp.shape[1]
    votes = hough_votes(vdisp, r_lo, r_hi, min_rise)
    k = int(np.argmax(votes))                                        # the first maximum in (d_bot, d_top) order
    return int(k % (2 * NB)) - NB, 1 + k // (2 * NB), int(votes.reshape(-1)[k])


def solve(S):
    """the ten int sums -> (a, b, c, rms) or None, the operations of gm_solve (csrc/ground_math.h) in their order"""
    n, Su, Sv, Sq, Suu, Suv, Svv, Suq, Svq, Sqq = (float(int(s)) for s in S)
    c00, c01, c02 = Svv * n - Sv * Sv, Suv * n - Sv * Su, Suv * Sv - Svv * Su
    c11, c12, c22 = Suu * n - Su * Su, Suu * Sv - Suv * Su, Suu * Svv - Suv * Suv
    det = (Suu * c00 - Suv * c01) + Su * c02
    if not det > 0.0:
        return None
    A = ((Suq * c00 - Svq * c01) + Sq * c02) / det
    B = ((Svq * c11 - Suq * c01) - Sq * c12) / det
    C = ((Suq * c02 - Svq * c12) + Sq * c22) / det
    rss = Sqq - ((A * Suq + B * Svq) + C * Sq)
    ms = rss / n
    return A / 16.0, B / 16.0, C / 16.0, math.sqrt(ms if ms > 0.0 else 0.0) / 16.0


def pose(a, b, c, uc, vc, f, baseline, cx, cy, doffs, v0):
    """(hs, nx, ny, nz) of gm_pose: the camera's height above the plane and its unit normal in the camera frame"""
    c_img = ((c - a * uc) - b * (v0 + vc)) + doffs
    nz = ((a * cx + b * cy) + c_img) / f
    norm = math.sqrt((a * a + b * b) + nz * nz)
    if not norm > 0.0:
        return 0.0, 0.0, 0.0, 0.0
    return baseline / norm, a / norm, b / norm, nz / norm


def _centred(rows, cols):
    return np.arange(cols, dtype=np.int64)[None, :] - cols // 2, np.arange(rows, dtype=np.int64)[:, None] - rows // 2


def plane_disp(plane, rows, cols):
    """float32 (rows,cols): p = (a32 * float(u') + b32 * float(v')) + c32 of one plane record"""
    a, b, c = (np.float32(plane[k]) for k in range(3))
    u, v = _centred(rows, cols)
    return (a * u.astype(np.float32) + b * v.astype(np.float32)) + c


def ground_plane_host(disp, max_disp=GROUND_MAX_DISP, calib=None, mask=None, mask_min=0.5, window=None, v0=0, fit_rows=None,
                      refine=GROUND_REFINE, tol=GROUND_TOL, min_disp=GROUND_MIN_DISP, min_rise=GROUND_MIN_RISE, min_votes=None,
                      min_inliers=GROUND_MIN_INLIERS):
    """The road plane of every map: v-disparity, a Hough vote for the line, `refine` rounds of least squares with roll
    (definitions: include/dca_hip.h, dca_ground_plane).  Returns a dict:
      plane  float64 lead + (PLANE_LEN,)       the plane record (PLANE_FIELDS)
      vdisp  int32   lead + (rows, max_disp)   the v-disparity histogram
      sums   int64   lead + (MAX_REFINE, 10)   the ten sums of every round (zeros for a round that did nothing)
    calib: a geometry.StereoCalib for the camera height and the normal (None: zeros); v0: the image row of window row 0."""
    name = "ground_plane_host"
    w, passes, lead = _frame(name, disp, mask, mask_min, window)
    B, rows, cols = w.shape
    NB, r_lo, r_hi, min_rise, min_votes, refine, min_inliers, min_disp, tol = plane_scalars(
        name, ValueError, rows, cols, max_disp, fit_rows, min_rise, min_votes, refine, min_inliers, min_disp, tol)
    cal = None if calib is None else calib_scalars(name, ValueError, calib, v0)
    planes = np.zeros((B, PLANE_LEN), np.float64)
    vdisps = np.zeros((B, rows, NB), np.int32)
    sums = np.zeros((B, MAX_REFINE, 10), np.int64)
    u, v = _centred(rows, cols)
    rr = np.arange(rows, dtype=np.int64)[:, None]
    fit = (rr >= r_lo) & (rr < r_hi)
    for i in range(B):
        d = w[i]
        valid, q = quantise(d, passes[i], min_disp, NB)
        flat = (rr * NB + (q >> 4))[valid]
        vdisps[i] = np.bincount(flat, minlength=rows * NB).reshape(rows, NB)
        d_top, d_bot, vote = hough_line(vdisps[i], r_lo, r_hi, min_rise)
        rec = planes[i]
        rec[1] = float(d_bot - d_top) / float(rows - 1)
        rec[2] = float(d_top) + rec[1] * float(rows // 2)
        rec[5] = 1.0 if vote < min_votes else 0.0
        rec[6:9] = d_top, d_bot, vote
        rec[13:15] = cols // 2, rows // 2
        for k in range(refine):
            if rec[5] != 0.0:
                break
            if k == 0:
                p = (np.float32(d_top) * (rows - 1 - rr).astype(np.float32) + np.float32(d_bot) * rr.astype(np.float32)) \
                    / np.float32(rows - 1)
            else:
                p = plane_disp(rec, rows, cols)
            with np.errstate(invalid="ignore", over="ignore"):
                inl = valid & fit & (np.abs(d - p) <= np.float32(tol))
            uu, vv, qq = np.broadcast_to(u, inl.shape)[inl], np.broadcast_to(v, inl.shape)[inl], q[inl]
            S = [int(inl.sum()), uu.sum(), vv.sum(), qq.sum(), (uu * uu).sum(), (uu * vv).sum(), (vv * vv).sum(),
                 (uu * qq).sum(), (vv * qq).sum(), (qq * qq).sum()]
            sums[i, k] = S
            res = solve(S) if S[0] >= min_inliers else None
            if res is None:
                rec[5] = 2.0
            else:
                rec[0:3], rec[3], rec[4], rec[15] = res[:3], S[0], res[3], k + 1
        if cal is not None:
            rec[9:13] = pose(float(rec[0]), float(rec[1]), float(rec[2]), float(rec[13]), float(rec[14]), *cal)
    return {"plane": planes.reshape(lead + (PLANE_LEN,)), "vdisp": vdisps.reshape(lead + (rows, NB)),
            "sums": sums.reshape(lead + (MAX_REFINE, 10))}


def ground_segment_host(disp, plane, calib, max_disp=GROUND_MAX_DISP, mask=None, mask_min=0.5, window=None,
                        min_disp=GROUND_MIN_DISP, tol_d=GROUND_TOL_D, h_ground=GROUND_H_GROUND, h_max=GROUND_H_MAX,
                        min_run=GROUND_MIN_RUN, grid=GROUND_GRID, outputs=None):
    """Labels, height above the road, free space per column and the bird's-eye grid of every map under the plane record(s)
    `plane` of `ground_plane_host(..., calib=calib)` (definitions: include/dca_hip.h, dca_ground_segment).  Returns a dict with
    the keys of `outputs` (default all of SEGMENT_OUTPUTS):
      label      uint8   lead + (rows, cols)   0 no data, 1 ground, 2 obstacle, 3 overhang, 4 below ground
      height     float32 lead + (rows, cols)   metres above the road, +0.0 where the label is 0
      free_row   int32   lead + (cols,)        the base row of the lowest obstacle of every column, -1 without one
      free_disp  float32 lead + (cols,)        the disparity there, +0.0 without one
      bev        int32   lead + (2, NZ, NX)    ground and obstacle pixels per cell of `grid` = (cell, x_half, z_max)"""
    name = "ground_segment_host"
    names = SEGMENT_OUTPUTS if outputs is None else tuple(outputs)
    if any(k not in SEGMENT_OUTPUTS for k in names):
        raise ValueError(f"{name}: outputs are chosen from {SEGMENT_OUTPUTS}, got {names}")
    w, passes, lead = _frame(name, disp, mask, mask_min, window)
    B, rows, cols = w.shape
    if rows > MAX_DIM or cols > MAX_DIM:
        raise ValueError(f"{name}: rows and cols are at most {MAX_DIM}, got {rows} x {cols}")
    NB, min_disp, tol_d, h_ground, h_max, min_run, (x_min, inv_cell, max_depth, NX, NZ) = segment_scalars(
        name, ValueError, max_disp, min_disp, tol_d, h_ground, h_max, min_run, grid)
    f64, _, cx64, _, doffs64, _ = calib_scalars(name, ValueError, calib)
    f, fb, cx, doffs = np.float32(f64), np.float32(calib.fb), np.float32(cx64), np.float32(doffs64)
    planes = np.asarray(plane, np.float64)
    if planes.shape != lead + (PLANE_LEN,):
        raise ValueError(f"{name}: plane must be float64 of shape {lead + (PLANE_LEN,)}, got {planes.shape}")
    planes = planes.reshape(B, PLANE_LEN)
    label = np.zeros((B, rows, cols), np.uint8)
    height = np.zeros((B, rows, cols), np.float32)
    free_row = np.full((B, cols), -1, np.int32)
    free_disp = np.zeros((B, cols), np.float32)
    bev = np.zeros((B, 2, NZ, NX), np.int32)
    col = np.arange(cols, dtype=np.int64)[None, :].astype(np.float32)
    for i in range(B):
        d, rec = w[i], planes[i]
        hs = np.float32(rec[9])
        valid, _ = quantise(d, passes[i], min_disp, NB)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            den = d + doffs
            ok = valid & (den > 0) & bool(rec[5] != 1.0 and hs > 0)
            p = plane_disp(rec, rows, cols)
            pden = p + doffs
            h = (hs * (den - pden)) / den
            ground = (np.abs(d - p) <= np.float32(tol_d)) | (np.abs(h) <= np.float32(h_ground))
            lab = np.where(ground, 1, np.where(h < 0, 4, np.where(h > np.float32(h_max), 3, 2)))
            lab = np.where(ok, lab, 0).astype(np.uint8)
            label[i] = lab
            height[i] = np.where(ok, h, np.float32(0))
            Z = fb / den
            X = ((col - cx) * Z) / f
            fx, fz = np.floor((X - np.float32(x_min)) * np.float32(inv_cell)), np.floor(Z * np.float32(inv_cell))
            keep = (fx >= 0) & (fx < np.float32(NX)) & (fz >= 0) & (fz < np.float32(NZ)) & (Z <= np.float32(max_depth))
        for ch, which in enumerate((1, 2)):
            sel = keep & (lab == which)
            cells = fz[sel].astype(np.int64) * NX + fx[sel].astype(np.int64)
            bev[i, ch] = np.bincount(cells, minlength=NZ * NX).reshape(NZ, NX)
        run = np.zeros(cols, np.int64)
        for r in range(rows - 1, -1, -1):
            run = np.where(lab[r] == 2, run + 1, 0)
            hit = (run == min_run) & (free_row[i] < 0)
            if hit.any():
                base = r + min_run - 1                                 # the run's lowest row, where it began
                free_row[i][hit] = base
                free_disp[i][hit] = d[base][hit]
    res = {"label": label.reshape(lead + (rows, cols)), "height": height.reshape(lead + (rows, cols)),
           "free_row": free_row.reshape(lead + (cols,)), "free_disp": free_disp.reshape(lead + (cols,)),
           "bev": bev.reshape(lead + (2, NZ, NX))}
    return {k: res[k] for k in SEGMENT_OUTPUTS if k in names}


def plane_pose(plane, calib, v0=0):
    """One plane record read back to the host -> dict(height, pitch, roll, horizon, normal): the camera's height above the road
    in metres; its pitch in degrees, positive when it looks down (the normal leans forward: asin of its Z component); its
    roll in degrees, atan2(n_x, n_y), positive when the road rises to the right of the image; the horizon's image row at the
    principal column, where a u + b v + c_img = 0 (None for a plane that faces the camera, b = 0).  In float64 from a, b, c and
    the record's own centre: a closed form, nothing is fitted."""
    rec = np.asarray(plane, np.float64).reshape(-1)
    if rec.size != PLANE_LEN:
        raise ValueError(f"plane_pose: one plane record of {PLANE_LEN} doubles, got shape {np.shape(plane)}")
    f, baseline, cx, cy, doffs, v0 = calib_scalars("plane_pose", ValueError, calib, v0)
    a, b, c, uc, vc = float(rec[0]), float(rec[1]), float(rec[2]), float(rec[13]), float(rec[14])
    hs, nx, ny, nz = pose(a, b, c, uc, vc, f, baseline, cx, cy, doffs, v0)
    if not hs > 0.0:
        raise ValueError("plane_pose: the record's plane has no normal (a = b = 0 and no offset)")
    c_img = ((c - a * uc) - b * (v0 + vc)) + doffs
    return {"height": hs, "pitch": math.degrees(math.atan2(nz, math.hypot(nx, ny))), "roll": math.degrees(math.atan2(nx, ny)),
            "horizon": None if b == 0.0 else -(a * cx + c_img) / b, "normal": (nx, ny, nz)}


def plane_from_pose(height, pitch, roll, calib, rows, cols, v0=0):
    """The plane record (a, b, c and the centre; everything else 0 but hs and the normal) of a road seen from `height` metres
    with `pitch` and `roll` in degrees as `plane_pose` defines them, in the window rows x cols whose row 0 is image row v0:
    the inverse of `plane_pose`, for synthetic scenes and for checking a calibration."""
    f, baseline, cx, cy, doffs, v0 = calib_scalars("plane_from_pose", ValueError, calib, v0)
    if not float(height) > 0.0:
        raise ValueError("plane_from_pose: height must be positive")
    pt, rl = math.radians(float(pitch)), math.radians(float(roll))
    n = (math.sin(rl) * math.cos(pt), math.cos(rl) * math.cos(pt), math.sin(pt))
    a, b, nzc = (baseline * v / float(height) for v in n)
    c_img = f * nzc - a * cx - b * cy
    rec = np.zeros(PLANE_LEN, np.float64)
    rec[13:15] = cols // 2, rows // 2
    rec[0:3] = a, b, c_img - doffs + a * rec[13] + b * (v0 + rec[14])
    rec[9:13] = pose(a, b, float(rec[2]), float(rec[13]), float(rec[14]), f, baseline, cx, cy, doffs, v0)
    return rec


# ------------------------------------------------------------------------------------------------
# The operators on the device (csrc/ground.hip), by the conventions of frame_ops.py: arguments are validated once, here, with
# its helpers; a refusal names the operator; a tensor that is not on a ROCm device is an error; no launch synchronises; with
# `out` and `workspace` passed in nothing is allocated either (hipGraph capture).  ops.py re-exports them.
# ------------------------------------------------------------------------------------------------
GROUND_PLANE_LEN = _C["DCA_GROUND_PLANE_LEN"]
GROUND_WS_LEN = _C["DCA_GROUND_WS_LEN"]
GROUND_SUMS_AT = 8                  # workspace[b, 8 + 10 k + j]: sum j of refinement round k (include/dca_hip.h)
GROUND_OUTPUTS = SEGMENT_OUTPUTS
_GROUND_PLANE_KINDS = {"plane": torch.float64, "vdisp": torch.int32}
_GROUND_KINDS = {"label": torch.uint8, "height": torch.float32, "free_row": torch.int32, "free_disp": torch.float32,
                 "bev": torch.int32}
assert (PLANE_LEN, WS_LEN, MAX_REFINE, MAX_DISP, MAX_DIM) == tuple(
    _C[k] for k in ("DCA_GROUND_PLANE_LEN", "DCA_GROUND_WS_LEN", "DCA_GROUND_MAX_REFINE", "DCA_GROUND_MAX_DISP",
                    "DCA_GROUND_MAX_DIM")), "ground.py restates other constants than include/dca_hip.h defines"


def ground_workspace(rows, cols, max_disp, device, batch=1):
    """the int64 (batch, GROUND_WS_LEN) workspace of `ground_plane(..., workspace=)` for windows up to rows x cols and up to
    max_disp bins (its size depends on the batch alone; the arguments are checked against the operator's limits).  The first
    launch of every call clears it; afterwards [b, 0] is the Hough key and [b, 8 + 10 k : 18 + 10 k] the ten sums of round k."""
    rows, cols, max_disp, batch = int(rows), int(cols), int(max_disp), int(batch)
    if not (2 <= rows <= MAX_DIM and 1 <= cols <= MAX_DIM and 8 <= max_disp <= MAX_DISP
            and 1 <= batch <= POSTFILTER_MAX_BATCH):
        raise RuntimeError(f"ground_workspace: 2 <= rows <= {MAX_DIM}, 1 <= cols <= {MAX_DIM}, 8 <= max_disp <= "
                           f"{MAX_DISP} and 1 <= batch <= {POSTFILTER_MAX_BATCH}, got {(rows, cols, max_disp, batch)}")
    return torch.empty((batch, GROUND_WS_LEN), device=device, dtype=torch.int64)


def ground_plane(disp, max_disp=GROUND_MAX_DISP, calib=None, mask=None, mask_min=0.5, window=None, v0=0, fit_rows=None,
                 refine=GROUND_REFINE, tol=GROUND_TOL, min_disp=GROUND_MIN_DISP,
                 min_rise=GROUND_MIN_RISE, min_votes=None, min_inliers=GROUND_MIN_INLIERS, workspace=None,
                 out=None):
    """The road plane d = a u' + b v' + c of disparity maps (Hc,Wc) / (B,Hc,Wc) / (B,1,Hc,Wc), images independent, over the
    window (y0, rows, cols) of every map, u' = col - cols // 2, v' = row - rows // 2 (definitions: include/dca_hip.h,
    dca_ground_plane): the v-disparity histogram of the valid pixels (d >= min_disp, bin below max_disp, mask >= mask_min), a
    Hough vote over the integer lines (d_top, d_bot) with d_bot - d_top >= min_rise through the fit rows `fit_rows` =
    (r_lo, r_hi) (default the lower half), then `refine` rounds of least squares with roll over the inliers within `tol` pixels.
    Returns a dict of device tensors:
      plane  float64 (..., GROUND_PLANE_LEN)   a, b, c, inliers, rms, status (0 fitted, 1 no line: best vote < min_votes, default
                                               the number of fit rows, 2 a round failed: fewer than min_inliers or a singular
                                               system, the last good plane stays), d_top, d_bot, vote, camera height, unit normal,
                                               cols // 2, rows // 2, rounds done (`ground.PLANE_FIELDS`; `ground.plane_pose`)
      vdisp  int32   (..., rows, max_disp)     the v-disparity histogram
    calib: a geometry.StereoCalib for the camera height and the normal (zeros without), v0: the image row of window row 0.
    out: a dict of buffers for either; workspace: `ground_workspace(...)` of a batch at least this large.  With both given
    nothing is allocated and the host never waits: the 2 + 2 refine launches (3 for refine = 0) can be captured into a
    hipGraph.  Bitwise reproducible: integer counts and sums (LDS and integer atomics), one fp64 solve in a written order."""
    name = "ground_plane"
    B, Hc, Wc, y0, rows, cols, mask_min, shape = _pf_frame(name, disp, mask, mask_min, window)
    NB, r_lo, r_hi, min_rise, min_votes, refine, min_inliers, min_disp, tol = plane_scalars(
        name, RuntimeError, rows, cols, max_disp, fit_rows, min_rise, min_votes, refine, min_inliers, min_disp, tol)
    cal = (0.0,) * 6 if calib is None else calib_scalars(name, RuntimeError, calib, v0)
    lead = shape[:-2]
    res = _out_dict(name, _GROUND_PLANE_KINDS, ("plane", "vdisp"), None, out,
                    lambda k: lead + ((GROUND_PLANE_LEN,) if k == "plane" else (rows, NB)), disp)
    if workspace is None:
        workspace = ground_workspace(rows, cols, NB, disp.device, B)
    _req_dev(workspace, name, "workspace", torch.int64, like=disp)
    if workspace.numel() < B * GROUND_WS_LEN:
        raise RuntimeError(f"{name}: workspace must hold at least {B * GROUND_WS_LEN} int64 (`ground_workspace`), got "
                           f"{workspace.numel()}")
    with torch.cuda.device_of(disp):
        _chk(_L().dca_ground_plane(_ptr(disp), _ptr(mask), _ptr(res["plane"]), _ptr(res["vdisp"]), _ptr(workspace), B, Hc, Wc,
                                   y0, rows, cols, NB, r_lo, r_hi, min_rise, min_votes, refine, min_inliers, min_disp, tol,
                                   mask_min, int(calib is not None), *cal, _stream()), "dca_ground_plane")
    return res


def ground_segment(disp, plane, calib, max_disp=GROUND_MAX_DISP, mask=None, mask_min=0.5, window=None,
                   min_disp=GROUND_MIN_DISP, tol_d=GROUND_TOL_D, h_ground=GROUND_H_GROUND,
                   h_max=GROUND_H_MAX, min_run=GROUND_MIN_RUN, grid=GROUND_GRID, outputs=None, out=None):
    """Labels, height above the road, free space per column and a bird's-eye occupancy grid of disparity maps (Hc,Wc) /
    (B,Hc,Wc) / (B,1,Hc,Wc) under `plane`, the device record(s) (..., GROUND_PLANE_LEN) of `ground_plane(..., calib=calib)` on
    the same window (definitions: include/dca_hip.h, dca_ground_segment).  With p the plane's disparity at a pixel and
    h = hs (d - p) / (d + doffs) its height above the road in metres: label 0 no data (not valid, or status 1), 1 ground
    (|d - p| <= tol_d or |h| <= h_ground), 4 below ground (h < 0), 3 overhang (h > h_max), 2 obstacle (the rest).
    Returns a dict of device tensors, those named in `outputs` (default all of GROUND_OUTPUTS; the others are neither computed
    nor written):
      label      uint8   (..., rows, cols)
      height     float32 (..., rows, cols)   h, +0.0 where the label is 0
      free_row   int32   (..., cols)         the base row of the lowest run of min_run obstacle pixels of every column, -1: none
      free_disp  float32 (..., cols)         the disparity there, +0.0: none
      bev        int32   (..., 2, NZ, NX)    ground / obstacle pixels per cell of `grid` = (cell, x_half, z_max) metres, with X and
                                             Z of `point_cloud`: NX = ceil(2 x_half / cell), NZ = ceil(z_max / cell)
    out: a dict of buffers for some or all of them.  Two launches, no host wait; with `out` nothing is allocated.  Bitwise
    reproducible: the grid is counted with integer atomics."""
    name = "ground_segment"
    B, Hc, Wc, y0, rows, cols, mask_min, shape = _pf_frame(name, disp, mask, mask_min, window)
    if rows > MAX_DIM or cols > MAX_DIM:
        raise RuntimeError(f"{name}: rows and cols are at most {MAX_DIM}, got {rows} x {cols}")
    NB, min_disp, tol_d, h_ground, h_max, min_run, (x_min, inv_cell, max_depth, NX, NZ) = segment_scalars(
        name, RuntimeError, max_disp, min_disp, tol_d, h_ground, h_max, min_run, grid)
    f, fb, cx, _, doffs = _geo_scalars(name, calib, mask_min, 0.0, 1.0)[:5]
    lead = shape[:-2]
    _req_dev(plane, name, "plane", torch.float64, lead + (GROUND_PLANE_LEN,), like=disp)
    shapes = {"label": shape, "height": shape, "free_row": lead + (cols,), "free_disp": lead + (cols,), "bev": lead + (2, NZ, NX)}
    names = GROUND_OUTPUTS if outputs is None else tuple(outputs)
    if not names:
        raise RuntimeError(f"{name}: outputs must name at least one of {GROUND_OUTPUTS}")
    always = ("free_row", "free_disp") if "free_row" in names or "free_disp" in names else ()      # one walk gives both
    res = _out_dict(name, _GROUND_KINDS, always, names, out, shapes.__getitem__, disp)
    with torch.cuda.device_of(disp):
        _chk(_L().dca_ground_segment(_ptr(disp), _ptr(mask), _ptr(plane), *(_ptr(res.get(k)) for k in GROUND_OUTPUTS), B, Hc, Wc,
                                     y0, rows, cols, NB, min_disp, mask_min, tol_d, h_ground, h_max, min_run, f, fb, cx, doffs,
                                     x_min, inv_cell, max_depth, NX, NZ, _stream()), "dca_ground_segment")
    return res
