"""Temporal stereo on the host, numpy only: the matrix G of the ego-motion, the validators, and the restatements of
include/dca_hip.h (dca_disp_reproject, dca_temporal_fuse) that the kernels of csrc/temporal.hip equal bit for bit
(tests/test_gpu_temporal.py) -- the documented CPU path for a user without a ROCm device; below them the operators themselves,
`temporal_workspace` / `disp_reproject` / `temporal_fuse` (`ops.disp_reproject`, ...), which take device tensors and have no
CPU fallback, as the other operators around the network have none.  DESIGN.md section 6p.

The STATE of a sequence is three dense (H,W) maps in image coordinates: disp float32 (+0.0: nothing), var float32 (px^2), age
uint8; it is passed as a dict with those keys.  Every float32 formula is evaluated one numpy operation at a time (each
rounded to float32): IEEE, no fused multiply-add."""
from __future__ import annotations

import math

import numpy as np
import torch

from ._call import _C, _L, _chk, _ptr, _req_no_grad, _stream
from .frame_ops import _mask_min, _out_dict, _req_dev, _window

MAX_RADIUS = 8                     # DCA_TEMPORAL_MAX_RADIUS of include/dca_hip.h: the largest half-size of the occlusion window
STATE_KEYS = ("disp", "var", "age")
REPROJECT_OUTPUTS = ("pred", "var", "age", "hints", "count")
FUSE_OUTPUTS = ("disp", "var", "age", "innov")

# defaults
TEMPORAL_MIN_DISP = 0.0625         # the project's "no measurement", +0.0, is never valid
TEMPORAL_MAX_DISP = 192.0          # the model's default maxdisp
TEMPORAL_MIN_RATIO = 0.125         # Z_cur / Z_prev below it: the point has come too close (or lies behind the camera)
TEMPORAL_OCCL = (1, 1, 1.0)        # (rx, ry, occl_px): the window closes the one-pixel cracks of forward splatting; the threshold
#                                    is absolute, 1 px (a relative one drops the far road)
TEMPORAL_Q = 0.0                   # process noise in px^2 per frame
TEMPORAL_HINT_MIN_AGE = 1          # every reprojected pixel is a hint (a reprojected pixel has age >= 1)
TEMPORAL_GATE = 3.0                # sigmas: gate2 = gate^2 = 9
TEMPORAL_VAR_MAX = math.inf
TEMPORAL_MEAS_VAR = 0.25           # px^2: a measurement good to half a pixel


def _mat3(a, b):
    """a (3,3) times b (3,n) as Python floats in a written order: no fused multiply-add, an exact zero stays one"""
    return [[(a[i][0] * b[0][j] + a[i][1] * b[1][j]) + a[i][2] * b[2][j] for j in range(len(b[0]))] for i in range(3)]


def reproject_matrix(calib, T_cur_from_prev):
    """G (3,4) float32 of `disp_reproject`:  G = (1/f) [ K R A | K t / baseline ]  with K = [[f,0,cx],[0,f,cy],[0,0,1]],
    A = [[1,0,-cx],[0,1,-cy],[0,0,f]] and (R | t) = T_cur_from_prev, the (4,4) or (3,4) pose of the PREVIOUS rectified left camera
    in the CURRENT one (`geometry.relative_pose`).  G (u, v, 1, d + doffs) = (x, y, z): the pixel is (x / z, y / z), z is
    Z_cur / Z_prev and the new d + doffs is the old one over z.  Formed in float64, rounded once; exactly [I | 0] for the
    identity."""
    try:
        f, baseline, cx, cy = (float(getattr(calib, k)) for k in ("f", "baseline", "cx", "cy"))
    except (AttributeError, TypeError, ValueError) as e:
        raise ValueError(f"reproject_matrix: calib must be a geometry.StereoCalib (f, baseline, cx, cy): {e}") from None
    T = np.asarray(T_cur_from_prev, np.float64)
    if T.shape not in ((4, 4), (3, 4)) or not np.isfinite(T).all():
        raise ValueError(f"reproject_matrix: the pose must be a finite (4,4) or (3,4) array, got shape {T.shape}")
    if not (math.isfinite(f) and math.isfinite(baseline) and f > 0 and baseline > 0 and math.isfinite(cx) and math.isfinite(cy)):
        raise ValueError("reproject_matrix: the calibration must be finite with f > 0 and baseline > 0")
    R = [[float(T[i, j]) for j in range(3)] for i in range(3)]
    t = [[float(T[i, 3])] for i in range(3)]
    K = [[f, 0.0, cx], [0.0, f, cy], [0.0, 0.0, 1.0]]
    A = [[1.0, 0.0, -cx], [0.0, 1.0, -cy], [0.0, 0.0, f]]
    KRA, Kt = _mat3(K, _mat3(R, A)), _mat3(K, t)
    G = np.array([[KRA[i][0] / f, KRA[i][1] / f, KRA[i][2] / f, (Kt[i][0] / baseline) / f] for i in range(3)], np.float64)
    with np.errstate(over="ignore"):
        G32 = G.astype(np.float32)
    if not np.isfinite(G32).all():
        raise ValueError("reproject_matrix: G does not fit float32")
    return G32


def _doffs(name, err, calib, doffs):
    if (calib is None) == (doffs is None):
        raise err(f"{name}: give calib (a geometry.StereoCalib) or doffs, one of them")
    try:
        return float(np.float32(calib.doffs if doffs is None else doffs))
    except (AttributeError, TypeError, ValueError):
        raise err(f"{name}: calib must be a geometry.StereoCalib and doffs a number") from None


def reproject_scalars(name, err, H, W, G, doffs, min_disp, max_disp, min_ratio, occl, q, hint_min_age, nan_ok=False):
    """The scalar arguments of dca_disp_reproject, checked as its launcher checks them (on the float32 values it is handed) ->
    (g: 12 floats, doffs, min_disp, max_disp, min_ratio, rx, ry, occl_px, q, hint_min_age) with the floats already rounded to
    float32; raises `err` otherwise.  G None: a matrix on the device, which nobody can check here (g is None then); nan_ok: a
    matrix that is NaN in all twelve entries (a failed estimate's) is let through: it keeps no source."""
    if H <= 0 or W <= 0 or H * W >= 1 << 31:
        raise err(f"{name}: the state must be a non-empty (H,W) map with H * W below 2^31, got {H} x {W}")
    try:
        with np.errstate(over="ignore"):
            g = None if G is None else np.asarray(G, np.float64).astype(np.float32)
    except (TypeError, ValueError):
        raise err(f"{name}: G must be a (3,4) array of numbers") from None
    if g is not None and (g.shape != (3, 4) or not (np.isfinite(g).all() or (nan_ok and np.isnan(g).all()))):
        raise err(f"{name}: G must be a finite (3,4) matrix (`temporal.reproject_matrix`){', or all NaN' if nan_ok else ''}, got "
                  f"shape {g.shape}")
    try:
        rx, ry, occl_px = int(occl[0]), int(occl[1]), float(np.float32(occl[2]))
        if len(occl) != 3 or rx != occl[0] or ry != occl[1]:
            raise ValueError
    except (TypeError, ValueError, IndexError):
        raise err(f"{name}: occl must be (rx, ry, occl_px) with integer radii, got {occl!r}") from None
    if not (0 <= rx <= MAX_RADIUS and 0 <= ry <= MAX_RADIUS):
        raise err(f"{name}: the radii of occl must lie in [0, {MAX_RADIUS}], got {rx} and {ry}")
    try:
        with np.errstate(over="ignore"):
            min_disp, max_disp, min_ratio, q = (float(np.float32(v)) for v in (min_disp, max_disp, min_ratio, q))
        whole = int(hint_min_age) == hint_min_age
        hint_min_age = int(hint_min_age)
    except (TypeError, ValueError):
        raise err(f"{name}: min_disp, max_disp, min_ratio and q are numbers, hint_min_age a whole number") from None
    if not (0.0 <= occl_px < math.inf and 0.0 <= q < math.inf and 0.0 <= min_ratio < math.inf):
        raise err(f"{name}: occl_px, q and min_ratio must be finite and >= 0, got {occl_px}, {q} and {min_ratio}")
    if not (0.0 <= doffs < math.inf and 0.0 <= min_disp <= max_disp < math.inf):
        raise err(f"{name}: doffs >= 0 and 0 <= min_disp <= max_disp, all finite in float32, got {doffs}, {min_disp} and {max_disp}")
    if not whole or not 0 <= hint_min_age <= 255:
        raise err(f"{name}: hint_min_age is a whole number in [0, 255], got {hint_min_age}")
    return (None if g is None else [float(v) for v in g.reshape(-1)]), doffs, min_disp, max_disp, min_ratio, rx, ry, occl_px, q, \
        hint_min_age


def fuse_scalars(name, err, meas_var, min_disp, gate, var_max):
    """The scalar arguments of dca_temporal_fuse -> (meas_var or None for a map, min_disp, gate2, var_max), the floats rounded to
    float32: gate in sigmas, gate2 = float32(gate * gate) (inf: the gate is off)."""
    try:
        with np.errstate(over="ignore"):
            vm = None if meas_var is None else float(np.float32(meas_var))
            min_disp, var_max = float(np.float32(min_disp)), float(np.float32(var_max))
            gate = float(gate)
            gate2 = float(np.float32(gate * gate)) if math.isfinite(gate) else gate * gate
    except (TypeError, ValueError):
        raise err(f"{name}: meas_var (unless a map), min_disp, gate and var_max are numbers") from None
    if vm is not None and not 0.0 < vm < math.inf:
        raise err(f"{name}: a scalar meas_var must be positive and finite in float32, got {meas_var}")
    if not 0.0 <= min_disp < math.inf:
        raise err(f"{name}: min_disp must be finite and >= 0, got {min_disp}")
    if not (gate >= 0.0 and gate2 >= 0.0 and var_max >= 0.0):
        raise err(f"{name}: gate and var_max must be >= 0 and not NaN (inf switches either off), got {gate} and {var_max}")
    return vm, min_disp, gate2, var_max


def _state_host(name, state):
    try:
        d, v, a = (np.asarray(state[k]) for k in STATE_KEYS)
    except (TypeError, KeyError, IndexError):
        raise ValueError(f"{name}: the state is a dict with the keys {STATE_KEYS}") from None
    if d.dtype != np.float32 or v.dtype != np.float32 or a.dtype != np.uint8 or d.ndim != 2 or d.size == 0 \
            or v.shape != d.shape or a.shape != d.shape:
        raise ValueError(f"{name}: the state is (H,W) disp float32, var float32 and age uint8 of one shape, got "
                         f"{d.dtype} {d.shape}, {v.dtype} {v.shape}, {a.dtype} {a.shape}")
    return d, v, a


def _pass_host(name, mask, shape, mask_min):
    if mask is None:
        return np.ones(shape, bool)
    m = np.asarray(mask)
    if m.dtype != np.float32 or m.shape != shape:
        raise ValueError(f"{name}: the mask must be float32 of shape {shape}, got {m.dtype} {m.shape}")
    if math.isnan(float(mask_min)):
        raise ValueError(f"{name}: mask_min must not be NaN")
    with np.errstate(invalid="ignore"):
        return m >= np.float32(mask_min)


def project_host(d, g, doffs, min_disp, max_disp, min_ratio):
    """tm_project (csrc/temporal_math.h) for every pixel of the float32 map d, operation for operation: (keep bool, target
    int64 = vf W + uf where kept, den' float32, z float32)"""
    f32 = np.float32
    H, W = d.shape
    g = [f32(v) for v in g]
    u = np.arange(W, dtype=np.int64)[None, :].astype(f32)
    v = np.arange(H, dtype=np.int64)[:, None].astype(f32)
    with np.errstate(all="ignore"):
        den = d + f32(doffs)
        x, y, z = (((g[4 * r] * u + g[4 * r + 1] * v) + g[4 * r + 2]) + g[4 * r + 3] * den for r in range(3))
        up, vp = x / z, y / z
        uf, vf = np.floor(up + f32(0.5)), np.floor(vp + f32(0.5))
        dn = den / z
        dp = dn - f32(doffs)
        keep = np.isfinite(d) & (d >= f32(min_disp)) & (z >= f32(min_ratio)) & (uf >= 0) & (uf < f32(W)) & (vf >= 0) \
            & (vf < f32(H)) & (dp >= f32(min_disp)) & (dp < f32(max_disp))
        target = np.where(keep, vf, f32(0)).astype(np.int64) * W + np.where(keep, uf, f32(0)).astype(np.int64)
    return keep, target, dn.astype(f32), np.broadcast_to(z, d.shape).astype(f32)


def disp_reproject_host(state, G, calib=None, doffs=None, max_disp=TEMPORAL_MAX_DISP, min_disp=TEMPORAL_MIN_DISP,
                        min_ratio=TEMPORAL_MIN_RATIO, occl=TEMPORAL_OCCL, q=TEMPORAL_Q, hint_min_age=TEMPORAL_HINT_MIN_AGE,
                        mask=None, mask_min=0.5, outputs=None):
    """numpy restatement of dca_disp_reproject (include/dca_hip.h), float32 operation for float32 operation in the same order,
    with `np.maximum.at` on the 64-bit keys as the scatter: the state {"disp","var","age"} of the previous frame warped by
    G = `reproject_matrix(calib, T_cur_from_prev)` -> a dict with the keys of `outputs` (default all of REPROJECT_OUTPUTS):
    pred, var float32 (H,W), age uint8 (H,W), hints float32 (H,W), count int64 (2,) = (visible targets, kept sources), and
    "keys": the workspace as the kernels leave it, uint64 (H,W).  Equal to `ops.disp_reproject` bit for bit.  A G that is all
    NaN -- what a failed `odometry.ego_motion_host` hands out -- is taken as `ops.disp_reproject` takes it from the device: every
    comparison of the keep test fails, nothing is kept, the prediction is empty."""
    name = "disp_reproject_host"
    names = REPROJECT_OUTPUTS if outputs is None else tuple(outputs)
    if not names or any(k not in REPROJECT_OUTPUTS for k in names):
        raise ValueError(f"{name}: outputs are chosen from {REPROJECT_OUTPUTS}, at least one, got {names}")
    d, var, age = _state_host(name, state)
    H, W = d.shape
    g, doffs, min_disp, max_disp, min_ratio, rx, ry, occl_px, q, hint_min_age = reproject_scalars(
        name, ValueError, H, W, G, _doffs(name, ValueError, calib, doffs), min_disp, max_disp, min_ratio, occl, q, hint_min_age,
        nan_ok=True)
    f32 = np.float32
    keep, target, dn, z = project_host(d, g, doffs, min_disp, max_disp, min_ratio)
    keep &= _pass_host(name, mask, d.shape, mask_min)
    src = np.arange(H * W, dtype=np.uint64).reshape(H, W)
    key = (dn.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - src)
    ws = np.zeros(H * W, np.uint64)
    np.maximum.at(ws, target[keep], key[keep])
    ws = ws.reshape(H, W)
    high = (ws >> np.uint64(32)).astype(np.uint32)
    pad = np.zeros((H + 2 * ry, W + 2 * rx), np.uint32)
    pad[ry:ry + H, rx:rx + W] = high
    rowmax = pad[:, :W].copy()
    for k in range(1, 2 * rx + 1):
        np.maximum(rowmax, pad[:, k:k + W], out=rowmax)
    hmax = rowmax[:H].copy()
    for k in range(1, 2 * ry + 1):
        np.maximum(hmax, rowmax[k:k + H], out=hmax)
    denp, denmax = high.view(f32), hmax.view(f32)
    with np.errstate(all="ignore"):
        visible = (ws != 0) & (denp + f32(occl_px) >= denmax)
        win = (np.uint64(0xFFFFFFFF) - (ws & np.uint64(0xFFFFFFFF))).astype(np.int64)
        win = np.where(visible, win, 0)
        zs = z.reshape(-1)[win]
        pred = np.where(visible, denp - f32(doffs), f32(0))
        pvar = np.where(visible, var.reshape(-1)[win] / (zs * zs) + f32(q), f32(0)).astype(f32)
        page = np.where(visible, np.minimum(age.reshape(-1)[win].astype(np.int64) + 1, 255), 0).astype(np.uint8)
        hints = np.where(visible & (page.astype(np.int64) >= hint_min_age), pred, f32(0))
    res = {"pred": pred.astype(f32), "var": pvar, "age": page, "hints": hints.astype(f32),
           "count": np.array([int(visible.sum()), int(keep.sum())], np.int64)}
    res = {k: res[k] for k in REPROJECT_OUTPUTS if k in names}
    res["keys"] = ws
    return res


def _window_host(name, Hc, Wc, window):
    try:
        y0, rows, cols = (0, Hc, Wc) if window is None else (int(v) for v in window)
    except (TypeError, ValueError):
        raise ValueError(f"{name}: window is (y0, rows, cols), got {window!r}") from None
    if y0 < 0 or rows <= 0 or cols <= 0 or y0 + rows > Hc or cols > Wc:
        raise ValueError(f"{name}: the {rows} x {cols} window at row {y0} does not fit the {Hc} x {Wc} map")
    return y0, rows, cols


def temporal_fuse_host(pred, meas, meas_var=TEMPORAL_MEAS_VAR, window=None, mask=None, mask_min=0.5, min_disp=TEMPORAL_MIN_DISP,
                       gate=TEMPORAL_GATE, var_max=TEMPORAL_VAR_MAX, outputs=None):
    """numpy restatement of dca_temporal_fuse (include/dca_hip.h): the prediction `pred` -- a dict with "pred", "var", "age"
    (rows,cols), what `disp_reproject_host` gives, or None on the first frame -- and the measurement `meas`, a float32 frame map
    (Hc,Wc) / (1,1,Hc,Wc) read through window = (y0, rows, cols), with variance `meas_var`, a scalar or a float32 map shaped like
    meas, -> a dict with the keys of `outputs` (default the state, as `ops.temporal_fuse`; chosen from FUSE_OUTPUTS): the new state
    disp, var float32, age uint8, and innov float32, all (rows,cols).  gate in sigmas (inf: off).  Equal to `ops.temporal_fuse` bit
    for bit."""
    name = "temporal_fuse_host"
    names = STATE_KEYS if outputs is None else tuple(outputs)
    if not names or any(k not in FUSE_OUTPUTS for k in names):
        raise ValueError(f"{name}: outputs are chosen from {FUSE_OUTPUTS}, at least one, got {names}")
    f32 = np.float32
    m = np.asarray(meas)
    if m.dtype != np.float32 or m.ndim < 2 or m.size == 0 or m.size != m.shape[-2] * m.shape[-1]:
        raise ValueError(f"{name}: the measurement is ONE float32 (Hc,Wc) map, got {m.dtype} {m.shape}")
    Hc, Wc = m.shape[-2:]
    m = m.reshape(Hc, Wc)
    y0, rows, cols = _window_host(name, Hc, Wc, window)
    is_map = isinstance(meas_var, (np.ndarray, torch.Tensor))
    vm_s, min_disp, gate2, var_max = fuse_scalars(name, ValueError, None if is_map else meas_var, min_disp, gate, var_max)
    if is_map:
        vmap = np.asarray(meas_var)
        if vmap.dtype != np.float32 or vmap.size != m.size:
            raise ValueError(f"{name}: a meas_var map must be float32 of the measurement's shape, got {vmap.dtype} {vmap.shape}")
        vm = vmap.reshape(Hc, Wc)[y0:y0 + rows, :cols]
    else:
        vm = np.full((rows, cols), vm_s, f32)
    if mask is not None and np.size(mask) != m.size:
        raise ValueError(f"{name}: the mask must be float32 of the measurement's shape, got shape {np.shape(mask)}")
    passes = _pass_host(name, None if mask is None else np.asarray(mask).reshape(Hc, Wc), (Hc, Wc), mask_min)[y0:y0 + rows, :cols]
    m = m[y0:y0 + rows, :cols]
    if pred is None:
        p, pv, pa = np.zeros((rows, cols), f32), np.zeros((rows, cols), f32), np.zeros((rows, cols), np.uint8)
    else:
        try:
            p, pv, pa = (np.asarray(pred[k]) for k in ("pred", "var", "age"))
        except (TypeError, KeyError, IndexError):
            raise ValueError(f"{name}: pred is a dict with the keys 'pred', 'var' and 'age', or None") from None
        if p.dtype != f32 or pv.dtype != f32 or pa.dtype != np.uint8 or not p.shape == pv.shape == pa.shape == (rows, cols):
            raise ValueError(f"{name}: pred holds float32, float32 and uint8 maps of the window's shape {(rows, cols)}")
    with np.errstate(all="ignore"):
        m_ok = np.isfinite(m) & (m >= f32(min_disp)) & passes & (vm > 0) & (vm < f32(np.inf))
        p_ok = (p > 0) & (pv >= 0) & (pv <= f32(var_max)) & (pred is not None)
        e, s = m - p, pv + vm
        both = m_ok & p_ok
        inside = both & (e * e <= f32(gate2) * s)
        k = pv / s
        use_m = m_ok & ~inside                       # only the measurement, or a new surface
        use_p = p_ok & ~m_ok                         # coast
        disp = np.where(inside, p + k * e, np.where(use_m, m, np.where(use_p, p, f32(0))))
        var = np.where(inside, pv - k * pv, np.where(use_m, vm, np.where(use_p, pv, f32(0))))
        age = np.where(inside | use_p, pa, np.uint8(0))
        innov = np.where(both, np.abs(e), f32(0))
    res = {"disp": disp.astype(f32), "var": var.astype(f32), "age": age.astype(np.uint8), "innov": innov.astype(f32)}
    return {k: res[k] for k in FUSE_OUTPUTS if k in names}


# ------------------------------------------------------------------------------------------------
# The operators on the device (csrc/temporal.hip), by the conventions of frame_ops.py: arguments are validated once, here, with
# its helpers; a refusal names the operator and launches nothing; a tensor that is not on a ROCm device is an error; no launch
# synchronises; with `out` and `workspace` passed in nothing is allocated either.  ops.py re-exports them.
# A host matrix goes to the kernels BY VALUE: a launch captured into a hipGraph would keep the pose it was captured with, so these
# operators are launched eagerly, like every operator around the graphed hot path.  A matrix that is already on the device
# (`odometry.ego_motion`) is read there by the same kernels (dca_disp_reproject_dev) and never comes back to the host.
# ------------------------------------------------------------------------------------------------
TEMPORAL_MAX_RADIUS = _C["DCA_TEMPORAL_MAX_RADIUS"]
TEMPORAL_REPROJECT_OUTPUTS = REPROJECT_OUTPUTS
TEMPORAL_FUSE_OUTPUTS = FUSE_OUTPUTS
_REPROJECT_KINDS = {"pred": torch.float32, "var": torch.float32, "age": torch.uint8, "hints": torch.float32, "count": torch.int64}
_FUSE_KINDS = {"disp": torch.float32, "var": torch.float32, "age": torch.uint8, "innov": torch.float32}
assert MAX_RADIUS == TEMPORAL_MAX_RADIUS, "temporal.py restates another radius than include/dca_hip.h defines"


def temporal_workspace(h, w, device):
    """the int64 (h * w,) workspace of `disp_reproject(..., workspace=)` for states up to h x w: one 64-bit key per pixel.  The
    first launch of every call clears it; afterwards it holds the winning keys."""
    h, w = int(h), int(w)
    if h <= 0 or w <= 0 or h * w >= 1 << 31:
        raise RuntimeError(f"temporal_workspace: h and w positive with h * w below 2^31, got {h} x {w}")
    return torch.empty(h * w, device=device, dtype=torch.int64)


def _overlaps(a, b):
    return a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr()


def disp_reproject(state, G, calib=None, doffs=None, max_disp=TEMPORAL_MAX_DISP, min_disp=TEMPORAL_MIN_DISP,
                   min_ratio=TEMPORAL_MIN_RATIO, occl=TEMPORAL_OCCL, q=TEMPORAL_Q, hint_min_age=TEMPORAL_HINT_MIN_AGE,
                   mask=None, mask_min=0.5, outputs=None, out=None, workspace=None):
    """The previous frame's state warped by the known ego-motion into the current left image, three launches (definitions:
    include/dca_hip.h, dca_disp_reproject; `temporal.disp_reproject_host` is the numpy restatement, equal bit for bit).
    state: {"disp": float32, "var": float32 (px^2), "age": uint8}, (H,W) each on the device, +0.0 = nothing.  G: the (3,4)
    matrix of `temporal.reproject_matrix(calib, T_cur_from_prev)`, on the host -- or a float32 (3,4) tensor on the DEVICE, what
    `ops.ego_motion` estimates: it goes to dca_disp_reproject_dev, is read by the kernels and never by the host, so it cannot be
    validated; a NaN in it (a failed estimate) keeps no source and leaves an empty prediction and count = (0, 0).  calib (a geometry.StereoCalib) or doffs: the
    disparity offset.  A source pixel is kept with a finite d >= min_disp, mask >= mask_min, a depth ratio z >= min_ratio, a
    target inside the image and a new disparity in [min_disp, max_disp); the nearest surface of a target wins (64-bit integer
    fetch_max of its den' bits and the source index: the same bits for every order of arrival); occl = (rx, ry, occl_px) drops a
    winner more than occl_px pixels of disparity behind the nearest winner within rx columns and ry rows ((0, 0, x): off).
    Returns a dict of device tensors, those named in `outputs` (default all; the others are neither computed nor written):
      pred   float32 (H,W)   the predicted disparity, +0.0 where nothing is visible
      var    float32 (H,W)   var[src] / z^2 + q: a disparity scales with 1 / z, q is the process noise in px^2
      age    uint8   (H,W)   min(age[src] + 1, 255)
      hints  float32 (H,W)   pred where age >= hint_min_age, else +0.0: the hint map of `hints_to_quarter`
      count  int64   (2,)    visible targets, kept sources
    out: a dict of buffers for some or all of them (none may be a buffer of the state); workspace: `temporal_workspace(H, W, ...)`.
    With both given nothing is allocated and the host never waits.  NOT for hipGraph capture: a host matrix is passed by value,
    and capture with a device matrix is untested."""
    name = "disp_reproject"
    try:
        d, var, age = (state[k] for k in STATE_KEYS)
    except (TypeError, KeyError, IndexError):
        raise RuntimeError(f"{name}: the state is a dict with the keys {STATE_KEYS}") from None
    _req_no_grad(name, d, var, mask)
    _req_dev(d, name, "state['disp']", torch.float32)
    if d.dim() != 2 or d.numel() == 0:
        raise RuntimeError(f"{name}: the state is (H,W) maps, got {tuple(d.shape)}")
    H, W = int(d.shape[0]), int(d.shape[1])
    _req_dev(var, name, "state['var']", torch.float32, (H, W), like=d)
    _req_dev(age, name, "state['age']", torch.uint8, (H, W), like=d)
    if mask is not None:
        _req_dev(mask, name, "the mask", torch.float32, (H, W), like=d)
    mask_min = _mask_min(name, mask_min, mask is not None)
    g_dev = None
    if isinstance(G, torch.Tensor) and G.is_cuda:
        g_dev = _req_dev(G, name, "a device G", torch.float32, (3, 4), like=d)
    g, doffs, min_disp, max_disp, min_ratio, rx, ry, occl_px, q, hint_min_age = reproject_scalars(
        name, RuntimeError, H, W, None if g_dev is not None else G, _doffs(name, RuntimeError, calib, doffs), min_disp, max_disp,
        min_ratio, occl, q, hint_min_age)
    if outputs is not None and not tuple(outputs):
        raise RuntimeError(f"{name}: outputs must name at least one of {REPROJECT_OUTPUTS}")
    res = _out_dict(name, _REPROJECT_KINDS, (), outputs, out, lambda k: (2,) if k == "count" else (H, W), d)
    if any(_overlaps(o, s) for o in res.values() for s in (d, var, age) + tuple(t for t in (mask, g_dev) if t is not None)):
        raise RuntimeError(f"{name}: an output must not be a buffer of the state or the mask (the operator is not in place)")
    if workspace is None:
        workspace = temporal_workspace(H, W, d.device)
    _req_dev(workspace, name, "workspace", torch.int64, like=d)
    if workspace.numel() < H * W:
        raise RuntimeError(f"{name}: workspace must hold at least {H * W} int64 (`temporal_workspace`), got {workspace.numel()}")
    with torch.cuda.device_of(d):
        if g_dev is not None:
            _chk(_L().dca_disp_reproject_dev(_ptr(d), _ptr(var), _ptr(age), _ptr(mask), mask_min, _ptr(g_dev), H, W, doffs, min_disp,
                                             max_disp, min_ratio, rx, ry, occl_px, q, hint_min_age,
                                             *(_ptr(res.get(k)) for k in REPROJECT_OUTPUTS), _ptr(workspace), _stream()),
                 "dca_disp_reproject_dev")
            return res
        _chk(_L().dca_disp_reproject(_ptr(d), _ptr(var), _ptr(age), _ptr(mask), mask_min, *g, H, W, doffs, min_disp, max_disp,
                                     min_ratio, rx, ry, occl_px, q, hint_min_age, *(_ptr(res.get(k)) for k in REPROJECT_OUTPUTS),
                                     _ptr(workspace), _stream()), "dca_disp_reproject")
    return res


def temporal_fuse(pred, meas, meas_var=TEMPORAL_MEAS_VAR, window=None, mask=None, mask_min=0.5, min_disp=TEMPORAL_MIN_DISP,
                  gate=TEMPORAL_GATE, var_max=TEMPORAL_VAR_MAX, outputs=None, out=None):
    """Prediction and measurement into a new state, per pixel, one launch (definitions: include/dca_hip.h, dca_temporal_fuse;
    `temporal.temporal_fuse_host` is the numpy restatement, equal bit for bit).  pred: the dict `disp_reproject` returns
    ("pred", "var", "age", (rows,cols) each), or None: no prediction (the first frame).  meas: ONE float32 frame map (Hc,Wc) /
    (1,1,Hc,Wc) on the device, read through window = (y0, rows, cols) (default whole) and never copied; mask: float32, shaped
    like meas, a measurement counts where mask >= mask_min; meas_var: its variance in px^2, a scalar or a float32 map shaped like
    meas (a pixel whose variance is not positive and finite is no measurement).  Where both are valid and the innovation
    e = m - pred passes the gate, e^2 <= gate^2 (pred_var + meas_var), the two are averaged by their variances and the age is
    kept; a pixel that fails it starts again from the measurement (age 0); a pixel with only a prediction of variance <= var_max
    coasts; gate = inf switches the gate off.
    Returns a dict of device tensors, those named in `outputs` (default the state: disp, var, age), (rows,cols) each:
      disp float32, var float32, age uint8   the new state
      innov float32                          |e| where both are valid, else +0.0
    out: a dict of buffers for some or all of them; they may be the buffers of `pred`, or of the state `disp_reproject` read."""
    name = "temporal_fuse"
    _req_no_grad(name, meas, mask)
    _req_dev(meas, name, "the measurement", torch.float32)
    if meas.dim() < 2 or meas.numel() == 0 or meas.numel() != meas.shape[-2] * meas.shape[-1]:
        raise RuntimeError(f"{name}: the measurement is ONE (Hc,Wc) or (1,1,Hc,Wc) map, got {tuple(meas.shape)}")
    Hc, Wc = int(meas.shape[-2]), int(meas.shape[-1])
    y0, rows, cols = _window(name, Hc, Wc, window, "measurement")
    vmap = None
    if isinstance(meas_var, torch.Tensor):
        vmap = _req_dev(meas_var, name, "the meas_var map", torch.float32, like=meas)
        if vmap.numel() != meas.numel():
            raise RuntimeError(f"{name}: a meas_var map must have the measurement's shape, got {tuple(vmap.shape)}")
    vm, min_disp, gate2, var_max = fuse_scalars(name, RuntimeError, None if vmap is not None else meas_var, min_disp, gate, var_max)
    if mask is not None:
        _req_dev(mask, name, "the mask", torch.float32, like=meas)
        if mask.numel() != meas.numel():
            raise RuntimeError(f"{name}: the mask must have the measurement's shape, got {tuple(mask.shape)}")
    mask_min = _mask_min(name, mask_min, mask is not None)
    p = pv = pa = None
    if pred is not None:
        try:
            p, pv, pa = (pred[k] for k in ("pred", "var", "age"))
        except (TypeError, KeyError, IndexError):
            raise RuntimeError(f"{name}: pred is a dict with the keys 'pred', 'var' and 'age', or None") from None
        _req_dev(p, name, "pred['pred']", torch.float32, (rows, cols), like=meas)
        _req_dev(pv, name, "pred['var']", torch.float32, (rows, cols), like=meas)
        _req_dev(pa, name, "pred['age']", torch.uint8, (rows, cols), like=meas)
    names = STATE_KEYS if outputs is None else tuple(outputs)
    if not names:
        raise RuntimeError(f"{name}: outputs must name at least one of {FUSE_OUTPUTS}")
    res = _out_dict(name, _FUSE_KINDS, (), names, out, lambda k: (rows, cols), meas)
    if any(_overlaps(o, t) for o in res.values() for t in (meas, mask, vmap) if t is not None):
        raise RuntimeError(f"{name}: an output must not be the measurement's, the mask's or the variance map's buffer")
    with torch.cuda.device_of(meas):
        _chk(_L().dca_temporal_fuse(_ptr(p), _ptr(pv), _ptr(pa), _ptr(meas), _ptr(mask), _ptr(vmap), 1.0 if vm is None else vm,
                                    *(_ptr(res.get(k)) for k in FUSE_OUTPUTS), Hc, Wc, y0, rows, cols, min_disp, mask_min, gate2,
                                    var_max, _stream()), "dca_temporal_fuse")
    return res
