"""Stereo visual odometry: the motion of the left camera between two frames -- the pose `temporal.disp_reproject` needs --
estimated from the previous frame's disparity and the grey images of both frames by inverse-compositional Gauss-Newton on a
photometric error over a pyramid (Comport et al. 2007, Steinbruecker et al. 2011, Kerl et al. 2013).  DESIGN.md section 6s.

On top the validators, the named defaults and the numpy restatements of include/dca_hip.h (dca_grey_pyramid, dca_disp_pyramid,
dca_ego_motion) that the kernels of csrc/odometry.hip equal bit for bit (tests/test_gpu_odometry.py) -- the documented CPU path
for a user without a ROCm device; below them the operators, `grey_pyramid` / `disp_pyramid` / `ego_motion` (`ops.ego_motion`,
...), which take device tensors and have no CPU fallback.

A PYRAMID of `levels` levels of an (H,W) map is one flat array, level 0 first, level l of shape (H >> l, W >> l)
(`pyramid_views`).  The per-pixel part is float32, one numpy operation at a time; the solve is float64 in Python floats, one
operation at a time in the written order of csrc/odometry_math.h: IEEE, no fused multiply-add, no sin or cos."""
from __future__ import annotations

import math

import numpy as np
import torch

from ._call import _C, _L, _chk, _ptr, _req_no_grad, _stream
from .frame_ops import _out, _req_dev, _req_u8

MAX_LEVELS = 8                     # DCA_ODO_MAX_LEVELS of include/dca_hip.h
MAX_ITERS = 64                     # DCA_ODO_MAX_ITERS
SUMS = 29                          # DCA_ODO_SUMS: 21 upper w q_i q_j, 6 w q_i r, w r r, the count
REC_LEN = 24                       # DCA_ODO_REC_LEN
FRAME_LEN = 35                     # DCA_ODO_FRAME_LEN: world pose (4,4), motion (4,4), count, residual, status
REC_TAU, REC_COUNT, REC_RESIDUAL, REC_STATUS, REC_ITERS = 12, 15, 16, 17, 18
MAX_PIXELS = 1 << 20               # the overflow budget of the int64 sums
EGO_OUTPUTS = ("rec", "G", "sums")

# defaults
ODOMETRY_LEVELS = 4
ODOMETRY_ITERS = 6
ODOMETRY_MIN_DISP = 0.0625         # temporal.TEMPORAL_MIN_DISP
ODOMETRY_MAX_DISP = 192.0
ODOMETRY_MIN_RATIO = 0.125         # temporal.TEMPORAL_MIN_RATIO
ODOMETRY_GRAD_MIN = 4              # |gx| + |gy| of the central differences (twice the gradient), grey levels
ODOMETRY_HUBER = 8.0               # grey levels
ODOMETRY_MIN_PIXELS = 32


def pyramid_shapes(H, W, levels):
    return [(H >> l, W >> l) for l in range(levels)]


def pyramid_len(H, W, levels):
    return sum(h * w for h, w in pyramid_shapes(H, W, levels))


def pyramid_views(pyr, H, W, levels):
    """the levels of a flat pyramid (numpy or torch) as 2-D views"""
    views, off = [], 0
    for h, w in pyramid_shapes(H, W, levels):
        views.append(pyr[off:off + h * w].reshape(h, w))
        off += h * w
    return views


def _levels(name, err, H, W, levels, limit):
    try:
        whole = int(levels) == levels
        levels = int(levels)
    except (TypeError, ValueError):
        raise err(f"{name}: levels is a whole number") from None
    if not whole or not 1 <= levels <= MAX_LEVELS:
        raise err(f"{name}: levels must lie in [1, {MAX_LEVELS}], got {levels}")
    if H <= 0 or W <= 0 or (H >> (levels - 1)) < 1 or (W >> (levels - 1)) < 1:
        raise err(f"{name}: the coarsest of {levels} levels of a {H} x {W} map has no pixel")
    if limit is not None and H * W > limit:
        raise err(f"{name}: H * W must not exceed {limit}, got {H} x {W}")
    return levels


def ego_scalars(name, err, H, W, calib, levels, iters, min_disp, max_disp, min_ratio, grad_min, huber, min_pixels):
    """The scalar arguments of dca_ego_motion, checked as its launcher checks them -> (levels, iters, (f, baseline, cx, cy, doffs)
    float64, min_disp, max_disp, min_ratio float32 as floats, grad_min, huber float32 as float, huber_k, min_pixels)"""
    levels = _levels(name, err, H, W, levels, MAX_PIXELS)
    try:
        cam = tuple(float(getattr(calib, k)) for k in ("f", "baseline", "cx", "cy", "doffs"))
    except (AttributeError, TypeError, ValueError):
        raise err(f"{name}: calib must be a geometry.StereoCalib (f, baseline, cx, cy, doffs)") from None
    if not (all(math.isfinite(v) for v in cam) and cam[0] > 0 and cam[1] > 0 and cam[4] >= 0):
        raise err(f"{name}: the calibration must be finite with f > 0, baseline > 0 and doffs >= 0")
    try:
        with np.errstate(over="ignore"):
            min_disp, max_disp, min_ratio, huber = (float(np.float32(v)) for v in (min_disp, max_disp, min_ratio, huber))
        if int(iters) != iters or int(grad_min) != grad_min or int(min_pixels) != min_pixels:
            raise ValueError
        iters, grad_min, min_pixels = int(iters), int(grad_min), int(min_pixels)
    except (TypeError, ValueError):
        raise err(f"{name}: min_disp, max_disp, min_ratio and huber are numbers; iters, grad_min and min_pixels whole numbers") from None
    if not 1 <= iters <= MAX_ITERS:
        raise err(f"{name}: iters must lie in [1, {MAX_ITERS}], got {iters}")
    if not (0.0 <= min_disp < max_disp < math.inf and 0.0 < min_ratio < math.inf):
        raise err(f"{name}: 0 <= min_disp < max_disp and min_ratio > 0, all finite in float32, got {min_disp}, {max_disp} and {min_ratio}")
    if not 0 <= grad_min <= 510 or min_pixels < 6:
        raise err(f"{name}: grad_min must lie in [0, 510] and min_pixels be at least 6, got {grad_min} and {min_pixels}")
    huber_k = int(np.rint(huber * 256.0)) if math.isfinite(huber) else 0
    if not 1 <= huber_k <= 65280:
        raise err(f"{name}: huber must be finite with 1 <= rint(256 huber) <= 65280, got {huber}")
    return levels, iters, cam, min_disp, max_disp, min_ratio, grad_min, huber, huber_k, min_pixels


def _pose34(name, err, T):
    try:
        T = np.asarray(T, np.float64)
    except (TypeError, ValueError):
        raise err(f"{name}: init is a (4,4) or (3,4) pose, a record of an earlier call, or None") from None
    if T.shape not in ((4, 4), (3, 4)) or not np.isfinite(T).all():
        raise err(f"{name}: a start pose must be a finite (4,4) or (3,4) array, got shape {T.shape}")
    return [float(v) for v in T[:3].reshape(-1)]


# ---- the arithmetic of csrc/odometry_math.h in Python floats (IEEE doubles), one operation at a time ---------------------------
def level_camera(cam, l):
    """(f_l, cx_l, cy_l, doffs_l) of (f, baseline, cx, cy, doffs)"""
    f, _, cx, cy, doffs = cam
    s = math.ldexp(1.0, l)
    return f / s, (cx + 0.5) / s - 0.5, (cy + 0.5) / s - 0.5, doffs / s


def exponents(f, cx, cy, doffs, max_disp, H, W):
    """om_exponents: e_i with 510 max|Ju_i, Jv_i| 2^e_i <= 2^17 over the H x W level"""
    A, Bv = max(abs(cx), abs(float(W - 1) - cx)), max(abs(cy), abs(float(H - 1) - cy))
    Dn = max_disp + doffs
    B = (Dn, Dn, max(A, Bv) * Dn / f, max(A * Bv / f, f + Bv * Bv / f), max(f + A * A / f, A * Bv / f), max(A, Bv))
    return [min(60, max(-60, 17 - math.frexp(510.0 * b)[1])) for b in B]


def _dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def form_g(R, tau, f, cx, cy):
    """om_form_g: G = (1/f) [ K R A | K tau ], float32 (12,); R a list of 9, tau of 3 (baselines)"""
    K = ((f, 0.0, cx), (0.0, f, cy), (0.0, 0.0, 1.0))
    A = ((1.0, 0.0, -cx), (0.0, 1.0, -cy), (0.0, 0.0, f))
    RA = [[_dot3(R[3 * i:3 * i + 3], [A[0][j], A[1][j], A[2][j]]) for j in range(3)] for i in range(3)]
    g = []
    for i in range(3):
        g += [_dot3(K[i], [RA[0][j], RA[1][j], RA[2][j]]) / f for j in range(3)] + [_dot3(K[i], tau) / f]
    with np.errstate(over="ignore"):
        return np.array(g, np.float64).astype(np.float32)


def ldl_solve(A, c):
    """om_ldl_solve: x with A x = c, or None if a pivot is not positive"""
    L, Dg, y, x = [[0.0] * 6 for _ in range(6)], [0.0] * 6, [0.0] * 6, [0.0] * 6
    for j in range(6):
        d = A[j][j]
        for k in range(j):
            d = d - (L[j][k] * L[j][k]) * Dg[k]
        if not d > 0.0:
            return None
        Dg[j] = d
        for i in range(j + 1, 6):
            s = A[i][j]
            for k in range(j):
                s = s - (L[i][k] * L[j][k]) * Dg[k]
            L[i][j] = s / d
    for i in range(6):
        s = c[i]
        for k in range(i):
            s = s - L[i][k] * y[k]
        y[i] = s
    for i in range(5, -1, -1):
        s = y[i] / Dg[i]
        for k in range(i + 1, 6):
            s = s - L[k][i] * x[k]
        x[i] = s
    return x


def _upper(i, j):
    return i * 6 - i * (i - 1) // 2 + (j - i)


def step(S, e):
    """om_step: the 29 sums (Python ints) and the exponents -> xi = (tau, omega), or None"""
    A = [[0.0] * 6 for _ in range(6)]
    c = [0.0] * 6
    for i in range(6):
        for j in range(i, 6):
            A[i][j] = A[j][i] = float(S[_upper(i, j)]) * math.ldexp(1.0, -e[i] - e[j])
        A[i][i] = A[i][i] * (1.0 + 0.0009765625)
        c[i] = float(S[21 + i]) * math.ldexp(1.0, -e[i] - 7)
    return ldl_solve(A, c)


def cayley(w):
    """om_cayley: the rotation of omega = w, a list of 9"""
    a0, a1, a2 = w[0] * 0.5, w[1] * 0.5, w[2] * 0.5
    n = (a0 * a0 + a1 * a1) + a2 * a2
    den, m = 1.0 + n, 1.0 - n
    return [(m + 2.0 * (a0 * a0)) / den, (2.0 * (a0 * a1) - 2.0 * a2) / den, (2.0 * (a0 * a2) + 2.0 * a1) / den,
            (2.0 * (a1 * a0) + 2.0 * a2) / den, (m + 2.0 * (a1 * a1)) / den, (2.0 * (a1 * a2) - 2.0 * a0) / den,
            (2.0 * (a2 * a0) - 2.0 * a1) / den, (2.0 * (a2 * a1) + 2.0 * a0) / den, (m + 2.0 * (a2 * a2)) / den]


def compose(R, tau, Rw, tw):
    """om_compose: T [Rw | tw]^-1 -> (R Rw^T, tau - R_new tw)"""
    Rn = [_dot3(R[3 * i:3 * i + 3], Rw[3 * j:3 * j + 3]) for i in range(3) for j in range(3)]
    return Rn, [tau[i] - _dot3(Rn[3 * i:3 * i + 3], tw) for i in range(3)]


def residual(S):
    return (float(S[27]) * math.ldexp(1.0, -22)) / float(S[28]) if S[28] > 0 else 0.0


# ---- the per-pixel part, float32 and integers -----------------------------------------------------------------------------------
def grey_pyramid_host(rgb, levels):
    """numpy restatement of dca_grey_pyramid: (H,W,3|4) uint8 -> the flat uint8 pyramid"""
    name = "grey_pyramid_host"
    rgb = np.asarray(rgb)
    if rgb.dtype != np.uint8 or rgb.ndim != 3 or rgb.shape[2] not in (3, 4) or rgb.size == 0:
        raise ValueError(f"{name}: expected a (H,W,3) or (H,W,4) uint8 image, got {rgb.dtype} {rgb.shape}")
    H, W = rgb.shape[:2]
    levels = _levels(name, ValueError, H, W, levels, (1 << 29) - 1)
    c = rgb.astype(np.int64)
    out = [(c[..., 0] + 2 * c[..., 1] + c[..., 2] + 2) >> 2]
    for h, w in pyramid_shapes(H, W, levels)[1:]:
        p = out[-1]
        out.append((p[0:2 * h:2, 0:2 * w:2] + p[0:2 * h:2, 1:2 * w:2] + p[1:2 * h:2, 0:2 * w:2] + p[1:2 * h:2, 1:2 * w:2] + 2) >> 2)
    return np.concatenate([p.reshape(-1) for p in out]).astype(np.uint8)


def disp_pyramid_host(disp, levels, min_disp=ODOMETRY_MIN_DISP):
    """numpy restatement of dca_disp_pyramid: (H,W) float32 -> the flat float32 pyramid; each further level the largest valid
    value (finite, >= min_disp) of the 2x2 block, halved, +0.0 where none is"""
    name = "disp_pyramid_host"
    disp = np.asarray(disp)
    if disp.dtype != np.float32 or disp.ndim != 2 or disp.size == 0:
        raise ValueError(f"{name}: expected a (H,W) float32 map, got {disp.dtype} {disp.shape}")
    H, W = disp.shape
    levels = _levels(name, ValueError, H, W, levels, (1 << 29) - 1)
    min_disp = float(np.float32(min_disp))
    if not 0.0 <= min_disp < math.inf:
        raise ValueError(f"{name}: min_disp must be finite and >= 0, got {min_disp}")
    out = [disp]
    for h, w in pyramid_shapes(H, W, levels)[1:]:
        p = out[-1]
        blk = np.stack([p[0:2 * h:2, 0:2 * w:2], p[0:2 * h:2, 1:2 * w:2], p[1:2 * h:2, 0:2 * w:2], p[1:2 * h:2, 1:2 * w:2]])
        with np.errstate(invalid="ignore"):
            ok = np.isfinite(blk) & (blk >= np.float32(min_disp))
        m = np.where(ok, blk, np.float32(-1)).max(0)
        out.append(np.where(ok.any(0), m * np.float32(0.5) + np.float32(0), np.float32(0)).astype(np.float32))   # (+ 0: no -0.0)
    return np.concatenate([p.reshape(-1) for p in out])


def level_sums(Ip, Ic, D, g, f, cx, cy, doffs, min_disp, max_disp, min_ratio, grad_min, huber_k, e):
    """The 29 sums of one iteration at one level (om_pixel and om_accumulate over the interior pixels), a list of Python ints.
    Ip, Ic uint8 (H,W), D float32 (H,W), g the 12 floats of G_l, the camera as float32-representable floats."""
    f32 = np.float32
    H, W = Ip.shape
    if H < 3 or W < 3:
        return [0] * SUMS
    g = [f32(v) for v in g]
    f, cx, cy, doffs = f32(f), f32(cx), f32(cy), f32(doffs)
    u = np.arange(1, W - 1, dtype=np.int64)[None, :].astype(f32)
    v = np.arange(1, H - 1, dtype=np.int64)[:, None].astype(f32)
    Ipi, Ici = Ip.astype(np.int64), Ic.astype(np.int64)
    d = D[1:-1, 1:-1]
    gx, gy = Ipi[1:-1, 2:] - Ipi[1:-1, :-2], Ipi[2:, 1:-1] - Ipi[:-2, 1:-1]
    with np.errstate(all="ignore"):
        ok = np.isfinite(d) & (d >= f32(min_disp)) & (d < f32(max_disp)) & (np.abs(gx) + np.abs(gy) >= grad_min)
        den = d + doffs
        x, y, z = (((g[4 * r] * u + g[4 * r + 1] * v) + g[4 * r + 2]) + g[4 * r + 3] * den for r in range(3))
        ok &= z >= f32(min_ratio)
        px, py = np.floor((x / z) * f32(16) + f32(0.5)), np.floor((y / z) * f32(16) + f32(0.5))
        ok &= (px >= 0) & (px < f32((W - 1) * 16)) & (py >= 0) & (py < f32((H - 1) * 16))
        ix, iy = np.where(ok, px, f32(0)).astype(np.int64), np.where(ok, py, f32(0)).astype(np.int64)
        x0, y0, fx, fy = ix >> 4, iy >> 4, ix & 15, iy & 15
        r = (16 - fy) * ((16 - fx) * Ici[y0, x0] + fx * Ici[y0, x0 + 1]) + fy * ((16 - fx) * Ici[y0 + 1, x0] + fx * Ici[y0 + 1, x0 + 1]) \
            - (Ipi[1:-1, 1:-1] << 8)
        a, b = u - cx, v - cy
        af, bf = a / f, b / f
        fgx, fgy = gx.astype(f32), gy.astype(f32)
        J = [fgx * den, fgy * den,
             fgx * (-(af * den)) + fgy * (-(bf * den)),
             fgx * (-(af * b)) + fgy * (-(f + bf * b)),
             fgx * (f + af * a) + fgy * (af * b),
             fgx * (-b) + fgy * a]
        q = [np.rint(np.where(ok, J[i] * f32(math.ldexp(1.0, e[i])), f32(0))).astype(np.int64) for i in range(6)]
    ar = np.abs(r)
    w = np.where(ar <= huber_k, 64, (64 * huber_k) // np.maximum(ar, 1))
    w = np.where(ok, w, 0)
    S = []
    for i in range(6):
        S += [int((w * q[i] * q[j]).sum(dtype=np.int64)) for j in range(i, 6)]
    S += [int((w * q[i] * r).sum(dtype=np.int64)) for i in range(6)]
    return S + [int((w * r * r).sum(dtype=np.int64)), int(ok.sum())]


def _check_pyramids(name, prev, cur, disp, hw, levels):
    try:
        H, W = (int(v) for v in hw)
    except (TypeError, ValueError):
        raise ValueError(f"{name}: hw is (H, W), got {hw!r}") from None
    prev, cur, disp = np.asarray(prev), np.asarray(cur), np.asarray(disp)
    n = pyramid_len(H, W, levels)
    if prev.dtype != np.uint8 or cur.dtype != np.uint8 or disp.dtype != np.float32 or not prev.shape == cur.shape == disp.shape == (n,):
        raise ValueError(f"{name}: prev and cur are uint8 and disp float32 flat pyramids of {n} elements ({levels} levels of "
                         f"{H} x {W}), got {prev.dtype} {prev.shape}, {cur.dtype} {cur.shape}, {disp.dtype} {disp.shape}")
    return prev, cur, disp


def ego_motion_host(prev, cur, disp, hw, calib, levels=ODOMETRY_LEVELS, iters=ODOMETRY_ITERS, min_disp=ODOMETRY_MIN_DISP,
                    max_disp=ODOMETRY_MAX_DISP, min_ratio=ODOMETRY_MIN_RATIO, grad_min=ODOMETRY_GRAD_MIN, huber=ODOMETRY_HUBER,
                    min_pixels=ODOMETRY_MIN_PIXELS, init=None):
    """numpy restatement of dca_ego_motion (include/dca_hip.h), operation for operation in the same order: prev, cur the grey
    pyramids (`grey_pyramid_host`) of the previous and the current left image, disp the disparity pyramid (`disp_pyramid_host`)
    of the previous frame, hw = (H, W) of level 0, calib a geometry.StereoCalib.  init: None (the identity), a (4,4) / (3,4)
    pose T_cur_from_prev in metres, or the "rec" of an earlier result.  Returns a dict:
      rec   float64 (24,)   [0:12] T_cur_from_prev (3,4), metres; [12:15] the translation in baselines; [15] count, [16] mean
                            weighted squared residual of the last iteration that ran; [17] status 0 ok / 1 failed; [18] iterations
      G     float32 (3,4)   `temporal.reproject_matrix` of the estimate for level 0; NaN if failed
      sums  int64 (levels * iters, 29)   the sums of every iteration in the order they ran
    Equal to `ops.ego_motion` bit for bit."""
    name = "ego_motion_host"
    H, W = (int(v) for v in hw) if np.ndim(hw) == 1 and len(hw) == 2 else (0, 0)
    levels, iters, cam, min_disp, max_disp, min_ratio, grad_min, huber, huber_k, min_pixels = ego_scalars(
        name, ValueError, H, W, calib, levels, iters, min_disp, max_disp, min_ratio, grad_min, huber, min_pixels)
    prev, cur, disp = _check_pyramids(name, prev, cur, disp, (H, W), levels)
    baseline = cam[1]
    R, tau = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0], [0.0, 0.0, 0.0]
    if isinstance(init, np.ndarray) and init.shape == (REC_LEN,) and init.dtype == np.float64:
        if init[REC_STATUS] == 0.0:
            R = [float(init[4 * i + j]) for i in range(3) for j in range(3)]
            tau = [float(v) for v in init[REC_TAU:REC_TAU + 3]]
    elif init is not None:
        t = _pose34(name, ValueError, init)
        R, tau = [t[4 * i + j] for i in range(3) for j in range(3)], [t[4 * i + 3] / baseline for i in range(3)]
    Ips, Ics, Ds = (pyramid_views(p, H, W, levels) for p in (prev, cur, disp))
    cam0 = level_camera(cam, 0)
    g0, gl = form_g(R, tau, *cam0[:3]), form_g(R, tau, *level_camera(cam, levels - 1)[:3])
    sums = np.zeros((levels * iters, SUMS), np.int64)
    count, res, status, done, slot = 0.0, 0.0, 0.0, 0.0, 0
    f32 = np.float32
    for l in range(levels - 1, -1, -1):
        fl, cxl, cyl, dl = level_camera(cam, l)
        nxt = level_camera(cam, max(l - 1, 0))
        mdl = float(f32(math.ldexp(max_disp, -l)))
        h, w = Ips[l].shape
        e = exponents(fl, cxl, cyl, dl, mdl, h, w)
        for it in range(iters):
            if status == 0.0:
                S = level_sums(Ips[l], Ics[l], Ds[l], gl, float(f32(fl)), float(f32(cxl)), float(f32(cyl)), float(f32(dl)), min_disp,
                               mdl, min_ratio, grad_min, huber_k, e)
                sums[slot] = S
                count, res, done = float(S[28]), residual(S), float(slot + 1)
                xi = step(S, e) if S[28] >= min_pixels else None
                if xi is None:
                    status = 1.0
                    g0 = gl = np.full(12, np.nan, f32)
                else:
                    R, tau = compose(R, tau, cayley(xi[3:]), xi[:3])
                    g0 = form_g(R, tau, *cam0[:3])
                    gl = form_g(R, tau, *((fl, cxl, cyl) if it + 1 < iters else nxt[:3]))
            slot += 1
    rec = np.zeros(REC_LEN, np.float64)
    for i in range(3):
        rec[4 * i:4 * i + 3] = R[3 * i:3 * i + 3]
        rec[4 * i + 3] = tau[i] * baseline
    rec[REC_TAU:REC_TAU + 3] = tau
    rec[REC_COUNT], rec[REC_RESIDUAL], rec[REC_STATUS], rec[REC_ITERS] = count, res, status, done
    return {"rec": rec, "G": g0.reshape(3, 4), "sums": sums}


def pose_chain_host(rec, world):
    """numpy restatement of dca_pose_chain (om_chain): rec a float64 (24,) record or None (a sequence starts), world the float64
    (12,) pose so far -> (the new world pose (12,), the frame's 35 doubles), Python floats in the written order"""
    W = [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0]
    T, tail = list(W), [0.0, 0.0, 0.0]
    if rec is not None:
        W, tail = [float(v) for v in world], [float(rec[REC_COUNT]), float(rec[REC_RESIDUAL]), float(rec[REC_STATUS])]
        if rec[REC_STATUS] == 0.0:
            T = [float(v) for v in rec[:12]]
            Ri = [T[4 * j + i] for i in range(3) for j in range(3)]
            ti = [-((T[i] * T[3] + T[4 + i] * T[7]) + T[8 + i] * T[11]) for i in range(3)]
            Wn = []
            for i in range(3):
                Wn += [(W[4 * i] * Ri[j] + W[4 * i + 1] * Ri[3 + j]) + W[4 * i + 2] * Ri[6 + j] for j in range(3)]
                Wn.append(((W[4 * i] * ti[0] + W[4 * i + 1] * ti[1]) + W[4 * i + 2] * ti[2]) + W[4 * i + 3])
            W = Wn
    last = [0.0, 0.0, 0.0, 1.0]
    return np.array(W, np.float64), np.array(W + last + T + last + tail, np.float64)


def pose44(rec):
    """the (4,4) float64 T_cur_from_prev (metres) of a record, host or device"""
    rec = rec.cpu().numpy() if isinstance(rec, torch.Tensor) else np.asarray(rec)
    T = np.eye(4)
    T[:3] = rec[:12].reshape(3, 4)
    return T


# ------------------------------------------------------------------------------------------------
# The operators on the device (csrc/odometry.hip), by the conventions of frame_ops.py: arguments are validated once, here; a
# refusal names the operator and launches nothing; a tensor that is not on a ROCm device is an error; no launch synchronises
# and nothing is read back.  ops.py re-exports them.
# ------------------------------------------------------------------------------------------------
ODOMETRY_MAX_LEVELS = _C["DCA_ODO_MAX_LEVELS"]
ODOMETRY_REC_LEN = _C["DCA_ODO_REC_LEN"]
ODOMETRY_SUMS = _C["DCA_ODO_SUMS"]
assert (MAX_LEVELS, MAX_ITERS, SUMS, REC_LEN, FRAME_LEN) == (ODOMETRY_MAX_LEVELS, _C["DCA_ODO_MAX_ITERS"], ODOMETRY_SUMS, ODOMETRY_REC_LEN,
                                                            _C["DCA_ODO_FRAME_LEN"]), \
    "odometry.py restates other constants than include/dca_hip.h defines"


def grey_pyramid(rgb_u8, levels=ODOMETRY_LEVELS, out=None):
    """The grey pyramid of an interleaved (H,W,3) / (H,W,4) uint8 image on the device, one launch per level: level 0 is
    (R + 2 G + B + 2) >> 2, each further level the 2x2 area mean (a + b + c + d + 2) >> 2; odd sizes drop the last row or column.
    Returns the flat uint8 pyramid of `pyramid_len(H, W, levels)` elements (`pyramid_views` gives the levels); out: a buffer for
    it.  `grey_pyramid_host` is the numpy restatement, equal bit for bit."""
    name = "grey_pyramid"
    _req_no_grad(name, rgb_u8)
    H, W, C = _req_u8(rgb_u8, name, "the image")
    levels = _levels(name, RuntimeError, H, W, levels, (1 << 29) - 1)
    res = _out(name, "out", out, torch.uint8, (pyramid_len(H, W, levels),), rgb_u8, alias=(rgb_u8,))
    with torch.cuda.device_of(rgb_u8):
        _chk(_L().dca_grey_pyramid(_ptr(rgb_u8), H, W, C, levels, _ptr(res), _stream()), "dca_grey_pyramid")
    return res


def disp_pyramid(disp, levels=ODOMETRY_LEVELS, min_disp=ODOMETRY_MIN_DISP, out=None):
    """The disparity pyramid of a (H,W) float32 map on the device, one launch per level: level 0 is the map, each further level
    the largest valid value (finite, >= min_disp: the nearest surface) of the 2x2 block, halved, +0.0 where none is valid.
    Returns the flat float32 pyramid; out: a buffer for it.  `disp_pyramid_host` is the numpy restatement, equal bit for bit."""
    name = "disp_pyramid"
    _req_no_grad(name, disp)
    _req_dev(disp, name, "the disparity", torch.float32)
    if disp.dim() != 2 or disp.numel() == 0:
        raise RuntimeError(f"{name}: expected a (H,W) map, got {tuple(disp.shape)}")
    H, W = int(disp.shape[0]), int(disp.shape[1])
    levels = _levels(name, RuntimeError, H, W, levels, (1 << 29) - 1)
    min_disp = float(np.float32(min_disp))
    if not 0.0 <= min_disp < math.inf:
        raise RuntimeError(f"{name}: min_disp must be finite and >= 0, got {min_disp}")
    res = _out(name, "out", out, torch.float32, (pyramid_len(H, W, levels),), disp, alias=(disp,))
    with torch.cuda.device_of(disp):
        _chk(_L().dca_disp_pyramid(_ptr(disp), H, W, levels, min_disp, _ptr(res), _stream()), "dca_disp_pyramid")
    return res


_EGO_KINDS = {"rec": torch.float64, "g": torch.float32, "sums": torch.int64}


def ego_motion(prev, cur, disp, hw, calib, levels=ODOMETRY_LEVELS, iters=ODOMETRY_ITERS, min_disp=ODOMETRY_MIN_DISP,
               max_disp=ODOMETRY_MAX_DISP, min_ratio=ODOMETRY_MIN_RATIO, grad_min=ODOMETRY_GRAD_MIN, huber=ODOMETRY_HUBER,
               min_pixels=ODOMETRY_MIN_PIXELS, init=None, outputs=None, out=None, workspace=None):
    """The motion of the left camera between two frames, estimated on the device: 1 + 2 levels iters small launches, nothing read
    back (definitions: include/dca_hip.h, dca_ego_motion; `odometry.ego_motion_host` is the numpy restatement, equal bit for bit).
    prev, cur: the flat grey pyramids (`grey_pyramid`) of the previous and the current left image; disp: the flat disparity
    pyramid (`disp_pyramid`) of the previous frame; hw = (H, W) of level 0, H * W <= 2^20; calib: a geometry.StereoCalib.
    init: None (start from the identity), a (4,4) / (3,4) host pose T_cur_from_prev in metres, or the float64 (24,) DEVICE record
    of an earlier call (constant velocity; a failed record starts from the identity; it may be out["rec"] itself).
    Returns a dict of device tensors:
      rec   float64 (24,)   [0:12] T_cur_from_prev (3,4), metres; [12:15] the translation in baselines; [15] count, [16] mean
                            weighted squared residual of the last iteration that ran; [17] status 0 ok / 1 failed; [18] iterations
      G     float32 (3,4)   the matrix of `ops.disp_reproject` for this motion, a view of the first half of the buffer "g";
                            NaN if the estimate failed (fewer than min_pixels pixels, a pivot that is not positive)
      sums  int64 (levels * iters, 29)   only if named in `outputs`: the sums of every iteration (a debug slot)
    out: a dict of buffers "rec", "g" (float32 (24,): G of level 0, then G of the running level) and "sums"; workspace: int64
    (29,).  With all given nothing is allocated; they may hold garbage."""
    name = "ego_motion"
    _req_no_grad(name, disp)
    try:
        H, W = (int(v) for v in hw)
    except (TypeError, ValueError):
        raise RuntimeError(f"{name}: hw is (H, W), got {hw!r}") from None
    levels, iters, cam, min_disp, max_disp, min_ratio, grad_min, huber, _, min_pixels = ego_scalars(
        name, RuntimeError, H, W, calib, levels, iters, min_disp, max_disp, min_ratio, grad_min, huber, min_pixels)
    n = pyramid_len(H, W, levels)
    _req_dev(prev, name, "the previous grey pyramid", torch.uint8, (n,))
    _req_dev(cur, name, "the current grey pyramid", torch.uint8, (n,), like=prev)
    _req_dev(disp, name, "the disparity pyramid", torch.float32, (n,), like=prev)
    names = ("rec", "G") if outputs is None else tuple(outputs)
    if not names or any(k not in EGO_OUTPUTS for k in names):
        raise RuntimeError(f"{name}: outputs are chosen from {EGO_OUTPUTS}, at least one, got {names}")
    out = {} if out is None else out
    if not isinstance(out, dict) or set(out) - set(_EGO_KINDS):
        raise RuntimeError(f"{name}: out must be a dict with keys out of {tuple(_EGO_KINDS)}")
    shapes = {"rec": (REC_LEN,), "g": (24,), "sums": (levels * iters, SUMS)}
    buf = {k: _out(name, f"out[{k!r}]", out.get(k), _EGO_KINDS[k], shapes[k], prev) for k in _EGO_KINDS
           if k != "sums" or "sums" in names}
    if workspace is None:
        workspace = torch.empty(SUMS, device=prev.device, dtype=torch.int64)
    _req_dev(workspace, name, "workspace", torch.int64, like=prev)
    if workspace.numel() < SUMS:
        raise RuntimeError(f"{name}: workspace must hold at least {SUMS} int64, got {workspace.numel()}")
    init_rec, t = None, [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0]
    if isinstance(init, torch.Tensor) and init.is_cuda:
        init_rec = _req_dev(init, name, "a device init record", torch.float64, (REC_LEN,), like=prev)
    elif init is not None:
        t = _pose34(name, RuntimeError, init.numpy() if isinstance(init, torch.Tensor) else init)
    with torch.cuda.device_of(prev):
        _chk(_L().dca_ego_motion(_ptr(prev), _ptr(cur), _ptr(disp), H, W, levels, iters, *cam, min_disp, max_disp, min_ratio,
                                 grad_min, huber, min_pixels, _ptr(init_rec), *t, _ptr(buf["rec"]), _ptr(buf["g"]),
                                 _ptr(workspace), _ptr(buf.get("sums")), _stream()), "dca_ego_motion")
    res = {"rec": buf["rec"], "G": buf["g"][:12].view(3, 4)}
    if "sums" in names:
        res["sums"] = buf["sums"]
    return res


def pose_chain(rec, world, out=None):
    """The world pose of a sequence kept on the device, one launch: world float64 (12,), the (3,4) pose of the current camera in
    the world, becomes world T^-1 with T the motion of the record `rec` (`ego_motion`'s "rec"; a failed record leaves it as it
    is); rec None: a sequence starts, world becomes the identity.  Returns the frame's float64 (35,) on the device: the world
    pose (4,4), the motion (4,4), count, residual, status.  `pose_chain_host` is the numpy restatement, equal bit for bit."""
    name = "pose_chain"
    _req_dev(world, name, "the world pose", torch.float64, (12,))
    if rec is not None:
        _req_dev(rec, name, "the record", torch.float64, (REC_LEN,), like=world)
    res = _out(name, "out", out, torch.float64, (FRAME_LEN,), world, alias=(world,) + (() if rec is None else (rec,)))
    with torch.cuda.device_of(world):
        _chk(_L().dca_pose_chain(_ptr(rec), _ptr(world), _ptr(res), _stream()), "dca_pose_chain")
    return res
