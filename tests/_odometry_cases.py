"""Seeded synthetic sequences for the visual-odometry tests (CPU and GPU): the scenes of tests/_temporal_cases.py with a smooth
texture painted on the WORLD -- a few sines of the hit point, the shortest period (1.1 m) twenty pixels at the nearest surface, a
constant where no ray hits -- so that an image rendered from another pose shows the same world and the photometric error of
the true motion is only that of sampling and of rounding to uint8.  A few thousand pixels each, plus two small images for the
edge cases (odd sizes, one workgroup, levels with fewer pixels than an estimate needs)."""
import functools
import math

import numpy as np

import _temporal_cases as C
from dcanet_amd import geometry as GEO
from dcanet_amd import odometry as OD
from dcanet_amd.geometry import StereoCalib

MAX_DISP = C.MAX_DISP
LEVELS, ITERS = 3, 6                                         # what the scenes' sizes allow: level 2 of 48 x 75 is 12 x 18
SCENES = C.SCENES
SMALL = (C.Scene("21x33", (21, 33), StereoCalib(20.0, C.BASELINE, 16.0, 7.5), (-1.2, -0.2, 0.5, 5.0, 6.0), 12.0),
         C.Scene("17x64", (17, 64), StereoCalib(36.0, C.BASELINE, 31.5, 5.5), (0.3, 1.5, 0.6, 6.0, 7.0), 14.0))
SKY = 90                                                     # the grey level where no ray hits


def _compose(*Ts):
    return functools.reduce(np.matmul, Ts)


# the camera's pose in the world after the move (camera coordinates -> world coordinates); before it, the identity
POSES = (("identity", np.eye(4)), ("forward0.2m", C.translation(z=0.2)), ("forward1m", C.translation(z=1.0)),
         ("back0.3m", C.translation(z=-0.3)), ("side0.1m", C.translation(x=0.1)), ("side0.3m", C.translation(x=0.3)),
         ("yaw0.5deg", C.yaw(0.5)), ("yaw2deg", C.yaw(2.0)), ("pitch0.3deg", C.pitch(0.3)), ("pitch1deg", C.pitch(1.0)),
         ("mixed", _compose(C.translation(x=0.08, y=-0.02, z=0.5), C.yaw(1.0), C.pitch(0.3))))
FAR = ("forward5m", C.translation(z=5.0))                    # footprints leave the image, points come too close


def texture(X, Y, Z):
    """grey level (float64) of the world point: four sines, periods 4.1, 2.9, 1.7 and 1.1 m (the nearest road pixel is about
    0.05 m wide: the shortest period is twenty of them)"""
    s = 38.0 * np.sin(2 * math.pi * (X + 0.3 * Y) / 4.1) + 30.0 * np.sin(2 * math.pi * (Z + 0.5 * Y) / 2.9 + 1.0) \
        + 26.0 * np.sin(2 * math.pi * (X - Z + Y) / 1.7 + 2.0) + 20.0 * np.sin(2 * math.pi * (X + Z + 2.0 * Y) / 1.1 + 3.0)
    return 128.0 + s


def render(scene, T_world_cam=None):
    """(disp float64 (H,W), rgb uint8 (H,W,3)) of the scene from the pose: the true disparity of _temporal_cases.render and the
    texture at the hit point of every ray, the same grey in the three channels (so the grey conversion returns it)"""
    T = np.eye(4) if T_world_cam is None else np.asarray(T_world_cam, np.float64)
    d = C.render(scene, T)
    (H, W), c = scene.hw, scene.calib
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    with np.errstate(all="ignore"):
        depth = np.where(d > 0, c.f * c.baseline / (d + c.doffs), 0.0)
    ray = np.stack([(u - c.cx) / c.f, (v - c.cy) / c.f, np.ones_like(u)], -1) * depth[..., None]
    P = ray @ T[:3, :3].T + T[:3, 3]
    grey = np.where(d > 0, texture(P[..., 0], P[..., 1], P[..., 2]), float(SKY))
    grey = np.clip(np.rint(grey), 0, 255).astype(np.uint8)
    return d, np.repeat(grey[..., None], 3, -1)


@functools.lru_cache(maxsize=None)
def _frame(scene_name, pose_name, noise, levels):
    scene = next(s for s in SCENES + SMALL if s.name == scene_name)
    T = dict(POSES + (FAR,))[pose_name]
    d, rgb_prev = render(scene)
    _, rgb_cur = render(scene, T)
    if noise:
        rng = np.random.default_rng(17)
        d = np.where(d > 0, d + rng.normal(0.0, noise, d.shape), 0.0)
    d = d.astype(np.float32)
    for a in (d, rgb_prev, rgb_cur):
        a.setflags(write=False)
    return {"disp": d, "rgb_prev": rgb_prev, "rgb_cur": rgb_cur,
            "prev": OD.grey_pyramid_host(rgb_prev, levels), "cur": OD.grey_pyramid_host(rgb_cur, levels),
            "dpyr": OD.disp_pyramid_host(d, levels), "T_true": GEO.relative_pose(np.eye(4), T)}


def frame(scene, pose_name, noise=0.0, levels=LEVELS):
    """the inputs of one estimate, computed once and shared (read-only): the previous frame's float32 disparity (with seeded
    Gaussian noise of `noise` px), both uint8 images, the three host pyramids and the true T_cur_from_prev"""
    return _frame(scene.name, pose_name, float(noise), int(levels))


def cases():
    """(id, scene, pose name, noise) for the three scenes, every pose, without and with 0.3 px of disparity noise"""
    return [(f"{s.name}/{n}/noise{z}", s, n, z) for s in SCENES for n, _ in POSES for z in (0.0, 0.3)]


def endpoint_error(scene, disp, T_est, T_true, min_disp=OD.ODOMETRY_MIN_DISP):
    """mean and maximum distance in pixels between the warps of every valid previous pixel under the two poses (float64)"""
    c = scene.calib
    H, W = disp.shape
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    ok = np.isfinite(disp) & (disp >= min_disp)
    Z = c.f * c.baseline / (disp[ok].astype(np.float64) + c.doffs)
    P = np.stack([(u[ok] - c.cx) / c.f * Z, (v[ok] - c.cy) / c.f * Z, Z, np.ones_like(Z)])
    out = []
    for T in (T_est, T_true):
        Q = np.asarray(T, np.float64)[:3] @ P
        out.append(np.stack([c.f * Q[0] / Q[2] + c.cx, c.f * Q[1] / Q[2] + c.cy]))
    front = (np.asarray(T_est)[2] @ P > 0) & (np.asarray(T_true)[2] @ P > 0)
    e = np.hypot(*(out[0] - out[1]))[front]
    return float(e.mean()), float(e.max())
