"""Seeded synthetic scenes for the temporal-stereo tests (CPU and GPU): a road 1.65 m below the camera, a box standing on it
and a backdrop, rendered ANALYTICALLY (ray casting, float64) from any camera pose, so that the state warped from one pose to
another can be compared with the scene re-rendered at the new pose.  A few thousand pixels each; the poses are those of a car:
identity, 1 m forward, 1 m back (minification: many sources per target), 0.3 m sideways, 2 degrees of yaw, 1 degree of pitch."""
import collections
import math

import numpy as np

from dcanet_amd.geometry import StereoCalib

BASELINE = 0.54
CAM_HEIGHT = 1.65
MAX_DISP = 64.0

Scene = collections.namedtuple("Scene", "name hw calib box backdrop")
# box = (x0, x1, y0, z0, z1): it stands on the road (its base is y = CAM_HEIGHT; y points down), backdrop: the plane Z = backdrop
SCENES = (Scene("48x75", (48, 75), StereoCalib(44.0, BASELINE, 36.5, 17.25), (-1.6, -0.4, 0.3, 6.0, 7.5), 18.0),
          Scene("53x131", (53, 131), StereoCalib(75.0, BASELINE, 66.0, 20.5), (0.5, 2.0, 0.4, 7.0, 9.0), 25.0),
          Scene("40x160", (40, 160), StereoCalib(90.0, BASELINE, 79.5, 13.5), (-0.5, 1.0, 0.45, 8.0, 9.5), 20.0))


def translation(x=0.0, y=0.0, z=0.0):
    T = np.eye(4)
    T[:3, 3] = x, y, z
    return T


def yaw(deg):
    a = math.radians(deg)
    T = np.eye(4)
    T[0, 0], T[0, 2], T[2, 0], T[2, 2] = math.cos(a), math.sin(a), -math.sin(a), math.cos(a)
    return T


def pitch(deg):
    a = math.radians(deg)
    T = np.eye(4)
    T[1, 1], T[1, 2], T[2, 1], T[2, 2] = math.cos(a), -math.sin(a), math.sin(a), math.cos(a)
    return T


# the camera's pose in the world after the move (camera coordinates -> world coordinates); before it, the identity
POSES = (("identity", np.eye(4)), ("forward1m", translation(z=1.0)), ("back1m", translation(z=-1.0)),
         ("side0.3m", translation(x=0.3)), ("yaw2deg", yaw(2.0)), ("pitch1deg", pitch(1.0)))


def render(scene, T_world_cam=None):
    """the true disparity float64 (H,W) of the scene seen from the pose T_world_cam (default the identity), 0 where a ray hits
    nothing in front of the camera"""
    T = np.eye(4) if T_world_cam is None else np.asarray(T_world_cam, np.float64)
    (H, W), c = scene.hw, scene.calib
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    ray = np.stack([(u - c.cx) / c.f, (v - c.cy) / c.f, np.ones_like(u)], -1)          # camera frame, Z = 1: t is the depth
    dirs = ray @ T[:3, :3].T
    org = T[:3, 3]
    best = np.full((H, W), np.inf)
    with np.errstate(all="ignore"):
        t = (CAM_HEIGHT - org[1]) / dirs[..., 1]                                       # the road y = CAM_HEIGHT
        best = np.where((t > 0) & (t < best), t, best)
        t = (scene.backdrop - org[2]) / dirs[..., 2]                                   # the backdrop
        hit = org[1] + t * dirs[..., 1]
        best = np.where((t > 0) & (t < best) & (hit <= CAM_HEIGHT), t, best)
        x0, x1, y0, z0, z1 = scene.box                                                 # the box: slabs
        lo, hi = np.array([x0, y0, z0]), np.array([x1, CAM_HEIGHT, z1])
        ta, tb = (lo - org) / dirs, (hi - org) / dirs
        tn, tf = np.minimum(ta, tb).max(-1), np.maximum(ta, tb).min(-1)
        best = np.where((tn <= tf) & (tn > 0) & (tn < best), tn, best)
        d = c.f * c.baseline / best - c.doffs
    return np.where(np.isfinite(best) & (d > 0), d, 0.0)


def state(scene, rng=None, noise=0.0, var=0.25, age=1, T_world_cam=None):
    """a state {"disp","var","age"} of the scene at a pose: the true disparity (plus seeded Gaussian noise), a constant variance
    and age where there is a surface"""
    d = render(scene, T_world_cam)
    if rng is not None and noise:
        d = np.where(d > 0, d + rng.normal(0.0, noise, d.shape), 0.0)
    d = d.astype(np.float32)
    return {"disp": d, "var": np.where(d > 0, np.float32(var), np.float32(0)).astype(np.float32),
            "age": np.where(d > 0, age, 0).astype(np.uint8)}


def cases():
    """(id, scene, pose name, T_world_cur) for every scene and pose"""
    return [(f"{s.name}/{n}", s, n, T) for s in SCENES for n, T in POSES]
