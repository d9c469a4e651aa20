"""Synthetic scenes for the ground-plane operators (dcanet_amd/ground.py, csrc/ground.hip), shared by test_ground_cpu.py and
test_gpu_ground.py: all generated from a seed, a few thousand pixels each.  A scene is a road plane in disparity space,
d = a u' + b v' + c with u' = col - cols // 2, v' = row - rows // 2, sky (no measurement, 0.0) where the plane has no positive
disparity, and objects on it: walls (constant disparity, resting on the road), pits (below the road), overhangs (above the
horizon) and posts (short obstacles in one column, for the free-space walk).

The sizes are the smallest that reach every branch: cols no multiple of 4 or 64, odd rows, more than one workgroup in every
kernel (53 x 131 with 64 bins: 14 row blocks, 32 vote blocks, 14 blocks of fit pixels, 28 of pixels, 3 of columns), a window
with y0 > 0 and cols < Wc whose surroundings hold plausible disparities, a batch of two different planes."""
import collections
import functools

import numpy as np

Case = collections.namedtuple("Case", "name d mask window max_disp calib v0 plane_kw seg_kw")
Scene = collections.namedtuple("Scene", "d p road wall a b c")


def _calib(f, baseline, cx, cy, doffs=0.0):
    from dcanet_amd.geometry import StereoCalib
    return StereoCalib(f, baseline, cx, cy, doffs)


def plane_map(rows, cols, a, b, c):
    """float64 (rows,cols): the plane's disparity"""
    u = np.arange(cols, dtype=np.float64)[None, :] - cols // 2
    v = np.arange(rows, dtype=np.float64)[:, None] - rows // 2
    return a * u + b * v + c


def scene(rows, cols, a, b, c, walls=(), pits=(), overhangs=(), posts=(), noise=0.0, seed=0):
    """d float32 (rows,cols); p float64: the true plane; road bool: true road pixels outside every object; wall bool.
    walls / pits: (r0, r1, c0, c1); a wall takes the road's disparity at its foot row r1 - 1 (middle column), a pit lies 3 px
    behind the road.  overhangs: (r0, r1, c0, c1, d).  posts: (r0, r1, c): one column wide, 3 px in front of the road at its foot row, so that
    every pixel of a post is an obstacle, the lowest included."""
    p = plane_map(rows, cols, a, b, c)
    road = p >= 0.25
    d = np.where(road, p, 0.0)
    wall = np.zeros((rows, cols), bool)
    for r0, r1, c0, c1 in walls:
        d[r0:r1, c0:c1] = p[r1 - 1, (c0 + c1) // 2]
        wall[r0:r1, c0:c1] = True
    for r0, r1, cc in posts:
        d[r0:r1, cc] = p[r1 - 1, cc] + 3.0
        wall[r0:r1, cc] = True
    for r0, r1, c0, c1 in pits:
        d[r0:r1, c0:c1] = p[r0:r1, c0:c1] - 3.0
        wall[r0:r1, c0:c1] = True
    for r0, r1, c0, c1, dd in overhangs:
        d[r0:r1, c0:c1] = dd
        wall[r0:r1, c0:c1] = True
    road &= ~wall
    if noise:
        rng = np.random.default_rng(seed)
        d = np.where(d > 0, d + rng.normal(0.0, noise, d.shape), d)
    return Scene(d.astype(np.float32), p, road, wall, a, b, c)


def plane_only_scenes():
    """(name, Scene, max_disp): noise-free planes at four shapes and rolls, the horizon above the window and inside its upper half"""
    return [("48x75 roll+ horizon above", scene(48, 75, 0.012, 1 / 3, 10.3), 32),
            ("53x131 roll- horizon inside", scene(53, 131, -0.01, 0.9, 0.9 * (26 - 12)), 64),
            ("40x70 no roll", scene(40, 70, 0.0, 0.55, 0.55 * (20 - 6.5)), 32),
            ("33x64 roll+ steep", scene(33, 64, 0.02, 1.4, 1.4 * (16 - 3.2)), 48)]


def wall_scenes():
    """(name, Scene, max_disp, calib): noise-free road, wall, sky and roll; the walls end below 2 x the camera height"""
    return [("48x75 roll+", scene(48, 75, 0.012, 1 / 3, 10.3, walls=[(14, 36, 40, 58)]), 32, _calib(60.0, 0.5, 37.0, -7.0)),
            ("53x131 roll-", scene(53, 131, -0.01, 0.9, 0.9 * (26 - 12), walls=[(20, 40, 60, 80), (30, 47, 5, 22)]), 64,
             _calib(80.0, 0.5, 65.0, 12.0))]


def _specials(d, rng, max_disp, n=4):
    """NaN, +-inf, zero, negative and >= max_disp disparities, and the largest that still has a bin, at random places"""
    vals = [np.nan, np.inf, -np.inf, 0.0, -3.0, float(max_disp), max_disp - 0.01, max_disp - 0.04, 1e30, 0.0625, 0.06]
    for v in vals:
        for _ in range(n):
            d[tuple(rng.integers(0, s) for s in d.shape)] = v
    return d


@functools.lru_cache(maxsize=None)
def _scene_a(seed=1):
    return scene(48, 75, 0.012, 1 / 3, 10.3, walls=[(14, 36, 40, 58)], posts=[(40, 42, 10), (30, 33, 10), (38, 41, 12), (44, 46, 14)],
                 noise=0.15, seed=seed)


@functools.lru_cache(maxsize=None)
def cases():
    """the cases of the GPU tests; every array is read-only"""
    out = []
    grid_a = (0.5, 3.0, 12.0)                        # 12 x 24 cells: many pixels per cell near the camera, the far road outside
    cal_a = _calib(60.0, 0.5, 37.0, -7.0)
    a = _scene_a()
    out.append(Case("road+wall 48x75 roll+", a.d, None, None, 32, cal_a, 0, {}, dict(grid=grid_a)))
    out.append(Case("same, refine 0", a.d, None, None, 32, cal_a, 0, dict(refine=0), dict(grid=grid_a)))
    out.append(Case("same, fit rows 20:45, min_run 1, tol 0.75", a.d, None, None, 32, cal_a, 0, dict(fit_rows=(20, 45), tol=0.75, refine=1),
                    dict(grid=grid_a, min_run=1, tol_d=0.5, h_ground=0.05)))

    # a 53 x 131 window at row 5 of a 64 x 140 frame; what surrounds it looks like a measurement; a mask; doffs and v0
    rng = np.random.default_rng(2)
    b = scene(53, 131, -0.01, 0.9, 0.9 * (26 - 12), walls=[(20, 40, 60, 80)], pits=[(40, 46, 90, 110)],
              overhangs=[(2, 8, 20, 50, 6.0)], posts=[(44, 46, 3), (36, 39, 3), (47, 50, 125)], noise=0.2, seed=3)
    frame = np.full((64, 140), 20.0, np.float32)
    frame[5:58, :131] = _specials(b.d.copy(), rng, 64)
    mask = np.ones((64, 140), np.float32)
    mask[5:58, :131] = rng.random((53, 131), dtype=np.float32) * 0.5 + np.float32(0.42)        # about 16 % below 0.5
    out.append(Case("window 53x131 of 64x140, mask, roll-, horizon inside", frame, mask, (5, 53, 131), 64,
                    _calib(80.0, 0.5, 65.0, 112.0, 3.5), 100, dict(refine=4),
                    dict(grid=(0.25, 2.0, 6.0), h_max=0.6, h_ground=0.03)))

    # the boundary d_top = -NB: the line from -32 at row 0 to 30 at row 39 (the candidate itself lies half a bin below)
    rr = np.arange(40, dtype=np.float64)[:, None]
    line = np.broadcast_to(-32.0 + 0.5 + 62.0 / 39.0 * rr, (40, 70))
    out.append(Case("d_top = -NB, 40x70", np.where(line >= 0.25, line, 0.0).astype(np.float32), None, None, 32,
                    _calib(60.0, 0.5, 35.0, 20.0), 0, dict(refine=1), dict(grid=(0.5, 3.0, 12.0))))

    # batch 2, another plane per frame; the second frame carries the special values
    rng = np.random.default_rng(4)
    two = np.stack([_scene_a(5).d, _specials(scene(48, 75, -0.015, 0.5, 0.5 * (24 - 9), walls=[(20, 34, 8, 30)], noise=0.1,
                                                   seed=6).d.copy(), rng, 32)])
    out.append(Case("batch 2, two planes", two, None, None, 32, cal_a, 0, dict(refine=3), dict(grid=grid_a)))
    out.append(Case("batch 2 as (B,1,H,W), window 3:45 x 70", two[:, None], None, (3, 42, 70), 32, cal_a, 3, {}, dict(grid=grid_a)))

    # status 1: a frame without a valid pixel, and a frame that is all wall: a line that rises by 4 over the 39 rows stays in
    # one bin for at most 10 of them, so no candidate collects more than 10 x 70 votes
    none = np.zeros((40, 70), np.float32)
    none[::2] = np.nan
    out.append(Case("no valid pixel | all wall (status 1)", np.stack([none, np.full((40, 70), 10.0, np.float32)]), None, None, 32,
                    _calib(60.0, 0.5, 35.0, 10.0), 0, dict(min_rise=4, min_votes=1000), dict(grid=(0.5, 3.0, 12.0))))

    # status 2: ten road pixels (fewer than min_inliers); twenty in ONE column (a singular system)
    road = plane_map(40, 70, 0.0, 0.55, 0.55 * (20 - 6.5)).astype(np.float32)
    few, column = np.zeros((40, 70), np.float32), np.zeros((40, 70), np.float32)
    few[np.arange(22, 32), np.arange(10, 60, 5)] = road[np.arange(22, 32), np.arange(10, 60, 5)]
    column[20:, 33] = road[20:, 33]
    out.append(Case("10 road pixels | one column (status 2)", np.stack([few, column]), None, None, 32,
                    _calib(60.0, 0.5, 35.0, 10.0), 0, dict(min_votes=4), dict(grid=(0.5, 3.0, 12.0))))

    # an exact tie: two rows of one bin each, every candidate through both bins has the same vote
    tie = np.zeros((40, 70), np.float32)
    tie[25], tie[35] = 5.2, 9.7
    out.append(Case("two rows: an exact tie", tie, None, None, 32, _calib(60.0, 0.5, 35.0, 10.0), 0, dict(min_votes=4),
                    dict(grid=(0.5, 3.0, 12.0))))
    for c in out:
        c.d.setflags(write=False)
        if c.mask is not None:
            c.mask.setflags(write=False)
    return out


def plane_kwargs(case):
    return dict(max_disp=case.max_disp, calib=case.calib, mask=case.mask, window=case.window, v0=case.v0, **case.plane_kw)


def segment_kwargs(case):
    return dict(max_disp=case.max_disp, mask=case.mask, window=case.window, **case.seg_kw)
