"""Sparse ground truth from a LiDAR scan on the MI355X (csrc/lidar.hip): `ops.lidar_disparity` and `geometry.LidarProjector`
bit for bit against `geometry.lidar_disparity_host`, the numpy restatement that tests/test_lidar_cpu.py checks against an
independent loop.

Why bitwise: the projection is IEEE fp32, one operation at a time, in numpy and in the kernel alike; the z-buffer is an
integer minimum, which no order of arrival changes; the window minimum and the counts are integer work."""
import numpy as np
import pytest
import torch

from _lidar_reference import (KITTI_HW, back_project, calib_for, identity_calib, lidar_loop, random_points, same_bits,
                              scan_points)

pytestmark = pytest.mark.gpu
DEV = "cuda"
ALL = ("disp", "depth", "disp_u16", "count")
F = np.float32
FILTERS = dict(min_depth=2.2, max_depth=58.0, min_disp=0.25, max_disp=20.0)
OPEN = dict(min_depth=2.0 ** -8, max_depth=2.0 ** 14, min_disp=0.0, max_disp=1.0e4)


def device_maps(pts, calib, **kw):
    from dcanet_amd import ops
    res = ops.lidar_disparity(torch.from_numpy(np.ascontiguousarray(pts)).to(DEV), calib, outputs=ALL, **kw)
    assert list(res) == list(ALL)
    return {k: v.cpu().numpy() for k, v in res.items()}


def check(pts, calib, name, **kw):
    """device == restatement, every output; returns the maps"""
    from dcanet_amd.geometry import lidar_disparity_host
    got, want = device_maps(pts, calib, **kw), lidar_disparity_host(pts, calib, outputs=ALL, **kw)
    for key in ALL:
        same_bits(got[key], want[key], f"{name}: {key}")
    return got


def at(u, v, z):
    """the point that M = [I|0] sends to (u, v) at depth z; exact for a power of two z"""
    return [F(u) * F(z), F(v) * F(z), F(z), 0.5]


def rows(points):
    return np.array(points, np.float32).reshape(-1, 4)


@pytest.mark.parametrize("occl", [(0, 0, 0.0), (2, 3, 0.05)])
def test_random_points(occl):
    calib = calib_for((37, 123))                        # the width is no multiple of 4 or of the tile
    pts = random_points(calib, 5000, seed=11, surface=occl[0] > 0)
    assert (pts[:, 0] < 0).sum() > 100                  # behind the sensor
    got = check(pts, calib, f"occl={occl}", occl=occl, **FILTERS)
    assert 1000 < got["count"][0] < got["count"][1] < 5000


@pytest.mark.parametrize("hw", [KITTI_HW, (530, 1242)])
def test_whole_scan(hw):
    """a whole synthetic scan at KITTI size (1833 tiles of the resolve launch) and into 530 x 1242: 2613 tiles, more than the
    2048 workgroups the launch has on 256 CUs, so workgroups walk more than one tile"""
    calib = calib_for(hw)
    pts = scan_points(calib, seed=3)
    kw = dict(occl=(2, 4, 0.1), min_depth=1.0, max_depth=100.0, min_disp=0.0, max_disp=192.0)
    got = check(pts, calib, "scan", **kw)
    assert len(pts) == 120000 and 10000 < got["count"][0] < got["count"][1] < 25000
    same_bits(check(pts[::-1], calib, "scan reversed", **kw)["disp"], got["disp"], "scan: both orders")


def test_collisions_in_any_order():
    calib = identity_calib((3, 5))
    rng = np.random.default_rng(2)
    z = 2.0 ** rng.integers(1, 4, 4096) * rng.integers(4, 8, 4096) / 4.0        # 12 depths for 4096 points in 15 pixels
    pts = rows([at(u, v, d) for u, v, d in zip(rng.uniform(-0.5, 4.5, 4096), rng.uniform(-0.5, 2.5, 4096), z)])
    kw = dict(occl=(1, 1, 0.5), **OPEN)
    a = check(pts, calib, "as given", **kw)
    b = check(pts[rng.permutation(4096)], calib, "permuted", **kw)
    assert a["count"][1] > 3500 and 0 < a["count"][0] <= 15
    for key in ALL:
        same_bits(a[key], b[key], f"both orders: {key}")


def test_sizes_strides_and_rows_beyond_n():
    from dcanet_amd import ops
    calib = calib_for((37, 123))
    pts = random_points(calib, 600, seed=4)
    kw = dict(occl=(1, 2, 0.3), **FILTERS)
    none = device_maps(pts, calib, n=0, **kw)
    assert not none["disp"].any() and not none["depth"].any() and not none["disp_u16"].any()
    assert none["count"].tolist() == [0, 0]
    empty = ops.lidar_disparity(torch.empty((0, 4), device=DEV), calib, outputs=ALL, **kw)
    assert not empty["disp"].any() and empty["count"].tolist() == [0, 0]
    pts[0, :3] = back_project(calib, np.array([60.0]), np.array([18.0]), np.array([10.0]))[0]     # a point that is kept
    for n in (1, 257):
        poisoned = pts.copy()
        poisoned[n:] = np.where(np.arange(600 - n)[:, None] % 2 == 0, F("nan"), F(1e30))
        got = check(poisoned, calib, f"n={n}", n=n, **kw)
        same_bits(got["disp"], device_maps(pts[:n], calib, **kw)["disp"], f"n={n} against the first rows alone")
        assert 0 < got["count"][0] <= got["count"][1] <= n
    full = check(pts, calib, "S=4", **kw)
    wide = np.concatenate([pts, np.full((600, 1), 7.0, np.float32)], axis=1)
    nan_col = pts.copy()
    nan_col[:, 3] = np.nan                              # the reflectance is never read
    for other, name in ((pts[:, :3], "S=3"), (wide, "S=5"), (nan_col, "NaN reflectance")):
        got = check(other, calib, name, **kw)
        for key in ALL:
            same_bits(got[key], full[key], f"{name}: {key}")


def test_boundaries():
    H, W = 4, 6
    calib = identity_calib((H, W))                      # fb = 8: d = 8 / z
    below = float(np.nextafter(F(-0.5), F(-1)))
    kw = dict(occl=(0, 0, 0.0), min_depth=1.0, max_depth=64.0, min_disp=0.0, max_disp=1.0e4)
    pts = rows([at(-0.5, 1, 2),                         # u = -0.5 rounds to column 0
                at(below, 2, 2),                        # the next float below is column -1
                at(W - 0.5, 1, 2), at(W - 1.5 + 0.25, 2, 2),     # column W is outside; W - 1.25 rounds to W - 1
                at(2, -0.5, 4), at(3, below, 4), at(4, H - 0.5, 4)])
    got = check(pts, calib, "edges", **kw)
    want = np.zeros((H, W), np.float32)
    want[1, 0] = want[2, W - 1] = 2
    want[0, 2] = 4
    same_bits(got["depth"], want, "edges: depth")
    assert got["count"].tolist() == [3, 3]

    up = lambda v: float(np.nextafter(F(v), F(np.inf)))
    down = lambda v: float(np.nextafter(F(v), F(0)))
    pts = rows([at(0, 0, 1.0), at(1, 0, down(1.0)), at(2, 0, 64.0), at(4, 0, up(64.0))])
    got = check(pts, calib, "depth range", **kw)
    want = np.zeros((H, W), np.float32)
    want[0, 0], want[0, 2] = 1, 64
    same_bits(got["depth"], want, "depth range: depth")

    bad = [F("nan"), F("inf"), F("-inf"), F(1e30), F(-1e30)]
    pts = rows([[b if k == 0 else 2, b if k == 1 else 2, b if k == 2 else 2, 0] for b in bad for k in range(3)]
               + [[b, b, b, b] for b in bad])
    got = check(pts, calib, "not finite", **kw)
    assert got["count"].tolist() == [0, 0] and not got["depth"].any()

    pts = rows([at(0, 0, 4.0), at(1, 0, 1.0), at(2, 0, 2.0)])        # d = 2, 8, 4
    got = check(pts, calib, "disparity range", occl=(0, 0, 0.0), min_depth=1.0, max_depth=64.0, min_disp=2.0, max_disp=8.0)
    want = np.zeros((H, W), np.float32)
    want[0, 0], want[0, 2] = 2, 4                       # d == min_disp is kept, d == max_disp is not
    same_bits(got["disp"], want, "disparity range: disp")
    assert got["count"].tolist() == [2, 3]

    pts = rows([at(0, 0, 2.0 ** -6), at(1, 0, 2.0 ** -5), at(2, 0, 8192.0), at(3, 0, 3.0), at(4, 0, 2.0 ** 13 / 1.5)])
    got = check(pts, calib, "uint16", occl=(0, 0, 0.0), **OPEN)
    # d = 512 and 256 saturate; 2^-10 * 256 + 0.5 = 0.75 is lifted to 1; 8 / 3 * 256 + 0.5 = 683.17; 1.5 * 2^-10: 0.875 -> 1
    assert got["disp_u16"][0, :5].tolist() == [65535, 65535, 1, 683, 1] and got["disp_u16"].sum() == 2 * 65535 + 685


def test_hidden_points():
    H, W = 12, 20
    calib = identity_calib((H, W))
    kw = dict(occl=(2, 1, 0.25), **OPEN)                # occl_scale = 1.25 exactly
    over = float(np.nextafter(F(5), F(np.inf)))
    scene = {(4, 5): 4.0,                               # a near point
             (4, 7): 8.0, (5, 7): 8.0, (3, 3): 8.0,     # inside its window of 5 columns x 3 rows: hidden
             (4, 8): 8.0, (6, 5): 8.0, (2, 4): 8.0,     # one column / one row outside: stay
             (9, 12): 4.0, (9, 13): 5.0, (9, 11): over,  # z == zmin * occl_scale stays, the next float goes
             (0, 0): 4.0, (0, 1): 8.0,                  # windows clipped at the four borders
             (H - 1, W - 1): 4.0, (H - 2, W - 1): 8.0,
             (1, W - 2): 4.0, (0, W - 1): 8.0,
             (H - 1, 2): 4.0, (H - 1, 0): 8.0}
    pts = rows([at(c, r, z) for (r, c), z in scene.items()])
    got = check(pts, calib, "hidden", **kw)
    gone = {(4, 7), (5, 7), (3, 3), (9, 11), (0, 1), (H - 2, W - 1), (0, W - 1), (H - 1, 0)}
    want = np.zeros((H, W), np.float32)
    for (r, c), z in scene.items():
        if (r, c) not in gone:
            want[r, c] = z
    same_bits(got["depth"], want, "hidden: depth")
    assert got["count"].tolist() == [len(scene) - len(gone), len(scene)]
    # radius 0 switches the test off, whatever rel
    off = check(pts, calib, "radius 0", occl=(0, 0, 0.25), **OPEN)
    assert off["count"].tolist() == [len(scene), len(scene)]
    calib = calib_for((37, 123))
    cloud = random_points(calib, 5000, seed=11, surface=True)
    a = check(cloud, calib, "radius 0, rel 0.25", occl=(0, 0, 0.25), **FILTERS)
    b = check(cloud, calib, "radius 0, rel 0", occl=(0, 0, 0.0), **FILTERS)
    for key in ALL:
        same_bits(a[key], b[key], f"radius 0: {key}")
    # the largest radius on an image smaller than the window, against the brute-force loop as well
    calib = calib_for((5, 7))
    cloud = random_points(calib, 40, seed=8)
    for occl in ((8, 8, 0.5), (8, 0, 0.5), (0, 8, 0.5)):
        got = check(cloud, calib, f"occl={occl}", occl=occl, **FILTERS)
        want = lidar_loop(cloud, calib, len(cloud), occl, **FILTERS)
        for key in ALL:
            same_bits(got[key], want[key], f"occl={occl} against the loop: {key}")
        assert 0 < got["count"][0] < got["count"][1]


def test_projector_streams_scans():
    from dcanet_amd.geometry import LidarProjector
    calib = calib_for((37, 123))
    kw = dict(occl=(2, 3, 0.05), **FILTERS)
    cloud = random_points(calib, 5000, seed=11, surface=True)
    scans = [cloud[:3000], cloud, cloud[4300:], cloud[:0]]          # a short scan after a long one, an empty one
    want = [device_maps(s, calib, **kw) for s in scans]
    for depth in (2, 1, 3):
        proj = LidarProjector(calib, DEV, capacity=5000, depth=depth, outputs=ALL, **kw)
        got = [{k: v.cpu().numpy() for k, v in maps.items()} for maps in proj.stream(scans)]
        assert len(got) == len(scans)
        for i, (g, w) in enumerate(zip(got, want)):
            for key in ALL:
                same_bits(g[key], w[key], f"depth {depth}, scan {i}: {key}")
        again = proj(scans[2])                                         # one at a time, after the ring went round
        same_bits(again["disp"].cpu().numpy(), want[2]["disp"], f"depth {depth}: call")
        assert (want[1]["disp"] > 0).sum() > (want[2]["disp"] > 0).sum() > 0
    with pytest.raises(ValueError, match="capacity"):
        proj(np.zeros((5001, 4), np.float32))
    with pytest.raises(ValueError):
        proj(cloud[:, :3])
    assert list(proj.stream([])) == []


def test_refusals_launch_nothing():
    from dcanet_amd import _lib, ops
    from dcanet_amd.geometry import LidarCalib, StereoCalib
    calib = calib_for((24, 40))
    H, W = calib.hw
    pts = torch.from_numpy(random_points(calib, 64, seed=1)).to(DEV)
    ok = dict(occl=(1, 1, 0.1), min_depth=1.0, max_depth=50.0, min_disp=0.0, max_disp=64.0)
    sentinel = 12345.0
    out = {"disp": torch.full((H, W), sentinel, device=DEV), "count": torch.full((2,), 77, device=DEV, dtype=torch.int64)}
    zbuf = torch.full((H * W,), 99, device=DEV, dtype=torch.int32)
    nan, inf = float("nan"), float("inf")
    huge = LidarCalib.from_matrix(calib.M, StereoCalib(1e30, 1e30, 0.0, 0.0), calib.hw)      # fb is +inf in float32
    cases = [dict(n=65), dict(n=-1), dict(occl=(9, 0, 0.1)), dict(occl=(0, 9, 0.1)), dict(occl=(-1, 0, 0.1)),
             dict(occl=(0, 0, -0.1)), dict(occl=(0, 0, nan)), dict(occl=(0, 0, inf)), dict(min_depth=0.0),
             dict(min_depth=-1.0), dict(max_depth=inf), dict(max_depth=nan), dict(max_depth=0.5), dict(min_disp=nan),
             dict(min_disp=-inf), dict(max_disp=inf), dict(max_disp=nan), dict(max_disp=-1.0), dict(calib=huge),
             dict(outputs=()), dict(outputs=("disp", "disp")), dict(points=pts[:, :2].contiguous()), dict(points=pts.cpu()),
             dict(points=pts.double()), dict(workspace=zbuf[:H * W - 1]), dict(out={"disp": out["disp"][:, :W - 1]})]
    for bad in cases:
        args = dict(points=pts, calib=calib, outputs=("disp", "count"), out=out, workspace=zbuf, **ok)
        args.update(bad)
        with pytest.raises(RuntimeError):
            ops.lidar_disparity(**args)
    with pytest.raises(RuntimeError, match="inference only"):
        ops.lidar_disparity(pts.clone().requires_grad_(), calib, **ok)

    # the launcher itself: hipErrorInvalidValue before anything is launched
    lib = _lib.load()
    names = ["points", "N", "S", "n"] + [f"m{r}{c}" for r in range(3) for c in range(4)] + [
        "H", "W", "fb", "doffs", "min_depth", "max_depth", "min_disp", "max_disp", "rx", "ry", "rel", "disp", "depth", "disp_u16",
        "count", "zbuf", "stream"]
    good = dict(points=pts.data_ptr(), N=64, S=4, n=64, H=H, W=W, fb=calib.stereo.fb, doffs=0.0, min_depth=1.0, max_depth=50.0,
                min_disp=0.0, max_disp=64.0, rx=1, ry=1, rel=0.1, disp=out["disp"].data_ptr(), depth=None, disp_u16=None,
                count=out["count"].data_ptr(), zbuf=zbuf.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    good.update({f"m{r}{c}": float(calib.M[r, c]) for r in range(3) for c in range(4)})
    raw = [dict(n=65), dict(n=-1), dict(S=2), dict(N=1 << 29, n=1 << 29), dict(N=1 << 40, n=1 << 31, S=3), dict(H=46341, W=46341),
           dict(H=0), dict(W=-1), dict(rx=-1), dict(rx=9), dict(ry=-1), dict(ry=9), dict(rel=-1e-9), dict(rel=nan),
           dict(rel=inf), dict(min_depth=0.0), dict(min_depth=nan), dict(max_depth=inf), dict(max_depth=nan),
           dict(max_depth=0.5), dict(min_disp=nan), dict(min_disp=inf), dict(max_disp=inf), dict(max_disp=nan),
           dict(max_disp=-1.0), dict(fb=0.0), dict(fb=-1.0), dict(fb=inf), dict(fb=nan), dict(doffs=nan), dict(m12=nan),
           dict(m20=inf), dict(points=None), dict(zbuf=None), dict(disp=None, count=None)]
    for bad in raw:
        rc = lib.dca_lidar_disparity(*[{**good, **bad}[k] for k in names])
        assert rc == 1, (bad, rc)                       # hipErrorInvalidValue
    torch.cuda.synchronize()
    assert (out["disp"] == sentinel).all() and (out["count"] == 77).all() and (zbuf == 99).all()
    assert lib.dca_lidar_disparity(*[good[k] for k in names]) == 0
    torch.cuda.synchronize()
    assert not (out["disp"] == sentinel).any() and out["count"][1] > 0
