"""Sparse ground truth from a LiDAR scan, host side: `geometry.lidar_disparity_host`, the numpy
restatement the GPU tests compare `ops.lidar_disparity` with bit for bit, against an independent per-point loop, against
float64, through a back-projection round trip; and `geometry.LidarCalib`."""
import numpy as np
import pytest

from _lidar_reference import (CAM_TO_CAM, KITTI_HW, VELO_TO_CAM, WIDE, back_project, calib_for, kitti_matrix64,
                              lidar_float64, lidar_loop, numbers, random_points, same_bits, scan_points)

ALL = ("disp", "depth", "disp_u16", "count")
REL = 16 * 2.0 ** -24        # the chain point -> x, z -> u; z -> d has about 8 roundings of 2^-24 each; twice that


@pytest.mark.parametrize("occl", [(0, 0, 0.0), (2, 3, 0.05)])
def test_restatement_equals_independent_loop(occl):
    from dcanet_amd.geometry import lidar_disparity_host
    calib = calib_for((37, 123))
    pts = random_points(calib, 5000, seed=11, surface=occl[0] > 0)
    filters = dict(min_depth=2.2, max_depth=58.0, min_disp=0.25, max_disp=20.0)
    got = lidar_disparity_host(pts, calib, occl=occl, outputs=ALL, **filters)
    want = lidar_loop(pts, calib, len(pts), occl, **filters)
    print("count", got["count"], "of", 37 * 123, "pixels")
    # about as many kept points as pixels: collisions; dropped points; pixels hidden or outside the disparity range
    assert 1000 < want["count"][0] < 0.8 * want["count"][1] and 3800 < want["count"][1] < 5000
    for key in ALL:
        same_bits(got[key], want[key], f"{key} occl={occl}")
    part = lidar_disparity_host(pts, calib, n=1234, occl=occl, outputs=("count", "disp"), **filters)
    want = lidar_loop(pts, calib, 1234, occl, **filters)
    assert list(part) == ["count", "disp"]
    same_bits(part["disp"], want["disp"], "n < N")
    same_bits(part["count"], want["count"], "n < N count")


def test_calibration_from_kitti_raw(tmp_path):
    from dcanet_amd.geometry import LidarCalib, RectifyMaps, StereoCalib, read_velodyne
    calib = LidarCalib.from_kitti_raw(CAM_TO_CAM, VELO_TO_CAM)
    M64 = kitti_matrix64()
    assert calib.M.dtype == np.float32 and calib.M.shape == (3, 4)
    assert np.array_equal(calib.M, M64.astype(np.float32))          # the float64 product, rounded once
    assert calib.hw == KITTI_HW == RectifyMaps.from_kitti_raw(CAM_TO_CAM).dst_hw
    Pl, Pr = numbers(CAM_TO_CAM, "P_rect_02").reshape(3, 4), numbers(CAM_TO_CAM, "P_rect_03").reshape(3, 4)
    want = StereoCalib.from_kitti(CAM_TO_CAM, "P2", "P3")
    assert calib.stereo == want and calib.stereo.doffs == 0.0 and calib.stereo.f == Pl[0, 0]
    assert calib.stereo.fb == float(np.float32(Pl[0, 3] - Pr[0, 3]))    # f (tx_l / f - tx_r / f), about 384.4
    assert abs(calib.stereo.baseline - 0.5327) < 1e-3
    # the right camera as the reference view; paths instead of texts
    cam, velo = tmp_path / "calib_cam_to_cam.txt", tmp_path / "calib_velo_to_cam.txt"
    cam.write_text(CAM_TO_CAM)
    velo.write_text(VELO_TO_CAM)
    again = LidarCalib.from_kitti_raw(str(cam), velo)
    assert np.array_equal(again.M, calib.M) and again.hw == calib.hw and again.stereo == calib.stereo
    # every key is needed, with its number count
    for text, keys in ((CAM_TO_CAM, ("P_rect_02", "P_rect_03", "R_rect_00", "S_rect_02")), (VELO_TO_CAM, ("R", "T"))):
        for key in keys:
            lines = text.splitlines()
            gone = "\n".join(l for l in lines if not l.startswith(key + ":"))
            short = "\n".join(l.rsplit(" ", 1)[0] if l.startswith(key + ":") else l for l in lines)
            for bad, match in ((gone, f"no {key} "), (short, f"{key} has ")):
                args = (bad, VELO_TO_CAM) if text is CAM_TO_CAM else (CAM_TO_CAM, bad)
                with pytest.raises(ValueError, match=match):
                    LidarCalib.from_kitti_raw(*args)
    # from_matrix: rounded once, checked
    m = LidarCalib.from_matrix(M64, calib.stereo, (10, 20))
    assert np.array_equal(m.M, calib.M) and m.hw == (10, 20)
    for bad in (np.eye(3), np.full((3, 4), np.nan), np.full((3, 4), 1e300)):
        with pytest.raises(ValueError):
            LidarCalib.from_matrix(bad, calib.stereo, (10, 20))
    with pytest.raises(ValueError):
        LidarCalib.from_matrix(M64, calib.stereo, (0, 20))
    # a scan file comes back as it is
    scan = np.random.default_rng(0).random((17, 4)).astype(np.float32)
    scan.tofile(tmp_path / "0000000000.bin")
    back = read_velodyne(tmp_path / "0000000000.bin")
    assert back.dtype == np.float32 and np.array_equal(back, scan)


@pytest.mark.parametrize("hw", [(24, 40), (37, 123), KITTI_HW])
def test_round_trip_through_back_projection(hw):
    from dcanet_amd.geometry import lidar_disparity_host
    calib = calib_for(hw)
    H, W = hw
    rng = np.random.default_rng(5)
    fb = calib.stereo.fb
    disp = rng.uniform(fb / 70.0, fb / 3.0, (H, W))                  # depths of 3 to 70 metres
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    z = fb / (disp + calib.stereo.doffs)
    pts = np.zeros((H * W, 4), np.float32)
    pts[:, :3] = back_project(calib, u.reshape(-1), v.reshape(-1), z.reshape(-1)).astype(np.float32)
    got = lidar_disparity_host(pts, calib, occl=(0, 0, 0.0), outputs=("disp", "count"), **WIDE)
    assert got["count"].tolist() == [H * W, H * W]                   # pixel centres are half a pixel from every boundary
    err = np.abs(got["disp"].astype(np.float64) - disp) / disp
    print(f"{H}x{W}: max relative error {err.max():.3e} (bound {REL:.3e})")
    assert (got["disp"] > 0).all() and err.max() <= REL
    perm = rng.permutation(H * W)
    same_bits(lidar_disparity_host(pts[perm], calib, occl=(0, 0, 0.0), **WIDE)["disp"], got["disp"], "permuted")


def test_against_float64_on_a_scan():
    from dcanet_amd.geometry import lidar_disparity_host
    calib = calib_for(KITTI_HW)
    pts = scan_points(calib, seed=3)
    assert len(pts) == 120000
    args = dict(occl=(2, 4, 0.1), min_depth=1.0, max_depth=100.0, min_disp=0.0, max_disp=192.0)
    got = lidar_disparity_host(pts, calib, **args)["disp"].astype(np.float64)
    want = lidar_float64(pts, calib, **args)
    a, b = got > 0, want > 0
    both = a & b
    err = np.abs(got[both] - want[both]) / want[both]
    print(f"valid {a.sum()} / {b.sum()}, masks differ at {(a != b).sum()}, max relative error {err.max():.3e}")
    assert b.sum() > 5000
    assert (a != b).sum() <= b.sum() / 1000
    # a point near a .5 boundary may sit in another pixel in float64: at most 1 valid pixel in 1000 differs
    assert err.max() <= REL


def test_host_refusals():
    from dcanet_amd.geometry import lidar_disparity_host
    calib = calib_for((24, 40))
    pts = random_points(calib, 16, seed=1)
    ok = dict(occl=(1, 1, 0.1), min_depth=1.0, max_depth=50.0, min_disp=0.0, max_disp=64.0)
    assert lidar_disparity_host(pts, calib, **ok)["disp"].shape == (24, 40)
    for bad in (dict(n=17), dict(n=-1), dict(occl=(9, 0, 0.1)), dict(occl=(0, -1, 0.1)), dict(occl=(0, 0, -0.1)),
                dict(occl=(0, 0, float("nan"))), dict(occl=(0, 0, float("inf"))), dict(min_depth=0.0), dict(min_depth=1e-50),
                dict(max_depth=float("inf")), dict(max_depth=0.5), dict(min_disp=float("nan")), dict(max_disp=float("inf")),
                dict(max_disp=-1.0), dict(outputs=()), dict(outputs=("disp", "flow"))):
        with pytest.raises(ValueError):
            lidar_disparity_host(pts, calib, **{**ok, **bad})
    with pytest.raises(ValueError):
        lidar_disparity_host(pts[:, :2], calib, **ok)
    with pytest.raises(ValueError):
        lidar_disparity_host(pts.astype(np.float64), calib, **ok)
