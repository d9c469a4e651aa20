"""Rectification maps and the host remap (dcanet_amd.geometry.RectifyMaps, rectify_pair_host) without a
GPU: the calibration parser, the identity, the camera model against a derivation that does not use the map formula, Bouguet's
construction by its properties, and the integer remap against tests/_rectify_reference.py bit for bit."""
import ctypes

import numpy as np
import pytest

import _rectify_reference as REF

# |a - b| of two fp64 evaluations of the same pixel coordinate (magnitude <= ~2e3 px) through chains of ~50 operations:
# measured below on the CPU (printed by the tests), gated at 100 x the measurement
MODEL_MEASURED = 4.6e-13          # px, test_model_against_forward_projection
STEREO_MEASURED = 4.6e-13         # px, test_from_stereo_properties (rows, disparity and raw pixel)


def _G():
    from dcanet_amd import geometry
    return geometry


def _distort_project(K, D, X):
    """raw pixel of points X (n,3) given in the RAW camera's frame: pinhole division, Brown distortion, K"""
    k1, k2, p1, p2, k3 = D
    x, y = X[:, 0] / X[:, 2], X[:, 1] / X[:, 2]
    r2 = x * x + y * y
    rad = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))
    xd = x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * rad + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    return K[0, 0] * xd + K[0, 1] * yd + K[0, 2], K[1, 1] * yd + K[1, 2]


# ---- parsing -------------------------------------------------------------------------------------------------------------------
def test_from_kitti_raw_parses_and_refuses():
    G = _G()
    text = REF.kitti_raw_text()
    maps = G.RectifyMaps.from_kitti_raw(text)
    K, D, R, P, src, dst = REF.kitti_raw_matrices()
    assert maps.src_hw == src == (512, 1392) and maps.dst_hw == dst == (375, 1242)
    assert maps.X.shape == maps.Y.shape == maps.valid.shape == (2, 375, 1242)
    assert maps.X.dtype == maps.Y.dtype == np.int32 and maps.valid.dtype == np.uint8
    for i in range(2):
        assert np.array_equal(maps.K[i], K[i]) and np.array_equal(maps.D[i], D[i])
        assert np.array_equal(maps.R[i], R[i]) and np.array_equal(maps.P[i], P[i])
    assert maps.calib == G.StereoCalib.from_kitti(text)
    assert abs(maps.calib.baseline - (44.9 + 339.6) / 721.5) < 1e-12 and maps.calib.f == 721.5
    assert 0.9 < maps.valid.mean() <= 1.0
    # the other pair of roles: camera 03 as view 0 has no camera to its right
    assert G.RectifyMaps.from_kitti_raw(text, left="03", right="02").calib is None
    lines = text.splitlines()
    for key in ("K_02", "D_03", "R_rect_02", "P_rect_03", "S_02", "S_rect_03"):
        without = "\n".join(ln for ln in lines if not ln.startswith(key + ":"))
        with pytest.raises(ValueError, match=key):
            G.RectifyMaps.from_kitti_raw(without)
        short = "\n".join(ln.rsplit(" ", 1)[0] if ln.startswith(key + ":") else ln for ln in lines)
        with pytest.raises(ValueError, match=f"{key} has"):
            G.RectifyMaps.from_kitti_raw(short)
        for bad in ("nan", "inf", "abc"):
            broken = "\n".join(ln.rsplit(" ", 1)[0] + " " + bad if ln.startswith(key + ":") else ln for ln in lines)
            with pytest.raises(ValueError, match=key):
                G.RectifyMaps.from_kitti_raw(broken)
    with pytest.raises(ValueError, match="16384"):
        G.RectifyMaps.from_fixed(np.zeros((2, 2, 2), np.int32), np.zeros((2, 2, 2), np.int32), (16385, 8))
    with pytest.raises(ValueError):
        G.RectifyMaps.from_fixed(np.zeros((2, 2, 2), np.int64), np.zeros((2, 2, 2), np.int64), (8, 8))


def test_from_kitti_raw_reads_a_file(tmp_path):
    G = _G()
    path = tmp_path / "calib_cam_to_cam.txt"
    path.write_text(REF.kitti_raw_text())
    a, b = G.RectifyMaps.from_kitti_raw(str(path)), G.RectifyMaps.from_kitti_raw(REF.kitti_raw_text())
    assert np.array_equal(a.X, b.X) and np.array_equal(a.Y, b.Y) and a.calib == b.calib


# ---- identity ------------------------------------------------------------------------------------------------------------------
def test_identity_and_integer_shift():
    G = _G()
    H, W = 40, 30
    K, D, R, P = REF.identity_matrices((H, W))
    maps = G.RectifyMaps.from_matrices(K, D, R, P, (H, W), (H, W))
    assert np.array_equal(maps.X, np.broadcast_to(32 * np.arange(W, dtype=np.int32), (2, H, W)))
    assert np.array_equal(maps.Y, np.broadcast_to(32 * np.arange(H, dtype=np.int32)[:, None], (2, H, W)))
    assert maps.valid.all()
    rs = np.random.RandomState(0)
    for C in (3, 4):
        left, right = rs.randint(0, 256, (H, W, C)).astype(np.uint8), rs.randint(0, 256, (H, W, C)).astype(np.uint8)
        if C == 4:
            left[..., 3] = right[..., 3] = 255
        gl, gr = G.rectify_pair_host(left, right, maps)
        assert gl.tobytes() == left.tobytes() and gr.tobytes() == right.tobytes()
    # the new principal point 4 columns to the right, 3 rows up: destination (u, v) reads source (u - 4, v + 3)
    Ps = [p.copy() for p in P]
    for p in Ps:
        p[0, 2] += 4
        p[1, 2] -= 3
    shifted = G.RectifyMaps.from_matrices(K, D, R, Ps, (H, W), (H, W))
    left, right = rs.randint(1, 256, (H, W, 3)).astype(np.uint8), rs.randint(1, 256, (H, W, 3)).astype(np.uint8)
    gl, gr = G.rectify_pair_host(left, right, shifted)
    for got, img, v in ((gl, left, shifted.valid[0]), (gr, right, shifted.valid[1])):
        want = np.zeros_like(img)
        want[:H - 3, 4:] = img[3:, :W - 4]
        assert got.tobytes() == want.tobytes()
        covered = np.zeros((H, W), np.uint8)
        covered[:H - 3, 4:] = 1
        assert np.array_equal(v, covered)


# ---- the model, without the map formula -------------------------------------------------------------------------------------------
def test_model_against_forward_projection():
    """A 3D point in a RAW camera's frame has a raw pixel (pinhole, distortion, K) and a rectified pixel (P R); the map at the
    rectified pixel must give the raw pixel.  Largest error measured on the CPU over both views of the KITTI-like and the
    smooth calibration, 4000 points each: 4.6e-13 px (fp64 round-off of the chain at coordinates up to ~1.4e3); the gate is
    100 x that."""
    G = _G()
    rs = np.random.RandomState(5)
    worst = 0.0
    K, D, R, P, src, dst = REF.kitti_raw_matrices()
    sets = [(G.RectifyMaps.from_kitti_raw(REF.kitti_raw_text()), (K, D, R, P))]
    mats = REF.smooth_matrices((37, 53), (29, 45))
    sets.append((G.RectifyMaps.from_matrices(*mats, (37, 53), (29, 45)), mats))
    for maps, (K, D, R, P) in sets:
        for view in range(2):
            n = 4000
            Z = rs.uniform(2.0, 60.0, n)
            X = np.stack([rs.uniform(-0.45, 0.45, n) * Z, rs.uniform(-0.15, 0.15, n) * Z, Z], 1)      # in front of the rig
            ur, vr = _distort_project(K[view], D[view], X)
            q = (P[view][:, :3] @ R[view] @ X.T)
            u, v = q[0] / q[2], q[1] / q[2]
            mx, my = maps.source_coords(view, u, v)
            worst = max(worst, np.abs(mx - ur).max(), np.abs(my - vr).max())
    print(f"model: max |source_coords - forward projection| = {worst:.3e} px")
    assert worst <= 100 * MODEL_MEASURED


def _random_rig(rs):
    K1 = np.array([[820 + rs.uniform(-20, 20), 0, 320 + rs.uniform(-8, 8)], [0, 815 + rs.uniform(-20, 20), 240 + rs.uniform(-8, 8)],
                   [0, 0, 1]])
    K2 = np.array([[790 + rs.uniform(-20, 20), 0, 322 + rs.uniform(-8, 8)], [0, 800 + rs.uniform(-20, 20), 238 + rs.uniform(-8, 8)],
                   [0, 0, 1]])
    D1 = np.array([-0.28, 0.1, 0.001, -0.002, -0.02]) * rs.uniform(0.5, 1.5, 5)
    D2 = np.array([-0.25, 0.08, -0.002, 0.001, 0.01]) * rs.uniform(0.5, 1.5, 5)
    R = REF.rotation(*np.deg2rad(rs.uniform(-5, 5, 3) / np.sqrt(3)))
    T = np.array([-0.3 * rs.uniform(0.8, 1.5), rs.uniform(-0.02, 0.02), rs.uniform(-0.02, 0.02)])
    return K1, D1, K2, D2, R, T


def test_from_stereo_properties():
    """Bouguet's construction by what it must achieve.  For random rigs (rotation up to ~5 degrees, baseline mostly along x) and
    random points X1 of camera 1's frame, X2 = R X1 + T: the rectified pixels P_k R_k X_k lie on one row, their disparity is
    f B / Z with maps.calib and Z the depth in the rectified frame, and the map at each rectified pixel gives that camera's
    raw pixel.  Largest error measured on the CPU over 8 rigs x 2000 points: 4.6e-13 px; the gate is 100 x that.  With the
    roles swapped view 0 and view 1 exchange their maps."""
    G = _G()
    rs = np.random.RandomState(7)
    worst = 0.0
    for _ in range(8):
        K1, D1, K2, D2, R, T = _random_rig(rs)
        maps = G.RectifyMaps.from_stereo(K1, D1, K2, D2, R, T, (480, 640))
        assert maps.src_hw == maps.dst_hw == (480, 640) and maps.calib is not None and maps.calib.doffs == 0.0
        assert abs(maps.calib.baseline - np.linalg.norm(T)) < 1e-12 and maps.calib.f == 0.5 * (K1[1, 1] + K2[1, 1])
        for Rk in maps.R:
            assert np.abs(Rk @ Rk.T - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(Rk) - 1) < 1e-14
        assert np.array_equal(maps.P[0][:, :3], maps.P[1][:, :3]) and maps.P[0][0, 3] == 0.0
        n = 2000
        Z = rs.uniform(2.0, 50.0, n)
        X1 = np.stack([rs.uniform(-0.3, 0.3, n) * Z, rs.uniform(-0.2, 0.2, n) * Z, Z], 1)
        X2 = X1 @ R.T + T
        pix = []
        for view, (Kk, Dk, Xk) in enumerate(((K1, D1, X1), (K2, D2, X2))):
            q = maps.P[view][:, :3] @ maps.R[view] @ Xk.T
            u, v = q[0] / q[2], q[1] / q[2]
            pix.append((u, v, q[2]))
            mx, my = maps.source_coords(view, u, v)
            ur, vr = _distort_project(Kk, Dk, Xk)
            worst = max(worst, np.abs(mx - ur).max(), np.abs(my - vr).max())
        (ul, vl, zl), (ur_, vr_, zr) = pix
        worst = max(worst, np.abs(vl - vr_).max(), np.abs(zl - zr).max())
        worst = max(worst, np.abs((ul - ur_) - maps.calib.f * maps.calib.baseline / zl).max())
        assert np.abs(maps.calib.cx - maps.P[0][0, 2]) == 0 and np.abs(maps.calib.cy - maps.P[0][1, 2]) == 0
        # camera 2 as the first camera: X1 = R^T X2 - R^T T
        swapped = G.RectifyMaps.from_stereo(K2, D2, K1, D1, R.T, -R.T @ T, (480, 640))
        assert swapped.calib is None                         # its view 1 lies to the LEFT of its view 0
        for a, b in ((0, 1), (1, 0)):
            assert np.abs(swapped.R[a] - maps.R[b]).max() < 1e-13
            assert np.abs(swapped.P[a][:, :3] - maps.P[b][:, :3]).max() < 1e-9
            assert np.abs(swapped.X[a].astype(np.int64) - maps.X[b]).max() <= 1
            assert np.abs(swapped.Y[a].astype(np.int64) - maps.Y[b]).max() <= 1
        assert abs(swapped.P[1][0, 3] + maps.P[1][0, 3]) < 1e-9
    print(f"from_stereo: max error of rows, disparity and raw pixel = {worst:.3e} px")
    assert worst <= 100 * STEREO_MEASURED
    with pytest.raises(ValueError, match="x axis"):
        G.RectifyMaps.from_stereo(K1, D1, K2, D2, R, [0.01, -0.3, 0.0], (480, 640))
    with pytest.raises(ValueError, match="rotation"):
        G.RectifyMaps.from_stereo(K1, D1, K2, D2, 1.1 * R, T, (480, 640))


# ---- the integer remap -------------------------------------------------------------------------------------------------------------
def _package_maps(case):
    """the package's maps of a shared case, built by the constructor a user would call"""
    G = _G()
    src, dst, c, kind = case
    X, Y, mats = REF.case_maps(case)
    if kind == "kitti":
        return G.RectifyMaps.from_kitti_raw(REF.kitti_raw_text())
    if mats is None:
        return G.RectifyMaps.from_fixed(X, Y, src)
    return G.RectifyMaps.from_matrices(*mats, src, dst)


@pytest.mark.parametrize("case", REF.CASES, ids=REF.case_id)
def test_maps_validity_and_host_remap_equal_the_reference(case):
    """Quantised maps: two fp64 evaluations of one coordinate differ by ~1e-12 px, so 32 m + 0.5 falls on different sides of an
    integer for about one entry in 10^9: the maps must agree except for at most one entry per case, and there by one unit.
    Validity and the remap are integer definitions: equal bit for bit on the package's own X, Y."""
    G = _G()
    src, dst, c, kind = case
    maps = _package_maps(case)
    X, Y, _ = REF.case_maps(case)
    assert maps.X.shape == X.shape and maps.dst_hw == dst and maps.src_hw == src
    dx, dy = np.abs(maps.X.astype(np.int64) - X), np.abs(maps.Y.astype(np.int64) - Y)
    assert dx.max() <= 1 and dy.max() <= 1 and int((dx > 0).sum() + (dy > 0).sum()) <= 1
    assert np.array_equal(maps.valid, REF.validity(maps.X, maps.Y, src))
    left, right = REF.case_images(case)
    want = REF.remap_pair(left, right, maps.X, maps.Y)
    got = G.rectify_pair_host(left, right, maps)
    for g, w in zip(got, want):
        assert g.dtype == np.uint8 and g.shape == dst + (c,) and g.tobytes() == w.tobytes()
    if kind == "random":
        if dst[0] * dst[1] >= 1000:
            assert 0 < maps.valid.mean() < 1
        if dst == (64, 128):         # 16384 entries per view: all 1024 (a, b) pairs, and taps at -1, 0, Ws-1 and Ws
            assert len(set(zip((maps.X & 31).reshape(-1).tolist(), (maps.Y & 31).reshape(-1).tolist()))) == 1024
            for x0 in (-1, 0, src[1] - 1, src[1]):
                assert ((maps.X >> 5) == x0).any()
            for y0 in (-1, 0, src[0] - 1, src[0]):
                assert ((maps.Y >> 5) == y0).any()
    if kind == "clamp":
        for end in (-16384 * 32, 16383 * 32, 16384 * 32):
            assert (maps.X == end).any() and (maps.Y == end).any()
        assert not maps.valid[(np.abs(maps.X) >= 16383 * 32) | (np.abs(maps.Y) >= 16383 * 32)].any()
    if kind == "smooth" and src == dst == (64, 128):
        assert maps.valid.all() and got[0].tobytes() == left.tobytes()


def test_bilinear_is_exact_on_a_linear_image():
    """I(r, c) = 2c + 3r + 5 on 40 x 30 (<= 181): bilinear interpolation reproduces a linear image, so at valid pixels
    |out - (2 mx + 3 my + 5)| <= 0.5 (rounding) + (2 + 3) / 64 (1/64 px of map quantisation per axis times the slopes)."""
    G = _G()
    src, dst = (40, 30), (36, 28)
    r, c = np.mgrid[0:40, 0:30]
    img = np.repeat((2 * c + 3 * r + 5).astype(np.uint8)[..., None], 3, 2)
    maps = G.RectifyMaps.from_matrices(*REF.smooth_matrices(src, dst), src, dst)
    out = G.rectify_pair_host(img, img, maps)
    u, v = np.meshgrid(np.arange(28.0), np.arange(36.0))
    for view in range(2):
        mx, my = maps.source_coords(view, u, v)
        ok = maps.valid[view] == 1
        assert 0.5 < ok.mean() < 1.0
        err = np.abs(out[view][..., 1].astype(np.float64) - (2 * mx + 3 * my + 5))[ok]
        print(f"view {view}: max |out - linear| = {err.max():.4f} at {int(ok.sum())} valid pixels")
        assert err.max() <= 0.5 + 5 / 64
        assert (out[view][..., 0] == out[view][..., 2]).all()


def test_host_remap_refuses_a_wrong_pair():
    G = _G()
    maps = G.RectifyMaps.from_fixed(np.zeros((2, 3, 4), np.int32), np.zeros((2, 3, 4), np.int32), (5, 6))
    ok = np.zeros((5, 6, 3), np.uint8)
    for bad in (np.zeros((5, 7, 3), np.uint8), np.zeros((5, 6, 2), np.uint8), np.zeros((5, 6, 3), np.float32),
                np.zeros((5, 6, 4), np.uint8)):
        with pytest.raises(ValueError):
            G.rectify_pair_host(ok, bad, maps)
    with pytest.raises(ValueError):
        maps.source_coords(0, 1.0, 1.0)


# ---- bindings -------------------------------------------------------------------------------------------------------------------
def test_rectify_pair_is_bound_and_the_abi_version_stays():
    from dcanet_amd import _lib
    assert _lib.ABI_VERSION == 21
    res, args = _lib.SIGNATURES["dca_rectify_pair"]
    assert res is ctypes.c_int and len(args) == 12
    assert args == [ctypes.c_void_p] * 3 + [ctypes.c_long] + [ctypes.c_void_p] * 2 + [ctypes.c_int] * 5 + [ctypes.c_void_p]
    assert _lib.CONSTANTS["DCA_RECT_FRAC_BITS"] == 5 and _lib.CONSTANTS["DCA_RECT_MAX_SRC"] == 16384
    lib = _lib.load()
    assert lib.dca_rectify_pair.argtypes == args and lib.dca_abi_version() == 21
    # argument checks come before any launch: no device is touched
    assert lib.dca_rectify_pair(None, None, None, 0, None, None, 1, 1, 1, 1, 3, None) != 0


# ---- the inference classes' keyword -------------------------------------------------------------------------------------------
def test_inference_classes_take_rectify_without_a_device():
    import torch
    from dcanet_amd.inference import (KittiInference, KittiInference3D, KittiInferenceLR, KittiInferenceWithConfidence)
    G = _G()
    src, dst = (70, 140), (60, 120)
    maps = G.RectifyMaps.from_matrices(*REF.smooth_matrices(src, dst), src, dst)
    net = torch.nn.Linear(1, 1)
    assert KittiInference(net).rectify is None
    for cls in (KittiInference, KittiInferenceWithConfidence, KittiInferenceLR):
        infer = cls(net, 64, 128, device_io=True, rectify=maps)
        assert infer.rectify is maps and (infer.crop_height, infer.crop_width) == (64, 128) and infer.device_io
    three = KittiInference3D(net, rectify=maps, device_io=True, crop_height=64, crop_width=128)
    assert three.rectify is maps and three.calib == maps.calib
    other = G.StereoCalib(100.0, 0.2, 60.0, 30.0)
    assert KittiInference3D(net, other, 64, 128, rectify=maps, device_io=True).calib == other
    with pytest.raises(ValueError, match="calib"):
        KittiInference3D(net, device_io=True)
    no_calib = G.RectifyMaps.from_fixed(maps.X, maps.Y, src)
    with pytest.raises(ValueError, match="calib"):
        KittiInference3D(net, rectify=no_calib, device_io=True, crop_height=64, crop_width=128)
    with pytest.raises(ValueError, match="mask_min"):
        KittiInference3D(net, rectify=maps, device_io=True, mask_min=0.0, crop_height=64, crop_width=128)
    with pytest.raises(ValueError):
        KittiInference(net, 64, 100, rectify=maps)           # 60 x 120 neither fits into 64 x 100 nor covers it
    with pytest.raises(TypeError, match="RectifyMaps"):
        KittiInference(net, rectify=(maps.X, maps.Y))
