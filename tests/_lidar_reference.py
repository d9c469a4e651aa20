"""Independent statements of dca_lidar_disparity (include/dca_hip.h) for the tests, sharing no code with the product:
`lidar_loop` -- one Python loop over the points with a dict as the z-buffer, every float32 operation spelled out;
`lidar_float64` -- the same formulas in float64; and the calibrations and scenes the CPU and GPU tests share."""
import numpy as np

# calibration texts with KITTI-like numbers (a raw drive's calib_cam_to_cam.txt and calib_velo_to_cam.txt)
CAM_TO_CAM = """calib_time: 09-Jan-2012 13:57:47
corner_dist: 9.950000e-02
S_02: 1.392000e+03 5.120000e+02
K_02: 9.597910e+02 0.000000e+00 6.960217e+02 0.000000e+00 9.569251e+02 2.241806e+02 0.000000e+00 0.000000e+00 1.000000e+00
D_02: -3.691481e-01 1.968681e-01 1.353473e-03 5.677587e-04 -6.770705e-02
R_02: 9.999758e-01 -5.267463e-03 -4.552439e-03 5.251945e-03 9.999804e-01 -3.413835e-03 4.570332e-03 3.389843e-03 9.999838e-01
T_02: 5.956621e-02 2.900141e-04 2.577209e-03
S_rect_02: 1.242000e+03 3.750000e+02
R_rect_02: 9.998817e-01 1.511453e-02 -2.841595e-03 -1.511724e-02 9.998853e-01 -9.338510e-04 2.827154e-03 9.766976e-04 9.999955e-01
P_rect_02: 7.215377e+02 0.000000e+00 6.095593e+02 4.485728e+01 0.000000e+00 7.215377e+02 1.728540e+02 2.163791e-01 0.000000e+00 0.000000e+00 1.000000e+00 2.745884e-03
S_03: 1.392000e+03 5.120000e+02
K_03: 9.037596e+02 0.000000e+00 6.957519e+02 0.000000e+00 9.019653e+02 2.242509e+02 0.000000e+00 0.000000e+00 1.000000e+00
D_03: -3.639558e-01 1.788651e-01 6.029694e-04 -3.922424e-04 -5.382460e-02
R_03: 9.995599e-01 1.699522e-02 -2.431313e-02 -1.704422e-02 9.998531e-01 -1.809756e-03 2.427880e-02 2.223358e-03 9.997028e-01
T_03: -4.731050e-01 5.551470e-03 -5.250882e-03
S_rect_03: 1.242000e+03 3.750000e+02
R_rect_03: 9.998321e-01 -7.193136e-03 1.685599e-02 7.232804e-03 9.999712e-01 -2.293585e-03 -1.683901e-02 2.415116e-03 9.998553e-01
P_rect_03: 7.215377e+02 0.000000e+00 6.095593e+02 -3.395242e+02 0.000000e+00 7.215377e+02 1.728540e+02 2.199936e+00 0.000000e+00 0.000000e+00 1.000000e+00 2.729905e-03
R_rect_00: 9.999239e-01 9.837760e-03 -7.445048e-03 -9.869795e-03 9.999421e-01 -4.278459e-03 7.402527e-03 4.351614e-03 9.999631e-01
"""
VELO_TO_CAM = """calib_time: 15-Mar-2012 11:37:23
R: 7.533745e-03 -9.999714e-01 -6.166020e-04 1.480249e-02 7.280733e-04 -9.998902e-01 9.998621e-01 7.523790e-03 1.480755e-02
T: -4.069766e-03 -7.631618e-02 -2.717806e-01
delta_f: 0.000000e+00 0.000000e+00
delta_c: 0.000000e+00 0.000000e+00
"""
KITTI_HW = (375, 1242)
WIDE = dict(min_depth=0.05, max_depth=1.0e4, min_disp=0.0, max_disp=1.0e5)       # filters that drop nothing in a scene


def numbers(text, key):
    for line in text.splitlines():
        if line.startswith(key + ":"):
            return np.array([float(x) for x in line.split(":", 1)[1].split()], np.float64)
    raise KeyError(key)


def kitti_matrix64():
    """M = P_rect_02 [R_rect_00 0; 0 1] [R T; 0 1] in float64, from the texts above"""
    R0, Tr = np.eye(4), np.eye(4)
    R0[:3, :3] = numbers(CAM_TO_CAM, "R_rect_00").reshape(3, 3)
    Tr[:3, :3] = numbers(VELO_TO_CAM, "R").reshape(3, 3)
    Tr[:3, 3] = numbers(VELO_TO_CAM, "T")
    return numbers(CAM_TO_CAM, "P_rect_02").reshape(3, 4) @ R0 @ Tr


def calib_for(hw):
    """the KITTI-like calibration, scaled down to an (H, W) image: rows 0 and 1 of M, f, cx, cy and the disparity scale"""
    from dcanet_amd.geometry import LidarCalib
    full = LidarCalib.from_kitti_raw(CAM_TO_CAM, VELO_TO_CAM)
    if tuple(hw) == KITTI_HW:
        return full
    sy, sx = hw[0] / KITTI_HW[0], hw[1] / KITTI_HW[1]
    return LidarCalib.from_matrix(np.diag([sx, sy, 1.0]) @ kitti_matrix64(), full.stereo.scaled(sx, sy), hw)


def identity_calib(hw, f=8.0, baseline=1.0):
    """M = [I|0]: a point (u z, v z, z) lands at (u, v) with depth z; fb = f * baseline, doffs = 0"""
    from dcanet_amd.geometry import LidarCalib, StereoCalib
    return LidarCalib.from_matrix(np.eye(3, 4), StereoCalib(f, baseline, 0.0, 0.0), hw)


def back_project(calib, u, v, z):
    """the float64 LiDAR coordinates whose projection through calib.M is (u z, v z, z): a 3x3 solve per point"""
    M = calib.M.astype(np.float64)
    rhs = np.stack([u * z, v * z, z], axis=-1) - M[:, 3]
    return np.linalg.solve(M[:, :3], rhs.reshape(-1, 3).T).T


def random_points(calib, count, seed, S=4, behind=0.05, zrange=(2.0, 60.0), surface=False):
    """`count` points whose pixels are uniform over the image and a 3 % margin around it, a share `behind` of them
    mirrored behind the sensor; (count,S) float32, further columns random.  Depths: uniform over zrange, or with `surface` a
    slanted plane from 10 to 19 metres across the image within 1 %, every fifth point 1.1 to 1.5 times farther (background
    seen through it)."""
    rng = np.random.default_rng(seed)
    H, W = calib.hw
    u = rng.uniform(-0.03 * W, 1.03 * W, count)
    v = rng.uniform(-0.03 * H, 1.03 * H, count)
    z = rng.uniform(*zrange, count)
    if surface:
        plane = 10.0 + 10.0 * np.clip(0.6 * u / W + 0.3 * v / H, 0.0, 1.0)
        z = plane * np.where(rng.random(count) < 0.2, rng.uniform(1.1, 1.5, count), rng.uniform(0.99, 1.01, count))
    z = np.where(rng.random(count) < behind, -z, z)
    pts = rng.random((count, S)).astype(np.float32)
    pts[:, :3] = back_project(calib, u, v, z).astype(np.float32)
    return pts


def scan_points(calib, beams=64, steps=1875, seed=0):
    """a synthetic scan, beams x steps points: 64 beams from +2 to -24.8 degrees of elevation, one full turn of azimuth, the
    sensor 1.73 m above a ground plane, with a wall of its own distance per 2 degrees of azimuth"""
    rng = np.random.default_rng(seed)
    elev = np.deg2rad(np.linspace(2.0, -24.8, beams))[:, None]
    azim = np.deg2rad(np.linspace(-180.0, 180.0, steps, endpoint=False))[None, :]
    wall = rng.uniform(5.0, 80.0, 180)[np.clip(((np.rad2deg(azim) + 180.0) / 2.0).astype(int), 0, 179)]
    with np.errstate(divide="ignore"):
        ground = np.where(elev < 0, 1.73 / np.sin(-elev), np.inf)
    rng_m = np.minimum(wall / np.cos(elev), ground) * rng.uniform(0.995, 1.005, (beams, steps))
    pts = np.zeros((beams * steps, 4), np.float32)
    pts[:, 0] = (rng_m * np.cos(elev) * np.cos(azim)).reshape(-1)
    pts[:, 1] = (rng_m * np.cos(elev) * np.sin(azim)).reshape(-1)
    pts[:, 2] = (rng_m * np.sin(elev)).reshape(-1)
    pts[:, 3] = rng.random(beams * steps)
    return pts


def lidar_loop(points, calib, n, occl, min_depth, max_depth, min_disp, max_disp):
    """point by point, pixel by pixel, one float32 operation at a time; the z-buffer is a dict.  Returns disp, depth,
    disp_u16 and count."""
    f = np.float32
    (H, W), M = calib.hw, np.asarray(calib.M, np.float32)
    fb, doffs = f(calib.stereo.fb), f(calib.stereo.doffs)
    rx, ry, scale = int(occl[0]), int(occl[1]), f(1.0 + float(occl[2]))
    lo, hi, dlo, dhi = f(min_depth), f(max_depth), f(min_disp), f(max_disp)
    zbuf, kept = {}, 0
    with np.errstate(all="ignore"):
        for i in range(n):
            X, Y, Z = f(points[i, 0]), f(points[i, 1]), f(points[i, 2])
            h = []
            for r in range(3):
                t = f(M[r, 0] * X)
                t = f(t + f(M[r, 1] * Y))
                t = f(t + f(M[r, 2] * Z))
                h.append(f(t + M[r, 3]))
            x, y, z = h
            uf, vf = np.floor(f(f(x / z) + f(0.5))), np.floor(f(f(y / z) + f(0.5)))
            if z >= lo and z <= hi and uf >= 0 and uf < f(W) and vf >= 0 and vf < f(H):
                kept += 1
                key = (int(vf), int(uf))
                if key not in zbuf or z < zbuf[key]:
                    zbuf[key] = z
        disp, depth = np.zeros((H, W), np.float32), np.zeros((H, W), np.float32)
        code = np.zeros((H, W), np.uint16)
        written = 0
        for (r, c), z in zbuf.items():
            zmin = z
            for rr in range(max(r - ry, 0), min(r + ry, H - 1) + 1):
                for cc in range(max(c - rx, 0), min(c + rx, W - 1) + 1):
                    if (rr, cc) in zbuf and zbuf[rr, cc] < zmin:
                        zmin = zbuf[rr, cc]
            d = f(f(fb / z) - doffs)
            if z <= f(zmin * scale) and d >= dlo and d < dhi:
                written += 1
                disp[r, c], depth[r, c] = d, z
                q = f(f(d * f(256.0)) + f(0.5))
                code[r, c] = 65535 if q >= 65535 else max(int(q), 1)
    return {"disp": disp, "depth": depth, "disp_u16": code, "count": np.array([written, kept], np.int64)}


def lidar_float64(points, calib, occl, min_depth, max_depth, min_disp, max_disp):
    """the same formulas in float64 (the matrix, fb and doffs are the float32 values the kernel is handed): disp, 0 where
    nothing is written"""
    (H, W), M = calib.hw, calib.M.astype(np.float64)
    P = points[:, :3].astype(np.float64)
    x, y, z = (M[r, 0] * P[:, 0] + M[r, 1] * P[:, 1] + M[r, 2] * P[:, 2] + M[r, 3] for r in range(3))
    with np.errstate(all="ignore"):
        uf, vf = np.floor(x / z + 0.5), np.floor(y / z + 0.5)
    keep = (z >= min_depth) & (z <= max_depth) & (uf >= 0) & (uf < W) & (vf >= 0) & (vf < H)
    zbuf = np.full((H, W), np.inf)
    order = np.argsort(-z[keep], kind="stable")                      # the nearest point is assigned last
    zbuf[vf[keep].astype(int)[order], uf[keep].astype(int)[order]] = z[keep][order]
    rx, ry = int(occl[0]), int(occl[1])
    pad = np.pad(zbuf, ((ry, ry), (rx, rx)), constant_values=np.inf)
    zmin = np.min([pad[dy:dy + H, dx:dx + W] for dy in range(2 * ry + 1) for dx in range(2 * rx + 1)], axis=0)
    with np.errstate(all="ignore"):
        d = float(calib.stereo.fb) / zbuf - float(calib.stereo.doffs)
    valid = np.isfinite(zbuf) & (zbuf <= zmin * (1.0 + float(occl[2]))) & (d >= min_disp) & (d < max_disp)
    return np.where(valid, d, 0.0)


def same_bits(got, want, name):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, got.dtype, want.shape, want.dtype)
    bad = np.nonzero((got.view(np.uint8) != want.view(np.uint8)).reshape(-1))[0]
    assert len(bad) == 0, f"{name}: {len(bad)} bytes differ, first at byte {int(bad[0])}"
