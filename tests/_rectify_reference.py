"""Independent numpy restatement of the rectification stage, written from the definitions and not
imported from the package: the map of a view from its matrices, its quantisation to 5 fractional bits, the validity of a
pixel's taps and the integer bilinear remap -- plus the cases the CPU and the GPU tests share (a synthetic KITTI-raw
calibration text, smooth calibrated maps for any size, random and clamped fixed-point maps)."""
import numpy as np

FRAC = 5
ONE = 1 << FRAC
LIMIT = 16384


# ---- the definitions ---------------------------------------------------------------------------------------------------------
def continuous_map(K, D, R, P, dst_hw):
    """(mx, my) float64 (Hd, Wd): the source coordinates of every destination pixel"""
    Hd, Wd = dst_hw
    K, R, P = (np.asarray(a, np.float64) for a in (K, R, P))
    k1, k2, p1, p2, k3 = (float(d) for d in D)
    uv1 = np.stack([np.tile(np.arange(Wd, dtype=np.float64), Hd), np.repeat(np.arange(Hd, dtype=np.float64), Wd),
                    np.ones(Hd * Wd)])
    xyw = np.linalg.inv(P[:, :3].dot(R)).dot(uv1)
    with np.errstate(all="ignore"):
        xp, yp = xyw[0] / xyw[2], xyw[1] / xyw[2]
        r2 = xp ** 2 + yp ** 2
        rad = 1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
        xpp = xp * rad + 2 * p1 * xp * yp + p2 * (r2 + 2 * xp ** 2)
        ypp = yp * rad + p1 * (r2 + 2 * yp ** 2) + 2 * p2 * xp * yp
        m = K.dot(np.stack([xpp, ypp, np.ones_like(xpp)]))
    return m[0].reshape(Hd, Wd), m[1].reshape(Hd, Wd)


def quantise(m):
    m = np.array(m, np.float64)
    m[np.isnan(m)] = -LIMIT
    m = np.minimum(np.maximum(m, -LIMIT), LIMIT - 1)
    return np.floor(ONE * m + 0.5).astype(np.int64).astype(np.int32)


def validity(X, Y, src_hw):
    Hs, Ws = src_hw
    X, Y = X.astype(np.int64), Y.astype(np.int64)
    x0, a, y0, b = X // ONE, X % ONE, Y // ONE, Y % ONE          # floor division: what >> and & give in two's complement
    x_last = np.where(a > 0, x0 + 1, x0)
    y_last = np.where(b > 0, y0 + 1, y0)
    return ((x0 >= 0) & (x_last <= Ws - 1) & (y0 >= 0) & (y_last <= Hs - 1)).astype(np.uint8)


def remap(img, X, Y):
    """one (Hs,Ws,C) uint8 image through one view's (Hd,Wd) maps: the source is laid into a frame of zeros one pixel wide, a
    tap further out is moved onto that frame"""
    Hs, Ws, C = img.shape
    padded = np.zeros((Hs + 2, Ws + 2, 3), np.int64)
    padded[1:-1, 1:-1] = img[:, :, :3]
    X, Y = X.astype(np.int64), Y.astype(np.int64)
    x0, a, y0, b = X // ONE, (X % ONE)[..., None], Y // ONE, (Y % ONE)[..., None]

    def p(r, c):
        return padded[np.clip(r, -1, Hs) + 1, np.clip(c, -1, Ws) + 1]

    acc = (ONE - a) * (ONE - b) * p(y0, x0) + a * (ONE - b) * p(y0, x0 + 1) + (ONE - a) * b * p(y0 + 1, x0) \
        + a * b * p(y0 + 1, x0 + 1) + 512
    out = np.full(X.shape + (C,), 255, np.uint8)
    out[..., :3] = acc // 1024
    return out


def remap_pair(left, right, X, Y):
    return remap(left, X[0], Y[0]), remap(right, X[1], Y[1])


# ---- shared cases -------------------------------------------------------------------------------------------------------------
def rotation(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz.dot(Ry).dot(Rx)


def kitti_raw_matrices():
    """plausible numbers of a KITTI raw drive: 1392 x 512 raw, 1242 x 375 rectified, cameras 02 / 03"""
    K = [np.array([[958.3, 0, 697.4], [0, 955.7, 225.9], [0, 0, 1]]), np.array([[902.6, 0, 694.1], [0, 900.2, 244.8], [0, 0, 1]])]
    D = [np.array([-0.3712, 0.2014, 0.0011, -0.0008, -0.0713]), np.array([-0.3644, 0.1822, -0.0009, 0.0013, -0.0586])]
    R = [rotation(0.004, -0.011, 0.006), rotation(-0.007, 0.013, -0.004)]
    P = [np.array([[721.5, 0, 609.6, 44.9], [0, 721.5, 172.9, 0.22], [0, 0, 1, 0.0027]]),
         np.array([[721.5, 0, 609.6, -339.6], [0, 721.5, 172.9, 2.2], [0, 0, 1, 0.0033]])]
    return K, D, R, P, (512, 1392), (375, 1242)


def kitti_raw_text():
    K, D, R, P, (Hs, Ws), (Hd, Wd) = kitti_raw_matrices()
    lines = ["calib_time: 09-Jan-2012 13:57:47", "corner_dist: 9.950000e-02"]
    for i, cam in enumerate(("02", "03")):
        def row(key, a):
            return f"{key}_{cam}: " + " ".join(f"{x:.17e}" for x in np.asarray(a, np.float64).reshape(-1))
        lines += [row("S", [Ws, Hs]), row("K", K[i]), row("D", D[i]), row("R", R[i]), row("T", [0.06 - 0.54 * i, 0, 0]),
                  row("S_rect", [Wd, Hd]), row("R_rect", R[i]), row("P_rect", P[i])]
    return "\n".join(lines) + "\n"


def smooth_matrices(src_hw, dst_hw):
    """a calibrated pair for any size: some distortion, small rectifying rotations, a destination that looks a little past
    the source on every side (borders with zeros and valid = 0)"""
    (Hs, Ws), (Hd, Wd) = src_hw, dst_hw
    f = 0.9 * max(Ws, Hs)
    K = [np.array([[f, 0, (Ws - 1) / 2 + 0.3], [0, 1.02 * f, (Hs - 1) / 2 - 0.2], [0, 0, 1]]),
         np.array([[0.97 * f, 0, (Ws - 1) / 2 - 0.4], [0, 0.98 * f, (Hs - 1) / 2 + 0.1], [0, 0, 1]])]
    D = [np.array([-0.25, 0.09, 0.002, -0.001, -0.01]), np.array([-0.21, 0.06, -0.001, 0.002, 0.005])]
    R = [rotation(0.01, -0.02, 0.015), rotation(-0.012, 0.018, -0.02)]
    fn = 0.8 * f * min(Wd / Ws, Hd / Hs)
    Pk = np.array([[fn, 0, (Wd - 1) / 2], [0, fn, (Hd - 1) / 2], [0, 0, 1]])
    P = [np.hstack([Pk, [[0.0], [0.0], [0.0]]]), np.hstack([Pk, [[-0.3 * fn], [0.0], [0.0]]])]
    return K, D, R, P


def identity_matrices(hw):
    H, W = hw
    K = np.array([[1.3 * W, 0, (W - 1) / 2], [0, 1.3 * W, (H - 1) / 2], [0, 0, 1]])
    P = [np.hstack([K, np.zeros((3, 1))]), np.hstack([K, [[-0.4 * 1.3 * W], [0.0], [0.0]]])]
    return [K, K], [np.zeros(5), np.zeros(5)], [np.eye(3), np.eye(3)], P


def random_fixed(seed, src_hw, dst_hw):
    """X uniform over [-3 * 32, (Ws + 2) * 32), Y likewise: every (a, b) pair, taps at -1, 0, Ws-1 and Ws"""
    rs = np.random.RandomState(seed)
    (Hs, Ws), (Hd, Wd) = src_hw, dst_hw
    X = rs.randint(-3 * ONE, (Ws + 2) * ONE, (2, Hd, Wd)).astype(np.int32)
    Y = rs.randint(-3 * ONE, (Hs + 2) * ONE, (2, Hd, Wd)).astype(np.int32)
    return X, Y


def clamp_fixed(seed, src_hw, dst_hw):
    """a random map in which about a third of the entries hold a clamp value: -16384 * 32, 16383 * 32 or +16384 * 32"""
    X, Y = random_fixed(seed, src_hw, dst_hw)
    rs = np.random.RandomState(seed + 1)
    ends = np.array([-LIMIT * ONE, (LIMIT - 1) * ONE, LIMIT * ONE], np.int32)
    for A in (X, Y):
        pick = rs.rand(*A.shape) < 1 / 6
        A[pick] = ends[rs.randint(0, 3, int(pick.sum()))]
    X.reshape(-1)[:3], Y.reshape(-1)[:3] = ends, ends[::-1]
    return X, Y


# (Hs, Ws), (Hd, Wd), C of the GPU cases; every one runs with the smooth, the random and the clamped map.  The last two: a
# source of one pixel (no pair of neighbours to load) and of two (the smallest with one)
SIZES = [((37, 53), (29, 45), 3), ((37, 53), (29, 45), 4), ((5, 3), (7, 9), 3), ((1, 7), (1, 7), 3),
         ((64, 128), (64, 128), 3), ((33, 41), (31, 43), 4), ((1, 1), (3, 5), 3), ((2, 1), (3, 5), 4)]
CASES = [(s, d, c, kind) for s, d, c in SIZES for kind in ("smooth", "random", "clamp")] + [((512, 1392), (375, 1242), 3, "kitti")]


def case_id(case):
    (hs, ws), (hd, wd), c, kind = case
    return f"{hs}x{ws}-{hd}x{wd}-c{c}-{kind}"


def case_maps(case):
    """(X, Y) int32 (2,Hd,Wd) of a case from THIS module's definitions, and the matrices it was built from (or None)"""
    src, dst, c, kind = case
    seed = src[0] * 131 + src[1] * 7 + dst[1] + c
    if kind == "random":
        return random_fixed(seed, src, dst) + (None,)
    if kind == "clamp":
        return clamp_fixed(seed, src, dst) + (None,)
    if kind == "kitti":
        mats = kitti_raw_matrices()[:4]
    else:
        mats = identity_matrices(src) if src == dst == (64, 128) else smooth_matrices(src, dst)
    m = [continuous_map(mats[0][i], mats[1][i], mats[2][i], mats[3][i], dst) for i in range(2)]
    return (np.stack([quantise(m[0][0]), quantise(m[1][0])]), np.stack([quantise(m[0][1]), quantise(m[1][1])]), mats)


def case_images(case):
    src, dst, c, kind = case
    rs = np.random.RandomState(src[0] + 3 * src[1] + c)
    return rs.randint(0, 256, src + (c,)).astype(np.uint8), rs.randint(0, 256, src + (c,)).astype(np.uint8)
