"""Stereo calibration and the exporters of the geometry stage: `StereoCalib` holds what
`ops.disp_to_depth` and `ops.point_cloud` need to turn a disparity in pixels into metres, read from a KITTI or a
Middlebury calibration file; `write_ply` / `read_ply` store the compacted vertex buffer as it is -- the device buffer IS
the body of a binary PLY file -- and `depth_png` writes the KITTI 16-bit depth format.  Host code only: no arithmetic on
the maps happens here.

`RectifyMaps` holds the fixed-point maps that rectify a RAW stereo pair, built once per calibration in
float64; `ops.rectify_pair` applies them on the device and `rectify_pair_host` is the numpy restatement of that kernel.

`LidarCalib` holds the projection of a LiDAR scan into the rectified left image; `ops.lidar_disparity`
turns a scan into sparse ground-truth maps on the device, `lidar_disparity_host` is its numpy restatement and
`LidarProjector` the staging ring that feeds the device from host scans."""
from __future__ import annotations

import dataclasses
import os
import re

import numpy as np

# the 16-byte record of dca_point_cloud (include/dca_hip.h)
PLY_VERTEX = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"),
                       ("red", "u1"), ("green", "u1"), ("blue", "u1"), ("alpha", "u1")])
assert PLY_VERTEX.itemsize == 16

_PLY_HEADER = ("ply\n"
               "format binary_little_endian 1.0\n"
               "element vertex {n}\n"
               "property float x\n"
               "property float y\n"
               "property float z\n"
               "property uchar red\n"
               "property uchar green\n"
               "property uchar blue\n"
               "property uchar alpha\n"
               "end_header\n")


def _text(text_or_path) -> str:
    """the calibration text itself, or the content of the file it names"""
    if isinstance(text_or_path, os.PathLike) or (isinstance(text_or_path, str) and "\n" not in text_or_path
                                                 and os.path.exists(text_or_path)):
        with open(text_or_path) as f:
            return f.read()
    return str(text_or_path)


@dataclasses.dataclass(frozen=True)
class StereoCalib:
    """A rectified pair: focal length `f` and principal point (`cx`, `cy`) of the LEFT camera in pixels, `baseline` in
    metres, `doffs` = cx_right - cx_left in pixels (0 for KITTI).  Depth Z = f * baseline / (d + doffs)."""
    f: float
    baseline: float
    cx: float
    cy: float
    doffs: float = 0.0

    def __post_init__(self):
        for k in ("f", "baseline", "cx", "cy", "doffs"):
            v = float(getattr(self, k))
            if not np.isfinite(v):
                raise ValueError(f"StereoCalib: {k} must be finite, got {v}")
            object.__setattr__(self, k, v)
        if self.f <= 0 or self.baseline <= 0:
            raise ValueError(f"StereoCalib: f and baseline must be positive, got {self.f} and {self.baseline}")

    @property
    def fb(self) -> float:
        """float32(f * baseline), the product formed in double precision and rounded once"""
        return float(np.float32(np.float64(self.f) * np.float64(self.baseline)))

    def scaled(self, sx: float, sy: float | None = None) -> "StereoCalib":
        """the calibration of the images resized by sx horizontally and sy (default sx) vertically: f, cx, doffs and the
        disparity scale with sx, cy with sy.  One focal length is kept, so X and Z stay exact and Y assumes sy == sx."""
        sy = sx if sy is None else sy
        return StereoCalib(self.f * sx, self.baseline, self.cx * sx, self.cy * sy, self.doffs * sx)

    @classmethod
    def from_kitti(cls, text_or_path, left: str = "P2", right: str = "P3") -> "StereoCalib":
        """KITTI calibration text: object-style keys (`P2:`) or raw-style keys (`P_rect_02:`), 12 numbers = a 3x4
        projection matrix each.  f = P_l[0,0], cx = P_l[0,2], cy = P_l[1,2], baseline = P_l[0,3] / P_l[0,0] -
        P_r[0,3] / P_r[0,0], doffs = P_r[0,2] - P_l[0,2]."""
        rows = {}
        for line in _text(text_or_path).splitlines():
            key, sep, rest = line.partition(":")
            if sep:
                rows[key.strip()] = rest.split()

        def matrix(name):
            m = re.fullmatch(r"P(\d)", name)
            for key in (name,) + ((f"P_rect_0{m.group(1)}",) if m else ()):
                if key in rows:
                    if len(rows[key]) != 12:
                        raise ValueError(f"from_kitti: {key} has {len(rows[key])} numbers, expected 12")
                    return np.array([float(x) for x in rows[key]], np.float64).reshape(3, 4)
            raise ValueError(f"from_kitti: no projection matrix {name} in the calibration text")

        Pl, Pr = matrix(left), matrix(right)
        return cls(Pl[0, 0], Pl[0, 3] / Pl[0, 0] - Pr[0, 3] / Pr[0, 0], Pl[0, 2], Pl[1, 2], Pr[0, 2] - Pl[0, 2])

    @classmethod
    def from_middlebury(cls, text_or_path) -> "StereoCalib":
        """Middlebury 2014 calib.txt: `cam0=[f 0 cx; 0 f cy; 0 0 1]`, `cam1`, `doffs`, `baseline` in millimetres (converted to
        metres here).  `doffs` is taken from its own line, which the dataset rounds as the ground truth expects."""
        vals = {}
        for line in _text(text_or_path).splitlines():
            key, sep, rest = line.partition("=")
            if sep:
                vals[key.strip()] = rest.strip()
        for key in ("cam0", "cam1", "doffs", "baseline"):
            if key not in vals:
                raise ValueError(f"from_middlebury: no `{key}=` line in the calibration text")
        cam0 = np.array([float(x) for x in re.split(r"[\s;]+", vals["cam0"].strip("[] "))], np.float64)
        if cam0.size != 9:
            raise ValueError(f"from_middlebury: cam0 has {cam0.size} numbers, expected 9")
        cam0 = cam0.reshape(3, 3)
        return cls(cam0[0, 0], float(vals["baseline"]) / 1000.0, cam0[0, 2], cam0[1, 2], float(vals["doffs"]))


def _as_vertices(vertices) -> np.ndarray:
    """a PLY_VERTEX array, or the (n,4) float32 form `ops.point_cloud` returns (the fourth column holds the colour bytes)"""
    if hasattr(vertices, "detach"):
        vertices = vertices.detach().cpu().numpy()
    v = np.ascontiguousarray(vertices)
    if v.dtype == PLY_VERTEX:
        return v.reshape(-1)
    if v.dtype == np.float32 and v.ndim == 2 and v.shape[1] == 4:
        return v.view(PLY_VERTEX).reshape(-1)
    raise ValueError(f"expected a PLY_VERTEX array or an (n,4) float32 array, got {v.dtype} {v.shape}")


def write_ply(path, vertices) -> int:
    """binary little-endian PLY with `x y z red green blue alpha` per vertex: the header, then the records' bytes as they
    are.  Returns the number of vertices."""
    v = _as_vertices(vertices)
    with open(path, "wb") as f:
        f.write(_PLY_HEADER.format(n=len(v)).encode("ascii"))
        f.write(v.tobytes())
    return len(v)


def read_ply(path) -> np.ndarray:
    """a file `write_ply` made -> its PLY_VERTEX array; any other header is refused"""
    with open(path, "rb") as f:
        data = f.read()
    end = data.find(b"end_header\n")
    if end < 0:
        raise ValueError(f"{path}: no PLY header")
    end += len(b"end_header\n")
    m = re.search(r"^element vertex (\d+)$", data[:end].decode("ascii", "replace"), flags=re.M)
    if not m or data[:end].decode("ascii", "replace") != _PLY_HEADER.format(n=m.group(1)):
        raise ValueError(f"{path}: not a header write_ply writes")
    n = int(m.group(1))
    if len(data) - end != n * PLY_VERTEX.itemsize:
        raise ValueError(f"{path}: {len(data) - end} bytes behind the header, expected {n} vertices of 16")
    return np.frombuffer(data, PLY_VERTEX, n, end).copy()


def depth_png(path, depth) -> None:
    """KITTI's 16-bit depth format: uint16(depth * 256), 0 = no measurement; a uint16 map (`disp_to_depth(u16=True)`) is
    written as it is."""
    from PIL import Image
    depth = np.asarray(depth)
    if depth.dtype != np.uint16:
        scaled = np.nan_to_num(depth.astype(np.float32) * np.float32(256), nan=0.0)
        depth = np.clip(np.trunc(scaled), 0, 65535).astype("uint16")
    Image.fromarray(depth).save(path, format="PNG")


# ---- rectification of a raw pair (csrc/rectify.hip) ---------------------------------------------------
RECT_FRAC_BITS = 5                 # DCA_RECT_FRAC_BITS of include/dca_hip.h: the maps' fractional bits
RECT_MAX_SRC = 16384               # DCA_RECT_MAX_SRC: the largest source height / width; also the clamp of a map coordinate
_RECT_ONE = 1 << RECT_FRAC_BITS


def _hw(hw, name):
    h, w = (int(v) for v in hw)
    if h <= 0 or w <= 0:
        raise ValueError(f"RectifyMaps: {name} must be positive, got {h} x {w}")
    return h, w


def _mat(a, shape, name):
    a = np.asarray(a, np.float64)
    if a.shape != shape or not np.isfinite(a).all():
        raise ValueError(f"RectifyMaps: {name} must be a finite {' x '.join(map(str, shape))} array, got shape {a.shape}")
    return a


def _rodrigues(om):
    """rotation vector -> rotation matrix (fp64)"""
    om = np.asarray(om, np.float64)
    th = float(np.linalg.norm(om))
    if th == 0.0:
        return np.eye(3)
    k = om / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1.0 - np.cos(th)) * (Kx @ Kx)


def _rotvec(R):
    """rotation matrix -> rotation vector (angle below pi)"""
    ax = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s = float(np.linalg.norm(ax)) / 2.0
    c = (float(np.trace(R)) - 1.0) / 2.0
    th = float(np.arctan2(s, c))
    if s < 1e-12:
        if c > 0:
            return np.zeros(3)
        raise ValueError("RectifyMaps.from_stereo: the two cameras look in opposite directions")
    return ax / (2.0 * s) * th


def _tap_validity(X, Y, src_hw):
    """valid = every tap the kernel reads with a non-zero weight lies inside the source"""
    Hs, Ws = src_hw
    x0, a, y0, b = X >> RECT_FRAC_BITS, X & (_RECT_ONE - 1), Y >> RECT_FRAC_BITS, Y & (_RECT_ONE - 1)
    ok = (x0 >= 0) & (x0 + (a > 0) < Ws) & (y0 >= 0) & (y0 + (b > 0) < Hs)
    return ok.astype(np.uint8)


def _quantise(m):
    """continuous source coordinate -> fixed point: clamp to [-16384, 16383] (NaN: -16384), floor(32 m + 0.5)"""
    m = np.where(np.isnan(m), -float(RECT_MAX_SRC), m)
    m = np.clip(m, -float(RECT_MAX_SRC), float(RECT_MAX_SRC - 1))
    return np.floor(_RECT_ONE * m + 0.5).astype(np.int32)


class RectifyMaps:
    """The rectifying maps of a stereo pair in fixed point, built ONCE per calibration on the host in float64; per frame
    `ops.rectify_pair` (device) or `rectify_pair_host` (numpy) gathers both images through them.
      X, Y      int32 (2, Hd, Wd): the source coordinates of every destination pixel of view 0 (left) / 1 (right), 5
                fractional bits
      valid     uint8 (2, Hd, Wd): 1 where every bilinear tap with a non-zero weight lies inside the source
      src_hw    (Hs, Ws) of the raw images, dst_hw (Hd, Wd) of the rectified ones; they may differ
      calib     the StereoCalib of the rectified pair (None from `from_fixed`, or when view 1 is not to the right of view 0)
    Map of destination pixel (u, v), with K, D = (k1, k2, p1, p2, k3), R, P of the view and Pk = P[:, :3] -- the model of
    OpenCV's initUndistortRectifyMap, in float64:
      [x y w] = (Pk R)^-1 [u v 1];  x' = x / w, y' = y / w, r2 = x'^2 + y'^2;  rad = 1 + k1 r2 + k2 r2^2 + k3 r2^3
      x'' = x' rad + 2 p1 x' y' + p2 (r2 + 2 x'^2);  y'' = y' rad + p1 (r2 + 2 y'^2) + 2 p2 x' y';  [mx my 1] = K [x'' y'' 1]
    """

    def __init__(self, X, Y, src_hw, calib=None, K=None, D=None, R=None, P=None):
        self.src_hw = _hw(src_hw, "src_hw")
        if max(self.src_hw) > RECT_MAX_SRC:
            raise ValueError(f"RectifyMaps: the source may be at most {RECT_MAX_SRC} x {RECT_MAX_SRC}, got "
                             f"{self.src_hw[0]} x {self.src_hw[1]}")
        X, Y = np.ascontiguousarray(X), np.ascontiguousarray(Y)
        if X.dtype != np.int32 or Y.dtype != np.int32 or X.ndim != 3 or X.shape[0] != 2 or X.shape != Y.shape or X.size == 0:
            raise ValueError(f"RectifyMaps: X and Y must be int32 (2, Hd, Wd) arrays of one shape, got {X.dtype} {X.shape} "
                             f"and {Y.dtype} {Y.shape}")
        self.X, self.Y = X, Y
        self.dst_hw = (int(X.shape[1]), int(X.shape[2]))
        self.valid = _tap_validity(X, Y, self.src_hw)
        self.calib = calib
        self.K, self.D, self.R, self.P = K, D, R, P
        self._device = {}            # device -> packed maps

    # ---- constructors -----------------------------------------------------------------------------------------------------
    @classmethod
    def from_fixed(cls, X, Y, src_hw) -> "RectifyMaps":
        """raw fixed-point arrays (any int32 is a legal coordinate); `valid` is recomputed, `calib` is None"""
        return cls(X, Y, src_hw)

    @classmethod
    def from_matrices(cls, K, D, R, P, src_hw, dst_hw) -> "RectifyMaps":
        """K (3x3), D (5), R (3x3), P (3x4) per view, each a sequence of two.  `calib` follows from the two P exactly as
        StereoCalib.from_kitti derives it."""
        for name, seq in (("K", K), ("D", D), ("R", R), ("P", P)):
            if len(seq) != 2:
                raise ValueError(f"RectifyMaps.from_matrices: {name} must hold one entry per view, got {len(seq)}")
        K = [_mat(k, (3, 3), "K") for k in K]
        D = [_mat(d, (5,), "D") for d in D]
        R = [_mat(r, (3, 3), "R_rect") for r in R]
        P = [_mat(p, (3, 4), "P_rect") for p in P]
        src_hw, (Hd, Wd) = _hw(src_hw, "src_hw"), _hw(dst_hw, "dst_hw")
        Pl, Pr = P
        try:
            calib = StereoCalib(Pl[0, 0], Pl[0, 3] / Pl[0, 0] - Pr[0, 3] / Pr[0, 0], Pl[0, 2], Pl[1, 2], Pr[0, 2] - Pl[0, 2])
        except (ValueError, ZeroDivisionError):
            calib = None             # view 1 is not to the right of view 0: no depth from u_l - u_r
        self = cls.__new__(cls)
        self.K, self.D, self.R, self.P = K, D, R, P
        u, v = np.meshgrid(np.arange(Wd, dtype=np.float64), np.arange(Hd, dtype=np.float64))
        with np.errstate(all="ignore"):
            m = [self.source_coords(i, u, v) for i in range(2)]
        X = np.stack([_quantise(m[0][0]), _quantise(m[1][0])])
        Y = np.stack([_quantise(m[0][1]), _quantise(m[1][1])])
        cls.__init__(self, X, Y, src_hw, calib, K, D, R, P)
        return self

    @classmethod
    def from_kitti_raw(cls, text_or_path, left: str = "02", right: str = "03") -> "RectifyMaps":
        """KITTI raw `calib_cam_to_cam.txt`: `K_xx` (9 numbers), `D_xx` (5), `R_rect_xx` (9), `P_rect_xx` (12), `S_xx` and
        `S_rect_xx` (2: width height) of the cameras `left` and `right`."""
        rows = {}
        for line in _text(text_or_path).splitlines():
            key, sep, rest = line.partition(":")
            if sep:
                rows[key.strip()] = rest.split()

        def numbers(key, count):
            if key not in rows:
                raise ValueError(f"from_kitti_raw: no {key} in the calibration text")
            if len(rows[key]) != count:
                raise ValueError(f"from_kitti_raw: {key} has {len(rows[key])} numbers, expected {count}")
            try:
                a = np.array([float(x) for x in rows[key]], np.float64)
            except ValueError:
                raise ValueError(f"from_kitti_raw: {key} holds something that is not a number") from None
            if not np.isfinite(a).all():
                raise ValueError(f"from_kitti_raw: {key} holds a number that is not finite")
            return a

        cams = (left, right)
        K = [numbers(f"K_{c}", 9).reshape(3, 3) for c in cams]
        D = [numbers(f"D_{c}", 5) for c in cams]
        R = [numbers(f"R_rect_{c}", 9).reshape(3, 3) for c in cams]
        P = [numbers(f"P_rect_{c}", 12).reshape(3, 4) for c in cams]
        S = [numbers(f"S_{c}", 2) for c in cams]
        Sr = [numbers(f"S_rect_{c}", 2) for c in cams]
        for name, s in (("S", S), ("S_rect", Sr)):
            if (s[0] != s[1]).any() or (s[0] != np.round(s[0])).any():
                raise ValueError(f"from_kitti_raw: {name}_{left} and {name}_{right} must be one integer size, got {s[0]} and {s[1]}")
        return cls.from_matrices(K, D, R, P, (int(S[0][1]), int(S[0][0])), (int(Sr[0][1]), int(Sr[0][0])))

    @classmethod
    def from_stereo(cls, K1, D1, K2, D2, R, T, src_hw, dst_hw=None) -> "RectifyMaps":
        """Intrinsics of both cameras and the pose of camera 2 relative to camera 1 (a point X1 of camera 1's frame is
        X2 = R X1 + T in camera 2's) -> the rectifying rotations and ONE new projection for both views (Bouguet's
        construction, as OpenCV's stereoRectify): both cameras turn by half of R towards each other, then together so that
        the baseline becomes the x axis.  The shared focal length is the mean of the two fy; the shared principal point is the
        mean over both cameras of the point that keeps the camera's raw optical axis at its raw principal point (zero-disparity
        form, doffs = 0).  No cropping or scaling: dst_hw defaults to src_hw."""
        K1, K2 = _mat(K1, (3, 3), "K1"), _mat(K2, (3, 3), "K2")
        R, T = _mat(R, (3, 3), "R"), _mat(np.asarray(T, np.float64).reshape(-1), (3,), "T")
        if np.abs(R @ R.T - np.eye(3)).max() > 1e-6 or np.linalg.det(R) < 0:
            raise ValueError("RectifyMaps.from_stereo: R is not a rotation matrix")
        rr = _rodrigues(-0.5 * _rotvec(R))                   # R^(-1/2)
        t = rr @ T
        if abs(t[0]) <= max(abs(t[1]), abs(t[2])):
            raise ValueError(f"RectifyMaps.from_stereo: the baseline {T} is not along the x axis of the cameras")
        uu = np.array([1.0 if t[0] > 0 else -1.0, 0.0, 0.0])
        ww = np.cross(t, uu)
        nw = float(np.linalg.norm(ww))
        wR = _rodrigues(ww * (np.arccos(abs(t[0]) / np.linalg.norm(t)) / nw)) if nw > 0 else np.eye(3)
        R1, R2 = wR @ rr.T, wR @ rr
        tx = float((R2 @ T)[0])                              # R2 X2 = R1 X1 + (tx, 0, 0)
        f = 0.5 * (K1[1, 1] + K2[1, 1])
        pp = []
        for Kk, Rk in ((K1, R1), (K2, R2)):
            z = Rk[:, 2]                                     # the raw optical axis in the rectified frame
            pp.append([Kk[0, 2] - f * z[0] / z[2], Kk[1, 2] - f * z[1] / z[2]])
        cx, cy = np.mean(pp, axis=0)
        P1 = np.array([[f, 0, cx, 0], [0, f, cy, 0], [0, 0, 1, 0]], np.float64)
        P2 = P1.copy()
        P2[0, 3] = tx * f
        src_hw = _hw(src_hw, "src_hw")
        return cls.from_matrices((K1, K2), (D1, D2), (R1, R2), (P1, P2), src_hw, src_hw if dst_hw is None else dst_hw)

    # ---- the continuous map --------------------------------------------------------------------------------------------------
    def source_coords(self, view, u, v):
        """(mx, my): the float64 source coordinates of the destination coordinates (u, v) of `view` (arrays of one shape,
        integer or not); only for maps built from matrices"""
        if self.K is None:
            raise ValueError("RectifyMaps.source_coords: these maps were not built from matrices")
        K, (k1, k2, p1, p2, k3), R, P = (getattr(self, n)[view] for n in "KDRP")
        u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
        iR = np.linalg.inv(P[:, :3] @ R)
        x = iR[0, 0] * u + iR[0, 1] * v + iR[0, 2]
        y = iR[1, 0] * u + iR[1, 1] * v + iR[1, 2]
        w = iR[2, 0] * u + iR[2, 1] * v + iR[2, 2]
        x, y = x / w, y / w
        r2 = x * x + y * y
        rad = 1.0 + k1 * r2 + k2 * r2 * r2 + k3 * r2 * r2 * r2
        xd = x * rad + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
        yd = y * rad + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
        return K[0, 0] * xd + K[0, 1] * yd + K[0, 2], K[1, 0] * xd + K[1, 1] * yd + K[1, 2]

    # ---- device copies ---------------------------------------------------------------------------------------------------------
    def device_maps(self, device):
        """(maps, plane) for dca_rectify_pair on `device`, uploaded once: an int32 (4, plane) tensor holding the planes
        X[0], Y[0], X[1], Y[1], each padded to `plane`, a multiple of 4 words"""
        import torch
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device not in self._device:
            n = self.dst_hw[0] * self.dst_hw[1]
            plane = (n + 3) & ~3
            packed = np.zeros((4, plane), np.int32)
            for i, a in enumerate((self.X[0], self.Y[0], self.X[1], self.Y[1])):
                packed[i, :n] = a.reshape(-1)
            self._device[device] = (torch.from_numpy(packed).to(device), plane)
        return self._device[device]


def rectify_pair_host(left, right, maps: RectifyMaps):
    """numpy restatement of dca_rectify_pair, integer operation for integer operation: two (Hs,Ws,C) uint8 images, C = 3 or
    4 -> the two rectified (Hd,Wd,C) images.  A tap outside the source reads 0; a fourth channel becomes 255."""
    left, right = np.asarray(left), np.asarray(right)
    Hs, Ws = maps.src_hw
    out = []
    for i, img in enumerate((left, right)):
        if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] not in (3, 4) or img.shape[:2] != (Hs, Ws):
            raise ValueError(f"rectify_pair_host: expected two ({Hs},{Ws},3) or ({Hs},{Ws},4) uint8 images, got {img.dtype} "
                             f"{img.shape}")
        if img.shape != left.shape:
            raise ValueError(f"rectify_pair_host: the images differ in shape: {left.shape} and {img.shape}")
        X, Y = maps.X[i], maps.Y[i]
        x0, a, y0, b = X >> RECT_FRAC_BITS, X & (_RECT_ONE - 1), Y >> RECT_FRAC_BITS, Y & (_RECT_ONE - 1)
        acc = np.full(X.shape + (3,), 512, np.int32)
        for dy, wy in ((0, _RECT_ONE - b), (1, b)):
            for dx, wx in ((0, _RECT_ONE - a), (1, a)):
                r, c = y0 + dy, x0 + dx
                inside = (r >= 0) & (r < Hs) & (c >= 0) & (c < Ws)
                tap = img[np.where(inside, r, 0), np.where(inside, c, 0), :3].astype(np.int32)
                acc += np.where(inside, wy * wx, 0)[..., None] * tap
        res = np.full(X.shape + (img.shape[2],), 255, np.uint8)
        res[..., :3] = (acc >> 10).astype(np.uint8)
        out.append(res)
    return out[0], out[1]


# ---- sparse ground truth from a LiDAR scan (csrc/lidar.hip) ---------------------------------------------
LIDAR_MAX_RADIUS = 8               # DCA_LIDAR_MAX_RADIUS of include/dca_hip.h: the largest half-size of the hidden-point window
LIDAR_OUTPUTS = ("disp", "depth", "disp_u16", "count")
# Default filters.  occl = (rx, ry, rel): the radii are read off the sensor's geometry (64 beams over about 27 degrees: about 5
# image rows between scan lines at KITTI's focal length; 0.09 degrees of azimuth: about 1 column); rel = 0.1 comes from
# nowhere, and none of the three was tuned on data.
LIDAR_OCCL = (2, 4, 0.1)
LIDAR_MIN_DEPTH = 1.0              # metres
LIDAR_MAX_DEPTH = 120.0            # the range of a Velodyne HDL-64E
LIDAR_MIN_DISP = 0.0
LIDAR_MAX_DISP = 192.0             # the model's default maxdisp: mask = gt > 0 && gt < maxdisp


def _kitti_rows(text_or_path):
    rows = {}
    for line in _text(text_or_path).splitlines():
        key, sep, rest = line.partition(":")
        if sep:
            rows[key.strip()] = rest.split()
    return rows


def _kitti_numbers(rows, key, count):
    if key not in rows:
        raise ValueError(f"from_kitti_raw: no {key} in the calibration text")
    if len(rows[key]) != count:
        raise ValueError(f"from_kitti_raw: {key} has {len(rows[key])} numbers, expected {count}")
    try:
        a = np.array([float(x) for x in rows[key]], np.float64)
    except ValueError:
        raise ValueError(f"from_kitti_raw: {key} holds something that is not a number") from None
    if not np.isfinite(a).all():
        raise ValueError(f"from_kitti_raw: {key} holds a number that is not finite")
    return a


class LidarCalib:
    """What `ops.lidar_disparity` needs to project a LiDAR scan into the rectified left image:
      M       float32 (3,4): LiDAR coordinates -> homogeneous pixels (x, y, z) of the rectified left camera, u = x / z,
              v = y / z, z the depth in metres; formed in float64 and rounded ONCE to 12 float32
      stereo  the StereoCalib of the rectified pair: disparity d = stereo.fb / z - stereo.doffs
      hw      (H, W) of the rectified image"""

    def __init__(self, M, stereo, hw):
        M = np.asarray(M, np.float64)
        if M.shape != (3, 4) or not np.isfinite(M).all():
            raise ValueError(f"LidarCalib: M must be a finite 3 x 4 array, got shape {M.shape}")
        with np.errstate(over="ignore"):
            M = M.astype(np.float32)
        if not np.isfinite(M).all():
            raise ValueError("LidarCalib: M does not fit float32")
        if not isinstance(stereo, StereoCalib):
            raise ValueError(f"LidarCalib: stereo must be a StereoCalib, got {type(stereo)}")
        h, w = (int(v) for v in hw)
        if h <= 0 or w <= 0 or h * w >= 1 << 31:
            raise ValueError(f"LidarCalib: hw must be positive with H * W below 2^31, got {h} x {w}")
        M.setflags(write=False)
        self.M, self.stereo, self.hw = M, stereo, (h, w)

    @classmethod
    def from_matrix(cls, M, stereo, hw) -> "LidarCalib":
        """M: any (3,4) array (rounded once from float64), stereo: a StereoCalib, hw: (H, W)"""
        return cls(M, stereo, hw)

    @classmethod
    def from_kitti_raw(cls, cam_to_cam, velo_to_cam, left: str = "02", right: str = "03") -> "LidarCalib":
        """KITTI raw `calib_cam_to_cam.txt` and `calib_velo_to_cam.txt` (texts or paths):
          M = P_rect_<left> . [R_rect_00 0; 0 1] . [R T; 0 1]
        with R (9 numbers) and T (3) of the velo-to-cam file, hw from S_rect_<left> (width height) and `stereo` from the two
        P_rect matrices by the formulas of `StereoCalib.from_kitti`.  `RectifyMaps.from_kitti_raw` rectifies into this very
        frame (KITTI's own rectified images), so the same M serves the dataset's rectified images and pairs rectified by
        `ops.rectify_pair`: `hw == maps.dst_hw`."""
        cam, velo = _kitti_rows(cam_to_cam), _kitti_rows(velo_to_cam)
        Pl = _kitti_numbers(cam, f"P_rect_{left}", 12).reshape(3, 4)
        Pr = _kitti_numbers(cam, f"P_rect_{right}", 12).reshape(3, 4)
        R0 = np.eye(4)
        R0[:3, :3] = _kitti_numbers(cam, "R_rect_00", 9).reshape(3, 3)
        S = _kitti_numbers(cam, f"S_rect_{left}", 2)
        if (S != np.round(S)).any():
            raise ValueError(f"from_kitti_raw: S_rect_{left} must be an integer size, got {S}")
        Tr = np.eye(4)
        Tr[:3, :3] = _kitti_numbers(velo, "R", 9).reshape(3, 3)
        Tr[:3, 3] = _kitti_numbers(velo, "T", 3)
        stereo = StereoCalib(Pl[0, 0], Pl[0, 3] / Pl[0, 0] - Pr[0, 3] / Pr[0, 0], Pl[0, 2], Pl[1, 2], Pr[0, 2] - Pl[0, 2])
        return cls(Pl @ R0 @ Tr, stereo, (int(S[1]), int(S[0])))


def read_velodyne(path) -> np.ndarray:
    """a KITTI `velodyne_points/data/*.bin` scan -> (N,4) float32 (x, y, z in metres, reflectance), the file as it is"""
    a = np.fromfile(path, dtype="<f4")
    if a.size % 4:
        raise ValueError(f"{path}: {a.size} floats are no whole number of (x, y, z, reflectance) records")
    return a.reshape(-1, 4)


def _lidar_scalars(name, err, calib, N, S, n, occl, min_depth, max_depth, min_disp, max_disp, outputs):
    """The scalar arguments of dca_lidar_disparity, checked as its launcher checks them (on the float32 values it is
    handed) -> (n, rx, ry, rel, fb, doffs, min_depth, max_depth, min_disp, max_disp) with the floats already rounded to
    float32 (rel stays a double: occl_scale = float32(1 + rel)); raises `err` otherwise."""
    if not isinstance(calib, LidarCalib):
        raise err(f"{name}: calib must be a geometry.LidarCalib, got {type(calib)}")
    n = N if n is None else int(n)
    if S < 3 or not 0 <= n <= N or n * S >= 1 << 31:
        raise err(f"{name}: expected (N,S) points with S >= 3, 0 <= n <= N and n * S below 2^31, got N = {N}, S = {S}, n = {n}")
    try:
        rx, ry, rel = int(occl[0]), int(occl[1]), float(occl[2])
        if len(occl) != 3 or rx != occl[0] or ry != occl[1]:
            raise ValueError
    except (TypeError, ValueError, IndexError):
        raise err(f"{name}: occl must be (rx, ry, rel) with integer radii, got {occl!r}") from None
    if not (0 <= rx <= LIDAR_MAX_RADIUS and 0 <= ry <= LIDAR_MAX_RADIUS):
        raise err(f"{name}: the radii of occl must lie in [0, {LIDAR_MAX_RADIUS}], got {rx} and {ry}")
    if not 0.0 <= rel < np.inf:
        raise err(f"{name}: rel of occl must be finite and >= 0, got {rel}")
    with np.errstate(over="ignore"):
        fb, doffs = float(np.float32(calib.stereo.fb)), float(np.float32(calib.stereo.doffs))
        min_depth, max_depth = float(np.float32(min_depth)), float(np.float32(max_depth))
        min_disp, max_disp = float(np.float32(min_disp)), float(np.float32(max_disp))
    if not (0.0 < fb < np.inf and np.isfinite(doffs)):
        raise err(f"{name}: the calibration needs a positive finite f * baseline and a finite doffs in float32")
    if not 0.0 < min_depth <= max_depth < np.inf:
        raise err(f"{name}: 0 < min_depth <= max_depth < inf in float32, got {min_depth} and {max_depth}")
    if not (np.isfinite(min_disp) and np.isfinite(max_disp) and min_disp <= max_disp):
        raise err(f"{name}: min_disp <= max_disp, both finite in float32, got {min_disp} and {max_disp}")
    outputs = tuple(outputs)
    if not outputs or len(set(outputs)) != len(outputs) or any(o not in LIDAR_OUTPUTS for o in outputs):
        raise err(f"{name}: outputs must be distinct names out of {LIDAR_OUTPUTS}, at least one, got {outputs!r}")
    return n, rx, ry, rel, fb, doffs, min_depth, max_depth, min_disp, max_disp, outputs


def lidar_disparity_host(points, calib: LidarCalib, n=None, occl=LIDAR_OCCL, min_depth=LIDAR_MIN_DEPTH,
                         max_depth=LIDAR_MAX_DEPTH, min_disp=LIDAR_MIN_DISP, max_disp=LIDAR_MAX_DISP, outputs=("disp",)):
    """numpy restatement of dca_lidar_disparity (include/dca_hip.h), float32 operation for float32 operation in the same
    order, with `np.minimum.at` as the z-buffer: points (N,S) float32, S >= 3, of which the leading n rows are read -> a
    dict with the keys of `outputs`: disp, depth float32 (H,W), disp_u16 uint16 (H,W), count int64 (2,) = (pixels written,
    points kept).  Equal to `ops.lidar_disparity` bit for bit."""
    points = np.asarray(points)
    if points.dtype != np.float32 or points.ndim != 2:
        raise ValueError(f"lidar_disparity_host: expected (N,S) float32 points, got {points.dtype} {points.shape}")
    n, rx, ry, rel, fb, doffs, min_depth, max_depth, min_disp, max_disp, outputs = _lidar_scalars(
        "lidar_disparity_host", ValueError, calib, points.shape[0], points.shape[1], n, occl, min_depth, max_depth, min_disp,
        max_disp, outputs)
    f32 = np.float32
    H, W = calib.hw
    m = calib.M
    X, Y, Z = (np.ascontiguousarray(points[:n, k]) for k in range(3))
    with np.errstate(all="ignore"):
        x, y, z = (((m[r, 0] * X + m[r, 1] * Y) + m[r, 2] * Z) + m[r, 3] for r in range(3))
        u, v = x / z, y / z
        uf, vf = np.floor(u + f32(0.5)), np.floor(v + f32(0.5))
        keep = (z >= f32(min_depth)) & (z <= f32(max_depth)) & (uf >= 0) & (uf < f32(W)) & (vf >= 0) & (vf < f32(H))
    zbuf = np.full(H * W, np.inf, f32)
    np.minimum.at(zbuf, vf[keep].astype(np.int64) * W + uf[keep].astype(np.int64), z[keep])
    zbuf = zbuf.reshape(H, W)
    pad = np.full((H + 2 * ry, W + 2 * rx), np.inf, f32)
    pad[ry:ry + H, rx:rx + W] = zbuf
    rowmin = pad[:, :W].copy()
    for k in range(1, 2 * rx + 1):
        np.minimum(rowmin, pad[:, k:k + W], out=rowmin)
    zmin = rowmin[:H].copy()
    for k in range(1, 2 * ry + 1):
        np.minimum(zmin, rowmin[k:k + H], out=zmin)
    with np.errstate(all="ignore"):
        d = f32(fb) / zbuf - f32(doffs)
        valid = np.isfinite(zbuf) & (zbuf <= zmin * f32(1.0 + rel)) & (d >= f32(min_disp)) & (d < f32(max_disp))
        q = d * f32(256.0) + f32(0.5)
    res = {}
    for key in outputs:
        if key == "disp":
            res[key] = np.where(valid, d, f32(0))
        elif key == "depth":
            res[key] = np.where(valid, zbuf, f32(0))
        elif key == "disp_u16":
            code = np.where(q >= 1, np.minimum(q, f32(65535)), f32(1))       # truncated below, saturated, at least 1
            res[key] = np.where(valid, code, f32(0)).astype(np.uint16)
        else:
            res[key] = np.array([int(valid.sum()), int(keep.sum())], np.int64)
    return res


class _LidarSlot:
    """one scan in flight: its pinned and device copies, its outputs and the two events that order them (training._Stage)"""

    def __init__(self, torch, device, capacity, S, hw, outputs):
        self.pin = torch.empty((capacity, S), dtype=torch.float32).pin_memory()
        self.dev = torch.empty((capacity, S), device=device, dtype=torch.float32)
        kinds = {"disp": (hw, torch.float32), "depth": (hw, torch.float32), "disp_u16": (hw, torch.uint16),
                 "count": ((2,), torch.int64)}
        self.out = {k: torch.empty(kinds[k][0], device=device, dtype=kinds[k][1]) for k in outputs}
        self.uploaded, self.computed = torch.cuda.Event(), torch.cuda.Event()
        self.n = 0


class LidarProjector:
    """`proj = LidarProjector(calib, "cuda"); maps = proj(read_velodyne(path))` -- `ops.lidar_disparity` behind a staging
    ring, as `TrainInput(device_io=True)` stages its samples: the scan is copied into a pinned buffer, uploaded on a copy
    stream, and the three launches are enqueued on the current stream behind the upload's event.  Everything is allocated
    here (`depth` slots of `capacity` points of `point_stride` floats, their outputs, one z-buffer): a call allocates
    nothing and waits for nothing but the upload that last left the slot's pinned buffer, `depth` scans ago.
    Returns the dict of `ops.lidar_disparity`; its maps are the slot's own and stay valid until `depth` more scans were
    projected.  `stream(scans)` yields the maps scan by scan with the upload of scan i + 1 enqueued before the kernels of
    scan i.  filters: occl, min_depth, max_depth, min_disp, max_disp and outputs of `ops.lidar_disparity`.  No queue
    setting is changed."""

    def __init__(self, calib, device="cuda", capacity=1 << 18, depth=2, point_stride=4, **filters):
        import torch
        unknown = set(filters) - {"occl", "min_depth", "max_depth", "min_disp", "max_disp", "outputs"}
        if unknown:
            raise ValueError(f"LidarProjector: unknown filters {sorted(unknown)}")
        self.capacity, self.depth, self.S = int(capacity), int(depth), int(point_stride)
        if self.capacity < 1 or self.depth < 1:
            raise ValueError("LidarProjector: capacity >= 1 and depth >= 1")
        outputs = filters.setdefault("outputs", ("disp",))
        _lidar_scalars("LidarProjector", ValueError, calib, self.capacity, self.S, 0, filters.get("occl", LIDAR_OCCL),
                       filters.get("min_depth", LIDAR_MIN_DEPTH), filters.get("max_depth", LIDAR_MAX_DEPTH),
                       filters.get("min_disp", LIDAR_MIN_DISP), filters.get("max_disp", LIDAR_MAX_DISP), outputs)
        self.calib, self.filters = calib, filters
        self.device = torch.device(device)
        self._ring = [_LidarSlot(torch, self.device, self.capacity, self.S, calib.hw, tuple(outputs)) for _ in range(self.depth)]
        self._zbuf = torch.empty(calib.hw[0] * calib.hw[1], device=self.device, dtype=torch.int32)
        self._copy = torch.cuda.Stream(self.device)
        self._copy.wait_stream(torch.cuda.current_stream(self.device))
        self._cur = 0

    def _upload(self, points):
        import torch
        points = np.asarray(points)
        if points.dtype != np.float32 or points.ndim != 2 or points.shape[1] != self.S:
            raise ValueError(f"LidarProjector: expected (n,{self.S}) float32 points, got {points.dtype} {points.shape}")
        n = points.shape[0]
        if n > self.capacity:
            raise ValueError(f"LidarProjector: a scan of {n} points exceeds the capacity of {self.capacity}")
        s = self._ring[self._cur]
        self._cur = (self._cur + 1) % self.depth
        s.uploaded.synchronize()                         # the previous copy out of the pinned buffer
        s.pin.numpy()[:n] = points
        s.n = n
        with torch.cuda.stream(self._copy):
            self._copy.wait_event(s.computed)            # the previous scan of this slot has been read
            s.dev[:n].copy_(s.pin[:n], non_blocking=True)
            s.uploaded.record(self._copy)
        return s

    def _project(self, s):
        import torch
        from . import ops
        compute = torch.cuda.current_stream(self.device)
        compute.wait_event(s.uploaded)
        with torch.cuda.device(self.device):
            res = ops.lidar_disparity(s.dev, self.calib, n=s.n, out=s.out, workspace=self._zbuf, **self.filters)
        s.computed.record(compute)
        return res

    def __call__(self, points):
        return self._project(self._upload(points))

    def stream(self, scans):
        """yields the maps of every scan in turn; with depth >= 2 the next scan's upload is enqueued first"""
        it = iter(scans)
        if self.depth < 2:
            for points in it:
                yield self(points)
            return
        try:
            cur = self._upload(next(it))
        except StopIteration:
            return
        for points in it:
            nxt = self._upload(points)
            yield self._project(cur)
            cur = nxt
        yield self._project(cur)


# ------------------------------------------------------------------------------------------------
# Camera poses of a drive, float64 on the host: what `temporal.reproject_matrix` takes is the pose of the
# previous rectified left camera in the current one, `relative_pose` of two world poses.
# ------------------------------------------------------------------------------------------------
EARTH_RADIUS = 6378137.0           # metres, the KITTI raw devkit's


def _pose44(T, name):
    T = np.asarray(T, np.float64)
    if T.shape == (3, 4):
        T = np.vstack([T, [0.0, 0.0, 0.0, 1.0]])
    if T.shape != (4, 4) or not np.isfinite(T).all():
        raise ValueError(f"{name}: a pose is a finite (4,4) or (3,4) array, got shape {T.shape}")
    return T


def _rigid_inv(T):
    """the inverse of a rigid motion [R t; 0 1]: [R' -R' t; 0 1]"""
    out = np.eye(4)
    out[:3, :3] = T[:3, :3].T
    out[:3, 3] = -T[:3, :3].T @ T[:3, 3]
    return out


def relative_pose(T_world_prev, T_world_cur) -> np.ndarray:
    """(4,4) float64 inv(T_world_cur) @ T_world_prev: the pose of the previous camera in the current one, from the two cameras'
    poses in one world (camera coordinates -> world coordinates, as KITTI's odometry poses are)"""
    return _rigid_inv(_pose44(T_world_cur, "relative_pose")) @ _pose44(T_world_prev, "relative_pose")


def read_kitti_poses(path, calib_text=None, camera: str = "P2") -> np.ndarray:
    """KITTI odometry `poses/XX.txt` (a path or the text): 12 numbers per line, the (3,4) pose of cam0 in the first frame's cam0
    -> (N,4,4) float64.  With `calib_text` (the sequence's calib.txt, a path or the text) the poses are moved to `camera`
    (default the left colour camera P2), which lies x = P[0,3] / P[0,0] beside cam0 along the rectified x axis:
    T' = S T inv(S) with S the translation by x; the first pose stays the identity."""
    poses = []
    for n, line in enumerate(_text(path).splitlines()):
        if not line.strip():
            continue
        try:
            vals = [float(v) for v in line.split()]
        except ValueError:
            raise ValueError(f"read_kitti_poses: line {n + 1} holds something that is not a number") from None
        if len(vals) != 12:
            raise ValueError(f"read_kitti_poses: line {n + 1} has {len(vals)} numbers, expected 12")
        poses.append(_pose44(np.array(vals).reshape(3, 4), "read_kitti_poses"))
    if not poses:
        raise ValueError("read_kitti_poses: no pose in the text")
    poses = np.stack(poses)
    if calib_text is not None:
        P = _kitti_numbers(_kitti_rows(calib_text), camera, 12).reshape(3, 4)
        if not P[0, 0] > 0:
            raise ValueError(f"read_kitti_poses: {camera} has no positive focal length")
        S, Si = np.eye(4), np.eye(4)
        S[0, 3] = P[0, 3] / P[0, 0]
        Si[0, 3] = -S[0, 3]
        poses = S @ poses @ Si
    return poses


def oxts_poses(rows, imu_to_velo, velo_to_cam, R_rect) -> np.ndarray:
    """The OXTS records of a KITTI raw drive -> (N,4,4) float64 poses of the rectified reference camera relative to its first
    frame, the raw devkit's construction restated: rows (N,>=6) = lat, lon (degrees), alt (metres), roll, pitch, yaw (radians),
    the leading columns of `oxts/data/*.txt`.  Mercator with scale = cos(lat_0 pi / 180) and the earth radius 6378137:
    x = scale lon pi r / 180, y = scale r log(tan((90 + lat) pi / 360)), z = alt;  R = Rz(yaw) Ry(pitch) Rx(roll);  the IMU's pose
    relative to its first one, then the chain C = [R_rect 0; 0 1] velo_to_cam imu_to_velo into the rectified camera:
    T_i = C inv(P_0) P_i inv(C).  imu_to_velo, velo_to_cam: (4,4) or (3,4); R_rect: (3,3) (R_rect_00)."""
    rows = np.asarray(rows, np.float64)
    if rows.ndim != 2 or rows.shape[0] < 1 or rows.shape[1] < 6 or not np.isfinite(rows[:, :6]).all():
        raise ValueError(f"oxts_poses: rows must be a finite (N,>=6) array, got shape {rows.shape}")
    R_rect = np.asarray(R_rect, np.float64)
    if R_rect.shape != (3, 3) or not np.isfinite(R_rect).all():
        raise ValueError(f"oxts_poses: R_rect must be a finite (3,3) array, got shape {R_rect.shape}")
    R0 = np.eye(4)
    R0[:3, :3] = R_rect
    C = R0 @ _pose44(velo_to_cam, "oxts_poses") @ _pose44(imu_to_velo, "oxts_poses")
    Ci = np.linalg.inv(C)
    scale = np.cos(rows[0, 0] * np.pi / 180.0)
    out = np.empty((rows.shape[0], 4, 4))
    P0i = t0 = None
    for i, (lat, lon, alt, roll, pitch, yaw) in enumerate(rows[:, :6]):
        P = np.eye(4)
        t = np.array([scale * lon * np.pi * EARTH_RADIUS / 180.0,
                      scale * EARTH_RADIUS * np.log(np.tan((90.0 + lat) * np.pi / 360.0)), alt])
        t0 = t if t0 is None else t0
        P[:3, 3] = t - t0              # (the first position is taken off before anything is rotated: no large numbers cancel)
        cr, sr, cp, sp, cy, sy = np.cos(roll), np.sin(roll), np.cos(pitch), np.sin(pitch), np.cos(yaw), np.sin(yaw)
        Rx = np.array([[1, 0, 0], [0, cr, -sr], [0, sr, cr]])
        Ry = np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]])
        Rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1]])
        P[:3, :3] = Rz @ Ry @ Rx
        if P0i is None:
            P0i = _rigid_inv(P)
        out[i] = C @ P0i @ P @ Ci
    return out
