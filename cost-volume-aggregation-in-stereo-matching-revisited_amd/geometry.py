"""Stereo calibration and the exporters of the geometry stage: `StereoCalib` holds what
`ops.disp_to_depth` and `ops.point_cloud` need to turn a disparity in pixels into metres, read from a KITTI or a
Middlebury calibration file; `write_ply` / `read_ply` store the compacted vertex buffer as it is -- the device buffer IS
the body of a binary PLY file -- and `depth_png` writes the KITTI 16-bit depth format.  Host code only: no arithmetic on
the maps happens here.

`RectifyMaps` holds the fixed-point maps that rectify a RAW stereo pair, built once per calibration in
float64; `ops.rectify_pair` applies them on the device and `rectify_pair_host` is the numpy restatement of that kernel."""
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
