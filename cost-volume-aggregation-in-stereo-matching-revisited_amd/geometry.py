"""Stereo calibration and the exporters of the geometry stage: `StereoCalib` holds what
`ops.disp_to_depth` and `ops.point_cloud` need to turn a disparity in pixels into metres, read from a KITTI or a
Middlebury calibration file; `write_ply` / `read_ply` store the compacted vertex buffer as it is -- the device buffer IS
the body of a binary PLY file -- and `depth_png` writes the KITTI 16-bit depth format.  Host code only: no arithmetic on
the maps happens here."""
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
