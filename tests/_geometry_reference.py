"""numpy float32 restatement of `dca_disp_to_depth` and `dca_point_cloud` (include/dca_hip.h), operation for operation, and
a constructive scene that reaches every way a pixel can be rejected -- no seeded luck.  Shared by tests/test_geometry_cpu.py
(which checks that the scene really populates every category on every shape the GPU test uses) and
tests/test_gpu_geometry.py (which compares the kernels with it bit for bit).

Why the comparison is bitwise: every operation of the formulas is ONE IEEE fp32 operation (add, subtract, multiply, divide,
int -> float of a small integer), rounded on its own on both sides; numpy's float32 array arithmetic does exactly that, and
the kernels are compiled without contraction and with IEEE division."""
import collections

import numpy as np

F = np.float32
TILE = 1024                  # DCA_PC_TILE; tests/test_geometry_cpu.py checks it against the header
VERTEX = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1"), ("alpha", "u1")])
REASONS = ("nan", "min_disp", "den", "z_not_positive", "max_depth", "mask", "stride", "kept")

Calib = collections.namedtuple("Calib", "f fb cx cy doffs")

# the scene's calibration: KITTI-like numbers that are NOT exact in fp32, and the issue's doffs = -2
_F, _B = 721.5377, 0.5327
CALIB = Calib(_F, float(F(np.float64(_F) * np.float64(_B))), 609.5593, 172.854, -2.0)
MIN_DISP = 0.5
MASK_MIN = 0.5
# Z == max_depth exactly at d = 10 (den = 8): `<=` keeps it, and d = 10 - 1/16 is the nearest rejected neighbour
MAX_DEPTH = float(F(CALIB.fb) / F(8.0))

# the windows of the bitwise GPU test: (rows, cols); 32 x 32 = TILE pixels, 25 x 41 = TILE + 1
SHAPES = ((1, 1), (3, 7), (5, 67), (4, 301), (9, 1301), (32, 32), (25, 41))
assert 32 * 32 == TILE and 25 * 41 == TILE + 1
Y0, V0 = 3, 5                # frame row / image row of window row 0


def scene(rows, cols, y0=Y0, v0=V0, channels=3):
    """(pred, mask, rgb) for a rows x cols window at frame row y0: pred, mask (rows + y0 + 2, cols + 3) float32, rgb
    (v0 + rows + 1, cols + 2, channels) uint8.  The category of window pixel i = r cols + c is i % 8:
      0 NaN   1 d < min_disp (0.25, 0, -3 in turn)   2 den <= 0 with d >= min_disp (1.5: den -0.5; 2.0: den 0)
      3 Z > max_depth (2.5, or 10 - 1/16: one step beyond the bound)   4 masked out (mask 0.25, or NaN)   5 d = +inf
      6 kept, d = 10 (Z == max_depth exactly) or 10 + k/16   7 kept, mask == mask_min exactly, d = 12 + k/8
    Everything outside the window would be KEPT (d = 16, mask 1): a kernel that reads the wrong rows shows up."""
    Hc, Wc = rows + y0 + 2, cols + 3
    pred = np.full((Hc, Wc), 16.0, F)
    mask = np.ones((Hc, Wc), F)
    i = np.arange(rows * cols)
    k = i // 8
    cat = i % 8
    d = np.empty(rows * cols, F)
    m = np.ones(rows * cols, F)
    d[cat == 0] = np.nan
    d[cat == 1] = np.choose(k[cat == 1] % 3, [0.25, 0.0, -3.0])
    d[cat == 2] = np.choose(k[cat == 2] % 2, [1.5, 2.0])
    d[cat == 3] = np.choose(k[cat == 3] % 2, [2.5, 10.0 - 1.0 / 16])
    d[cat == 4] = 20.0 + (k[cat == 4] % 64) / 4.0
    m[cat == 4] = np.choose(k[cat == 4] % 2, [0.25, np.nan])
    d[cat == 5] = np.inf
    d[cat == 6] = 10.0 + (k[cat == 6] % 5 != 0) * ((k[cat == 6] * 37) % 1000) / 16.0
    d[cat == 7] = 12.0 + ((k[cat == 7] * 53) % 500) / 8.0
    m[cat == 7] = MASK_MIN
    pred[y0:y0 + rows, :cols] = d.reshape(rows, cols)
    mask[y0:y0 + rows, :cols] = m.reshape(rows, cols)
    H, W = v0 + rows + 1, cols + 2
    y, x, ch = np.meshgrid(np.arange(H), np.arange(W), np.arange(channels), indexing="ij")
    rgb = ((y * 31 + x * 7 + ch * 101 + 13) % 256).astype(np.uint8)
    if channels == 4:
        rgb[..., 3] = 7          # a fourth channel is ignored: alpha is 255 in every record
    return pred, mask, rgb


def geometry_reference(pred, calib, window=None, v0=0, stride=1, mask=None, mask_min=MASK_MIN, min_disp=MIN_DISP,
                       max_depth=MAX_DEPTH, rgb=None, scale=256.0):
    """dict of: `depth` (rows,cols) float32 and `depth_u16` (stride 1, as dca_disp_to_depth), `keep` (rows,cols) bool,
    `vertices` (VERTEX records of ALL kept pixels in row-major order), `count` (their number), `tile_offsets`
    (tiles + 1 int32) and `reasons`: REASONS -> pixels, each counted under the first condition it fails."""
    pred = np.asarray(pred, F)
    Hc, Wc = pred.shape
    y0, rows, cols = (0, Hc, Wc) if window is None else window
    d = pred[y0:y0 + rows, :cols]
    f, fb, cx, cy, doffs = (F(v) for v in (calib.f, calib.fb, calib.cx, calib.cy, calib.doffs))
    with np.errstate(all="ignore"):
        den = d + doffs
        Z = fb / den
        u = np.arange(cols).astype(F)[None, :]
        v = (v0 + np.arange(rows)).astype(F)[:, None]
        X = ((u - cx) * Z) / f
        Y = ((v - cy) * Z) / f
        tests = [("nan", ~np.isnan(d)), ("min_disp", d >= F(min_disp)), ("den", den > 0), ("z_not_positive", Z > 0),
                 ("max_depth", Z <= F(max_depth))]
        if mask is not None:
            tests.append(("mask", np.asarray(mask, F)[y0:y0 + rows, :cols] >= F(mask_min)))
        dense = np.ones((rows, cols), bool)
        reasons = dict.fromkeys(REASONS, 0)
        for name, ok in tests:
            reasons[name] = int((dense & ~ok).sum())
            dense &= ok
        on_grid = (np.arange(rows) % stride == 0)[:, None] & (np.arange(cols) % stride == 0)[None, :]
        keep = dense & on_grid
        reasons["stride"], reasons["kept"] = int((dense & ~on_grid).sum()), int(keep.sum())
        depth = np.where(dense, Z, F(0)).astype(F)
        prod = depth * F(scale)
        u16 = np.where(prod > 0, np.where(prod >= F(65535), F(65535), np.trunc(prod)), F(0)).astype(np.uint16)
    vert = np.zeros(int(keep.sum()), VERTEX)
    vert["x"], vert["y"], vert["z"] = X[keep], np.broadcast_to(Y, keep.shape)[keep], Z[keep]
    vert["alpha"] = 255
    if rgb is None:
        vert["red"] = vert["green"] = vert["blue"] = 255
    else:
        colours = np.asarray(rgb)[v0:v0 + rows, :cols]
        for j, name in enumerate(("red", "green", "blue")):
            vert[name] = colours[..., j][keep]
    flat = keep.reshape(-1)
    tiles = -(-flat.size // TILE)
    before = np.concatenate([[0], np.cumsum(flat)])
    offsets = before[np.minimum(np.arange(tiles + 1) * TILE, flat.size)].astype(np.int32)
    return dict(depth=depth, depth_u16=u16, keep=keep, vertices=vert, count=int(keep.sum()), tile_offsets=offsets,
                reasons=reasons)
