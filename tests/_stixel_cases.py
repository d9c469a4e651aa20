"""Synthetic scenes for the stixel operator (dcanet_amd/stixel.py, csrc/stixel.hip), shared by test_stixel_cpu.py and
test_gpu_stixel.py, all generated from a seed.

`column_scene` is the 60-cell column with a known answer: a road of 40 - 0.8 k px, a wall at the road's depth over the cells
20..35, the road again over 36..39, a second wall over 40..48, sky at 0.3 px above it, 0.25 px Gaussian noise, 5 % of the cells
without a measurement.  `map_scene` is the same column as a full-resolution map, to go through the cell median.

`cases()` are the device cases, the smallest shapes at which each mechanism of the kernels can break: the dynamic programme
shares the candidates kb among the 64 lanes of ONE wave, so 2, 63, 64, 65 cells (below, at and above one pass), 128, 129, 130
(two passes), 200 (four) and 1024 (the limit: sixteen passes and the largest LDS footprint); widths 1, 5 and 16 with cols % width != 0; row_step 2 with rows % row_step != 0; a window at
y0 = 5 in a larger frame that holds plausible disparities around it; a mask; a batch of two planes; NaN, +-inf, 0, negative
and >= max_disp; a record of status 1 and one without a calibration; a column without a valid cell and one with a single one;
lists shorter than the segmentation (max_segments 1 and 2); min_valid above 1; constants other than the defaults."""
import collections
import functools

import numpy as np

Case = collections.namedtuple("Case", "name d plane mask kw")
TRUTH = ((0, 19, 0), (20, 35, 1), (36, 39, 0), (40, 48, 1), (49, 59, 2))      # (kb, kt, class) of column_scene, bottom-up


def road_px(k):
    return 40.0 - 0.8 * np.asarray(k, np.float64)


def column_scene(seed):
    """(q, g) int64 (60,): the cells' disparities in sixteenths (-1: none) and the road's, bottom-up"""
    rng = np.random.default_rng(seed)
    k = np.arange(60)
    d = road_px(k)
    d[20:36], d[40:49], d[49:] = road_px(20), road_px(40), 0.3
    d = d + rng.normal(0.0, 0.25, 60)
    q = np.where(rng.random(60) < 0.05, -1, np.maximum(np.floor(d * 16 + 0.5), 0)).astype(np.int64)
    return q, np.floor(road_px(k) * 16 + 0.5).astype(np.int64)


def record(rows, cols, a, b, c, status=0.0, hs=1.5):
    """a plane record as `ground_plane` leaves it, reduced to what the stixel operator reads"""
    rec = np.zeros(16, np.float64)
    rec[0:3], rec[5], rec[9], rec[13], rec[14] = (a, b, c), status, hs, cols // 2, rows // 2
    return rec


def map_scene(seed, width, row_step, columns=4, spare_cols=2):
    """column_scene as a map: (d float32 (rows,cols), record).  rows = 60 row_step + (row_step - 1) rows at the top that no cell
    covers, cols = columns width + spare_cols; the road is the plane that has 40 - 0.8 k px at the centre row of cell k; noise per
    pixel, 5 % of the pixels 0.0 (no measurement)."""
    rng = np.random.default_rng(seed)
    rows, cols = 60 * row_step + row_step - 1, columns * width + spare_cols
    b = 0.8 / row_step
    centre0 = rows - row_step + row_step // 2                     # the centre row of cell 0
    c = 40.0 + b * (rows // 2 - centre0)                           # p(row) = b (row - rows // 2) + c = 40 at centre0
    row = np.arange(rows, dtype=np.float64)
    p = b * (row - rows // 2) + c
    k = (rows - 1 - row) // row_step                               # the cell of a row (>= 60 in the spare rows)
    col = np.where((k >= 20) & (k <= 35), road_px(20), np.where((k >= 40) & (k <= 48), road_px(40), np.where(k >= 49, 0.3, p)))
    d = col[:, None] + rng.normal(0.0, 0.25, (rows, cols))
    d[rng.random((rows, cols)) < 0.05] = 0.0
    return d.astype(np.float32), record(rows, cols, 0.0, b, c)


def _specials(d, rng, max_disp, n=3):
    for v in (np.nan, np.inf, -np.inf, 0.0, -3.0, float(max_disp), max_disp - 0.01, max_disp - 0.04, 1e30, 0.0625, 0.06):
        for _ in range(n):
            d[tuple(rng.integers(0, s) for s in d.shape)] = v
    return d


def random_scene(rows, cols, seed, max_disp=64, specials=True, roll=0.004):
    """(d, record): a road with roll under a sky, per column block of 3 pixels up to two walls standing on it or hanging over
    it, noise, holes; every class, contact penalty and truncation occurs somewhere"""
    rng = np.random.default_rng(seed)
    b = (max_disp * 0.6) / rows
    c = b * (rows // 2 - rows * 0.3)                               # the horizon at 30 % of the window
    u = np.arange(cols, dtype=np.float64)[None, :] - cols // 2
    v = np.arange(rows, dtype=np.float64)[:, None] - rows // 2
    p = roll * u + b * v + c
    d = np.where(p >= 0.2, p, 0.15)
    for c0 in range(0, cols, 3):
        for _ in range(int(rng.integers(0, 3))):
            foot = int(rng.integers(rows // 3, rows))
            top = max(0, foot - int(rng.integers(1, max(2, rows // 2))))
            lift = float(rng.choice([0.0, 0.0, 2.5, -2.5]))         # on the road, in front of it, behind it
            d[top:foot + 1, c0:c0 + 3] = max(p[foot, min(c0 + 1, cols - 1)], 0.0) + lift
    d = d + rng.normal(0.0, 0.2, d.shape)
    d[rng.random(d.shape) < 0.08] = 0.0
    d = d.astype(np.float32)
    if specials:
        _specials(d, rng, max_disp)
    return d, record(rows, cols, roll, b, c)


@functools.lru_cache(maxsize=None)
def cases():
    out = []

    def add(name, rows, cols, seed, plane=None, mask=None, d=None, **kw):
        dd, rec = random_scene(rows, cols, seed, kw.get("max_disp", 64))
        out.append(Case(name, dd if d is None else d, rec if plane is None else plane, mask, kw))

    add("H=2 width 1", 2, 3, 1, width=1, max_disp=64)
    add("H=63 width 5, cols % 5 = 2", 63, 17, 2, width=5, max_disp=64)
    add("H=64 width 16, cols % 16 = 3", 64, 35, 3, width=16, max_disp=64)
    add("H=65 row_step 2, rows % 2 = 1", 131, 11, 4, width=5, row_step=2, max_disp=64)
    add("H=128 width 2", 128, 7, 5, width=2, max_disp=64)
    add("H=129 width 3, max_segments 2", 129, 7, 6, width=3, max_disp=64, max_segments=2)
    add("H=130 width 4, max_disp 1024", 130, 9, 7, width=4, max_disp=1024)
    add("H=200 width 2, row_step 1", 200, 5, 8, width=2, max_disp=64)
    add("H=1024 width 2: the largest column, 63.5 KB of LDS", 1024, 3, 16, width=2, max_disp=64)
    add("H=16 row_step 8 width 16: cells of 128 pixels, min_valid 40", 130, 33, 9, width=16, row_step=8, max_disp=64, min_valid=40)
    add("max_segments 1", 48, 10, 10, width=5, max_disp=64, max_segments=1)
    add("other constants: ground on ground, a dear first object, no far", 70, 12, 11, width=3, max_disp=64,
        params=dict(Tg=300, Ts=50, eps=4, below=77, float=1 << 20, mu_min=0, far=0, seg=(10, 20, 30), first=(5, 4000, 0),
                    T=((7, 0, 3), (0, 11, 0), (-1, 900, -1))))
    # a window at y0 = 5 of a larger frame with plausible disparities around it, a mask, a batch of two planes
    rng = np.random.default_rng(12)
    frames, recs = [], []
    for i in range(2):
        win, rec = random_scene(66, 33, 20 + i, 64, roll=0.004 - 0.01 * i)
        frame = (20.0 + 5.0 * rng.random((80, 40))).astype(np.float32)
        frame[5:71, :33] = win
        frames.append(frame), recs.append(rec)
    mask = (rng.random((2, 80, 40)) * 1.2).astype(np.float32)
    out.append(Case("batch 2: window 66x33 at y0 = 5 of 80x40, mask, two planes", np.stack(frames), np.stack(recs), mask,
                    dict(width=5, row_step=1, max_disp=64, window=(5, 66, 33), mask_min=0.3)))
    # records without a segmentation: status 1, no calibration; beside a good one
    d, rec = random_scene(40, 12, 13)
    out.append(Case("batch 3: status 1 | no camera height | status 2", np.stack([d, d, d]),
                    np.stack([record(40, 12, *rec[0:3], status=1.0), record(40, 12, *rec[0:3], hs=0.0), record(40, 12, *rec[0:3], status=2.0)]),
                    None, dict(width=4, max_disp=64)))
    # column 0 without a valid cell, column 1 with a single valid pixel, column 2 whole
    d, rec = random_scene(50, 9, 14, specials=False)
    d[:, 0:3] = 0.0
    d[:, 3:6] = np.nan
    d[31, 4] = 7.25
    out.append(Case("no valid cell | a single valid cell | a column", d, rec, None, dict(width=3, max_disp=64)))
    # a plane of NaN and infinities: g is clamped, nothing overflows
    d, rec = random_scene(40, 8, 15)
    out.append(Case("batch 2: a NaN plane | an infinite plane", np.stack([d, d]),
                    np.stack([record(40, 8, np.nan, 0.5, 1.0), record(40, 8, 0.0, np.inf, -1e300)]), None, dict(width=2, max_disp=64)))
    return tuple(out)
