"""Seeded stereo pairs for semi-global matching (dcanet_amd/sgm.py, csrc/sgm.hip), shared by test_sgm_cpu.py and
test_gpu_sgm.py; every array is read-only.  Each case is the smallest shape at which one thing can go wrong:

  tiny        9 x 20, D = 8        the image barely larger than the 9 x 7 census window; W < 64
  plane       23 x 67, D = 24, C=3 random texture, right = left shifted by PLANE_D = 9; D no multiple of the 64 lanes
  narrow      16 x 48, D = 64      W < D: most bins out of view
  two_planes  40 x 150, D = 80     a foreground square at d = 14 on a background at d = 4, with its occlusion band; 64 < D < 128;
                                   with 4 and with 8 paths
  wide_d      33 x 130, D = 192, C=4  three bins per lane, W < D, the alpha channel ignored
  max_d       12 x 300, D = 256    the largest D, grey input, W beyond one census tile and beyond D
  tall        70 x 33, D = 16      vertical and diagonal scans longer than a census tile is high; W < 64
  flat        10 x 40, D = 16      a constant image: every cost ties, the lowest index wins, den = 0
  extremes    12 x 40, D = 24      (P1, P2) = (1, 1) and (4095, 4095), u = 0 and 99, min_disp 0 and 5: the uint16 bound of S
                                   and the integer tests

`expected(name)` is the restatement's result with every output and the census, computed once per process."""
import collections
import functools

import numpy as np

Case = collections.namedtuple("Case", "name left right kw")
SEED = 0
PLANE_D = 9
FG_D, BG_D = 14, 4                                  # two_planes
FG_BOX = (10, 30, 60, 100)                          # rows [10, 30), columns [60, 100) of the LEFT image


def _ro(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def shifted_pair(rng, H, W, d, C=None, noise=0):
    """random texture: right(y, x - d) = left(y, x); what enters the right image from beyond the left one is random too"""
    shape = (H, W + d) if C is None else (H, W + d, C)
    wide = rng.integers(0, 256, shape, dtype=np.uint8)
    left, right = wide[:, :W].copy(), wide[:, d:].copy()
    if noise:
        right = np.clip(right.astype(np.int64) + rng.integers(-noise, noise + 1, right.shape), 0, 255).astype(np.uint8)
    return left, right


def two_planes_pair(rng, H=40, W=150):
    """(left, right, disparity of the left image, occluded): the square of FG_BOX at FG_D in front of a plane at BG_D, each with
    a texture of its own; `occluded` marks the left pixels whose point the square hides in the right image or that lie left of it"""
    y0, y1, x0, x1 = FG_BOX
    back = rng.integers(0, 256, (H, W + BG_D), dtype=np.uint8)          # in right-image columns, BG_D spare ones on the left
    fore = rng.integers(0, 256, (H, W), dtype=np.uint8)                 # in left-image columns
    left = back[:, :W].copy()                                           # left(x) = back(x - BG_D + BG_D)
    right = back[:, BG_D:].copy()                                       # right(x) = back(x + BG_D) = left(x + BG_D)
    left[y0:y1, x0:x1] = fore[y0:y1, x0:x1]
    right[y0:y1, x0 - FG_D:x1 - FG_D] = fore[y0:y1, x0:x1]
    disp = np.full((H, W), BG_D, np.int64)
    disp[y0:y1, x0:x1] = FG_D
    occluded = np.zeros((H, W), bool)
    occluded[:, :BG_D] = True
    xr = np.arange(W) - BG_D                                            # where a background pixel lies in the right image
    occluded[y0:y1] |= ((xr >= x0 - FG_D) & (xr < x1 - FG_D))[None, :]
    occluded[y0:y1, x0:x1] = False
    return left, right, disp, occluded


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    rng = lambda: np.random.default_rng(SEED)           # every case from the seed itself: none depends on the ones before it

    def add(name, left, right, **kw):
        out.append(Case(name, _ro(left), _ro(right), kw))

    add("tiny", *shifted_pair(rng(), 9, 20, 2), max_disp=8)
    add("plane", *shifted_pair(rng(), 23, 67, PLANE_D, 3), max_disp=24)
    add("narrow", *shifted_pair(rng(), 16, 48, 5, noise=3), max_disp=64)
    l, r, _, _ = two_planes_pair(rng())
    add("two_planes-8", l, r, max_disp=80, paths=8)
    add("two_planes-4", l, r, max_disp=80, paths=4)
    add("wide_d", *shifted_pair(rng(), 33, 130, 20, 4, noise=2), max_disp=192)
    add("max_d", *shifted_pair(rng(), 12, 300, 100, noise=2), max_disp=256)
    add("tall", *shifted_pair(rng(), 70, 33, 3, noise=4), max_disp=16, paths=8)
    flat = np.full((10, 40), 97, np.uint8)
    add("flat", flat, flat, max_disp=16)
    l, r = shifted_pair(rng(), 12, 40, 6, noise=8)
    for P, u, md in ((1, 0, 0), (4095, 99, 5), (1, 99, 5), (4095, 0, 0)):
        add(f"extremes-P{P}-u{u}-min{md}", l, r, max_disp=24, P1=P, P2=P, uniqueness=u, min_disp=md)
    return tuple(out)


def case(name):
    return next(c for c in cases() if c.name == name)


def names():
    return [c.name for c in cases()]


@functools.lru_cache(maxsize=None)
def expected(name):
    """{output: array} of `sgm_host` with every output, plus "census" (2,H,W) uint64, read-only"""
    from dcanet_amd import sgm
    c = case(name)
    res = sgm.sgm_host(c.left, c.right, outputs=sgm.SGM_OUTPUTS, **c.kw)
    res["census"] = np.stack([sgm.census_host(c.left), sgm.census_host(c.right)])
    return {k: _ro(v) for k, v in res.items()}
