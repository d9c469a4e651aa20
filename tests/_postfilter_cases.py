"""Inputs of the post-filter tests (tests/test_postfilter_cpu.py, tests/test_gpu_postfilter.py): small maps on which the
speckle filter and the median can go wrong -- more than one tile in both directions, partial tiles, components that
cross every tile edge, the `>` and `<=` boundaries, values that are no numbers -- each with what is known about it in
closed form.  Sizes are derived from the kernels' tile, read from the header.  Everything is generated once and never
modified."""
import collections
import functools

import numpy as np

from dcanet_amd import _lib
from dcanet_amd.postfilter import speckle_filter_host

TH, TW = _lib.CONSTANTS["DCA_SPK_TILE_H"], _lib.CONSTANTS["DCA_SPK_TILE_W"]

# d, mask: (Hc,Wc) float32 (mask may be None); window: (y0, rows, cols) or None; sizes: the closed form, a dict
# {component size: number of components} over the ACTIVE pixels of the window, or None where there is none
Case = collections.namedtuple("Case", "name d mask window max_size max_diff sizes")


def _planes(H, W, x_split, y0=0):
    y, x = np.mgrid[-y0:H - y0, 0:W].astype(np.float32)
    return (np.float32(20) + np.float32(0.05) * x + np.float32(0.02) * y + np.where(x >= x_split, np.float32(7.3), 0)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def scene(H, W, seed):
    """(d, mask): two slanted planes 20 + 0.05 x + 0.02 y, the right half 7.3 nearer; a 9 x 20 object at 55.5; a 3 x 4 speckle
    at 3.25; 3 % of the pixels raised by U(3, 30) (salt); 2 % masked out.  With max_diff = 1 the planes and the object are
    large components, the speckle is one of 12 pixels, the salt is single pixels: max_size = 50 removes some and keeps most."""
    rng = np.random.default_rng(seed)
    d = _planes(H, W, W // 2)
    if H >= 20 and W >= 40:
        oy, ox = H // 4, W // 8
        d[oy:oy + 9, ox:ox + 20] = 55.5
        sy, sx = H // 2 + 3, W // 2 + 9
        d[sy:sy + 3, sx:sx + 4] = 3.25
    salt = rng.random((H, W)) < 0.03
    d[salt] += rng.uniform(3, 30, int(salt.sum())).astype(np.float32)
    mask = (rng.random((H, W)) >= 0.02).astype(np.float32)
    d.setflags(write=False)
    mask.setflags(write=False)
    if H >= 20 and W >= 40:
        ref = speckle_filter_host(d, 50, 1.0, mask=mask)
        active = mask >= 0.5
        assert (ref["valid"] == 1).any() and (active & (ref["valid"] == 0)).any(), "scene: both classes must occur"
    return d, mask


def _snake(masked):
    H, W = 2 * TH + 3, 2 * TW + 5
    d = np.full((H, W), 50, np.float32)
    d[0::2] = 10
    d[1::4, W - 1] = 10                                    # rows 1, 5, 9 ...: joined at the right end
    d[3::4, 0] = 10                                        # rows 3, 7, 11 ...: at the left end
    even, odd = (H + 1) // 2, H // 2
    snake = even * W + (even - 1)                          # every even row and one pixel between two of them
    sizes = {snake: 1}
    mask = None
    if masked:
        mask = (d == 10).astype(np.float32)
    else:
        sizes[W - 1] = odd                                 # what is left of every odd row, cut off from the others
    return Case("snake, rest masked" if masked else "snake", d, mask, None, snake - 1, 1.0, sizes)


def _specials():
    """columns of NaN, +inf and -inf between regions of ONE value (each would bridge two components if it were a number
    that joins), and a column of -0.0 inside a region at 0.25, which IS a finite value and active"""
    H, W = 5, TW + 8
    d = np.full((H, W), 5, np.float32)
    d[:, 10], d[:, 30], d[:, 50] = np.nan, np.inf, -np.inf
    d[:, 60:] = 0.25
    d[:, TW + 2] = -0.0
    return Case("specials", d, None, None, 0, 1.0, {H * 10: 1, H * 19: 2, H * 9: 1, H * (W - 60): 1})


def _window():
    """the 37 x 83 scene at row 5 of a 48 x 96 frame whose padding continues the planes: a neighbour read outside the window
    would enlarge the components at its border"""
    d, mask = scene(37, 83, 1)
    frame = _planes(48, 96, 83 // 2, y0=5)                 # in the window's own coordinates: the padding joins its border
    frame[5:42, :83] = d
    fmask = np.ones((48, 96), np.float32)
    fmask[5:42, :83] = mask
    return Case("window", frame, fmask, (5, 37, 83), 50, 1.0, None)


@functools.lru_cache(maxsize=None)
def speckle_cases():
    rng = np.random.default_rng(5)
    cases = []
    for H, W in ((37, 83), (70, 150)):
        d, mask = scene(H, W, 1)
        cases.append(Case(f"scene {H}x{W}", d, mask, None, 50, 1.0, None))
    cases += [_snake(False), _snake(True)]
    H, W = 3 * TH, 3 * TW + 1
    const = np.full((H, W), 7.5, np.float32)
    cases.append(Case("constant, kept", const, None, None, H * W - 1, 0.0, {H * W: 1}))
    cases.append(Case("constant, removed", const, None, None, H * W, 0.0, {H * W: 1}))
    H, W = TH + 1, TW + 3
    y, x = np.mgrid[0:H, 0:W]
    board = np.where((x + y) % 2 == 0, 0, 10).astype(np.float32)
    cases.append(Case("checkerboard, identity", board, None, None, 0, 1.0, {1: H * W}))
    cases.append(Case("checkerboard, removed", board, None, None, 1, 1.0, {1: H * W}))
    H, W = TH + 3, 2 * TW + 2
    x = np.broadcast_to(np.arange(W, dtype=np.float32), (H, W))
    cases.append(Case("ramp 0.75, chained", (np.float32(0.75) * x).astype(np.float32), None, None, 50, 1.0, {H * W: 1}))
    cases.append(Case("ramp 1.25, columns", (np.float32(1.25) * x).astype(np.float32), None, None, H - 1, 1.0, {H: W}))
    cases.append(Case("ramp 0.5, equality", (np.float32(0.5) * x).astype(np.float32), None, None, 50, 0.5, {H * W: 1}))
    cases.append(_specials())
    cases.append(_window())
    for H, W in ((5, 7), (1, 1), (1, TW + 1), (TH + 1, 1)):
        d = rng.integers(0, 4, (H, W)).astype(np.float32)
        cases.append(Case(f"tiny {H}x{W}", d, None, None, 1, 1.0, None))
    for c in cases:
        c.d.setflags(write=False)
    return tuple(cases)


def _median_special():
    """5 x 7: a centre whose neighbours are all inactive, neighbourhoods with an even number of candidates, both zeros"""
    d = np.array([[1, 2, np.nan, np.nan, np.nan, 4, 5],
                  [3, np.inf, np.nan, 9, np.nan, -0.0, 0.0],
                  [6, 7, np.nan, np.nan, np.nan, 0.0, -0.0],
                  [-1, -2, 8, -np.inf, 2.5, -0.0, 0.0],
                  [0.0, -0.0, 1.5, 3.5, -3, 0.0, -0.0]], np.float32)
    return d


@functools.lru_cache(maxsize=None)
def median_cases():
    """(name, d, mask, window)"""
    rng = np.random.default_rng(9)
    cases = [("special 5x7", _median_special(), None, None)]
    d, mask = scene(5, 7, 3)
    cases.append(("scene 5x7", d, None, None))
    noisy = (rng.random((5, 7)) >= 0.4).astype(np.float32)
    cases.append(("scene 5x7, masked", d, noisy, None))
    d, mask = scene(37, 83, 1)
    cases.append(("scene 37x83", d, None, None))
    cases.append(("scene 37x83, masked", d, mask, None))
    w = _window()
    cases.append(("window", w.d, None, w.window))
    cases.append(("window, masked", w.d, w.mask, w.window))
    d = rng.integers(-2, 3, (TH + 2, 2 * TW + 3)).astype(np.float32) * np.float32(0.0)      # zeros of both signs
    cases.append(("zeros of both signs", d, None, None))
    for c in cases:
        c[1].setflags(write=False)
    return tuple(cases)


def flipped(a):
    """the second image of the B = 2 tests: the first one mirrored, so a component leaking across images is caught"""
    return None if a is None else np.ascontiguousarray(np.stack([a, a[:, ::-1]]))


def component_census(size, active):
    """{component size: number of components} from a size map: a component of s pixels contributes s pixels of size s"""
    sizes, counts = np.unique(size[active], return_counts=True)
    assert (counts % sizes == 0).all()
    return {int(s): int(c // s) for s, c in zip(sizes, counts)}
