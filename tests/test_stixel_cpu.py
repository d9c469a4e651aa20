"""CPU checks of the stixel operator: the numpy restatement of dcanet_amd/stixel.py against a brute force over every
segmentation and labelling, against the TRUTH of a synthetic column (tests/_stixel_cases.py) and against closed forms, the
operator's refusals, the library's symbol, and the host check of csrc/stixel_math.h under sanitizers.  The kernels are compared
with the restatement, bit for bit, in test_gpu_stixel.py."""
import ctypes
import itertools
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import _stixel_cases as C
from dcanet_amd import ground as G
from dcanet_amd import stixel as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def energy_of(q, g, segs, p):
    """the energy of a labelled segmentation [(kb, kt, c), ...], cell by cell from the definition of include/dca_hip.h, in
    Python integers; None if a pair of classes is forbidden.  Written apart from stixel.py: no prefix sums, no keys."""
    total, below = 0, None
    for kb, kt, c in segs:
        vals = [int(q[k]) for k in range(kb, kt + 1) if q[k] >= 0]
        n = len(vals)
        mu = (2 * sum(vals) + n) // (2 * n) if n else -1
        if c == 0:
            total += sum(min((int(q[k]) - int(g[k])) ** 2, p["Tg"]) for k in range(kb, kt + 1) if q[k] >= 0)
        elif c == 1:
            total += sum((v - mu) ** 2 for v in vals) + (p["far"] if 0 <= mu < p["mu_min"] else 0)
        else:
            total += sum(min(v * v, p["Ts"]) for v in vals)
        total += p["seg"][c]
        if below is None:
            total += p["first"][c]
        else:
            if p["T"][below][c] < 0:
                return None
            total += p["T"][below][c]
            if c == 1 and below == 0:
                total += p["below"] if mu > g[kb] + p["eps"] else (p["float"] if mu < g[kb] - p["eps"] else 0)
        below = c
    return total


def brute_force(q, g, p):
    """the least energy over every segmentation and every labelling"""
    H, best = len(q), None
    for cuts in itertools.product((0, 1), repeat=H - 1):
        ends = [k for k in range(H - 1) if cuts[k]] + [H - 1]
        bounds = list(zip([0] + [e + 1 for e in ends[:-1]], ends))
        for labels in itertools.product((0, 1, 2), repeat=len(bounds)):
            e = energy_of(q, g, [(kb, kt, c) for (kb, kt), c in zip(bounds, labels)], p)
            if e is not None and (best is None or e < best):
                best = e
    return best


OTHER = dict(Tg=300, Ts=50, eps=4, below=77, float=600, mu_min=40, far=90, seg=(10, 20, 30), first=(5, 400, 0),
             T=((7, 0, 3), (0, 11, 0), (-1, 900, -1)))


@pytest.mark.parametrize("params", [None, OTHER], ids=["defaults", "other constants"])
def test_recursion_equals_brute_force_on_small_columns(params):
    """40 random columns of 1 to 7 cells (q in [-1, 200), one cell in five without a measurement, g in [-50, 200)): the
    recursion's energy is the minimum over EVERY segmentation and labelling, and the segmentation it returns has that energy"""
    p = S.energy_params("test", ValueError, params)
    rng = np.random.default_rng(0)
    for i in range(40):
        H = 1 + i % 7
        q = np.where(rng.random(H) < 0.2, -1, rng.integers(0, 200, H))
        g = rng.integers(-50, 200, H)
        energy, segs = S.column_stixels(q, g, params)
        assert energy == brute_force(q, g, p), (i, q, g)
        assert energy == energy_of(q, g, [s[:3] for s in segs], p), (i, segs)
        assert segs[0][0] == 0 and segs[-1][1] == H - 1 and all(a[1] + 1 == b[0] for a, b in zip(segs, segs[1:]))


def _check_truth(segs, what):
    assert len(segs) == 5, (what, segs)
    for (kb, kt, c), (tb, tt, tc) in zip(segs, C.TRUTH):
        assert c == tc and abs(kb - tb) <= 1 and abs(kt - tt) <= 1, (what, segs)


@pytest.mark.parametrize("seed", range(30))
def test_synthetic_column_is_cut_into_its_five_segments(seed):
    """road, wall, road, wall, sky with 0.25 px noise and 5 % holes: five segments, the classes exact, every boundary within one
    cell.  An object's disparity is a mean over at least 6 measured cells of its wall (9 cells, one lost to the margin, two to
    holes) and at most one foreign cell, the sky's at worst (7.7 px away, one part in ten): within 4 x 0.25 / sqrt(6) + 7.7 / 10
    + 1 / 32 < 1.25 px of the wall's"""
    q, g = C.column_scene(seed)
    energy, segs = S.column_stixels(q, g)
    print(seed, energy, segs)
    _check_truth([s[:3] for s in segs], seed)
    assert abs(segs[1][3] / 16 - C.road_px(20)) <= 1.25 and abs(segs[3][3] / 16 - C.road_px(40)) <= 1.25
    assert segs[0][3] == segs[2][3] == segs[4][3] == -1


@pytest.mark.parametrize("row_step", [1, 2])
def test_synthetic_scene_as_a_map_through_the_cell_median(row_step):
    """the same scene at full resolution, width 5: every stixel column gives the five segments within one cell; the list holds
    their window rows; the spare rows at the top and the spare columns on the right are not covered"""
    d, rec = C.map_scene(3, 5, row_step)
    rows, cols = d.shape
    r = S.stixels_host(d, rec, 64, width=5, row_step=row_step)
    assert r["cells"].shape == (60, 4, 2) and r["cells"].dtype == np.int16 and r["stixels"].shape == (4, 16, 4)
    g_true = np.floor(C.road_px(np.arange(60)) * 16 + 0.5)
    assert np.abs(r["cells"][:, :, 1] - g_true[:, None]).max() <= 1, "the road at the cells' centres"
    for s in range(4):
        n = int(r["count"][s])
        segs = [(int((rows - 1 - last) // row_step), int((rows - 1 - first) // row_step), int(c))
                for first, last, c, mu in r["stixels"][s, :n]]
        _check_truth(segs, (row_step, s))
        for (kb, kt, c), (first, last, cc, mu) in zip(segs, r["stixels"][s, :n]):
            assert (first, last) == (rows - (kt + 1) * row_step, rows - kb * row_step - 1)
            assert (r["seg_class"][kb:kt + 1, s] == c).all()
            assert (r["seg_disp"][kb:kt + 1, s] == (np.float32(mu) / np.float32(16) if c == 1 else 0)).all()
        assert (r["stixels"][s, n:] == 0).all() and r["stixels"][s, 0, 1] == rows - 1 and r["stixels"][s, n - 1, 0] == rows - 60 * row_step
    assert r["energy"].dtype == np.int64 and (r["energy"] > 0).all() and r["count"].dtype == np.int32


def test_simple_columns():
    """a road alone, a wall alone, no measurement at all, a single measured cell"""
    g = np.floor(C.road_px(np.arange(40)) * 16 + 0.5).astype(np.int64)
    assert S.column_stixels(g, g) == (S.STIXEL_SEG[0], [(0, 39, 0, -1)])
    wall = np.full(40, 300)
    assert S.column_stixels(wall, g) == (S.STIXEL_SEG[1] + 0, [(0, 39, 1, 300)]), "nothing below it: no contact to pay for"
    none = np.full(40, -1)
    assert S.column_stixels(none, g) == (S.STIXEL_SEG[0], [(0, 39, 0, -1)]), "every class costs its segment: the first class"
    one = none.copy()
    one[17] = int(g[17]) + 3
    assert S.column_stixels(one, g) == (S.STIXEL_SEG[0] + 9, [(0, 39, 0, -1)]), "9 < 256: the deviation, not a cut"
    one[17] = 5                                       # far behind the road and nearer to infinity than mu_min: sky, 25
    assert S.column_stixels(one, g) == (S.STIXEL_SEG[2] + 25, [(0, 39, 2, -1)])
    # status 1 and a record without a camera height: no segmentation, but the cells
    d, rec = C.map_scene(0, 5, 1)
    for bad in (C.record(*d.shape, *rec[0:3], status=1.0), C.record(*d.shape, *rec[0:3], hs=0.0)):
        r = S.stixels_host(d, bad, 64)
        assert (r["count"] == 0).all() and (r["energy"] == 0).all() and (r["stixels"] == 0).all() and (r["seg_disp"] == 0).all()
        assert (r["seg_class"] == S.NO_CLASS).all() and (r["cells"] == S.stixels_host(d, rec, 64)["cells"]).all()


def test_a_tie_goes_to_the_lowest_cut_then_the_lowest_class():
    """with free segments and free contacts a column of exact road costs 0 as one ground segment and 0 as any run of ground and
    empty-handed classes: the key takes the smallest kb -- one segment -- and then the smallest class"""
    free = dict(seg=(0, 0, 0), below=0, float=0, far=0)
    g = np.arange(100, 88, -1)
    assert S.column_stixels(g, g, free) == (0, [(0, 11, 0, -1)])
    # cells 0..5 on the road, 6..11 an exact wall: ground then object costs 0; object, cut anywhere, object costs 0 too --
    # cost[11][object] is reached from kb = 6 on ground (cp 0) and from kb = 6 on object (cp 1): the same cost, the same kb, cp 0
    q = np.concatenate([g[:6], np.full(6, 50)])
    p = S.energy_params("t", ValueError, free)
    cost, back = S.columns_dp(q.reshape(-1, 1), g.reshape(-1, 1), p)
    assert cost[0, 11].tolist()[1] == 0 and int(back[0, 11, 1]) == (6 << 2 | 0)
    assert S.column_stixels(q, g, free) == (0, [(0, 5, 0, -1), (6, 11, 1, 50)])
    # all three classes tie at the top of an empty column: class 0
    assert S.column_stixels(np.full(5, -1), g[:5], free) == (0, [(0, 4, 0, -1)])
    assert int(back[0, 0, 0]) == S.NONE and int(back[0, 3, 0]) >> 2 == 0, "a bottom segment has no class below"


def test_more_segments_than_the_list_holds():
    q, g = C.column_scene(1)
    d = (np.where(q < 0, 0, q) / 16).astype(np.float32)[::-1].reshape(60, 1)       # one pixel per cell, row 59 the bottom
    rec = C.record(60, 1, 0.0, 0.8, 40.0 - 0.8 * 29)                                  # p(row) = 40 - 0.8 (59 - row)
    full = S.stixels_host(d, rec, 64, width=1, max_segments=16)
    for m in (1, 3):
        r = S.stixels_host(d, rec, 64, width=1, max_segments=m)
        assert r["count"].tolist() == [5] and r["stixels"].shape == (1, m, 4), "the true count"
        assert (r["stixels"][0] == full["stixels"][0, :m]).all(), "the lowest segments are kept"
        assert r["energy"] == full["energy"] and (r["seg_class"] == full["seg_class"]).all()
    assert full["stixels"][0, :5, 2].tolist() == [0, 1, 0, 1, 2] and (full["cells"][:, 0, 1] == g).all()
    assert set(S.stixels_host(d, rec, 64, width=1, outputs=("count", "cells"))) == {"count", "cells"}


def test_the_device_cases_hold_what_they_are_there_for():
    """the cell counts around one and two passes of a wave, lists shorter than the segmentation, all three classes, objects that
    pay `below` and `float`, a column without a measurement and one with a single one, records without a segmentation"""
    every = [(c, S.stixels_host(c.d, c.plane, mask=c.mask, **c.kw)) for c in C.cases()]

    class by:                                          # by["H=200"]: the one case whose name starts so
        def __class_getitem__(cls, prefix):
            (hit,) = [cr for cr in every if cr[0].name.startswith(prefix)]
            return hit

    cells = sorted({r["cells"].shape[-3] for _, r in every})
    assert all(h in cells for h in (2, 63, 64, 65, 128, 129, 130, 200)), cells
    assert {c.kw["width"] for c, _ in every} >= {1, 5, 16} and {c.kw.get("row_step", 1) for c, _ in every} >= {1, 2, 8}
    for name, m in (("max_segments 1", 1), ("H=129 width 3", 2)):
        assert by[name][1]["stixels"].shape[-2] == m and by[name][1]["count"].min() > m, "the list is shorter than the segmentation"
    r = by["batch 2: window"][1]
    assert all((r["seg_class"] == k).sum() > 20 for k in range(3)) and r["cells"].shape == (2, 66, 6, 2)
    # contacts: an object directly on ground, with a mean on either side of the road's band
    case, r = by["H=200 width 2"]
    p = S.energy_params("t", ValueError)
    paid = set()
    for s in range(r["count"].shape[0]):
        st = r["stixels"][s, :r["count"][s]]
        for below, seg in zip(st, st[1:]):
            if below[2] == 0 and seg[2] == 1:
                g = int(r["cells"][200 - 1 - seg[1], s, 1])
                paid.add("below" if seg[3] > g + p["eps"] else "float" if seg[3] < g - p["eps"] else "none")
    assert paid >= {"none"} and len(paid) >= 2, paid
    r = by["batch 3"][1]
    assert (r["count"][:2] == 0).all() and (r["count"][2] > 0).all() and (r["seg_class"][:2] == S.NO_CLASS).all()
    r = by["no valid cell | a single valid cell | a column"][1]
    assert (r["cells"][:, 0, 0] == -1).all() and (r["cells"][:, 1, 0] >= 0).sum() == 1 and r["count"].tolist()[:2] == [1, 1]
    r = by["batch 2: a NaN plane"][1]
    assert (r["cells"][0, :, :, 1] == -16 * 64).all(), "a NaN plane: g at the lower end"


@pytest.mark.parametrize("height,pitch,roll,doffs", [(1.65, 2.0, 0.0, 0.0), (1.2, -1.5, 3.0, 0.0), (0.8, 5.0, -4.0, 12.5)])
def test_stixels_metric_against_analytic_walls(height, pitch, roll, doffs):
    """upright rectangles at chosen depths whose feet stand at a chosen height over an analytic road: X, Z and the heights of
    foot and head, from the rays of the stixel's middle column and its first and last row, to 1e-9"""
    from dcanet_amd.geometry import StereoCalib
    calib = StereoCalib(721.5, 0.54, 609.6, 172.9, doffs)
    rows, cols, width = 375, 1242, 5
    rec = G.plane_from_pose(height, pitch, roll, calib, rows, cols)
    n = np.array(G.plane_pose(rec, calib)["normal"])
    st = np.zeros((cols // width, 4, 4), np.int32)
    cnt = np.zeros(cols // width, np.int32)
    want = []
    for s, first, last, mu in ((3, 120, 200, 16 * 30), (100, 150, 260, 16 * 12 + 5), (247, 10, 370, 99)):
        st[s, 0] = (last + 1, rows - 1, 0, -1)
        st[s, 1] = (first, last, 1, mu)
        st[s, 2] = (0, first - 1, 2, -1)
        cnt[s] = 3
        d = mu / 16
        Z = calib.f * calib.baseline / (d + doffs)
        u = s * width + (width - 1) / 2
        point = lambda row: Z * np.array([(u - calib.cx) / calib.f, (row - calib.cy) / calib.f, 1.0])
        want.append((s, 1, d, Z, point(0)[0], height - float(n @ point(last)), height - float(n @ point(first))))
    st[50, 0], cnt[50] = (0, rows - 1, 1, -1), 1                   # an object without a disparity is not a stixel in metres
    st[60, 0], cnt[60] = (0, rows - 1, 1, 40), 0                   # beyond the count
    got = S.stixels_metric(st, cnt, rec, calib, width)
    assert got["column"].tolist() == [3, 100, 247] and got["index"].tolist() == [1, 1, 1]
    for i, (s, j, d, Z, X, base, top) in enumerate(want):
        for key, w in (("disp", d), ("Z", Z), ("X", X), ("base", base), ("top", top)):
            assert abs(got[key][i] - w) <= 1e-9 * max(1.0, abs(w)), (s, key, got[key][i], w)
    assert (got["top"] > got["base"]).all()
    for bad in (dict(stixels=st[:, :, :3]), dict(count=cnt[:5]), dict(plane=rec[:4]), dict(width=0), dict(calib=None),
                dict(plane=C.record(rows, cols, 0.0, 0.3, 5.0, hs=0.0))):
        with pytest.raises(ValueError, match="stixels_metric:"):
            S.stixels_metric(**{**dict(stixels=st, count=cnt, plane=rec, calib=calib, width=width), **bad})


def _call(lib, **kw):
    p = [ctypes.c_void_p(64 * k) for k in range(1, 11)]
    a = dict(d=p[0], mask=None, plane=p[1], ws=p[2], cells=p[3], seg_class=p[4], seg_disp=p[5], count=p[6], stixels=p[7], energy=p[8],
             B=1, Hc=48, Wc=80, y0=0, rows=48, cols=75, max_disp=32, width=5, row_step=1, min_valid=1, max_segments=16,
             min_disp=0.0625, mask_min=0.5, Tg=1024, Ts=1024, eps=16, below=2048, hang=512, mu_min=16, far=2048, seg0=256, seg1=384,
             seg2=256, first0=0, first1=0, first2=0, t00=-1, t01=0, t02=0, t10=0, t11=0, t12=0, t20=-1, t21=-1, t22=-1)
    a.update(kw)
    return lib.dca_stixels(*a.values(), None)


BIG = (1 << 20) + 1
REFUSALS = [dict(d=None), dict(plane=None), dict(plane=ctypes.c_void_p(132)), dict(ws=None, cells=None),
            dict(cells=None, seg_class=None, seg_disp=None, count=None, stixels=None, energy=None), dict(B=0), dict(B=65536), dict(y0=1),
            dict(cols=81), dict(Hc=1 << 16, Wc=1 << 15), dict(Hc=32776, rows=32776, row_step=8, Wc=8, cols=8),
            dict(Wc=32769, cols=32769), dict(max_disp=7), dict(max_disp=1025), dict(min_disp=-0.5), dict(min_disp=math.inf),
            dict(min_disp=math.nan), dict(mask=ctypes.c_void_p(4096), mask_min=math.nan), dict(width=0), dict(width=17), dict(row_step=0),
            dict(row_step=9), dict(rows=1, Hc=1), dict(row_step=8, rows=15), dict(Hc=1025, rows=1025), dict(cols=4), dict(min_valid=0),
            dict(min_valid=6), dict(max_segments=0), dict(max_segments=65), dict(Tg=-1), dict(Ts=BIG), dict(eps=-1), dict(below=BIG),
            dict(hang=-1), dict(mu_min=BIG), dict(far=-1), dict(seg0=-1), dict(seg1=BIG), dict(seg2=-1), dict(first0=BIG), dict(first1=-1),
            dict(first2=BIG), dict(t00=-2), dict(t01=BIG), dict(t12=-2), dict(t22=BIG), dict(count=ctypes.c_void_p(130)),
            dict(energy=ctypes.c_void_p(132)), dict(cells=ctypes.c_void_p(130)), dict(cells=None, ws=ctypes.c_void_p(130))]


def test_stixel_library_abi_symbol_and_refusals():
    """the library loads with ABI 21 -- an entry point was added, none changed -- exports dca_stixels with the types of the
    header, and its launcher refuses everything the header lists with hipErrorInvalidValue (1), without touching a device"""
    from ctypes import c_float as f, c_int as i, c_void_p as p
    from dcanet_amd import _lib, ops
    lib = _lib.load()
    assert _lib.ABI_VERSION == 21 and lib.dca_abi_version() == 21
    assert _lib.SIGNATURES["dca_stixels"] == (i, [p] * 10 + [i] * 11 + [f] * 2 + [i] * 22 + [p])
    assert lib.dca_stixels is not None and ops.stixels is S.stixels and ops.stixel_workspace is S.stixel_workspace
    assert ops.STIXEL_OUTPUTS == S.STIXEL_OUTPUTS == tuple(S._STIXEL_KINDS)
    consts = dict(WIDTH=16, ROW_STEP=8, CELLS=1024, SEGMENTS=64, CONST=1 << 20)
    assert all(_lib.CONSTANTS["DCA_STIXEL_MAX_" + k] == v for k, v in consts.items()) and _lib.CONSTANTS["DCA_STIXEL_NO_CLASS"] == 255
    assert (S.STIXEL_TG, S.STIXEL_TS, S.STIXEL_EPS, S.STIXEL_BELOW, S.STIXEL_FLOAT, S.STIXEL_SEG, S.STIXEL_MU_MIN, S.STIXEL_FAR,
            S.STIXEL_FIRST) == (1024, 1024, 16, 2048, 512, (256, 384, 256), 16, 2048, (0, 0, 0)), "the issue's defaults"
    assert S.STIXEL_T == ((-1, 0, 0), (0, 0, 0), (-1, -1, -1)), "no ground on ground, nothing on sky"
    assert len(S._abi_params(S.energy_params("t", ValueError))) == 22
    for bad in REFUSALS:
        assert _call(lib, **bad) == 1, bad


def test_stixel_operator_refuses_with_its_name():
    """every refusal of the header, raised where the operator validates once -- `stixel.grid_scalars` and `energy_params`,
    which it calls with RuntimeError and the restatement with ValueError -- and named"""
    from dcanet_amd import ops
    a = torch.zeros(48, 75)
    with pytest.raises(RuntimeError, match=r"stixels: .*no CPU fallback"):
        ops.stixels(a, torch.zeros(16).double(), 32)
    with pytest.raises(RuntimeError, match="inference only"):
        ops.stixels(a.clone().requires_grad_(), torch.zeros(16).double(), 32)
    good = dict(rows=48, cols=75, max_disp=32, width=5, row_step=1, min_valid=1, max_segments=16, min_disp=0.0625)
    assert S.grid_scalars("stixels", RuntimeError, **good) == (32, 5, 1, 1, 16, 0.0625, 48, 15)
    assert S.grid_scalars("stixels", RuntimeError, **{**good, **dict(rows=47, row_step=2, cols=74, width=16)})[-2:] == (23, 4)
    for bad in (dict(rows=32769, row_step=8), dict(cols=32769), dict(max_disp=7), dict(max_disp=1025), dict(max_disp=32.5),
                dict(max_disp="x"), dict(width=0), dict(width=17), dict(width=2.5), dict(row_step=0), dict(row_step=9), dict(rows=1),
                dict(rows=1025), dict(rows=15, row_step=8), dict(cols=4), dict(min_valid=0), dict(min_valid=6), dict(min_valid=None),
                dict(max_segments=0), dict(max_segments=65), dict(max_segments=1.5), dict(min_disp=-0.5), dict(min_disp=math.inf),
                dict(min_disp=math.nan)):
        for err, name in ((RuntimeError, "stixels"), (ValueError, "stixels_host")):
            with pytest.raises(err, match=name + ":"):
                S.grid_scalars(name, err, **{**good, **bad})
    p = S.energy_params("stixels", RuntimeError, dict(Tg=7, T=[[0, 0, 0], [0, 0, 0], [0, 0, -1]]))
    assert p["Tg"] == 7 and p["T"][2] == (0, 0, -1) and p["seg"] == S.STIXEL_SEG and p["float"] == S.STIXEL_FLOAT
    for bad in (dict(Tg=-1), dict(Ts=BIG), dict(eps=1.5), dict(below="x"), dict(float=-1), dict(mu_min=BIG), dict(far=None),
                dict(seg=(1, 2)), dict(seg=(1, 2, -1)), dict(first=(0, 0, BIG)), dict(first=5), dict(T=((0, 0, 0), (0, 0, 0))),
                dict(T=((0, 0, 0), (0, 0, 0), (0, 0, -2))), dict(T=((0, 0, 0), (0, 0, 0), (0, 0, BIG))), dict(nope=1), [1]):
        for err, name in ((RuntimeError, "stixels"), (ValueError, "stixels_host")):
            with pytest.raises(err, match=name + ":"):
                S.energy_params(name, err, bad)
    for bad in (dict(rows=1), dict(width=17), dict(row_step=9), dict(cols=4), dict(batch=0), dict(rows=1025)):
        with pytest.raises(RuntimeError, match="stixel_workspace"):
            ops.stixel_workspace(**{**dict(rows=48, cols=75, device="cpu"), **bad})
    assert ops.stixel_workspace(48, 75, "cpu", 5, 2, batch=3).shape == (3, 24, 15, 2)
    # the restatement's own checks
    z = np.zeros((48, 75), np.float32)
    rec = np.zeros(G.PLANE_LEN)
    for bad in (dict(disp=z.astype(np.float64)), dict(window=(0, 49, 75)), dict(window=(1, 48, 75)), dict(mask=z[:10]),
                dict(mask=z, mask_min=math.nan), dict(outputs=("nope",)), dict(outputs=()), dict(plane=rec[:8]),
                dict(plane=np.zeros((2, G.PLANE_LEN))), dict(width=80), dict(params=dict(Tg=-1))):
        with pytest.raises(ValueError, match="stixels_host:"):
            S.stixels_host(**{**dict(disp=z, plane=rec, max_disp=32), **bad})


def test_stixel_inference_wrapper_host_logic():
    """KittiInferenceStixels takes KittiInferenceGround's arguments but the per-pixel stage's, plus its own"""
    from dcanet_amd.geometry import StereoCalib
    from dcanet_amd.inference import FrameStixels, KittiInferenceGround, KittiInferenceStixels
    net = torch.nn.Linear(1, 1)
    net.maxdisp = 192
    calib = StereoCalib(721.5, 0.54, 609.6, 172.9)
    g = KittiInferenceStixels(net, calib, 64, 128, graph=False)
    assert isinstance(g, KittiInferenceGround) and g.device_io and (g.width, g.row_step, g.max_segments) == (5, 1, 16)
    assert g.Frame is FrameStixels and FrameStixels._fields == ("disp", "plane", "count", "stixels", "energy") and g.max_disp == 192
    fields = dict((n, (dt, sh)) for n, dt, sh in g._fields(30, 101, False))
    assert set(fields) == set(FrameStixels._fields) and fields["stixels"] == (torch.int32, (20, 16, 4))
    assert fields["energy"] == (torch.int64, (20,)) and fields["count"] == (torch.int32, (20,)) and fields["disp"][1] == (30, 101)
    off = 0
    for n, dt, sh in g._fields(31, 99, False):           # back to back from byte 0, every field at a multiple of its element size
        assert off % dt.itemsize == 0, n
        off += math.prod(sh) * dt.itemsize
    h = KittiInferenceStixels(net, calib, mask="lr", tau=2.0, speckle=(100, 1.0), median=3, max_disp=64, width=8, row_step=2,
                              max_segments=4, plane=dict(refine=1), stixel=dict(min_valid=3, params=dict(far=0)))
    assert (h.width, h.row_step, h.max_segments, h.mask_mode, h.median) == (8, 2, 4, "lr", 3) and h.stixel_kw["min_valid"] == 3
    for bad in (dict(calib=None), dict(device_io=False), dict(width=0), dict(width=17), dict(row_step=9), dict(max_segments=65),
                dict(stixel=dict(min_valid=6)), dict(stixel=dict(params=dict(Tg=-1))), dict(stixel=dict(nope=1)),
                dict(grid=(0.5, 10.0, 30.0)), dict(segment=dict(min_run=2)), dict(plane=dict(refine=7)), dict(max_disp=4)):
        with pytest.raises((ValueError, RuntimeError, TypeError)):
            KittiInferenceStixels(net, **{**dict(calib=calib), **bad})


def test_stixel_math_host_check_under_sanitizers(tmp_path):
    """tools/stixel_math_check.cpp: the recursion of csrc/stixel_math.h against its own brute force, the rank selection, the
    rounded mean, the key and the clamps, compiled for the host with AddressSanitizer and UBSan as a stand-alone program,
    exits 0"""
    cxx = next((c for c in (shutil.which("clang++"), "/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++",
                            shutil.which("g++")) if c and os.path.exists(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "stixel_check")
    csrc = os.path.join(ROOT, "cost-volume-aggregation-in-stereo-matching-revisited_amd", "csrc")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc,
           os.path.join(ROOT, "tools", "stixel_math_check.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok"), run.stdout[-2000:] + run.stderr[-2000:]
