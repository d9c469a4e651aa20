"""High-resolution pairs without a GPU (dcanet_amd/highres.py, csrc/highres.hip): the C ABI of the three entry points, the
numpy restatements against independent straightforward formulas on tiny hand-made inputs, the weight tables, the property the
upsampler exists for -- depth edges follow the colour edges of the full-resolution image where a bilinear resize smears them
-- and `host_sample(downscale=)`."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("dca_area_downscale_u8", "dca_area_downscale_f32", "dca_guided_upsample")


def test_header_declares_and_library_exports_the_entry_points():
    from ctypes import c_float as f, c_int as i, c_void_p as p
    from dcanet_amd import _lib
    header = open(os.path.join(ROOT, "include", "dca_hip.h")).read()
    declared = set(re.findall(r"^(?:int|long)\s+(dca_\w+)\s*\(", header, flags=re.M))
    assert set(ENTRY_POINTS) <= declared
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert getattr(lib, name) is not None
    assert _lib.ABI_VERSION == 21                    # entry points were added, none changed
    S = _lib.SIGNATURES
    assert S["dca_area_downscale_u8"] == (i, [p, p, p, i, i, i, i, p])
    assert S["dca_area_downscale_f32"] == (i, [p, p, i, i, i, i, i, p])
    assert S["dca_guided_upsample"] == (i, [p] * 8 + [i] * 10 + [f, p])
    C = _lib.CONSTANTS
    assert (C["DCA_HR_MAX_SCALE"], C["DCA_HR_MAX_RADIUS"], C["DCA_HR_RANGE_LEN"]) == (4, 3, 766)


def test_ops_reexports_the_wrappers_and_frame_ops_does_not_define_them():
    from dcanet_amd import frame_ops, highres, ops
    for name in ("area_downscale_pair", "area_downscale_disp", "guided_upsample"):
        assert getattr(ops, name) is getattr(highres, name) and not hasattr(frame_ops, name)


# ---- the downscales on hand-made inputs -----------------------------------------------------------------------------------
def _mean_u8(block):
    """(sum + cnt // 2) // cnt in Python integers"""
    vals = [int(v) for v in np.asarray(block).reshape(-1)]
    return (sum(vals) + len(vals) // 2) // len(vals)


def test_area_downscale_pair_host_on_hand_made_blocks():
    from dcanet_amd.highres import area_downscale_pair_host
    img = np.zeros((2, 4, 3), np.uint8)
    img[:, 0:2] = np.array([[0, 0], [0, 2]], np.uint8)[:, :, None]           # [0,0,0,2] -> (2 + 2) >> 2 = 1
    img[:, 2:4] = 255                                                        # 255 -> 255
    out = area_downscale_pair_host(img, img[:, ::-1].copy(), 2)
    assert out.shape == (2, 1, 2, 3) and out.dtype == np.uint8
    assert out[0].tolist() == [[[1, 1, 1], [255, 255, 255]]] and out[1].tolist() == [[[255, 255, 255], [1, 1, 1]]]
    assert area_downscale_pair_host(np.full((2, 2, 3), 1, np.uint8) * np.array([[1, 0], [1, 0]], np.uint8)[:, :, None],
                                    img[:2, :2], 2)[0].tolist() == [[[1, 1, 1]]]       # [1,0,1,0]: 2 + 2 >> 2 = 1: a tie rounds up
    rng = np.random.default_rng(5)
    for s in (2, 3, 4):                              # partial last blocks in both directions, C = 4
        a, b = (rng.integers(0, 256, (7, 13, 4), dtype=np.uint8) for _ in range(2))
        out = area_downscale_pair_host(a, b, s)
        h, w = -(-7 // s), -(-13 // s)
        assert out.shape == (2, h, w, 4)
        for n, src in enumerate((a, b)):
            for j in range(h):
                for i in range(w):
                    for c in range(4):
                        assert out[n, j, i, c] == _mean_u8(src[j * s:(j + 1) * s, i * s:(i + 1) * s, c]), (s, n, j, i, c)


def test_area_downscale_disp_host_on_hand_made_blocks():
    from dcanet_amd.highres import area_downscale_disp_host
    d = np.array([[1, 2, 8, np.inf, 5], [3, 6, 8, 8, 7], [4, 4, 1, 1, 9]], np.float32)
    got = area_downscale_disp_host(d, 2)
    want = np.array([[(1 + 2 + 3 + 6) / 4 / 2, 0, (5 + 7) / 2 / 2], [(4 + 4) / 2 / 2, (1 + 1) / 2 / 2, 9 / 1 / 2]], np.float32)
    assert got.dtype == np.float32 and np.array_equal(got, want)              # an inf in a block -> 0; partial blocks
    keep = area_downscale_disp_host(d, 2, inf_to_zero=False)
    assert np.isinf(keep[0, 1]) and np.array_equal(keep[keep < np.inf], want[keep < np.inf])
    assert np.array_equal(area_downscale_disp_host(d[::-1].copy(), 2, flip_rows=True), want)
    nan = d.copy()
    nan[0, 0] = np.nan
    assert area_downscale_disp_host(nan, 2)[0, 0] == 0 and np.isnan(area_downscale_disp_host(nan, 2, inf_to_zero=False)[0, 0])
    rng = np.random.default_rng(6)
    x = rng.uniform(0, 200, (7, 13)).astype(np.float32)
    for s in (3, 4):                                 # the order of the fp32 sum: row-major inside the block
        got = area_downscale_disp_host(x, s)
        for j in range(got.shape[0]):
            for i in range(got.shape[1]):
                vals = x[j * s:(j + 1) * s, i * s:(i + 1) * s].reshape(-1)
                acc = vals[0]
                for v in vals[1:]:
                    acc = np.float32(acc + v)
                assert got[j, i] == np.float32(np.float32(acc / np.float32(len(vals))) / np.float32(s))


def test_restatements_refuse_what_the_kernels_refuse():
    from dcanet_amd.highres import area_downscale_disp_host, area_downscale_pair_host, jbu_tables
    img = np.zeros((4, 4, 3), np.uint8)
    for s in (1, 5, 2.0, True):
        with pytest.raises(ValueError):
            area_downscale_pair_host(img, img, s)
        with pytest.raises(ValueError):
            area_downscale_disp_host(np.zeros((4, 4), np.float32), s)
        with pytest.raises(ValueError):
            jbu_tables(s)
    with pytest.raises(ValueError):
        jbu_tables(2, radius=4)
    with pytest.raises(ValueError):
        area_downscale_disp_host(np.zeros((4, 4), np.float64), 2)


# ---- the tables -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [2, 3, 4])
@pytest.mark.parametrize("r", [1, 2, 3])
def test_jbu_tables(s, r):
    from dcanet_amd.highres import jbu_tables
    ws, wr = jbu_tables(s, r, sigma_s=0.8, sigma_r=17.0, floor=1e-3)
    assert ws.shape == (s, 2 * r + 1) and wr.shape == (766,) and ws.dtype == wr.dtype == np.float32
    for p in range(s):
        for t in range(-r, r + 1):
            assert ws[p][t + r] == ws[s - 1 - p][r - t]                       # symmetric, exactly
            want = np.exp(-(t - ((p + 0.5) / s - 0.5)) ** 2 / (2 * 0.8 ** 2))
            assert abs(float(ws[p][t + r]) - want) <= 1e-7 * want + 1e-45
    assert (np.diff(wr) <= 0).all() and (wr >= np.float32(1e-3)).all() and wr[0] == 1 and wr[-1] == np.float32(1e-3)
    k = np.arange(766.0)
    assert np.array_equal(wr, np.maximum(np.exp(-k * k / (2 * 17.0 ** 2)), 1e-3).astype(np.float32))


# ---- the upsampler ----------------------------------------------------------------------------------------------------------
def _naive_upsample(disp_lo, glo, ghi, s, ws, wr, window, mask, mask_min):
    """the header's definition with Python loops, one float32 operation at a time"""
    y0, rows, cols = window
    H, W = ghi.shape[:2]
    r = (ws.shape[1] - 1) // 2
    out, valid = np.zeros((H, W), np.float32), np.zeros((H, W), np.float32)
    for y in range(H):
        for x in range(W):
            num = den = np.float32(0)
            for a in range(-r, r + 1):
                for b in range(-r, r + 1):
                    j, i = y // s + a, x // s + b
                    if not (0 <= j < rows and 0 <= i < cols):
                        continue
                    d = disp_lo[y0 + j, i]
                    if not (np.isfinite(d) and d > 0) or (mask is not None and not mask[y0 + j, i] >= np.float32(mask_min)):
                        continue
                    k = sum(abs(int(ghi[y, x, c]) - int(glo[j, i, c])) for c in range(3))
                    wgt = np.float32(np.float32(ws[y % s][a + r] * ws[x % s][b + r]) * wr[k])
                    num = np.float32(num + np.float32(wgt * d))
                    den = np.float32(den + wgt)
            if den > 0:
                out[y, x], valid[y, x] = np.float32(np.float32(num / den) * np.float32(s)), 1
    return out, valid


@pytest.mark.parametrize("s,r,C", [(2, 1, 3), (3, 2, 4), (4, 3, 3)])
def test_guided_upsample_host_is_the_definition(s, r, C):
    from dcanet_amd.highres import guided_upsample_host, jbu_tables
    rng = np.random.default_rng(10 * s + r)
    rows, cols, y0 = 4, 5, 2
    H, W = rows * s - 1, cols * s - (s - 1)
    disp = rng.uniform(1, 50, (y0 + rows, cols + 3)).astype(np.float32)
    disp[y0 + 1, 1], disp[y0 + 2, 3], disp[y0, 0], disp[y0 + 3, 4] = np.nan, np.inf, 0, -2
    disp[:y0] = 1e6                                  # poison outside the window
    disp[:, cols:] = 1e6
    mask = rng.uniform(0, 1, disp.shape).astype(np.float32)
    glo = rng.integers(0, 256, (rows, cols, C), dtype=np.uint8)
    ghi = np.repeat(np.repeat(glo, s, 0), s, 1)[:H, :W].copy()
    ghi[..., :3] = np.clip(ghi[..., :3].astype(int) + rng.integers(-9, 10, (H, W, 3)), 0, 255).astype(np.uint8)
    tables = jbu_tables(s, r)
    for m in (None, mask):
        got = guided_upsample_host(disp, glo, ghi, s, tables, (y0, rows, cols), m, 0.4, counts=True)
        want, want_v = _naive_upsample(disp, glo, ghi, s, *tables, (y0, rows, cols), m, 0.4)
        assert got["disp"].dtype == got["valid"].dtype == np.float32 and got["disp"].shape == (H, W)
        assert np.array_equal(got["valid"], want_v) and got["disp"].tobytes() == want.tobytes()
        assert (got["taps"] > 0).tolist() == (want_v == 1).tolist() and got["taps"].max() <= (2 * r + 1) ** 2
        assert float(got["disp"].max()) < 50 * s + 1             # a poison value took no part
    assert set(guided_upsample_host(disp, glo, ghi, s, tables, (y0, rows, cols), outputs=("valid",))) == {"valid"}
    for bad in (dict(window=(y0, rows + 1, cols)), dict(window=(y0, rows, cols - 1)), dict(tables=jbu_tables(3 if s == 2 else 2, r))):
        kw = dict(window=(y0, rows, cols), tables=tables)
        kw.update(bad)
        with pytest.raises(ValueError):
            guided_upsample_host(disp, glo, ghi, s, kw["tables"], kw["window"])


def two_surface_scene(s, seed=0, H=96, W=120):
    """A seeded scene of two slanted surfaces that meet along a slanted line which is not on the pixel grid, in distinct
    colours with small noise: (truth (H,W) float32, image (H,W,3) uint8, the edge's column per row).  What a perfect network
    would hand back at 1/s: the area mean of the truth divided by s."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    edge = 0.43 * W + 0.137 + 0.21 * ys                      # the first column of the near surface, a fraction of a pixel
    near = xs >= edge
    truth = np.where(near, 41.0 + 0.02 * xs + 0.01 * ys, 12.0 + 0.03 * xs - 0.01 * ys).astype(np.float32)
    colour = np.where(near[..., None], np.array([40.0, 90.0, 210.0]), np.array([200.0, 60.0, 40.0]))
    image = np.clip(np.rint(colour + rng.normal(0.0, 2.0, (H, W, 3))), 0, 255).astype(np.uint8)
    return truth, image, edge[:, 0]


def bilinear_resize(lo, H, W, s):
    """lo (h,w) -> (H,W): the bilinear resize with pixel centres aligned (half-pixel offsets, borders clamped), values times s"""
    def axis(n, m):
        c = np.clip((np.arange(n) + 0.5) / s - 0.5, 0, m - 1)
        i0 = np.minimum(np.floor(c).astype(int), m - 1)
        return i0, np.minimum(i0 + 1, m - 1), c - i0
    j0, j1, fy = axis(H, lo.shape[0])
    i0, i1, fx = axis(W, lo.shape[1])
    lo = lo.astype(np.float64)
    top = lo[j0][:, i0] * (1 - fx) + lo[j0][:, i1] * fx
    bot = lo[j1][:, i0] * (1 - fx) + lo[j1][:, i1] * fx
    return (top * (1 - fy[:, None]) + bot * fy[:, None]) * s


@pytest.mark.parametrize("s", [2, 3, 4])
def test_guided_upsampling_keeps_the_depth_edge_where_bilinear_smears_it(s):
    """The share of pixels within s columns of the edge that are off by more than 1 px (full resolution) must stay below HALF
    of the bilinear resize's share.  Half is a loose condition, no tuned gate: measured 0.0 against 0.6 or more."""
    from dcanet_amd.highres import area_downscale_disp_host, area_downscale_pair_host, guided_upsample_host, jbu_tables
    truth, image, edge = two_surface_scene(s)
    H, W = truth.shape
    lo = area_downscale_disp_host(truth, s, inf_to_zero=False)
    glo = area_downscale_pair_host(image, image, s)[0]
    got = guided_upsample_host(lo, glo, image, s, jbu_tables(s))
    band = np.abs(np.arange(W)[None, :] + 0.5 - edge[:, None]) <= s
    assert band.sum() >= 2 * s * H - H
    bad_guided = float((np.abs(got["disp"] - truth) > 1)[band].mean())
    bad_bilinear = float((np.abs(bilinear_resize(lo, H, W, s) - truth) > 1)[band].mean())
    print(f"s={s}: share of the {int(band.sum())} edge-band pixels off by more than 1 px: guided {bad_guided:.3f}, "
          f"bilinear {bad_bilinear:.3f}")
    assert (got["valid"] == 1).all()
    assert bad_bilinear > 0.3, "the scene has no edge to smear"
    assert bad_guided < 0.5 * bad_bilinear


# ---- training ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,inf", [("kitti", False), ("sceneflow", True)])
def test_host_sample_downscale_is_host_sample_on_downscaled_inputs(kind, inf):
    from dcanet_amd.highres import area_downscale_disp_host, area_downscale_pair_host
    from dcanet_amd.training import AugParams, host_sample
    rng = np.random.default_rng(3)
    left, right = (rng.integers(0, 256, (37, 51, 3), dtype=np.uint8) for _ in range(2))
    disp = rng.uniform(0, 90, (37, 51)).astype(np.float32)
    if inf:
        disp[5, 7] = disp[20, 30] = np.inf
    p = AugParams(3, 2, (1.2, 0.8), (0.9, 1.1), (1.1, 0.9), (1, 5, 2, 9))
    kw = dict(crop=(16, 20), maxdisp=40, kind=kind, scale=1.0, inf_to_zero=inf)
    got = host_sample(left, right, disp, p, downscale=2, flip_rows=True, **kw)
    small = area_downscale_pair_host(left, right, 2)
    want = host_sample(small[0], small[1], area_downscale_disp_host(disp, 2, inf, True), p, **kw)
    assert all(g.tobytes() == w.tobytes() and g.shape == w.shape for g, w in zip(got, want))
    assert got[2].shape == (16, 20) and got[3].any() and (inf is False or np.isfinite(got[2]).all())
    if kind != "kitti":
        return
    u16 = (np.where(np.isfinite(disp), disp, 0) * 256).astype(np.uint16)       # a PNG payload is widened first, exactly
    a = host_sample(left, right, u16, p, downscale=2, crop=(16, 20), maxdisp=40, kind=kind)
    b = host_sample(left, right, u16.astype(np.float32), p, downscale=2, crop=(16, 20), maxdisp=40, kind=kind, scale=1.0 / 256)
    assert all(g.tobytes() == w.tobytes() for g, w in zip(a, b))
    with pytest.raises(ValueError):
        host_sample(left, right, disp, p, downscale=5, **kw)
