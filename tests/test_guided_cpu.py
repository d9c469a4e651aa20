"""Guided stereo without a GPU (dcanet_amd/guided.py, csrc/guided.hip): the C ABI of the three entry
points, the numpy restatements against independent loops and the float64 formula written here, the two properties the
definition promises (a cell without a hint leaves its column bit-identical; the half-plane x < d stays exactly 0) and the
argument errors of the public ops that are raised before a device is needed."""
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("dca_hints_to_quarter", "dca_volume_modulate", "dca_cost_volume_guided_fwd")
MAXDISP = 48


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
    assert S["dca_hints_to_quarter"] == (i, [p, p, p] + [i] * 9 + [f, p])
    assert S["dca_volume_modulate"] == (i, [p, p, p] + [i] * 5 + [f, f, p])
    # dca_cost_volume_fwd's arguments, then hints4, k, 1 / (2 c^2) in front of the stream
    assert S["dca_cost_volume_guided_fwd"] == (i, S["dca_cost_volume_fwd"][1][:-1] + [p, f, f, p])


def test_one_factor_definition_is_called_by_both_routes():
    csrc = os.path.join(ROOT, "cost-volume-aggregation-in-stereo-matching-revisited_amd", "csrc")
    text = {n: open(os.path.join(csrc, n)).read() for n in ("guided_math.h", "guided.hip", "volume_fused.hip")}
    assert len(re.findall(r"float dca_guide_factor\(", text["guided_math.h"])) == 1
    for n in ("guided.hip", "volume_fused.hip"):
        assert '#include "guided_math.h"' in text[n] and "dca_guide_factor(" in text[n] and "expf(" not in text[n], n


def test_ops_reexports_the_wrapper():
    from dcanet_amd import frame_ops, guided, ops
    assert ops.hints_to_quarter is guided.hints_to_quarter and not hasattr(frame_ops, "hints_to_quarter")
    assert callable(ops.volume_modulate) and ops.GUIDE == (10.0, 1.0)


# ---- the downsample ---------------------------------------------------------------------------------------------------------
def special_image():
    """13 x 22 float32: every kind of value the definition names, and a seeded sprinkle of valid hints"""
    rng = np.random.default_rng(11)
    img = np.zeros((13, 22), np.float32)
    sel = rng.random(img.shape) < 0.15
    img[sel] = (rng.random(img.shape).astype(np.float32) * np.float32(MAXDISP - 1) + np.float32(0.5))[sel]
    img[0, 0:4] = [0.0, -1.0, np.nan, np.inf]                   # frame rows 3..3 of cell row 0: nothing valid in this block
    img[1:5, 0:4] = 0
    img[0, 4:8] = [MAXDISP, MAXDISP - 0.25, 0.0, 0.0]           # maxdisp itself is no hint, maxdisp - 0.25 is
    img[1:5, 4:8] = 0
    img[5:9, 8:12] = 0
    img[6, 9], img[7, 10] = 7.5, 21.25                          # two valid hints in one block (frame rows 8..11): the larger
    img[9:13, 20:22] = 0
    img[12, 20:22] = [-np.inf, 3.0]                             # the last columns: a cell cut by the image's right edge
    return img


def brute_quarter(img, Hc, Wc, place, maxdisp):
    src_y0, dst_y0, rows, cols = place
    out = np.zeros((Hc // 4, Wc // 4), np.float32)
    for Y in range(Hc // 4):
        for X in range(Wc // 4):
            best = None
            for fy in range(4 * Y, 4 * Y + 4):
                for fx in range(4 * X, 4 * X + 4):
                    if not (dst_y0 <= fy < dst_y0 + rows and fx < cols):
                        continue
                    v = float(img[src_y0 + fy - dst_y0, fx])
                    if not math.isnan(v) and 0.0 < v < maxdisp and (best is None or v > best):
                        best = v
            out[Y, X] = np.float32(0.0) if best is None else np.float32(0.25) * np.float32(best)
    return out


def test_hints_to_quarter_host_against_a_loop():
    from dcanet_amd.guided import hints_to_quarter_host
    from dcanet_amd.inference import placement
    img = special_image()
    place = placement(13, 22, 16, 24)
    assert place == (0, 3, 13, 22)                              # rows, cols and dst_y0 are no multiples of 4
    got, n = hints_to_quarter_host(img, (16, 24), place, MAXDISP, count=True)
    want = brute_quarter(img, 16, 24, place, MAXDISP)
    assert got.dtype == np.float32 and got.shape == (4, 6)
    assert got.tobytes() == want.tobytes()                      # bit for bit, the sign of the zeros included
    assert n == int((want > 0).sum()) and 0 < n < want.size
    assert got[0, 0] == 0 and not np.signbit(got[0, 0])         # 0, -1, NaN, +inf: no hint
    assert got[0, 1] == np.float32((MAXDISP - 0.25) * 0.25)
    assert got[2, 2] == np.float32(21.25 * 0.25)
    assert got[3, 5] == np.float32(0.75)
    assert np.isfinite(got).all()
    # a batch, and the map that already has the frame's size
    both = hints_to_quarter_host(np.stack([img, img[::-1].copy()]), (16, 24), place, MAXDISP)
    assert both.shape == (2, 4, 6) and both[0].tobytes() == want.tobytes()
    assert both[1].tobytes() == brute_quarter(img[::-1], 16, 24, place, MAXDISP).tobytes()
    frame = np.zeros((16, 24), np.float32)
    frame[3:, :22] = img
    assert hints_to_quarter_host(frame, (16, 24), None, MAXDISP).tobytes() == want.tobytes()
    # a crop: the image is larger than the frame
    big = np.random.default_rng(2).random((23, 30)).astype(np.float32) * 40
    place = placement(23, 30, 16, 24)
    assert place == (3, 0, 16, 24)
    assert hints_to_quarter_host(big, (16, 24), place, MAXDISP).tobytes() == brute_quarter(big, 16, 24, place, MAXDISP).tobytes()


def test_hints_to_quarter_host_refuses():
    from dcanet_amd.guided import hints_to_quarter_host
    img = np.zeros((13, 22), np.float32)
    for bad in (lambda: hints_to_quarter_host(img.astype(np.float64), (16, 24), (0, 3, 13, 22)),
                lambda: hints_to_quarter_host(img, (16, 24)),                       # no placement, not the frame's size
                lambda: hints_to_quarter_host(img, (18, 24), (0, 3, 13, 22)),       # 18 % 4
                lambda: hints_to_quarter_host(img, (16, 24), (0, 4, 13, 22)),       # 4 + 13 > 16
                lambda: hints_to_quarter_host(img, (16, 24), (1, 3, 13, 22)),       # 1 + 13 > 13
                lambda: hints_to_quarter_host(img, (16, 24), (0, 3, 13)),
                lambda: hints_to_quarter_host(img, (16, 24), (0, 3, 13, 22), maxdisp=0)):
        with pytest.raises(RuntimeError, match="hints_to_quarter_host"):
            bad()


# ---- the factor and the multiply ----------------------------------------------------------------------------------------------
def hint_maps(B, H, W, D):
    """hints in bins: 0.25, D - 1, fractional values, and a run of cells without one"""
    rng = np.random.default_rng(5)
    h4 = (rng.random((B, H, W)).astype(np.float32) * np.float32(D))
    h4[rng.random((B, H, W)) < 0.5] = 0
    h4[:, 0, 0], h4[:, 0, 1], h4[:, 0, 2] = 0.25, D - 1, 3.3125
    h4[:, -1, W // 2:] = 0
    return h4


def factor64(D, h4, k, c):
    d = np.arange(D, dtype=np.float64).reshape(D, 1, 1)
    h = h4.astype(np.float64)[..., None, :, :]
    return np.where(h > 0, k * np.exp(-((d - h) ** 2) / (2 * c * c)), 1.0)


@pytest.mark.parametrize("guide", [(10.0, 1.0), (3.0, 0.5), (1.5, 4.0)])
def test_volume_modulate_host_against_the_float64_formula(guide):
    from dcanet_amd.guided import guide_factor_host, volume_modulate_host
    B, C, D, H, W = 2, 3, 12, 5, 9
    rng = np.random.default_rng(7)
    vol = rng.standard_normal((B, C, D, H, W)).astype(np.float32)
    for d in range(D):
        vol[:, :, d, :, :d] = 0                                  # the zero half-plane of a cost volume
    h4 = hint_maps(B, H, W, D)
    m = guide_factor_host(D, h4, guide)
    assert m.dtype == np.float32 and m.shape == (B, D, H, W)
    m64 = factor64(D, h4, *guide)
    # three float32 roundings and a float32 exp: a few ulps of the factor
    assert np.abs(m - m64).max() <= 8 * 2.0 ** -24 * guide[0]
    got = volume_modulate_host(vol, h4, guide)
    want = vol.astype(np.float64) * m64[:, None]
    assert got.dtype == np.float32 and got.shape == vol.shape
    assert np.abs(got - want).max() <= 16 * 2.0 ** -24 * max(1.0, np.abs(want).max())
    # a cell without a hint leaves its column bit-identical ...
    none = np.broadcast_to((h4 <= 0)[:, None, None], vol.shape)
    assert none.any() and got[none].tobytes() == vol[none].tobytes()
    assert (m[np.broadcast_to((h4 <= 0)[:, None], m.shape)] == 1).all()
    # ... a cell with one does not, and its largest factor sits at the bin next to the hint
    assert (got[~none] != vol[~none]).any()
    b, y, x = 0, 0, 2
    assert int(m[b, :, y, x].argmax()) == 3 and m[b, 3, y, x] == pytest.approx(guide[0] * math.exp(-(0.3125 ** 2) / (2 * guide[1] ** 2)),
                                                                             rel=1e-6)
    # ... and the half-plane x < d stays exactly 0
    for d in range(1, D):
        assert not got[:, :, d, :, :d].any()
    # NaN is no hint
    h4n = h4.copy()
    h4n[0, 1, 1] = np.nan
    assert (guide_factor_host(D, h4n, guide)[0, :, 1, 1] == 1).all()


def test_guide_params():
    from dcanet_amd.guided import guide_params
    assert guide_params("x", (10.0, 1.0)) == (10.0, 0.5)
    assert guide_params("x", (2, 0.5)) == (2.0, 2.0)
    for bad in ((0.0, 1.0), (-1.0, 1.0), (10.0, 0.0), (10.0, -2.0), (math.inf, 1.0), (10.0, math.inf), (math.nan, 1.0),
                (10.0, math.nan), (10.0,), 10.0, (10.0, 1e-30), (1e39, 1.0)):
        with pytest.raises(RuntimeError, match="^x: guide"):
            guide_params("x", bad)


def test_public_ops_refuse_without_a_device():
    import dcanet_amd  # noqa: F401
    from dcanet_amd import ops
    vol, h4 = torch.zeros(1, 2, 4, 3, 8), torch.zeros(1, 3, 8)
    with pytest.raises(RuntimeError, match="hints_to_quarter: hints must be on the ROCm device; there is no CPU fallback"):
        ops.hints_to_quarter(torch.zeros(16, 24), (16, 24))
    with pytest.raises(RuntimeError, match="volume_modulate: hints4 must be on the ROCm device; there is no CPU fallback"):
        ops.volume_modulate(vol, h4)
    with pytest.raises(RuntimeError, match="volume_modulate: guide"):
        ops.volume_modulate(vol, h4, k=0.0)
    with pytest.raises(RuntimeError, match="volume_modulate: guide"):
        ops.volume_modulate(vol, h4, c=float("nan"))
    with pytest.raises(RuntimeError, match="volume_modulate: expected a \\(B,C,D,H,W\\) volume"):
        ops.volume_modulate(vol[0], h4)
    f = torch.zeros(1, 8, 3, 8)
    with pytest.raises(RuntimeError, match="cost_volume: hints4 must be on the ROCm device"):
        ops.cost_volume(f, f, 4, 2, hints4=h4)
    with pytest.raises(RuntimeError, match="cost_volume: guide"):
        ops.cost_volume(f, f, 4, 2, hints4=h4, guide=(10.0, 0.0))


def test_wrapper_and_model_signatures():
    import inspect
    import dcanet_amd  # noqa: F401
    from dcanet_amd.graph import GraphedHotPath
    from dcanet_amd.inference import KittiInference, KittiInferenceGuided
    from dcanet_amd.models.gwcnet_dca_g import GwcNet
    for fn, names in ((GwcNet.hot_path, ("hints4", "guide")), (GwcNet.forward, ("hints", "guide")),
                      (GwcNet.predict, ("hints", "guide")), (GraphedHotPath.__init__, ("hints4",)),
                      (GraphedHotPath.__call__, ("hints4",)), (KittiInferenceGuided.__init__, ("lidar", "guide"))):
        p = inspect.signature(fn).parameters
        assert all(n in p for n in names), (fn, names)
    assert "hints" not in inspect.signature(GwcNet.predict_lr).parameters
    assert inspect.signature(GwcNet.forward).parameters["hints"].kind is inspect.Parameter.KEYWORD_ONLY
    assert issubclass(KittiInferenceGuided, KittiInference)
    m = GwcNet(32, use_concat_volume=False).eval()
    with pytest.raises(ValueError, match="needs device_io=True"):
        KittiInferenceGuided(m, 64, 128, device_io=False)
    with pytest.raises(RuntimeError, match="guide"):
        KittiInferenceGuided(m, 64, 128, guide=(0.0, 1.0))
    with pytest.raises(TypeError, match="LidarCalib"):
        KittiInferenceGuided(m, 64, 128, lidar="calib")
