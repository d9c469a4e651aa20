"""Left-right consistency, the parts that need no GPU: the two C entry points of csrc/lr_consistency.hip are bound and
refuse bad arguments before anything touches a device, the operators refuse CPU tensors, KittiInferenceLR takes
KittiInference's arguments plus `tau`, and the numpy restatement the GPU tests compare against (tests/_lr_reference.py)
reaches every fill case on its scene -- and is exact in fp32, which is why those comparisons are bitwise."""
import ctypes
import math

import numpy as np
import pytest
import torch

from _lr_reference import CATEGORIES, SHAPES, lr_reference, scene


def test_lr_entry_points_are_bound_and_exported():
    from dcanet_amd import _lib
    lib = _lib.load()
    for name in ("dca_mirror_pair", "dca_lr_consistency"):
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    assert lib.dca_abi_version() == 21 and _lib.ABI_VERSION == 21


def test_lr_launchers_refuse_bad_arguments_before_any_launch():
    """hipErrorInvalidValue (1) without touching a device"""
    from dcanet_amd import _lib
    lib = _lib.load()
    p, q, r, s = (ctypes.c_void_p(16 * k) for k in range(1, 5))
    mp = lib.dca_mirror_pair
    assert mp(None, q, r, s, 3, 4, 5, None) == 1 and mp(p, None, r, s, 3, 4, 5, None) == 1
    assert mp(p, q, None, s, 3, 4, 5, None) == 1 and mp(p, q, r, None, 3, 4, 5, None) == 1
    assert mp(p, q, r, s, 0, 4, 5, None) == 1 and mp(p, q, r, s, 3, 0, 5, None) == 1 and mp(p, q, r, s, 3, 4, -1, None) == 1
    assert mp(p, q, p, s, 3, 4, 5, None) == 1 and mp(p, q, r, q, 3, 4, 5, None) == 1        # in place
    lr = lib.dca_lr_consistency
    assert lr(None, q, r, s, r, s, 1, 4, 8, 8, 1.0, None) == 1                               # dl
    assert lr(p, None, r, s, r, s, 1, 4, 8, 8, 1.0, None) == 1                               # drm
    assert lr(p, q, r, None, r, s, 1, 4, 8, 8, 1.0, None) == 1                               # valid is required
    assert lr(p, q, None, None, None, None, 1, 4, 8, 8, 1.0, None) == 1
    assert lr(p, q, r, s, r, s, 1, 4, 8, 0, 1.0, None) == 1                                  # cols = 0
    assert lr(p, q, r, s, r, s, 1, 4, 8, 9, 1.0, None) == 1                                  # cols > W
    assert lr(p, q, r, s, r, s, 1, 4, 8, -3, 1.0, None) == 1
    assert lr(p, q, r, s, r, s, 1, 4, 8193, 8193, 1.0, None) == 1                            # W > 8192
    assert lr(p, q, r, s, r, s, 1, 4, 8193, 100, 1.0, None) == 1
    assert lr(p, q, r, s, r, s, 1, 4, 8, 8, -0.5, None) == 1                                 # tau < 0
    assert lr(p, q, r, s, r, s, 1, 4, 8, 8, math.nan, None) == 1
    assert lr(p, q, r, s, r, s, 1, 4, 8, 8, math.inf, None) == 1                             # would validate out-of-view pixels
    for dims in ((0, 4, 8), (1, 0, 8), (1, 4, 0), (-1, 4, 8), (1, -4, 8)):
        assert lr(p, q, r, s, r, s, *dims, 1, 1.0, None) == 1, dims


def test_lr_constants_match_the_header():
    import os
    import re
    from dcanet_amd import ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "dca_hip.h")).read()
    assert int(re.search(r"^#define DCA_LR_MAX_W (\d+)$", header, flags=re.M).group(1)) == ops.LR_MAX_W == 8192


def test_lr_operators_refuse_cpu_tensors():
    from dcanet_amd import ops
    a, b = torch.zeros(1, 3, 4, 8), torch.zeros(1, 3, 4, 8)
    with pytest.raises(RuntimeError):
        ops.mirror_pair(a, b)
    with pytest.raises(RuntimeError):
        ops.lr_consistency(a[:, :1], b[:, :1])
    with pytest.raises(RuntimeError):
        ops.lr_consistency(a[0], b[0], tau=0.5, cols=4)


def test_lr_wrapper_host_logic():
    """KittiInferenceLR takes KittiInference's arguments plus `tau`, and hands out two maps where the base hands out one"""
    from dcanet_amd.inference import KittiInference, KittiInferenceLR, KittiInferenceWithConfidence
    net = torch.nn.Linear(1, 1)
    assert KittiInference(net).nmaps == 1 and KittiInferenceWithConfidence(net).nmaps == 2
    infer = KittiInferenceLR(net, 64, 128, graph=False, device_io=True, tau=2.5)
    assert infer.tau == 2.5 and (infer.crop_height, infer.crop_width) == (64, 128)
    assert infer.device_io is True and infer.graph is False and infer.dtype is None
    assert infer.nmaps == 2 and infer.confidence is False
    assert isinstance(infer, KittiInference) and not isinstance(infer, KittiInferenceWithConfidence)
    d = KittiInferenceLR(net, dtype=torch.float16)
    assert d.tau == 1.0 and d.dtype is torch.float16 and d.graph is True and (d.crop_height, d.crop_width) == (384, 1248)
    for bad in (-1.0, math.nan, math.inf):
        with pytest.raises(ValueError):
            KittiInferenceLR(net, tau=bad)


def test_predict_lr_is_part_of_the_model():
    from dcanet_amd.models.gwcnet_dca_g import GwcNet
    import inspect
    sig = inspect.signature(GwcNet.predict_lr)
    assert list(sig.parameters) == ["self", "left", "right", "tau"] and sig.parameters["tau"].default == 1.0


def test_the_restatement_reaches_every_fill_case_and_is_exact_in_fp32():
    """Across the GPU test's shapes the scene yields every fill category and pixels with diff == tau exactly (so `<=` is
    tested); the same formulas in float32 give the float64 result bit for bit, so the GPU comparison needs no tolerance."""
    tau = 1.0
    total = dict.fromkeys(CATEGORIES, 0)
    for shape in SHAPES:
        dl, drm = scene(shape)
        assert dl.shape == drm.shape == shape and dl.dtype == drm.dtype == np.float32
        for a in (dl, drm):                                     # multiples of 1/16 below 2^11
            assert np.array_equal(a * 16, np.round(a * 16)) and np.abs(a).max() < 2048
        ref = lr_reference(dl, drm, tau)
        f32 = lr_reference(dl, drm, tau, dtype=np.float32)
        for k in ("diff", "valid", "filled", "disp_right"):
            assert ref[k].dtype == np.float32 and ref[k].tobytes() == f32[k].tobytes(), (shape, k)
        cat = ref["categories"]
        assert cat["out_of_view"] > 0, shape
        if shape[2] >= 67:
            assert ref["diff_eq_tau"] > 0, shape
        if shape != (1, 1, 1):
            assert cat["right_only"] > 0 and cat["both"] > 0, shape
            assert 0 < ref["valid"].sum() < ref["valid"].size
        if shape in ((2, 3, 7), (2, 4, 301)):
            assert cat["left_only"] > 0, shape
        if shape in ((1, 1, 1), (1, 5, 67), (2, 4, 301)):
            assert cat["empty_row"] > 0, shape
        # valid pixels keep dl; every filled value is a value of a valid pixel of the same row
        keep = ref["valid"] == 1
        assert np.array_equal(ref["filled"][keep], dl[keep])
        for k in CATEGORIES:
            total[k] += ref["categories"][k]
        print(shape, ref["categories"], "diff == tau:", ref["diff_eq_tau"])
    assert all(total[k] > 0 for k in CATEGORIES), total
    # the narrower active widths of the GPU test: nothing at or beyond cols is a match target or a fill source
    for shape, cols in (((2, 4, 301), 250), ((1, 5, 67), 1)):
        dl, drm = scene(shape)
        ref = lr_reference(dl, drm, tau, cols)
        assert not ref["valid"][..., cols:].any() and np.isinf(ref["diff"][..., cols:]).all()
        assert np.array_equal(ref["filled"][..., cols:], dl[..., cols:])
        poisoned = drm.copy()
        poisoned[..., :shape[2] - cols] = 777.0                 # right-image columns >= cols sit at mirrored index < W - cols
        dl2 = dl.copy()
        dl2[..., cols:] = -555.0
        again = lr_reference(dl2, poisoned, tau, cols)
        for k in ("diff", "valid"):
            assert again[k].tobytes() == ref[k].tobytes()
        assert np.array_equal(again["filled"][..., :cols], ref["filled"][..., :cols])
