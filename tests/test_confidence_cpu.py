"""Per-pixel confidence, the parts that need no GPU: the host arithmetic of the risk-coverage curve
(dcanet_amd.evaluation.risk_coverage) and the argument checks of the three C entry points of csrc/confidence.hip."""
import ctypes
import warnings

import numpy as np


def _state(rows, nbins):
    st = np.zeros((nbins, 3), np.int64)
    for b, (n, err, bad) in rows.items():
        st[b] = (n, int(err * 1048576), bad)
    return st


def test_risk_coverage_on_a_hand_built_state():
    from dcanet_amd.evaluation import risk_coverage
    # bins 7 (most confident), 5, 2, 0 hold pixels; 1, 3, 4, 6 are empty
    st = _state({7: (10, 2.5, 0), 5: (30, 30.0, 3), 2: (40, 120.0, 20), 0: (20, 200.0, 18)}, 8)
    r = risk_coverage(st)
    assert np.array_equal(r["counts"], [20, 0, 40, 0, 0, 30, 0, 10]) and r["pixels"] == 100
    assert len(r["coverage"]) == len(r["epe"]) == len(r["bad3"]) == len(r["threshold"]) == 4      # empty bins skipped
    assert np.array_equal(r["threshold"], [7 / 8, 5 / 8, 2 / 8, 0.0])
    assert np.array_equal(r["coverage"], [0.1, 0.4, 0.8, 1.0])
    assert np.all(np.diff(r["coverage"]) > 0) and r["coverage"][-1] == 1.0
    assert np.array_equal(r["epe"], [2.5 / 10, 32.5 / 40, 152.5 / 80, 352.5 / 100])
    assert r["epe"][-1] == st[:, 1].sum() / 1048576 / st[:, 0].sum()                            # total error / total count
    assert np.array_equal(r["bad3"], [0.0, 3 / 40, 23 / 80, 41 / 100])
    c, e = [0.0, 0.1, 0.4, 0.8, 1.0], [0.25, 0.25, 32.5 / 40, 152.5 / 80, 3.525]                  # held at epe[0] below 0.1
    want = sum((c[i + 1] - c[i]) * (e[i + 1] + e[i]) / 2 for i in range(4))
    assert abs(r["aurc_epe"] - want) < 1e-12
    # a confidence that says nothing about the error: every bin has the same mean error -> the area is that error
    flat = risk_coverage(_state({b: (10 * (b + 1), 1.5 * 10 * (b + 1), 0) for b in range(8)}, 8))
    assert abs(flat["aurc_epe"] - 1.5) < 1e-12 and np.allclose(flat["epe"], 1.5, rtol=0, atol=1e-12)
    # a confidence that ranks the errors scores better than one that ranks them backwards
    assert r["aurc_epe"] < risk_coverage(st[::-1].copy())["aurc_epe"]


def test_risk_coverage_of_an_empty_state_is_zero_without_a_warning():
    from dcanet_amd.evaluation import risk_coverage
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        r = risk_coverage(np.zeros((64, 3), np.int64))
    assert r["pixels"] == 0 and r["aurc_epe"] == 0.0 and not r["counts"].any() and r["counts"].shape == (64,)
    assert all(len(r[k]) == 0 for k in ("coverage", "epe", "bad3", "threshold"))


def test_confidence_launchers_refuse_bad_arguments_before_any_launch():
    """hipErrorInvalidValue (1) without touching a device"""
    from dcanet_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(16)
    assert lib.dca_softargmin_stats(p, p, 1, 0, 10, 1, None) == 1                 # K = 0
    assert lib.dca_softargmin_stats(p, p, 1, 8, 10, -1, None) == 1                # radius < 0
    assert lib.dca_softargmin_stats(p, p, 0, 8, 10, 1, None) == 1
    assert lib.dca_softargmin_stats(None, p, 1, 8, 10, 1, None) == 1
    scales = (ctypes.c_float * 9)(*([1.0] * 9))
    sp = ctypes.cast(scales, ctypes.c_void_p)
    assert lib.dca_convex_up4_planes(p, p, sp, p, 1, 0, 4, 4, None) == 1          # P = 0
    assert lib.dca_convex_up4_planes(p, p, sp, p, 1, 9, 4, 4, None) == 1          # P = 9
    assert lib.dca_convex_up4_planes(p, p, sp, ctypes.c_void_p(20), 1, 2, 4, 4, None) == 1      # unaligned output
    assert lib.dca_convex_up4_planes(p, p, None, p, 1, 2, 4, 4, None) == 1
    assert lib.dca_conf_histogram(p, p, p, p, 1, 10, 1, 192.0, None) == 1         # nbins = 1
    assert lib.dca_conf_histogram(p, p, p, p, 1, 10, 1025, 192.0, None) == 1      # nbins = 1025
    assert lib.dca_conf_histogram(p, p, p, None, 1, 10, 64, 192.0, None) == 1


def test_plane_indices_match_the_header():
    import os
    import re
    from dcanet_amd import ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "dca_hip.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"^#define (DCA_CONF_\w+) (\d+)$", header, flags=re.M)}
    assert defs == {"DCA_CONF_DISP": ops.CONF_DISP, "DCA_CONF_DUNI": ops.CONF_DUNI, "DCA_CONF_MASS": ops.CONF_MASS,
                    "DCA_CONF_ENT": ops.CONF_ENT, "DCA_CONF_STD": ops.CONF_STD, "DCA_CONF_PLANES": ops.CONF_PLANES,
                    "DCA_CONF_MAX_PLANES": ops.CONF_MAX_PLANES, "DCA_CONF_MAX_BINS": ops.CONF_MAX_BINS,
                    "DCA_CONF_ERR_SCALE": ops.CONF_ERR_SCALE}


def test_confidence_wrapper_host_logic(tmp_path):
    """KittiInferenceWithConfidence takes KittiInference's arguments plus `radius`; the 16-bit confidence PNG"""
    import pytest
    import torch
    from PIL import Image
    from dcanet_amd.inference import KittiInference, KittiInferenceWithConfidence, confidence_png
    plain = KittiInference(torch.nn.Linear(1, 1))
    assert plain.confidence is False
    infer = KittiInferenceWithConfidence(torch.nn.Linear(1, 1), 64, 128, graph=False, device_io=True, radius=2)
    assert infer.confidence is True and infer.radius == 2 and (infer.crop_height, infer.crop_width) == (64, 128)
    assert infer.device_io is True and infer.graph is False
    assert KittiInferenceWithConfidence(torch.nn.Linear(1, 1)).radius == 1
    with pytest.raises(ValueError):
        KittiInferenceWithConfidence(torch.nn.Linear(1, 1), radius=-1)
    conf = np.array([[0.0, 0.5, 1.0], [0.25, 1e-6, 0.999999]], np.float32)
    want = (conf * np.float32(65535)).astype(np.uint16)
    confidence_png(str(tmp_path / "a.png"), conf)
    confidence_png(str(tmp_path / "b.png"), want)
    for name in ("a.png", "b.png"):
        assert np.array_equal(np.asarray(Image.open(tmp_path / name)), want)
