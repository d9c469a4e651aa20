"""CPU-only checks of the evaluation step's host side (dcanet_amd.evaluation): the metric math against the results of
the reference's own `mytest` / `SegmentationMetric` (tests/golden/eval_step.npz, tools/make_eval_golden.py), the
padding geometry, the cross-rank sum of the run state, the no-CPU-fallback rule, and that the fixture regenerates
bit-identically where the reference tree is at hand."""
import importlib.util
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _tool():
    spec = importlib.util.spec_from_file_location("make_eval_golden", os.path.join(ROOT, "tools", "make_eval_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


def test_metric_math_equals_reference_fixture(golden):
    from dcanet_amd import evaluation as E
    fx = golden("eval_step")
    cms, want = fx["confusion0"], fx["values0"]
    assert cms.shape == (3, 24, 24) and cms.sum() > 0
    # SegmentationMetric used like the reference uses it: never reset between the heads
    metric = E.SegmentationMetric(24)
    for k in range(3):
        metric.addMatrix(cms[k])
        assert rel(metric.meanPixelAccuracy(), want[4 + k]) <= 1e-12
        assert rel(metric.meanIntersectionOverUnion(), want[7 + k]) <= 1e-12
    vals = E.batch_values(fx["records0"], cms)
    for i, k in enumerate(E.KEYS):
        # loss / epe / 1px / 3px of the fixture went through fp32 in the reference; the rest is fp64 from integers
        assert rel(vals[k], want[i]) <= (5e-6 if i < 4 else 1e-12), (k, vals[k], want[i])
    assert E.batch_values(fx["records1"], fx["confusion1"]) == dict.fromkeys(E.KEYS, 0.0)      # empty mask
    assert (fx["values1"] == 0).all()


def test_segmentation_metric_from_label_maps():
    from dcanet_amd.evaluation import SegmentationMetric
    rs = np.random.RandomState(0)
    label, pred = rs.randint(-2, 7, (2, 9, 11)), rs.randint(0, 5, (2, 9, 11))
    m = SegmentationMetric(5)
    m.addBatch(pred, label)
    keep = (label >= 0) & (label < 5)
    want = np.zeros((5, 5))
    np.add.at(want, (label[keep], pred[keep]), 1)
    assert (m.confusionMatrix == want).all() and want.sum() == keep.sum()
    assert rel(m.pixelAccuracy(), np.trace(want) / want.sum()) <= 1e-15
    assert rel(m.meanPixelAccuracy(), np.mean(np.diag(want) / want.sum(1))) <= 1e-15
    iou = np.diag(want) / (want.sum(0) + want.sum(1) - np.diag(want))
    assert rel(m.meanIntersectionOverUnion(), iou.mean()) <= 1e-15
    assert rel(m.Frequency_Weighted_Intersection_over_Union(), (want.sum(1) / want.sum() * iou).sum()) <= 1e-15
    m.reset()
    assert m.confusionMatrix.sum() == 0
    m.addMatrix(np.diag([3, 0, 1, 0, 0]))       # classes 1, 3, 4 never occur: left out of the mean, not counted as 0
    assert m.meanPixelAccuracy() == 1.0 and m.meanIntersectionOverUnion() == 1.0


def test_state_result_is_the_mean_over_batches(golden):
    from dcanet_amd import evaluation as E
    fx = golden("eval_step")
    state = np.zeros(E.STATE_HEAD + 3 * 24 * 24)
    state[E.BATCHES] = 2                                       # the fixture's batch and its empty-mask batch
    state[E.SUMS:E.SUMS + 10] = fx["values0"] + fx["values1"]
    state[E.STATE_HEAD:] = fx["confusion0"].reshape(-1)
    state[E.IMG_KEPT], state[E.IMG_SEEN], state[E.IMG_EPE] = 2, 4, 3.0
    res = E.state_result(state)
    for i, k in enumerate(E.KEYS):
        assert res[k] == fx["values0"][i] / 2
    assert res["image_epe"] == 1.5 and res["batches"] == 2 and res["images"] == 4
    assert (res["confusion"] == fx["confusion0"]).all()
    assert rel(res["head_mpa"][0], fx["values0"][4]) <= 1e-12            # head 0 alone = the reference's mpa0
    m = E.SegmentationMetric(24)
    m.addMatrix(fx["confusion0"][2])
    assert res["head_mIoU"][2] == m.meanIntersectionOverUnion() and res["head_mIoU"][2] != fx["values0"][9]
    empty = E.state_result(np.zeros_like(state))
    assert empty["loss"] == 0 and empty["batches"] == 0 and empty["image_epe"] == 0


@pytest.mark.parametrize("H,W,top,right", [(540, 960, 4, 0), (250, 470, 6, 10), (256, 512, 0, 0), (60, 120, 4, 8)])
def test_pad16_geometry(H, W, top, right):
    from dcanet_amd.evaluation import pad16
    L, R = torch.rand(2, 3, H, W) + 1, torch.rand(2, 3, H, W) + 1
    Lp, Rp, t, r = pad16(L, R)
    assert (t, r) == (top, right) and Lp.shape == Rp.shape == (2, 3, H + top, W + right)
    assert Lp.shape[2] % 16 == 0 and Lp.shape[3] % 16 == 0
    assert torch.equal(Lp[:, :, top:, :W], L) and torch.equal(Rp[:, :, top:, :W], R)       # image in the bottom-left corner
    assert Lp[:, :, :top].abs().sum() == 0 and Lp[:, :, :, W:].abs().sum() == 0
    if not (top or right):
        assert Lp is L and Rp is R


def test_eval_ops_refuse_cpu_tensors():
    from dcanet_amd import ops
    from dcanet_amd.evaluation import EvalStep, mytest  # noqa: F401  (exported)
    gt, pred = torch.rand(1, 16, 32), torch.rand(1, 1, 16, 32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.disp_metrics(pred, gt, 192)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.region_confusion([torch.rand(1, 24, 2, 4)] * 3, gt)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.eval_accumulate(torch.zeros(32 + 3 * 24 * 24, dtype=torch.float64), torch.zeros(1, 8, dtype=torch.float64),
                            torch.zeros(3, 24, 24, dtype=torch.int64), gt.shape)


def test_state_length_and_abi():
    from dcanet_amd import _lib
    lib = _lib.load()
    assert lib.dca_abi_version() == 21
    assert lib.dca_eval_state_len(24) == 32 + 3 * 24 * 24 and lib.dca_eval_state_len(65) == 0
    assert lib.dca_disp_metrics_workspace(2, 540, 960) > 0 and lib.dca_disp_metrics_workspace(0, 1, 1) == 0
    # invalid arguments are refused before anything is launched (no GPU needed to see that)
    assert lib.dca_region_confusion(None, None, None, None, None, 3, 1, 24, 2, 4, 16, 32, None) != 0
    assert lib.dca_disp_metrics(None, None, None, None, None, 1, 16, 32, 0, 0, 192.0, None) != 0
    assert lib.dca_eval_accumulate(None, None, None, 1, 3, 24, 16, 32, None) != 0


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_all_reduce_state_two_gloo_ranks():
    from dcanet_amd.evaluation import STATE_HEAD
    world, port = 2, _free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(r), LOCAL_RANK=str(r),
                   WORLD_SIZE=str(world))
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "_eval_dp_worker.py")], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    got = []
    for p in procs:
        out, err = p.communicate(timeout=180)
        assert p.returncode == 0, err[-2000:]
        line = [ln for ln in out.splitlines() if ln.startswith("RESULT ")][0]
        got.append(np.asarray(json.loads(line[7:])))
    want = np.zeros(STATE_HEAD + 3 * 24 * 24)
    for r in range(world):
        s = np.random.RandomState(40 + r).rand(want.size) * 1e6
        s[STATE_HEAD:] = np.floor(s[STATE_HEAD:])
        want += s
    assert (got[0] == got[1]).all() and (got[0] == want).all()      # two terms: the sum is exact and order-free


def test_all_reduce_state_without_process_group_is_identity():
    from dcanet_amd.evaluation import all_reduce_state
    s = torch.arange(5, dtype=torch.float64)
    assert all_reduce_state(s) is s and s.tolist() == [0, 1, 2, 3, 4]


def _reference_root():
    for cand in (os.environ.get("DCA_REFERENCE_ROOT"), os.path.join(os.path.dirname(ROOT), "reference")):
        if cand and os.path.exists(os.path.join(cand, "main_dca.py")):
            return cand
    return None


@pytest.mark.skipif(_reference_root() is None, reason="reference tree not available (DCA_REFERENCE_ROOT)")
def test_fixture_regenerates_bit_identically(golden):
    fx, new = golden("eval_step"), _tool().make(_reference_root())
    assert set(fx) == set(new)
    for k in fx:
        assert fx[k].dtype == new[k].dtype and fx[k].shape == new[k].shape, k
        assert fx[k].tobytes() == np.ascontiguousarray(new[k]).tobytes(), k


def test_synthetic_batch_is_informative():
    """all 24 classes, invalid and out-of-range pixels, error counts and accuracies away from 0 and 1"""
    gt, pred, vols = _tool().synthetic_batch(1, 1, 540, 960)
    assert gt.min() < 0 and gt.max() > 192 and pred.shape == (1, 1, 544, 960) and vols[0].shape == (1, 24, 68, 120)
    e = np.abs(pred[0, 0, 4:] - gt[0])
    assert 0.3 < (e > 1).mean() < 0.9 and 0.02 < (e > 3).mean() < 0.5
    cls = np.floor(gt[0, :536].reshape(67, 8, 120, 8).mean(axis=(1, 3)) / 8)
    assert set(range(24)) <= set(cls.ravel().astype(int).tolist())
    acc = (vols[2][0].argmax(0)[1:] == cls).mean()
    assert 0.1 < acc < 0.9


def test_state_layout_constants_match_header():
    import re
    from dcanet_amd import evaluation as E
    from dcanet_amd import ops
    header = open(os.path.join(ROOT, "include", "dca_hip.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"^#define (DCA_EVAL_\w+) (\d+)$", header, flags=re.M)}
    assert defs == {"DCA_EVAL_REC": ops.EVAL_REC, "DCA_EVAL_MAX_CLASSES": ops.EVAL_MAX_CLASSES,
                    "DCA_EVAL_STATE_HEAD": E.STATE_HEAD, "DCA_EVAL_BATCHES": E.BATCHES, "DCA_EVAL_SUMS": E.SUMS,
                    "DCA_EVAL_IMG_KEPT": E.IMG_KEPT, "DCA_EVAL_IMG_EPE": E.IMG_EPE, "DCA_EVAL_IMG_D1": E.IMG_D1,
                    "DCA_EVAL_IMG_THRES": E.IMG_THRES, "DCA_EVAL_IMG_SEEN": E.IMG_SEEN, "DCA_EVAL_PIXELS": E.PIXELS}
