"""Writes tests/golden/eval_step.npz: the results of the REFERENCE's own evaluation step (`mytest` and
`SegmentationMetric` of main_dca.py) on synthetic batches, computed on the CPU.

    python tools/make_eval_golden.py --reference /path/to/reference [--out tests/golden/eval_step.npz]

main_dca.py cannot be imported (it parses arguments and builds a CUDA model at import), so the file is parsed with
`ast` and only those two definitions are compiled, into a namespace whose `model` returns prepared tensors and whose
`args` say `cuda=False, maxdisp=192`.  No reference text enters this repository: the fixture holds seeds, shapes and
recorded numbers only; the inputs are re-made from `synthetic_batch(seed, ...)` (numpy RandomState streams and
+ - * / arithmetic: bit-stable) by whoever reads the fixture."""
import argparse
import ast
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (seed, B, H, W, all_invalid): the reference hard-codes 540 // 8 x 960 // 8 and 24 classes
CASES = [(1, 2, 540, 960, False), (2, 2, 540, 960, True)]
MAXDISP = 192
HEAD_NOISE = (0.25, 0.45, 0.7)


def synthetic_batch(seed, B, H, W, C=24, maxdisp=192, invalid=False, hp=None, wp=None):
    """Inputs of one evaluation batch as float32 numpy arrays:
    gt (B,H,W): a tilted plane from about -10 to 220 plus smooth bumps, so that every class, invalid (<= 0) and
        out-of-range (>= maxdisp) pixels occur (invalid=True: everything <= 0, the empty-mask case);
    pred (B,1,Hp,Wp): ground truth + N(0, 2 px) in the bottom-left H x W corner of the frame padded to multiples of 16;
    volumes: 3 x (B,C,hp,wp), 1/8 resolution of the padded frame: a peak at the cell's class plus noise that grows from
        head to head."""
    rs = np.random.RandomState(seed)
    Hp, Wp = H + (-H % 16), W + (-W % 16)
    hp, wp = hp or Hp // 8, wp or Wp // 8
    h, w = H // 8, W // 8
    scale = maxdisp / 192.0
    y, x = np.arange(H, dtype=np.float64)[:, None] / H, np.arange(W, dtype=np.float64)[None, :] / W
    gts = []
    for b in range(B):
        a = 0.25 + 0.5 * rs.rand()
        g = -10.0 + 230.0 * (a * x + (1.0 - a) * y)
        for _ in range(6):                                   # smooth bumps: (1 - r^2)^2 inside a disc
            cy, cx, rad, amp = rs.rand(), rs.rand(), 0.08 + 0.2 * rs.rand(), 24.0 * (rs.rand() - 0.5)
            r2 = ((y - cy) ** 2 + (x - cx) ** 2) / (rad * rad)
            g = g + amp * np.where(r2 < 1.0, (1.0 - r2) ** 2, 0.0)
        g = g * scale + 0.3 * rs.standard_normal((H, W))
        if invalid:
            g = -np.abs(g) - 1.0
        gts.append(g)
    gt = np.stack(gts).astype(np.float32)
    pred = np.zeros((B, 1, Hp, Wp), np.float32)
    pred[:, 0, Hp - H:, :W] = gt + (2.0 * rs.standard_normal((B, H, W))).astype(np.float32)
    pred[:, 0, :Hp - H, :] = rs.standard_normal((B, Hp - H, Wp)).astype(np.float32)      # the padding is never read
    pred[:, 0, :, W:] = rs.standard_normal((B, Hp, Wp - W)).astype(np.float32)
    cls = np.floor(gt[:, :8 * h, :8 * w].astype(np.float64).reshape(B, h, 8, w, 8).mean(axis=(2, 4)) / 8.0)
    cells = np.full((B, hp, wp), -100.0)
    cells[:, hp - h:, :w] = cls
    c = np.arange(C, dtype=np.float64)[None, :, None, None]
    volumes = []
    for k in range(3):
        peak = 1.0 / (1.0 + (c - cells[:, None]) ** 2)
        volumes.append((peak + HEAD_NOISE[k] * rs.standard_normal((B, C, hp, wp))).astype(np.float32))
    return gt, pred, volumes


def image_records(gt, pred, maxdisp, mask=None):
    """(B,8) float64: the per-image sums dca_disp_metrics produces, with e = |pred - gt| in fp32 and fp64 accumulation."""
    B, H, W = gt.shape
    p = pred.reshape(B, pred.shape[-2], pred.shape[-1])[:, pred.shape[-2] - H:, :W]
    e = np.abs(p - gt)                                               # float32
    m = ((gt > 0) & (gt < np.float32(maxdisp))) if mask is None else mask
    sl1 = np.where(e < 1, np.float32(0.5) * e * e, e - np.float32(0.5))
    rec = np.zeros((B, 8))
    for b in range(B):
        eb, gb = e[b][m[b]], gt[b][m[b]]
        rec[b] = [m[b].sum(), (gt[b] > 0).sum(), eb.astype(np.float64).sum(), sl1[b][m[b]].astype(np.float64).sum(),
                  (eb > 1).sum(), (eb > 2).sum(), (eb > 3).sum(),
                  ((eb > 3) & (eb / np.abs(gb) > np.float32(0.05))).sum()]
    return rec


def load_reference(reference_root):
    """namespace with the reference's `mytest` and `SegmentationMetric`, compiled from its main_dca.py"""
    import torch
    import torch.nn.functional as F
    from torch.autograd import Variable
    path = os.path.join(reference_root, "main_dca.py")
    tree = ast.parse(open(path).read(), path)
    keep = [n for n in tree.body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in ("mytest", "SegmentationMetric")]
    assert sorted(n.name for n in keep) == ["SegmentationMetric", "mytest"], "main_dca.py does not define both"
    ns = {"torch": torch, "np": np, "F": F, "Variable": Variable, "print": lambda *a, **k: None,
          "args": argparse.Namespace(cuda=False, maxdisp=MAXDISP)}
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), ns)
    return ns


def run_reference(ns, gt, pred, volumes):
    """the reference's `mytest` on one batch -> (ten values, the three per-head confusion matrices)"""
    import torch

    class Model:
        def eval(self):
            return self

        def __call__(self, left, right):
            return torch.from_numpy(pred), [torch.from_numpy(v) for v in volumes]

    per_head = []
    base = ns["SegmentationMetric_reference"]

    class Recording(base):
        def addBatch(self, imgPredict, imgLabel):
            per_head.append(self.genConfusionMatrix(imgPredict, imgLabel).astype(np.int64))
            base.addBatch(self, imgPredict, imgLabel)

    ns["model"], ns["SegmentationMetric"] = Model(), Recording
    B, H, W = gt.shape
    img = torch.zeros(B, 3, H, W)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        loss, metrics, mpa, miou = ns["mytest"](img, img, torch.from_numpy(gt))
    vals = [float(loss), metrics["epe"], metrics["1px"], metrics["3px"], mpa["mpa0"], mpa["mpa1"], mpa["mpa2"],
            miou["mIoU0"], miou["mIoU1"], miou["mIoU2"]]
    cms = np.stack(per_head) if per_head else np.zeros((3, 24, 24), np.int64)
    return np.asarray(vals, dtype=np.float64), cms


def make(reference_root):
    ns = load_reference(reference_root)
    ns["SegmentationMetric_reference"] = ns["SegmentationMetric"]
    out = {"cases": np.asarray([[s, B, H, W, int(inv)] for s, B, H, W, inv in CASES], dtype=np.int64),
           "maxdisp": np.asarray(MAXDISP, dtype=np.int64)}
    for i, (seed, B, H, W, inv) in enumerate(CASES):
        gt, pred, volumes = synthetic_batch(seed, B, H, W, 24, MAXDISP, inv)
        vals, cms = run_reference(ns, gt, pred, volumes)
        out[f"values{i}"], out[f"confusion{i}"] = vals, cms
        out[f"records{i}"] = image_records(gt, pred, MAXDISP)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference tree (holds main_dca.py)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "eval_step.npz"))
    a = ap.parse_args()
    out = make(a.reference)
    np.savez_compressed(a.out, **out)
    for k, v in out.items():
        print(k, v.shape, v.dtype, v.reshape(-1)[:10] if v.size <= 16 else "")


if __name__ == "__main__":
    sys.exit(main())
