"""Writes tests/golden/disp_smoothness.npz: the value and the autograd gradient of the REFERENCE's own
`loss_disp_smoothness` (util.py:76-86, defined there and never called) on small seeded inputs, computed on the CPU in
float64.

    python tools/make_selfsup_golden.py --reference /path/to/reference [--out tests/golden/disp_smoothness.npz]

util.py is parsed with `ast` and only that one definition is compiled, into a namespace that holds `torch`.  No reference
text enters this repository: the fixture holds the inputs (numpy RandomState streams), the recorded value and the recorded
gradient only."""
import argparse
import ast
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, SHAPE = 20, (2, 9, 14)          # B, H, W


def inputs(seed=SEED, shape=SHAPE):
    """disp (B,1,H,W), img (B,3,H,W) float64: a tilted plane with steps plus noise under a random image"""
    B, H, W = shape
    rs = np.random.RandomState(seed)
    y, x = np.arange(H, dtype=np.float64)[:, None], np.arange(W, dtype=np.float64)[None, :]
    disp = np.stack([4.0 + 0.7 * x + 0.3 * y + 5.0 * (x > W // 2) + rs.standard_normal((H, W)) for _ in range(B)])[:, None]
    img = rs.standard_normal((B, 3, H, W))
    return disp, img


def load_reference(reference_root):
    import torch
    path = os.path.join(reference_root, "util.py")
    tree = ast.parse(open(path).read(), path)
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "loss_disp_smoothness"]
    assert len(keep) == 1, "util.py does not define loss_disp_smoothness"
    ns = {"torch": torch}
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), ns)
    return ns["loss_disp_smoothness"]


def make(reference_root):
    import torch
    fn = load_reference(reference_root)
    disp, img = inputs()
    d = torch.from_numpy(disp).requires_grad_()
    value = fn(d, torch.from_numpy(img))
    grad, = torch.autograd.grad(value, d)
    return {"disp": disp, "img": img, "value": np.asarray(value.item(), dtype=np.float64), "grad": grad.numpy()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference tree (holds util.py)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "disp_smoothness.npz"))
    a = ap.parse_args()
    out = make(a.reference)
    np.savez_compressed(a.out, **out)
    for k, v in out.items():
        print(k, v.shape, v.dtype, v.reshape(-1)[:4])


if __name__ == "__main__":
    sys.exit(main())
