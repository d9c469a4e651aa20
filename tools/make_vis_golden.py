"""Writes tests/golden/vis_error_image.npz: seeded inputs and the results of the REFERENCE's own error map
(`disp_error_image_func.forward` of utils/visualization.py) on them, computed on the CPU.

    python tools/make_vis_golden.py --reference /path/to/reference [--out tests/golden/vis_error_image.npz]

The reference's file is loaded from the given path at run time (`forward` is an old-style method: called unbound, with None for
`self`).  No reference text enters this repository: the fixture holds the inputs and the recorded float32 (B,3,H,W) images.

Every case holds, outside the legend's rectangle (rows < 10, columns < 200): about 30 % gt = 0, a few gt < 0, estimates
that are NaN, +inf and -inf where gt > 0, one pixel exactly on each bin edge through the absolute branch (gt = 40 <= 60, so
e / 3 is the smaller term; e = 3 * 2^k, k = -4..4) and pixels with gt > 60, where the relative term is the smaller one."""
import argparse
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (seed, B, H, W): H > 10 and W < 200 (legend clipped in width); H < 10 and W > 200; 12 x 200 (legend exactly as wide)
CASES = [(11, 2, 13, 47), (12, 1, 7, 230), (13, 1, 12, 200)]


def inputs(seed, B, H, W):
    """(est, gt) float32 (B,H,W)"""
    rs = np.random.RandomState(seed)
    gt = (5.0 + 150.0 * rs.rand(B, H, W)).astype(np.float32)                 # both branches: gt below and above 60
    # errors from 0.01 to ~100 px, log-uniform: all ten bins
    est = (gt + np.exp(rs.uniform(np.log(0.01), np.log(100.0), (B, H, W))) * rs.choice([-1.0, 1.0], (B, H, W))).astype(np.float32)
    gt[rs.rand(B, H, W) < 0.3] = 0.0
    free = [(r, c) for r in range(H) for c in range(W) if r >= 10 or c >= 200]      # not under the legend
    order = rs.permutation(len(free))
    spots = iter([free[i] for i in order])
    for b in range(B):
        for k in range(-4, 5):                                                # exactly on an edge, absolute branch
            r, c = next(spots)
            gt[b, r, c], est[b, r, c] = 40.0, 40.0 - 3.0 * 2.0 ** k
        for bad in (np.nan, np.inf, -np.inf):                                 # masked in, no bin
            r, c = next(spots)
            gt[b, r, c], est[b, r, c] = 30.0, bad
        for e in (0.5, 4.0, 30.0):                                            # relative branch: gt = 120 > 60
            r, c = next(spots)
            gt[b, r, c], est[b, r, c] = 120.0, 120.0 + e
        for _ in range(3):
            r, c = next(spots)
            gt[b, r, c] = -1.0 - rs.rand()
        r, c = next(spots)
        gt[b, r, c], est[b, r, c] = 0.0, np.nan                               # masked out: the NaN must not show
    return est, gt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference tree (the directory that holds utils/)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "vis_error_image.npz"))
    a = ap.parse_args()
    import torch
    # the file alone: the package's __init__ pulls in the TensorBoard helpers and their dependencies
    spec = importlib.util.spec_from_file_location("_reference_visualization",
                                                  os.path.join(os.path.abspath(a.reference), "utils", "visualization.py"))
    vis = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(vis)
    out = {"cases": np.array(CASES, dtype=np.int64)}
    for i, case in enumerate(CASES):
        est, gt = inputs(*case)
        with np.errstate(all="ignore"):
            img = vis.disp_error_image_func.forward(None, torch.from_numpy(est), torch.from_numpy(gt))
        img = img.numpy()
        assert img.dtype == np.float32 and img.shape == (case[1], 3) + case[2:]
        out[f"est{i}"], out[f"gt{i}"], out[f"image{i}"] = est, gt, img
    np.savez_compressed(a.out, **out)
    print(a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
