"""Left-right consistency restated in numpy (include/dca_hip.h, dca_lr_consistency) and the closed-form scene the GPU tests
run it on.  Shared by tests/test_lr_cpu.py (which checks that the scene exercises every branch) and tests/test_gpu_lr.py
(which compares the kernel with it bit for bit)."""
import numpy as np

# the kernel test's shapes (B,H,W): one column; less than a wave; no wave multiple; more columns than threads (runs longer
# than 1); a ragged last run
SHAPES = [(1, 1, 1), (2, 3, 7), (1, 5, 67), (2, 4, 301), (1, 2, 1301)]
BACKGROUND, BOX = 3.5, 11.25
CATEGORIES = ("left_only", "right_only", "both", "empty_row", "out_of_view")


def scene(shape, seed=10):
    """Two planes with exact maps: the background at 3.5 and a box at 11.25 over the middle third of the columns and all
    rows but the first and the last; in the right view the box lies 11.25 columns further left.  Seeded noise k/16,
    k in [-24, 24], on a seeded 30 % of the left pixels; for H > 3 the whole last row is off by +5 (a row without a valid
    pixel).  Every value is a multiple of 1/16 below 2^11, so x - d, the interpolation weight, both products and their sum
    are exact in fp32: the fp32 kernel must equal the fp64 restatement bit for bit, with or without fma contraction.
    The default seed is one at which the fill cases fall as tests/test_lr_cpu.py lists them, per shape.
    Returns (dl, drm) float32 (B,H,W); drm is the right map mirrored, as the mirrored pass of the network produces it."""
    B, H, W = shape
    rng = np.random.RandomState(1000 * seed + 7 * W + H)
    x = np.arange(W, dtype=np.float64)
    rows = np.zeros(H, bool)
    rows[1:H - 1] = True
    lo, hi = W // 3, (2 * W) // 3
    box_l = rows[:, None] & ((x >= lo) & (x < hi))[None]
    box_r = rows[:, None] & ((x + BOX >= lo) & (x + BOX < hi))[None]
    dl = np.broadcast_to(np.where(box_l, BOX, BACKGROUND), (B, H, W)).copy()
    dr = np.broadcast_to(np.where(box_r, BOX, BACKGROUND), (B, H, W)).copy()
    noisy = rng.random_sample((B, H, W)) < 0.3
    dl = dl + np.where(noisy, rng.randint(-24, 25, (B, H, W)) / 16.0, 0.0)
    if H > 3:
        dl[:, -1] += 5.0
    return dl.astype(np.float32), np.ascontiguousarray(dr[..., ::-1]).astype(np.float32)


def lr_reference(dl, drm, tau, cols=None, dtype=np.float64):
    """dl, drm (B,H,W) float32 -> dict of float32 (B,H,W) maps diff, valid, filled, disp_right, plus `categories`: the count
    of invalid pixels x < cols per fill case (CATEGORIES; out_of_view counts pixels, whatever fills them).  The arithmetic
    runs in `dtype`; `filled` and `disp_right` are copies of input values, bit for bit."""
    dl, drm = np.asarray(dl, np.float32), np.asarray(drm, np.float32)
    B, H, W = dl.shape
    cols = W if cols is None else int(cols)
    assert 1 <= cols <= W and tau >= 0
    d = dl.astype(dtype)
    dR32 = drm[..., ::-1]
    dR = dR32.astype(dtype)
    x = np.arange(W)
    with np.errstate(invalid="ignore", over="ignore"):
        xr = x.astype(dtype) - d
        inview = (d > 0) & (xr >= 0) & (x < cols)
        fl = np.floor(np.where(inview, xr, 0))
        i0 = fl.astype(np.int64)
        f = np.where(inview, xr, 0) - fl
        i1 = np.minimum(i0 + 1, cols - 1)
        r = (1 - f) * np.take_along_axis(dR, i0, -1) + f * np.take_along_axis(dR, i1, -1)
        diff = np.where(inview, np.abs(d - r), np.inf)
        valid = diff <= dtype(tau)
    filled = dl.copy()
    cat = dict.fromkeys(CATEGORIES, 0)
    cat["out_of_view"] = int((~inview & (x < cols)).sum())
    for b in range(B):
        for y in range(H):
            vi = np.nonzero(valid[b, y, :cols])[0]
            for xx in np.nonzero(~valid[b, y, :cols])[0]:
                if len(vi) == 0:
                    cat["empty_row"] += 1
                    continue
                p = np.searchsorted(vi, xx)
                if 0 < p < len(vi):
                    a, c = dl[b, y, vi[p - 1]], dl[b, y, vi[p]]
                    filled[b, y, xx] = c if c < a else a
                    cat["both"] += 1
                elif p > 0:
                    filled[b, y, xx] = dl[b, y, vi[p - 1]]
                    cat["left_only"] += 1
                else:
                    filled[b, y, xx] = dl[b, y, vi[p]]
                    cat["right_only"] += 1
    return {"diff": diff.astype(np.float32), "valid": valid.astype(np.float32), "filled": filled,
            "disp_right": np.ascontiguousarray(dR32), "categories": cat,
            "diff_eq_tau": int((diff == dtype(tau)).sum())}
