"""Disparity post-filter on the host, numpy only: the restatement of include/dca_hip.h (dca_speckle_filter,
dca_median_filter) that the kernels of csrc/postfilter.hip equal bit for bit (tests/test_gpu_postfilter.py), and the
documented CPU path for a user without a ROCm device (`ops.speckle_filter` / `ops.median_filter` have no CPU fallback).

Both take ONE map (Hc,Wc) or a batch (B,Hc,Wc) / (B,1,Hc,Wc) of independent maps, float32, an optional mask of the same shape
with `mask_min`, and an optional window (y0, rows, cols) at frame row y0, column 0; outputs are (rows,cols) per image with
the leading dimensions of the input.  A window pixel is ACTIVE iff it is finite and (mask is None or mask >= mask_min)."""
import numpy as np

SPECKLE_OUTPUTS = ("disp", "valid", "size")


def _frame(name, disp, mask, mask_min, window):
    """(maps (B,rows,cols) float32 -- the window, active (B,rows,cols) bool, the leading shape of the outputs)"""
    d = np.asarray(disp)
    if d.dtype != np.float32 or d.ndim < 2 or d.size == 0:
        raise ValueError(f"{name}: expected a non-empty float32 (Hc,Wc), (B,Hc,Wc) or (B,1,Hc,Wc) map, got {d.dtype} {d.shape}")
    if d.ndim > 4 or (d.ndim == 4 and d.shape[1] != 1):
        raise ValueError(f"{name}: expected (Hc,Wc), (B,Hc,Wc) or (B,1,Hc,Wc), got {d.shape}")
    Hc, Wc = d.shape[-2:]
    y0, rows, cols = (0, Hc, Wc) if window is None else (int(v) for v in window)
    if y0 < 0 or rows <= 0 or cols <= 0 or y0 + rows > Hc or cols > Wc:
        raise ValueError(f"{name}: the {rows} x {cols} window at row {y0} does not fit the {Hc} x {Wc} map")
    lead = d.shape[:-2]
    w = d.reshape(-1, Hc, Wc)[:, y0:y0 + rows, :cols]
    with np.errstate(invalid="ignore"):
        active = np.abs(w) < np.inf                              # a NaN fails the comparison
    if mask is not None:
        m = np.asarray(mask)
        if m.dtype != np.float32 or m.shape != d.shape:
            raise ValueError(f"{name}: the mask must be float32 of the map's shape {d.shape}, got {m.dtype} {m.shape}")
        if np.isnan(mask_min):
            raise ValueError(f"{name}: mask_min must not be NaN")
        with np.errstate(invalid="ignore"):
            active &= m.reshape(-1, Hc, Wc)[:, y0:y0 + rows, :cols] >= np.float32(mask_min)
    return w, active, lead


def component_sizes(d, active, max_diff):
    """(rows,cols) float32 d, bool active -> int32 size of every pixel's component (0: inactive).  Union-find over all
    joined pairs at once: every pair hooks the larger of its two labels under the smaller one (labels only decrease and
    label[x] <= x), then the labels are flattened by pointer jumping; repeated until no pair has two labels."""
    rows, cols = d.shape
    n = rows * cols
    idx = np.arange(n, dtype=np.int64).reshape(rows, cols)
    md = np.float32(max_diff)
    pairs = []
    with np.errstate(invalid="ignore", over="ignore"):
        for a, b in ((np.s_[:, :-1], np.s_[:, 1:]), (np.s_[:-1, :], np.s_[1:, :])):
            join = active[a] & active[b] & (np.abs(d[a] - d[b]) <= md)        # float32 - float32, rounded to float32
            pairs.append((idx[a][join], idx[b][join]))
    u = np.concatenate([p[0] for p in pairs])
    v = np.concatenate([p[1] for p in pairs])
    label = np.arange(n, dtype=np.int64)
    while True:
        lu, lv = label[u], label[v]
        if np.array_equal(lu, lv):
            break
        lo = np.minimum(lu, lv)
        np.minimum.at(label, lu, lo)
        np.minimum.at(label, lv, lo)
        while True:
            nxt = label[label]
            if np.array_equal(nxt, label):
                break
            label = nxt
    size = np.bincount(label, minlength=n)[label].astype(np.int32).reshape(rows, cols)
    size[~active] = 0
    return size


def speckle_filter_host(disp, max_size, max_diff, mask=None, mask_min=0.5, window=None, fill=0.0, outputs=None):
    """The speckle filter: two 4-neighbours inside the window are joined iff both are active and |a - b| <= max_diff in
    float32 (equality joins; chained: a ramp with small steps is ONE component).  Returns a dict with the keys of `outputs`
    (default all; `valid` always):
      size   int32    the pixel's component size, 0 for an inactive pixel
      valid  float32  1.0 where active and size > max_size, 0.0 elsewhere
      disp   float32  the input bit for bit where valid, `fill` elsewhere"""
    name = "speckle_filter_host"
    max_size, max_diff = int(max_size), float(max_diff)
    if max_size < 0 or not 0.0 <= max_diff < np.inf:
        raise ValueError(f"{name}: max_size >= 0 and max_diff finite and >= 0, got {max_size} and {max_diff}")
    names = SPECKLE_OUTPUTS if outputs is None else tuple(outputs)
    if any(k not in SPECKLE_OUTPUTS for k in names):
        raise ValueError(f"{name}: outputs are chosen from {SPECKLE_OUTPUTS}, got {names}")
    w, active, lead = _frame(name, disp, mask, mask_min, window)
    size = np.stack([component_sizes(w[b], active[b], max_diff) for b in range(w.shape[0])])
    keep = active & (size > max_size)
    shape = lead + w.shape[1:]
    res = {"valid": keep.astype(np.float32).reshape(shape)}
    if "size" in names:
        res["size"] = size.reshape(shape)
    if "disp" in names:
        res["disp"] = np.where(keep, w, np.float32(fill)).astype(np.float32).reshape(shape)
    return res


def order_key(bits):
    """uint32 bits of float32 values -> the uint32 key whose unsigned order is the median's total order (-0.0 < +0.0)"""
    bits = np.asarray(bits, np.uint32)
    return bits ^ ((bits.view(np.int32) >> 31).view(np.uint32) | np.uint32(0x80000000))


def median_filter_host(disp, ksize, mask=None, mask_min=0.5, window=None):
    """The masked median: for an active centre the candidates are the active pixels of the ksize x ksize neighbourhood
    inside the window (no border replication); with n of them the output is the candidate of rank (n - 1) // 2 in the
    order of `order_key` -- the lower median for even n -- an input value bit for bit.  An inactive centre is copied
    unchanged.  ksize: 3 or 5.  Returns float32 (rows,cols) per image."""
    name = "median_filter_host"
    if ksize not in (3, 5):
        raise ValueError(f"{name}: ksize is 3 or 5, got {ksize!r}")
    w, active, lead = _frame(name, disp, mask, mask_min, window)
    B, rows, cols = w.shape
    R = ksize // 2
    none = np.int64(1) << 32                                     # above every key: the inactive candidates sort last
    keys = np.where(active, order_key(np.ascontiguousarray(w).view(np.uint32)).astype(np.int64), none)
    padded = np.full((B, rows + 2 * R, cols + 2 * R), none, np.int64)
    padded[:, R:R + rows, R:R + cols] = keys
    stack = np.sort(np.stack([padded[:, dy:dy + rows, dx:dx + cols] for dy in range(ksize) for dx in range(ksize)]), axis=0)
    n = (stack < none).sum(axis=0)
    rank = np.maximum(n - 1, 0) // 2
    k = np.take_along_axis(stack, rank[None], axis=0)[0]
    k = np.where(active, k, 0).astype(np.uint32)
    bits = np.where(k & np.uint32(0x80000000), k ^ np.uint32(0x80000000), ~k)
    out = np.where(active, bits.view(np.float32), w).astype(np.float32)
    # np.where on float32 copies bits, NaN payloads included
    return out.reshape(lead + (rows, cols))
