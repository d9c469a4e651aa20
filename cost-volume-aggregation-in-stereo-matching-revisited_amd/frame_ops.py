"""The operators around the network, each a thin host wrapper over the C ABI of libdca_hip.so (include/dca_hip.h):
evaluation metrics, risk-coverage histogram, left-right consistency, self-supervised loss, inference frame I/O,
rectification, training inputs, depth and point cloud, LiDAR ground truth, post-filter, pictures.  ops.py re-exports every
public name, so callers say `ops.disp_export`.  Nothing here carries autograd except the self-supervised loss; no launch
synchronises; all buffers are torch's.

Arguments are validated by the helpers at the top, one per kind of check, and a refusal names the operator.  As in ops.py,
a tensor that is not on a ROCm device is an error, never a detour through eager PyTorch.
"""
from __future__ import annotations

import ctypes
import math

import torch

from . import geometry as _geometry
from ._call import _C, _L, _chk, _ptr, _req, _req_no_grad, _stream


# ------------------------------------------------------------------------------------------------
# Argument checks, one of each kind
# ------------------------------------------------------------------------------------------------
def _req_dev(t, name, what, dtype, shape=None, like=None):
    """t as it is (no copy is made): a contiguous tensor on the ROCm device of `dtype` (one, or a tuple to choose from),
    of `shape` and on the device of `like` where those are given"""
    dtypes = dtype if isinstance(dtype, tuple) else (dtype,)
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name}: {what} must be on the ROCm device; there is no CPU fallback")
    if t.dtype not in dtypes or not t.is_contiguous():
        raise RuntimeError(f"{name}: {what} must be a contiguous {' or '.join(str(d) for d in dtypes)} tensor, got {t.dtype}"
                           f"{'' if t.is_contiguous() else ' (not contiguous)'}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise RuntimeError(f"{name}: {what} must have shape {tuple(shape)}, got {tuple(t.shape)}")
    if like is not None and t.device != like.device:
        raise RuntimeError(f"{name}: {what} must be on the input's device {like.device}, got {t.device}")
    return t


def _req_f32_same(name, a, b, what):
    """two contiguous float32 tensors of one non-empty shape on one ROCm device, as they are (no copy is made)"""
    _req_dev(a, name, what, torch.float32)
    _req_dev(b, name, what, torch.float32, like=a)
    if a.shape != b.shape or a.numel() == 0:
        raise RuntimeError(f"{name}: {what} must have one non-empty shape, got {tuple(a.shape)} and {tuple(b.shape)}")


def _req_u8(t, name, what, like=None):
    """an interleaved (H,W,3) / (H,W,4) uint8 image with H * W < 2^31 -> (H, W, C)"""
    _req_dev(t, name, what, torch.uint8, like=like)
    if t.dim() != 3 or t.shape[2] not in (3, 4) or t.numel() == 0 or t.shape[0] * t.shape[1] >= 1 << 31:
        raise RuntimeError(f"{name}: {what} must be a (H,W,3) or (H,W,4) uint8 image with H * W below 2^31, got {tuple(t.shape)}")
    return tuple(int(s) for s in t.shape)


def _req_u8_pair(left, right, name):
    shape = _req_u8(left, name, "the left image")
    if _req_u8(right, name, "the right image") != shape:
        raise RuntimeError(f"{name}: expected two (H,W,3) or (H,W,4) uint8 images of one shape, got {tuple(left.shape)} and "
                           f"{tuple(right.shape)}")
    return shape


def _fit(name, Hc, Wc, y0, x0, rows, cols, what, empty=False):
    """(y0, x0, rows, cols) as ints: a rows x cols window at row y0, column x0 inside the Hc x Wc `what`, Hc * Wc < 2^31
    (pixel offsets are 32-bit); `empty` admits rows == 0 or cols == 0"""
    try:
        y0, x0, rows, cols = int(y0), int(x0), int(rows), int(cols)
    except (TypeError, ValueError):
        raise RuntimeError(f"{name}: a window is given in whole numbers, got {(y0, x0, rows, cols)!r}") from None
    if min(y0, x0) < 0 or min(rows, cols) < (0 if empty else 1) or y0 + rows > Hc or x0 + cols > Wc or min(Hc, Wc) < 1 \
            or Hc * Wc >= 1 << 31:
        raise RuntimeError(f"{name}: the {rows} x {cols} window at ({y0}, {x0}) does not fit the {Hc} x {Wc} {what} (of fewer "
                           "than 2^31 pixels)")
    return y0, x0, rows, cols


def _window(name, Hc, Wc, window, what):
    """window = (y0, rows, cols), columns from 0, default the whole Hc x Wc `what` -> (y0, rows, cols) as `_fit` has them"""
    try:
        y0, rows, cols = (0, Hc, Wc) if window is None else window
    except (TypeError, ValueError):
        raise RuntimeError(f"{name}: window is (y0, rows, cols), got {window!r}") from None
    y0, _, rows, cols = _fit(name, Hc, Wc, y0, 0, rows, cols, what)
    return y0, rows, cols


def _maps(name, disp, mask, batched, max_batch=None, what="the disparity", inference=True):
    """the float32 map(s) (...,Hc,Wc) and the optional mask of the same shape -> (B, Hc, Wc) of a batch of at most max_batch
    maps, or of ONE frame (B = 1)"""
    if inference:
        _req_no_grad(name, disp, mask)
    _req_dev(disp, name, what, torch.float32)
    if disp.dim() < 2 or disp.numel() == 0:
        raise RuntimeError(f"{name}: expected a (Hc,Wc) map{' or a (B,Hc,Wc) batch' if batched else ''}, got {tuple(disp.shape)}")
    Hc, Wc = int(disp.shape[-2]), int(disp.shape[-1])
    B = disp.numel() // (Hc * Wc)
    if B != 1 and not batched:
        raise RuntimeError(f"{name}: expected the (Hc,Wc) map of one frame, got {tuple(disp.shape)}")
    if max_batch is not None and B > max_batch:
        raise RuntimeError(f"{name}: at most {max_batch} maps, got {B}")
    if mask is not None:
        _req_f32_same(name, disp, mask, f"{what} and the mask")
    return B, Hc, Wc


def _mask_min(name, mask_min, masked=True):
    """mask_min as a float; NaN is refused where a mask is compared with it"""
    mask_min = float(mask_min)
    if masked and math.isnan(mask_min):
        raise RuntimeError(f"{name}: mask_min must not be NaN")
    return mask_min


def _out(name, what, given, dtype, shape, like, alias=()):
    """the caller's buffer `given` after checking it (dtype, shape, on `like`'s device, not the storage of a tensor in
    `alias`), or a fresh one"""
    if given is None:
        return torch.empty(shape, device=like.device, dtype=dtype)
    _req_dev(given, name, what, dtype, shape, like=like)
    if any(given.untyped_storage().data_ptr() == t.untyped_storage().data_ptr() for t in alias):
        raise RuntimeError(f"{name}: {what} must be a buffer of its own: it must not alias an input (the operator is not in place)")
    return given


def _out_dict(name, kinds, always, outputs, out, shape_of, like):
    """{key: tensor} for the keys of `kinds` (key -> dtype, in the library's order) that are in `outputs` (default all) or in
    `always`: the caller's out[key] after checking it, or a fresh tensor of shape_of(key)"""
    names = tuple(kinds) if outputs is None else tuple(outputs)
    if any(n not in kinds for n in names):
        raise RuntimeError(f"{name}: outputs are chosen from {tuple(kinds)}, got {names}")
    out = {} if out is None else out
    if not isinstance(out, dict) or set(out) - set(kinds):
        raise RuntimeError(f"{name}: out must be a dict with keys out of {tuple(kinds)}")
    return {k: _out(name, f"out[{k!r}]", out.get(k), kinds[k], shape_of(k), like) for k in kinds if k in names or k in always}


def _workspace(name, what, t, words, like):
    """an int32 buffer of at least `words` words on `like`'s device"""
    _req_dev(t, name, what, torch.int32, like=like)
    if t.numel() < words:
        raise RuntimeError(f"{name}: {what} must hold at least {words} int32, got {t.numel()}")
    return t


def _pred_over_gt(name, pred, gt):
    """pred (B,Hp,Wp) or (B,1,Hp,Wp), padded on top and on the right, over gt (B,H,W) -> (pred (B,Hp,Wp), gt, B, H, W, Hp, Wp)"""
    pred, gt = _req(pred, name), _req(gt, name)
    if pred.dim() == 4 and pred.shape[1] == 1:
        pred = pred[:, 0]
    if pred.dim() != 3 or gt.dim() != 3 or pred.shape[0] != gt.shape[0]:
        raise RuntimeError(f"{name}: expected pred (B,Hp,Wp) and gt (B,H,W), got {tuple(pred.shape)} and {tuple(gt.shape)}")
    (B, Hp, Wp), (H, W) = pred.shape, gt.shape[1:]
    if Hp < H or Wp < W:
        raise RuntimeError(f"{name}: the prediction is smaller than the ground truth")
    return pred, gt, B, H, W, Hp, Wp


# ------------------------------------------------------------------------------------------------
# Evaluation step (main_dca.py:143-246 `mytest`): disparity metrics, region confusion matrices, run state
# (csrc/eval_metrics.hip; state layout in include/dca_hip.h).  No launch synchronises; all buffers are torch's.
# ------------------------------------------------------------------------------------------------
EVAL_REC = _C["DCA_EVAL_REC"]
EVAL_STATE_HEAD = _C["DCA_EVAL_STATE_HEAD"]
EVAL_MAX_CLASSES = _C["DCA_EVAL_MAX_CLASSES"]


def disp_metrics(pred, gt, maxdisp, mask=None):
    """Per-image error statistics of a (padded) prediction against the ground truth in one pass: pred (B,Hp,Wp) or
    (B,1,Hp,Wp) with Hp >= H, Wp >= W (rows padded on top, columns on the right: the crop of main_dca.py:171-174 is
    done by addressing), gt (B,H,W), mask bool (B,H,W) or None (gt > 0 & gt < maxdisp).  Returns (B,8) float64:
    #mask, #(gt>0), sum e, sum smooth_l1(e), #(e>1), #(e>2), #(e>3), #(e>3 & e/|gt|>0.05), e = |pred - gt| in fp32."""
    pred, gt, B, H, W, Hp, Wp = _pred_over_gt("disp_metrics", pred, gt)
    if mask is not None:
        mask = mask.contiguous() if isinstance(mask, torch.Tensor) else mask       # a strided mask is copied
        _req_dev(mask, "disp_metrics", "the mask", torch.bool, gt.shape)
    rec = torch.empty((B, EVAL_REC), device=gt.device, dtype=torch.float64)
    with torch.cuda.device_of(gt):
        ws = torch.empty(_L().dca_disp_metrics_workspace(B, H, W), device=gt.device, dtype=torch.uint8)
        _chk(_L().dca_disp_metrics(_ptr(pred), _ptr(gt), _ptr(mask), _ptr(rec), _ptr(ws), B, H, W, Hp - H, Wp - W,
                                   float(maxdisp), _stream()), "dca_disp_metrics")
    return rec


def region_confusion(volumes, gt):
    """Confusion matrices of 1..3 region-probability volumes (B,C,hp,wp) (or (B,1,C,hp,wp)) at 1/8 resolution against
    label = floor(adaptive_avg_pool2d(gt / 8, (H//8, W//8))), gt (B,H,W); prediction = arg-max over C at row
    i + (hp - H//8), column j.  Returns (len(volumes), C, C) int64, rows = label, columns = prediction."""
    if isinstance(volumes, torch.Tensor):
        volumes = [volumes]
    vols = []
    for v in volumes:
        v = _req(v, "region_confusion")
        vols.append(v[:, 0] if v.dim() == 5 and v.shape[1] == 1 else v)
    gt = _req(gt, "region_confusion")
    if not 1 <= len(vols) <= 3 or any(v.dim() != 4 or v.shape != vols[0].shape for v in vols):
        raise RuntimeError("region_confusion: expected 1 to 3 volumes (B,C,hp,wp) of one shape")
    (B, C, hp, wp), (H, W) = vols[0].shape, gt.shape[1:]
    if gt.dim() != 3 or gt.shape[0] != B or H < 8 or W < 8 or hp < H // 8 or wp < W // 8 or C > EVAL_MAX_CLASSES:
        raise RuntimeError(f"region_confusion: volumes {tuple(vols[0].shape)} do not fit the ground truth {tuple(gt.shape)} "
                           f"(C <= {EVAL_MAX_CLASSES})")
    cm = torch.empty((len(vols), C, C), device=gt.device, dtype=torch.int64)
    p = [_ptr(v) for v in vols] + [None] * (3 - len(vols))
    with torch.cuda.device_of(gt):
        _chk(_L().dca_region_confusion(p[0], p[1], p[2], _ptr(gt), _ptr(cm), len(vols), B, C, hp, wp, H, W, _stream()),
             "dca_region_confusion")
    return cm


def eval_state(num_classes, device):
    """zeroed run state of `eval_accumulate` (float64; layout: include/dca_hip.h)"""
    n = _L().dca_eval_state_len(int(num_classes))
    if n <= 0:
        raise RuntimeError(f"eval_state: 1 <= num_classes <= {EVAL_MAX_CLASSES}")
    return torch.zeros(n, device=device, dtype=torch.float64)


def eval_accumulate(state, rec, cm, gt_shape):
    """Adds one batch -- rec of `disp_metrics`, cm of `region_confusion` -- to the run state, in place."""
    for t, dt, what in ((state, torch.float64, "state"), (rec, torch.float64, "rec"), (cm, torch.int64, "cm")):
        _req_dev(t, "eval_accumulate", what, dt)
    nvol, C = cm.shape[0], cm.shape[1]
    if state.numel() != _L().dca_eval_state_len(C) or rec.dim() != 2 or rec.shape[1] != EVAL_REC or cm.shape[2] != C:
        raise RuntimeError("eval_accumulate: state / rec / cm do not fit together")
    with torch.cuda.device_of(state):
        _chk(_L().dca_eval_accumulate(_ptr(rec), _ptr(cm), _ptr(state), rec.shape[0], nvol, C, int(gt_shape[-2]),
                                      int(gt_shape[-1]), _stream()), "dca_eval_accumulate")
    return state


CONF_MAX_BINS = _C["DCA_CONF_MAX_BINS"]
CONF_ERR_SCALE = _C["DCA_CONF_ERR_SCALE"]     # the error sums of `conf_histogram` are in units of 2^-20 pixels


def conf_histogram(conf, pred, gt, state, maxdisp):
    """Adds the pixels of one batch to a risk-coverage state, in place: conf, pred, gt float32 of one shape, state
    (nbins,3) int64 on the device.  Per confidence bin min(nbins-1, int(clamp(conf,0,1) * nbins)): the count of pixels
    with 0 < gt < maxdisp and a confidence that is not NaN, the sum of trunc(|pred - gt| * 2^20) and the count of
    |pred - gt| > 3.  Integer atomics only: bitwise reproducible.  One launch, no synchronisation."""
    conf, pred, gt = (_req(t, "conf_histogram") for t in (conf, pred, gt))
    if conf.shape != pred.shape or conf.shape != gt.shape or conf.numel() == 0:
        raise RuntimeError(f"conf_histogram: conf, pred and gt must have one non-empty shape, got {tuple(conf.shape)}, "
                           f"{tuple(pred.shape)} and {tuple(gt.shape)}")
    _req_dev(state, "conf_histogram", "the state", torch.int64)
    if any(t.device != conf.device for t in (pred, gt, state)):
        raise RuntimeError(f"conf_histogram: conf, pred, gt and the state must be on one device, got {conf.device}, "
                           f"{pred.device}, {gt.device} and {state.device}")
    if state.dim() != 2 or state.shape[1] != 3 or not 2 <= state.shape[0] <= CONF_MAX_BINS:
        raise RuntimeError(f"conf_histogram: the state must be (nbins,3), 2 <= nbins <= {CONF_MAX_BINS}, got {tuple(state.shape)}")
    with torch.cuda.device_of(conf):
        _chk(_L().dca_conf_histogram(_ptr(conf), _ptr(pred), _ptr(gt), _ptr(state), 1, conf.numel(), state.shape[0],
                                     float(maxdisp), _stream()), "dca_conf_histogram")
    return state


# ------------------------------------------------------------------------------------------------
# Left-right consistency (csrc/lr_consistency.hip): inference only, no counterpart in the reference
# ------------------------------------------------------------------------------------------------
LR_MAX_W = _C["DCA_LR_MAX_W"]
LR_OUTPUTS = ("diff", "valid", "filled", "disp_right")
_LR_KINDS = dict.fromkeys(LR_OUTPUTS, torch.float32)


def mirror_pair(left, right, out=None):
    """(left, right) (...,H,W) float32 -> (flipW(right), flipW(left)), bit copies, one launch: the mirrored, swapped pair on
    which the unchanged network computes the RIGHT view's disparity in mirrored coordinates (include/dca_hip.h).
    out: a contiguous float32 (2, *left.shape) buffer to write into (allocated when None); the results are its two halves."""
    _req_no_grad("mirror_pair", left, right)
    _req_f32_same("mirror_pair", left, right, "left and right")
    if left.dim() < 2:
        raise RuntimeError(f"mirror_pair: expected (...,H,W) images, got {tuple(left.shape)}")
    out = _out("mirror_pair", "out", out, torch.float32, (2,) + tuple(left.shape), left, alias=(left, right))
    H, W = int(left.shape[-2]), int(left.shape[-1])
    with torch.cuda.device_of(left):
        _chk(_L().dca_mirror_pair(_ptr(left), _ptr(right), _ptr(out[0]), _ptr(out[1]), left.numel() // (H * W), H, W,
                                  _stream()), "dca_mirror_pair")
    return out[0], out[1]


def lr_consistency(disp_left, disp_right_mirrored, tau=1.0, cols=None, outputs=None):
    """Cross-check of a left disparity map against the right view's, invalidation and background fill, ONE launch
    (definitions: include/dca_hip.h, dca_lr_consistency).  disp_left, disp_right_mirrored: (B,1,H,W) or (B,H,W) float32;
    the second is what the network gives on `mirror_pair(left, right)`: right-image column i at index W-1-i.  tau: finite,
    >= 0.  cols (default W): only columns [0, cols) of either image take part (a frame zero-padded on the right).
    Returns a dict of maps shaped like the input: `diff` (|d - r|, +inf out of view), `valid` (1.0 / 0.0), `filled`
    (valid pixels bit for bit; invalid ones from the nearest valid neighbours in the row, the smaller of the two) and
    `disp_right` (the right view's disparity in its own coordinates).  outputs: the names wanted (default all four;
    `valid` is always computed) -- the others are neither computed nor written.  W <= 8192.  Bitwise reproducible."""
    _req_no_grad("lr_consistency", disp_left, disp_right_mirrored)
    _req_f32_same("lr_consistency", disp_left, disp_right_mirrored, "the two disparity maps")
    shape = tuple(disp_left.shape)
    if len(shape) not in (3, 4) or (len(shape) == 4 and shape[1] != 1):
        raise RuntimeError(f"lr_consistency: expected (B,1,H,W) or (B,H,W) disparity maps, got {shape}")
    B, H, W = shape[0], shape[-2], shape[-1]
    tau = float(tau)
    if not (0.0 <= tau < math.inf):
        raise RuntimeError(f"lr_consistency: tau must be finite and >= 0, got {tau}")
    cols = W if cols is None else int(cols)
    if not 1 <= cols <= W or W > LR_MAX_W:
        raise RuntimeError(f"lr_consistency: 1 <= cols <= W <= {LR_MAX_W}, got cols {cols} and W {W}")
    res = _out_dict("lr_consistency", _LR_KINDS, ("valid",), outputs, None, lambda k: shape, disp_left)
    with torch.cuda.device_of(disp_left):
        _chk(_L().dca_lr_consistency(_ptr(disp_left), _ptr(disp_right_mirrored), *(_ptr(res.get(n)) for n in LR_OUTPUTS),
                                     B, H, W, cols, tau, _stream()), "dca_lr_consistency")
    return res


# ------------------------------------------------------------------------------------------------
# Self-supervised loss (csrc/selfsup.hip): view synthesis + edge-aware smoothness, all levels of a
# step in one launch per direction.  The smoothness term is the reference's util.py:76-86; the rest has no counterpart.
# ------------------------------------------------------------------------------------------------
SELFSUP_MAX_LEVELS = _C["DCA_SELFSUP_MAX_LEVELS"]
SELFSUP_TILE = (_C["DCA_SELFSUP_TILE_H"], _C["DCA_SELFSUP_TILE_W"])
SELFSUP_SUMS = _C["DCA_SELFSUP_SUMS"]
SELFSUP_OUT = _C["DCA_SELFSUP_OUT"]
SELFSUP_MAX_SAMPLE = (1 << 31) - 1          # 3 H W, the elements of one sample's image: offsets inside a sample are 32-bit


def _selfsup_check(left, right, disps, weights, valid, scalars):
    """validates the arguments of `selfsup_loss`; returns (B, H, W, weights as floats, valid_u8)"""
    name = "selfsup_loss"
    _req_dev(left, name, "the left image", torch.float32)
    _req_dev(right, name, "the right image", torch.float32, like=left)
    if left.dim() != 4 or left.shape[1] != 3 or left.shape != right.shape:
        raise RuntimeError(f"{name}: expected two (B,3,H,W) images of one shape, got {tuple(left.shape)} and {tuple(right.shape)}")
    B, _, H, W = (int(s) for s in left.shape)
    if B < 1 or H < 3 or W < 3:
        raise RuntimeError(f"{name}: the 3x3 windows need B >= 1, H >= 3 and W >= 3, got {tuple(left.shape)}")
    if 3 * H * W > SELFSUP_MAX_SAMPLE or W > 1 << 24 or B > 65535:
        raise RuntimeError(f"{name}: 3 H W <= {SELFSUP_MAX_SAMPLE} (offsets inside a sample are 32-bit), W <= 2^24 and "
                           f"B <= 65535, got {tuple(left.shape)}")
    disps = list(disps)
    if not 1 <= len(disps) <= SELFSUP_MAX_LEVELS or len(weights) != len(disps):
        raise RuntimeError(f"{name}: 1 to {SELFSUP_MAX_LEVELS} disparity maps with one weight each, got {len(disps)} maps and "
                           f"{len(weights)} weights")
    maps = [(d, "a disparity map", torch.float32) for d in disps]
    if valid is not None:
        maps.append((valid, "valid", (torch.float32, torch.bool)))
    for t, what, dtype in maps:
        _req_dev(t, name, what, dtype, like=left)
        if tuple(t.shape) not in ((B, H, W), (B, 1, H, W)):
            raise RuntimeError(f"{name}: {what} must be ({B},{H},{W}) or ({B},1,{H},{W}), got {tuple(t.shape)}")
    if valid is not None and valid.requires_grad:
        raise RuntimeError(f"{name}: valid carries no gradient")
    valid_u8 = int(valid is not None and valid.dtype == torch.bool)
    alpha, lam, c1, c2 = scalars
    if not (0.0 <= alpha <= 1.0) or not (c1 > 0.0 and c2 > 0.0) or lam != lam:
        raise RuntimeError(f"{name}: 0 <= alpha <= 1, c1 > 0, c2 > 0 and a lam that is a number, got alpha {alpha}, lam {lam}, "
                           f"c1 {c1}, c2 {c2}")
    return B, H, W, [float(w) for w in weights], valid_u8


class _SelfSupLoss(torch.autograd.Function):
    """sum_l w_l (photo_scale photo_l + lam smooth_l) and the detached (L,3) per-level (photo, smooth, sum M)"""

    @staticmethod
    def forward(ctx, left, right, valid, weights, scalars, photo_scale, *disps):
        B, H, W, weights, valid_u8 = _selfsup_check(left, right, disps, weights, valid, scalars)
        n = len(disps)
        tiles = -(-H // SELFSUP_TILE[0]) * -(-W // SELFSUP_TILE[1])
        work = torch.empty((n * B * tiles * SELFSUP_SUMS,), device=left.device, dtype=torch.float64)
        out = torch.empty((n * SELFSUP_OUT + 1,), device=left.device, dtype=torch.float32)
        dptr = (ctypes.c_void_p * n)(*[d.data_ptr() for d in disps])
        wts = (ctypes.c_float * n)(*weights)
        with torch.cuda.device_of(left):
            _chk(_L().dca_selfsup_loss_fwd(_ptr(left), _ptr(right), dptr, wts, n, _ptr(valid), valid_u8, _ptr(work), _ptr(out),
                                           B, H, W, *scalars, photo_scale, _stream()), "dca_selfsup_loss_fwd")
        ctx.save_for_backward(left, right, valid, out, *disps)
        ctx.meta = (B, H, W, weights, valid_u8, scalars, photo_scale)
        stats = out[:n * SELFSUP_OUT].view(n, SELFSUP_OUT)[:, :3]
        ctx.mark_non_differentiable(stats)
        return out[n * SELFSUP_OUT], stats

    @staticmethod
    def backward(ctx, gloss, _gstats):
        left, right, valid, out, *disps = ctx.saved_tensors
        B, H, W, weights, valid_u8, scalars, photo_scale = ctx.meta
        n = len(disps)
        gloss = _req(gloss.reshape(1), "selfsup_loss.backward")
        gds = [torch.empty_like(d) for d in disps]
        dptr = (ctypes.c_void_p * n)(*[d.data_ptr() for d in disps])
        gptr = (ctypes.c_void_p * n)(*[g.data_ptr() for g in gds])
        wts = (ctypes.c_float * n)(*weights)
        with torch.cuda.device_of(left):
            _chk(_L().dca_selfsup_loss_bwd(_ptr(left), _ptr(right), dptr, gptr, wts, n, _ptr(valid), valid_u8, _ptr(out),
                                           _ptr(gloss), B, H, W, *scalars, photo_scale, _stream()), "dca_selfsup_loss_bwd")
        return (None,) * 6 + tuple(gds)


def selfsup_loss(left, right, disps, weights, valid=None, alpha=0.85, lam=0.1, c1=1e-4, c2=9e-4, photo_scale=1.0):
    """Self-supervised stereo loss of up to 8 disparity maps in one launch per direction (definitions: include/dca_hip.h,
    dca_selfsup_loss_fwd): sum_l weights[l] (photo_l + lam smooth_l), where photo_l compares `left` with `right` warped
    along the row by disps[l] (alpha SSIM over 3x3 windows + (1 - alpha) L1, at interior pixels that are in view and
    `valid`) and smooth_l is the reference's edge-aware `loss_disp_smoothness` (util.py:76-86).
    left, right: (B,3,H,W) float32, used as given; disps: (B,H,W) or (B,1,H,W) contiguous float32, full-resolution pixels;
    valid: (B,H,W) float32 or bool, no gradient, default all ones; photo_scale: 1, or 0 for the smoothness term alone.
    3 H W < 2^31 per sample.  Returns (loss, stats): a 0-dim float32 tensor with a gradient to the disparity maps only,
    and the detached (L,3) float32 per-level (photo, smooth, sum M) for logging.  Bitwise reproducible; no host
    synchronisation; graph-capturable."""
    scalars = (float(alpha), float(lam), float(c1), float(c2))
    return _SelfSupLoss.apply(left, right, valid, tuple(float(w) for w in weights), scalars, float(photo_scale), *disps)


# ------------------------------------------------------------------------------------------------
# Inference frame I/O (my_img.py:47-110 around the model call): per-plane normalisation as histogram -> table -> look-up,
# placement in the zero-padded frame, export of the cropped disparity (csrc/frame_io.hip).  No launch synchronises.
# ------------------------------------------------------------------------------------------------
def frame_histogram(left_u8, right_u8):
    """Histograms of the colour planes of two interleaved (H,W,C) uint8 images, C = 3 or 4 (a fourth channel is ignored).
    Returns (2,3,256) int32 counts (image, plane, value); bitwise reproducible."""
    H, W, C = _req_u8_pair(left_u8, right_u8, "frame_histogram")
    hist = torch.empty((2, 3, 256), device=left_u8.device, dtype=torch.int32)
    with torch.cuda.device_of(left_u8):
        _chk(_L().dca_frame_hist(_ptr(left_u8), _ptr(right_u8), _ptr(hist), H, W, C, _stream()), "dca_frame_hist")
    return hist


def frame_lut(hist, n_pixels):
    """hist of `frame_histogram` and the pixel count H*W -> (lut (2,3,256) float32, stats (2,3,2) float64 = mean, std):
    lut[i,c,v] = float32((v - mean) / std) in fp64 with the population std (my_img.py:59-68);
    inference.lut_from_histogram is its numpy restatement, equal bit for bit."""
    _req_dev(hist, "frame_lut", "hist", torch.int32, (2, 3, 256))
    if not 0 < int(n_pixels) < 1 << 31:
        raise RuntimeError("frame_lut: 0 < n_pixels < 2^31")
    lut = torch.empty((2, 3, 256), device=hist.device, dtype=torch.float32)
    stats = torch.empty((2, 3, 2), device=hist.device, dtype=torch.float64)
    with torch.cuda.device_of(hist):
        _chk(_L().dca_frame_lut(_ptr(hist), int(n_pixels), _ptr(lut), _ptr(stats), _stream()), "dca_frame_lut")
    return lut, stats


def frame_apply(left_u8, right_u8, lut, frame_hw, src_y0, dst_y0, rows, cols, out=None):
    """Table look-up and placement: the rows x cols window of the (H,W,C) uint8 images starting at source row src_y0,
    column 0, goes through lut (2,3,256) into the planar frames at row dst_y0, column 0; every other frame element
    becomes +0.0.  out: (2,3,Hc,Wc) float32, written whole (allocated when None).  Returns the (1,3,Hc,Wc) views
    (left, right) of it, the tensors `GwcNet.forward` takes."""
    H, W, C = _req_u8_pair(left_u8, right_u8, "frame_apply")
    Hc, Wc = int(frame_hw[0]), int(frame_hw[1])
    _req_dev(lut, "frame_apply", "lut", torch.float32, (2, 3, 256))
    src_y0, _, rows, cols = _fit("frame_apply", H, W, src_y0, 0, rows, cols, "source", empty=True)
    dst_y0 = _fit("frame_apply", Hc, Wc, dst_y0, 0, rows, cols, "frame", empty=True)[0]
    out = _out("frame_apply", "out", out, torch.float32, (2, 3, Hc, Wc), left_u8)
    with torch.cuda.device_of(left_u8):
        _chk(_L().dca_frame_apply(_ptr(left_u8), _ptr(right_u8), _ptr(lut), _ptr(out[0]), _ptr(out[1]), H, W, C, Hc, Wc,
                                  src_y0, dst_y0, rows, cols, _stream()), "dca_frame_apply")
    return out[0:1], out[1:2]


def disp_export(pred, y0, h, w, scale=256.0, f32=True, u16=False, out_f32=None, out_u16=None):
    """The h x w window of the prediction (Hc,Wc) / (1,1,Hc,Wc) starting at row y0, column 0 (my_img.py:105-108), as
    float32 (bit copy) and / or uint16(pred * scale) (my_img.py:110; truncated, saturated to [0, 65535], NaN -> 0).
    Returns (float32 (h,w) or None, uint16 (h,w) or None); out_f32 / out_u16: buffers of that shape to write into."""
    _, Hc, Wc = _maps("disp_export", pred, None, False, what="the prediction", inference=False)
    y0, h, w = _window("disp_export", Hc, Wc, (y0, h, w), "prediction")
    if not (f32 or u16):
        raise RuntimeError("disp_export: nothing to export (f32 and u16 are both off)")
    of = _out("disp_export", "out_f32", out_f32, torch.float32, (h, w), pred) if f32 else None
    ou = _out("disp_export", "out_u16", out_u16, torch.uint16, (h, w), pred) if u16 else None
    with torch.cuda.device_of(pred):
        _chk(_L().dca_disp_export(_ptr(pred), _ptr(of), _ptr(ou), Hc, Wc, y0, h, w, float(scale), _stream()),
             "dca_disp_export")
    return of, ou


# ------------------------------------------------------------------------------------------------
# Rectification of a raw pair in front of the frame I/O (csrc/rectify.hip): one launch gathers both
# images through the fixed-point maps of a geometry.RectifyMaps.  No launch synchronises.
# ------------------------------------------------------------------------------------------------
RECT_MAX_SRC = _C["DCA_RECT_MAX_SRC"]


def _overlap(a, b):
    return a.data_ptr() < b.data_ptr() + b.numel() * b.element_size() and \
        b.data_ptr() < a.data_ptr() + a.numel() * a.element_size()


def rectify_pair(left_u8, right_u8, maps, out=None):
    """The raw (Hs,Ws,C) uint8 pair, C = 3 or 4, through `maps` (a geometry.RectifyMaps with src_hw == (Hs,Ws)) -> the two
    rectified (Hd,Wd,C) uint8 images, one launch: bilinear with 5 fractional bits per axis, zero outside the source, a
    fourth channel 255 (definitions: include/dca_hip.h, dca_rectify_pair; geometry.rectify_pair_host is the numpy
    restatement, equal bit for bit).  out: a (2,Hd,Wd,C) uint8 buffer or a pair of (Hd,Wd,C) buffers to write into, which
    must not overlap the inputs or each other.  With `out` given and the maps already on the device (their first use uploads
    them) nothing is allocated and the host never waits: the launch can be captured into a hipGraph."""
    name = "rectify_pair"
    Hs, Ws, C = _req_u8_pair(left_u8, right_u8, name)
    if not hasattr(maps, "device_maps") or not hasattr(maps, "src_hw"):
        raise RuntimeError(f"{name}: maps must be a geometry.RectifyMaps, got {type(maps)}")
    if (Hs, Ws) != tuple(maps.src_hw):
        raise RuntimeError(f"{name}: the maps were built for {maps.src_hw[0]} x {maps.src_hw[1]} images, got {Hs} x {Ws}")
    if left_u8.device != right_u8.device:
        raise RuntimeError(f"{name}: the two images must be on one device")
    Hd, Wd = maps.dst_hw
    if max(Hs, Ws) > RECT_MAX_SRC or Hs * Ws * C >= 1 << 31 or Hd * Wd * C >= 1 << 31:
        raise RuntimeError(f"{name}: the source may be at most {RECT_MAX_SRC} x {RECT_MAX_SRC} and every image must stay "
                           "below 2^31 bytes")
    if out is None:
        out = torch.empty((2, Hd, Wd, C), device=left_u8.device, dtype=torch.uint8)
    if not isinstance(out, (torch.Tensor, tuple, list)) or len(out) != 2:
        raise RuntimeError(f"{name}: out must be a (2,{Hd},{Wd},{C}) uint8 buffer or a pair of ({Hd},{Wd},{C}) buffers")
    ol, orr = (_req_dev(out[i], name, f"out[{i}]", torch.uint8, (Hd, Wd, C), like=left_u8) for i in (0, 1))
    if any(_overlap(t, u) for t in (ol, orr) for u in (left_u8, right_u8)) or _overlap(ol, orr):
        raise RuntimeError(f"{name}: out[0] and out[1] must not alias an input image or each other")
    dmaps, plane = maps.device_maps(left_u8.device)
    with torch.cuda.device_of(left_u8):
        _chk(_L().dca_rectify_pair(_ptr(left_u8), _ptr(right_u8), _ptr(dmaps), plane, _ptr(ol), _ptr(orr), Hs, Ws, Hd, Wd, C,
                                   _stream()), "dca_rectify_pair")
    return ol, orr


# ------------------------------------------------------------------------------------------------
# Training inputs (dataloader/datasets.py:221-254, 270-317 after the decode): photometric augmentation as one byte table
# per image, crop, occlusion patch, normalisation, ground-truth crop and mask (csrc/train_io.hip).  No launch synchronises;
# dcanet_amd.training holds the numpy restatements and the TrainInput / TrainStep classes built on these.
# ------------------------------------------------------------------------------------------------
def train_luma_sum(left_u8, right_u8, bg):
    """Sum of PIL's convert("L") of each image after its byte table bg (2,256) uint8 (gamma o brightness): (2,) int64,
    S[i] = sum over pixels of (19595 R' + 38470 G' + 7471 B' + 32768) >> 16 with X' = bg[i][X]."""
    H, W, C = _req_u8_pair(left_u8, right_u8, "train_luma_sum")
    _req_dev(bg, "train_luma_sum", "bg", torch.uint8, (2, 256))
    S = torch.empty(2, device=left_u8.device, dtype=torch.int64)
    with torch.cuda.device_of(left_u8):
        _chk(_L().dca_train_luma_sum(_ptr(left_u8), _ptr(right_u8), _ptr(bg), _ptr(S), H, W, C, _stream()),
             "dca_train_luma_sum")
    return S


def train_tables(S, n_pixels, bg, contrast, norm):
    """S of `train_luma_sum`, the pixel count, bg (2,256) uint8, the two contrast factors and norm (2,3,256) float32 ->
    (U (2,256) uint8 = contrast o bg, T (2,3,256) float32 = norm o U); training.contrast_table restates the blend."""
    _req_dev(S, "train_tables", "S", torch.int64, (2,))
    _req_dev(bg, "train_tables", "bg", torch.uint8, (2, 256))
    _req_dev(norm, "train_tables", "norm", torch.float32, (2, 3, 256))
    f0, f1 = float(contrast[0]), float(contrast[1])
    if not 0 < int(n_pixels) < 1 << 31 or not (math.isfinite(f0) and math.isfinite(f1)):
        raise RuntimeError("train_tables: 0 < n_pixels < 2^31 and finite contrast factors")
    U = torch.empty((2, 256), device=S.device, dtype=torch.uint8)
    T = torch.empty((2, 3, 256), device=S.device, dtype=torch.float32)
    with torch.cuda.device_of(S):
        _chk(_L().dca_train_tables(_ptr(S), int(n_pixels), _ptr(bg), f0, f1, _ptr(norm), _ptr(U), _ptr(T), _stream()),
             "dca_train_tables")
    return U, T


def train_patch_colour(right_u8, U, y1, x1, th, tw):
    """Per channel floor(mean of U[1][byte]) over the th x tw window at (y1, x1) of the right image: (3,) uint8, the
    colour of the occlusion patch (datasets.py:306)."""
    H, W, C = _req_u8(right_u8, "train_patch_colour", "the right image")
    _req_dev(U, "train_patch_colour", "U", torch.uint8, (2, 256))
    y1, x1, th, tw = _fit("train_patch_colour", H, W, y1, x1, th, tw, "source")
    sums = torch.empty(3, device=U.device, dtype=torch.int64)
    colour = torch.empty(3, device=U.device, dtype=torch.uint8)
    with torch.cuda.device_of(U):
        _chk(_L().dca_train_patch_colour(_ptr(right_u8), _ptr(U), _ptr(sums), _ptr(colour), H, W, C, y1, x1, th, tw,
                                         _stream()), "dca_train_patch_colour")
    return colour


def train_crop_norm(left_u8, right_u8, T, y1, x1, out_left, out_right, patch=None, norm=None, colour=None):
    """The th x tw window at (y1, x1) of both (H,W,C) uint8 images through T (2,3,256) into out_left, out_right
    (3,th,tw) float32 -- contiguous views, e.g. slot b of a (B,3,th,tw) batch.  patch = (r0, r1, c0, c1): rows r0:r1,
    columns c0:c1 of the RIGHT crop become norm[1][ch][colour[ch]] (norm (2,3,256), colour (3,) uint8 on the device)."""
    H, W, C = _req_u8_pair(left_u8, right_u8, "train_crop_norm")
    _req_dev(T, "train_crop_norm", "T", torch.float32, (2, 3, 256))
    _req_dev(out_left, "train_crop_norm", "out_left", torch.float32, like=left_u8)
    if out_left.dim() != 3 or out_left.shape[0] != 3:
        raise RuntimeError(f"train_crop_norm: out_left must be (3,th,tw), got {tuple(out_left.shape)}")
    th, tw = int(out_left.shape[1]), int(out_left.shape[2])
    _req_dev(out_right, "train_crop_norm", "out_right", torch.float32, (3, th, tw), like=left_u8)
    y1, x1, th, tw = _fit("train_crop_norm", H, W, y1, x1, th, tw, "source")
    py0 = px0 = ph = pw = 0
    if patch is not None:
        r0, r1, c0, c1 = (int(v) for v in patch)
        if not (0 <= r0 <= r1 <= th and 0 <= c0 <= c1 <= tw):
            raise RuntimeError(f"train_crop_norm: the patch rows {r0}:{r1}, columns {c0}:{c1} leave the {th} x {tw} crop")
        py0, px0, ph, pw = r0, c0, r1 - r0, c1 - c0
    if ph > 0 and pw > 0:
        _req_dev(norm, "train_crop_norm", "norm", torch.float32, (2, 3, 256))
        _req_dev(colour, "train_crop_norm", "colour", torch.uint8, (3,))
    else:
        py0 = px0 = ph = pw = 0
        norm = colour = None
    with torch.cuda.device_of(left_u8):
        _chk(_L().dca_train_crop_norm(_ptr(left_u8), _ptr(right_u8), _ptr(T), _ptr(norm), _ptr(colour), _ptr(out_left),
                                      _ptr(out_right), H, W, C, y1, x1, th, tw, py0, px0, ph, pw, _stream()),
             "dca_train_crop_norm")
    return out_left, out_right


def train_disp_crop(disp, y1, x1, maxdisp, out_gt, out_mask, flip_rows=False, scale=1.0, inf_to_zero=False):
    """disp (H,W) float32 or uint16 on the device -> out_gt (th,tw) float32 = the window at (y1, x1) * scale and out_mask
    (th,tw) bool = gt > 0 & gt < maxdisp (main_dca.py:127).  flip_rows: the source is a bottom-up PFM payload;
    inf_to_zero: +inf -> 0 (the Middlebury loaders)."""
    _req_dev(disp, "train_disp_crop", "the disparity", (torch.float32, torch.uint16))
    if disp.dim() != 2 or disp.numel() == 0:
        raise RuntimeError(f"train_disp_crop: expected a (H,W) disparity, got {tuple(disp.shape)}")
    H, W = int(disp.shape[0]), int(disp.shape[1])
    _req_dev(out_gt, "train_disp_crop", "out_gt", torch.float32, like=disp)
    if out_gt.dim() != 2:
        raise RuntimeError(f"train_disp_crop: out_gt must be (th,tw), got {tuple(out_gt.shape)}")
    th, tw = int(out_gt.shape[0]), int(out_gt.shape[1])
    _req_dev(out_mask, "train_disp_crop", "out_mask", torch.bool, (th, tw), like=disp)
    y1, x1, th, tw = _fit("train_disp_crop", H, W, y1, x1, th, tw, "source")
    with torch.cuda.device_of(disp):
        _chk(_L().dca_train_disp_crop(_ptr(disp), int(disp.dtype == torch.uint16), _ptr(out_gt), _ptr(out_mask), H, W, y1, x1,
                                      th, tw, int(bool(flip_rows)), float(scale), int(bool(inf_to_zero)), float(maxdisp),
                                      _stream()), "dca_train_disp_crop")
    return out_gt, out_mask


# ------------------------------------------------------------------------------------------------
# Geometry from calibrated disparity (csrc/geometry.hip): metric depth and a compacted, coloured point
# cloud from the maps the pipeline already holds on the device.  Inference only, no counterpart in the reference.  No launch
# synchronises; with every buffer passed in nothing is allocated either (hipGraph capture).
# ------------------------------------------------------------------------------------------------
PC_TILE = _C["DCA_PC_TILE"]
PC_RECORD_BYTES = _C["DCA_PC_RECORD_BYTES"]
GEO_MIN_DISP = 0.0           # default filters: any non-negative disparity ...
GEO_MAX_DEPTH = 80.0         # ... up to the range the KITTI depth benchmark evaluates (metres)


def _geo_frame(name, pred, mask, window):
    """the (Hc,Wc) / (1,1,Hc,Wc) prediction, the optional mask of its shape and the window (y0, rows, cols), default whole"""
    _, Hc, Wc = _maps(name, pred, mask, False, what="the prediction")
    return (Hc, Wc) + _window(name, Hc, Wc, window, "prediction")


def _geo_scalars(name, calib, mask_min, min_disp, max_depth):
    """(f, fb, cx, cy, doffs, min_disp, max_depth, mask_min) as floats, within the ranges of include/dca_hip.h"""
    try:
        f, fb, cx, cy, doffs = (float(getattr(calib, k)) for k in ("f", "fb", "cx", "cy", "doffs"))
    except (AttributeError, TypeError, ValueError) as e:
        raise RuntimeError(f"{name}: calib must be a geometry.StereoCalib (f, fb, cx, cy, doffs): {e}") from None
    min_disp, max_depth = float(min_disp), float(max_depth)
    if not (0.0 < f < math.inf and 0.0 < fb < math.inf and all(math.isfinite(v) for v in (cx, cy, doffs))):
        raise RuntimeError(f"{name}: the calibration must be finite with f > 0 and f * baseline > 0")
    if not 0.0 <= min_disp < math.inf:
        raise RuntimeError(f"{name}: min_disp must be finite and >= 0, got {min_disp}")
    if not 0.0 < max_depth < math.inf:
        raise RuntimeError(f"{name}: max_depth must be finite and > 0, got {max_depth}")
    return f, fb, cx, cy, doffs, min_disp, max_depth, _mask_min(name, mask_min)


def disp_to_depth(pred, calib, window=None, mask=None, mask_min=0.5, min_disp=GEO_MIN_DISP, max_depth=GEO_MAX_DEPTH,
                  f32=True, u16=False, scale=256.0, out_f32=None, out_u16=None):
    """Dense metric depth of the window (y0, rows, cols) of a disparity map (Hc,Wc) / (1,1,Hc,Wc), one launch:
    Z = calib.fb / (d + calib.doffs) where d >= min_disp, 0 < Z <= max_depth and (mask is None or mask >= mask_min),
    +0.0 elsewhere (the KITTI depth convention; definitions: include/dca_hip.h).  mask: float32, shaped like pred.
    Returns (float32 (rows,cols) or None, uint16 (rows,cols) = trunc(Z * scale) saturated, or None); out_f32 / out_u16:
    buffers of that shape to write into."""
    Hc, Wc, y0, rows, cols = _geo_frame("disp_to_depth", pred, mask, window)
    f, fb, cx, cy, doffs, min_disp, max_depth, mask_min = _geo_scalars("disp_to_depth", calib, mask_min, min_disp, max_depth)
    if not (f32 or u16):
        raise RuntimeError("disp_to_depth: nothing to compute (f32 and u16 are both off)")
    if u16 and not 0.0 < float(scale) < math.inf:
        raise RuntimeError(f"disp_to_depth: scale must be finite and > 0, got {scale}")
    of = _out("disp_to_depth", "out_f32", out_f32, torch.float32, (rows, cols), pred) if f32 else None
    ou = _out("disp_to_depth", "out_u16", out_u16, torch.uint16, (rows, cols), pred) if u16 else None
    with torch.cuda.device_of(pred):
        _chk(_L().dca_disp_to_depth(_ptr(pred), _ptr(mask), _ptr(of), _ptr(ou), Hc, Wc, y0, rows, cols, fb, doffs, min_disp,
                                    max_depth, mask_min, float(scale), _stream()), "dca_disp_to_depth")
    return of, ou


def point_cloud_tiles(rows, cols):
    """workgroups of the compaction of a rows x cols window: ceil(rows * cols / PC_TILE)"""
    tiles = int(_L().dca_point_cloud_tiles(int(rows), int(cols)))
    if tiles <= 0:
        raise RuntimeError(f"point_cloud: a {rows} x {cols} window is empty or has 2^31 pixels or more")
    return tiles


def point_cloud_workspace(rows, cols, device):
    """(tile_offsets int32 (tiles + 1,), count int64 (2,)) for `point_cloud(..., workspace=)` on windows up to rows x cols"""
    return (torch.empty(point_cloud_tiles(rows, cols) + 1, device=device, dtype=torch.int32),
            torch.empty(2, device=device, dtype=torch.int64))


def point_cloud(pred, calib, rgb=None, mask=None, window=None, v0=0, stride=1, cap=None, out=None, workspace=None,
                mask_min=0.5, min_disp=GEO_MIN_DISP, max_depth=GEO_MAX_DEPTH):
    """The kept pixels of the window (y0, rows, cols) of a disparity map (Hc,Wc) / (1,1,Hc,Wc) as a compacted point cloud in
    the left camera's frame, in row-major window order, three launches and no atomics: bitwise reproducible, order included
    (definitions: include/dca_hip.h, dca_point_cloud).  A pixel (r, c) is kept under the filters of `disp_to_depth` and
    r % stride == c % stride == 0; its image coordinates are (u, v) = (c, v0 + r).  rgb: the (H,W,3) / (H,W,4) uint8 source
    image, read at (v0 + r, c); None: white.  mask: float32, shaped like pred.
    Returns (vertices, count, tile_offsets):
      vertices      (cap,4) float32: x, y, z and the colour bytes r, g, b, 255 in the fourth column -- 16-byte records, the
                    body of a binary PLY file (`geometry.write_ply`); only the first count[1] rows are written
      count         (2,) int64 on the device: kept pixels, records written = min(kept, cap)
      tile_offsets  (tiles + 1,) int32 on the device: kept pixels before every tile of PC_TILE window pixels, then the total
    cap: room in vertices, default the worst case ceil(rows / stride) * ceil(cols / stride), or out's.  out: a (cap,4)
    float32 buffer; workspace: `point_cloud_workspace(...)` of a window at least this large.  With both given nothing is
    allocated and the host never waits: the launches can be captured into a hipGraph."""
    name = "point_cloud"
    Hc, Wc, y0, rows, cols = _geo_frame(name, pred, mask, window)
    f, fb, cx, cy, doffs, min_disp, max_depth, mask_min = _geo_scalars(name, calib, mask_min, min_disp, max_depth)
    v0, stride = int(v0), int(stride)
    if stride < 1 or v0 < 0:
        raise RuntimeError(f"{name}: stride >= 1 and v0 >= 0, got stride {stride} and v0 {v0}")
    C = Hs = Ws = 0
    if rgb is not None:
        Hs, Ws, C = _req_u8(rgb, name, "rgb", like=pred)
        _window(name, Hs, Ws, (v0, rows, cols), "image")
    tiles = point_cloud_tiles(rows, cols)
    if out is not None:
        _req_dev(out, name, "out", torch.float32, like=pred)
        if out.dim() != 2 or out.shape[1] != 4 or out.data_ptr() % PC_RECORD_BYTES:
            raise RuntimeError(f"{name}: out must be a 16-byte aligned (cap,4) float32 buffer, got {tuple(out.shape)}")
        if cap is not None and int(cap) > out.shape[0]:
            raise RuntimeError(f"{name}: cap {cap} exceeds the {out.shape[0]} records of out")
    if cap is None:
        cap = out.shape[0] if out is not None else -(-rows // stride) * -(-cols // stride)
    cap = int(cap)
    if cap < 0:
        raise RuntimeError(f"{name}: cap >= 0, got {cap}")
    if out is None:
        out = torch.empty((cap, 4), device=pred.device, dtype=torch.float32)
    if workspace is None:
        workspace = point_cloud_workspace(rows, cols, pred.device)
    offs, count = workspace
    if _workspace(name, "workspace[0] (tile_offsets)", offs, tiles + 1, pred).dim() != 1:
        raise RuntimeError(f"{name}: workspace[0] must be a flat buffer, got {tuple(offs.shape)}")
    _req_dev(count, name, "workspace[1] (count)", torch.int64, (2,), like=pred)
    with torch.cuda.device_of(pred):
        _chk(_L().dca_point_cloud(_ptr(pred), _ptr(mask), _ptr(rgb), C, Hs, Ws, _ptr(out) if cap else None, cap, _ptr(offs),
                                  _ptr(count), Hc, Wc, y0, rows, cols, v0, stride, f, fb, cx, cy, doffs, min_disp, max_depth,
                                  mask_min, _stream()), "dca_point_cloud")
    return out[:cap], count, offs[:tiles + 1]


# ------------------------------------------------------------------------------------------------
# Sparse ground truth from a LiDAR scan (csrc/lidar.hip): the points of one scan, projected into the
# rectified left image through a z-buffer and a hidden-point test.  No counterpart in the reference.  No launch
# synchronises; with `out` and `workspace` passed in nothing is allocated either.
# ------------------------------------------------------------------------------------------------
LIDAR_MAX_RADIUS = _C["DCA_LIDAR_MAX_RADIUS"]
_LIDAR_KINDS = {"disp": torch.float32, "depth": torch.float32, "disp_u16": torch.uint16, "count": torch.int64}


def lidar_disparity(points, calib, n=None, occl=_geometry.LIDAR_OCCL, min_depth=_geometry.LIDAR_MIN_DEPTH,
                    max_depth=_geometry.LIDAR_MAX_DEPTH, min_disp=_geometry.LIDAR_MIN_DISP,
                    max_disp=_geometry.LIDAR_MAX_DISP, outputs=("disp",), out=None, workspace=None):
    """One LiDAR scan -> sparse ground-truth maps in the rectified left image, three launches (definitions:
    include/dca_hip.h, dca_lidar_disparity; `geometry.lidar_disparity_host` is the numpy restatement, equal bit for bit).
    points: (N,S) float32 on the device, S >= 3 (a KITTI scan: S = 4); the leading n rows (default all) and their first three
    columns are read.  calib: a geometry.LidarCalib.  A point is kept with min_depth <= z <= max_depth inside the image;
    the nearest point of a pixel wins (integer atomicMin on the depth's bits: the same bits for every order of the points);
    occl = (rx, ry, rel) drops a pixel whose z exceeds (1 + rel) times the smallest z within rx columns and ry rows,
    (0, 0, rel) switches that off; a pixel is written where min_disp <= d < max_disp, d = fb / z - doffs.
    Returns a dict with the keys of `outputs`:
      disp      (H,W) float32: d, +0.0 where there is no measurement (the KITTI convention)
      depth     (H,W) float32: z in metres, +0.0 elsewhere
      disp_u16  (H,W) uint16: the KITTI disparity PNG payload, trunc(d * 256 + 0.5) saturated, >= 1 where written, 0 elsewhere
      count     (2,) int64 on the device: pixels written, points kept
    out: a dict of buffers for some or all of them; workspace: an int32 buffer of at least H * W words (the z-buffer)."""
    name = "lidar_disparity"
    _req_no_grad(name, points)
    _req_dev(points, name, "points", torch.float32)
    if points.dim() != 2:
        raise RuntimeError(f"{name}: expected (N,S) points, got {tuple(points.shape)}")
    N, S = int(points.shape[0]), int(points.shape[1])
    n, rx, ry, rel, fb, doffs, min_depth, max_depth, min_disp, max_disp, outputs = _geometry._lidar_scalars(
        name, RuntimeError, calib, N, S, n, occl, min_depth, max_depth, min_disp, max_disp, outputs)
    H, W = calib.hw
    res = _out_dict(name, _LIDAR_KINDS, (), outputs, out, lambda k: (2,) if k == "count" else (H, W), points)
    if workspace is None:
        workspace = torch.empty(H * W, device=points.device, dtype=torch.int32)
    _workspace(name, "workspace", workspace, H * W, points)
    m = [float(v) for v in calib.M.reshape(-1)]
    with torch.cuda.device_of(points):
        _chk(_L().dca_lidar_disparity(_ptr(points) if N else None, N, S, n, *m, H, W, fb, doffs, min_depth, max_depth, min_disp,
                                      max_disp, rx, ry, rel, _ptr(res.get("disp")), _ptr(res.get("depth")),
                                      _ptr(res.get("disp_u16")), _ptr(res.get("count")), _ptr(workspace), _stream()),
             "dca_lidar_disparity")
    return res


# ------------------------------------------------------------------------------------------------
# Disparity post-filter (csrc/postfilter.hip): speckle removal -- connected components of similar
# disparity, the small ones dropped -- and a small masked median.  Inference only, no counterpart in the reference;
# `postfilter.speckle_filter_host` / `median_filter_host` are the numpy restatements, equal bit for bit.  No launch
# synchronises; with `out` and `workspace` passed in nothing is allocated either (hipGraph capture).
# ------------------------------------------------------------------------------------------------
SPECKLE_TILE = (_C["DCA_SPK_TILE_H"], _C["DCA_SPK_TILE_W"])
SPECKLE_OUTPUTS = ("disp", "valid", "size")
_SPECKLE_KINDS = {"disp": torch.float32, "valid": torch.float32, "size": torch.int32}
POSTFILTER_MAX_BATCH = 65535


def _pf_frame(name, disp, mask, mask_min, window):
    """the maps (Hc,Wc) / (B,Hc,Wc) / (B,1,Hc,Wc), the optional mask of their shape and the window (y0, rows, cols), default
    whole, as `_geo_frame` takes them for one frame -> (B, Hc, Wc, y0, rows, cols, mask_min, the outputs' shape)"""
    B, Hc, Wc = _maps(name, disp, mask, True, POSTFILTER_MAX_BATCH)
    shape = tuple(disp.shape)
    if len(shape) > 4 or (len(shape) == 4 and shape[1] != 1):
        raise RuntimeError(f"{name}: expected (Hc,Wc), (B,Hc,Wc) or (B,1,Hc,Wc) disparity maps, got {shape}")
    y0, rows, cols = _window(name, Hc, Wc, window, "map")
    return B, Hc, Wc, y0, rows, cols, _mask_min(name, mask_min, mask is not None), shape[:-2] + (rows, cols)


def speckle_workspace(rows, cols, device, batch=1):
    """(label, count): the two int32 buffers of batch * rows * cols words for `speckle_filter(..., workspace=)` on windows up
    to rows x cols; a call writes every word it reads, nothing has to be cleared between calls"""
    n = int(batch) * int(rows) * int(cols)
    if n <= 0 or int(rows) * int(cols) >= 1 << 31:
        raise RuntimeError(f"speckle_workspace: a {rows} x {cols} window, batch {batch}, is empty or has 2^31 pixels or more")
    return torch.empty(n, device=device, dtype=torch.int32), torch.empty(n, device=device, dtype=torch.int32)


def speckle_filter(disp, max_size, max_diff, mask=None, mask_min=0.5, window=None, fill=0.0, outputs=None, out=None,
                   workspace=None):
    """Speckle filter of disparity maps (Hc,Wc) / (B,Hc,Wc) / (B,1,Hc,Wc), images independent, over the window (y0, rows, cols)
    of every map (definitions: include/dca_hip.h, dca_speckle_filter).  A window pixel is active iff it is finite and (mask is
    None or mask >= mask_min); two 4-neighbours are joined iff both are active and |a - b| <= max_diff in float32 (equality
    joins; chained, a ramp with small steps is one component).  max_size: an integer >= 0; components of at most max_size
    pixels are removed (0: the identity on active pixels).  Returns a dict of (rows,cols) maps per image:
      disp   float32  the input bit for bit where valid, `fill` elsewhere (+0.0: "no measurement")
      valid  float32  1.0 where active and size > max_size, 0.0 elsewhere
      size   int32    the pixel's component size, 0 for an inactive pixel
    outputs: the names wanted (default all three; `valid` is always computed) -- the others are neither computed nor written.
    out: a dict of buffers for some or all of them; workspace: `speckle_workspace(...)` of a window and batch at least this
    large.  With both given nothing is allocated and the host never waits: the four launches can be captured into a
    hipGraph.  Bitwise reproducible: tile-local union-find in LDS, a merge across tile edges with integer atomics."""
    name = "speckle_filter"
    B, Hc, Wc, y0, rows, cols, mask_min, shape = _pf_frame(name, disp, mask, mask_min, window)
    try:
        ok = int(max_size) == max_size and 0 <= int(max_size) < 1 << 31 and 0.0 <= float(max_diff) < math.inf
        max_diff, fill = float(max_diff), float(fill)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise RuntimeError(f"{name}: max_size must be an integer >= 0, max_diff finite and >= 0 and fill a number, got "
                           f"{max_size!r}, {max_diff!r} and {fill!r}")
    res = _out_dict(name, _SPECKLE_KINDS, ("valid",), outputs, out, lambda k: shape, disp)
    if workspace is None:
        workspace = speckle_workspace(rows, cols, disp.device, B)
    try:
        label, count = workspace
    except (TypeError, ValueError):
        raise RuntimeError(f"{name}: workspace is the (label, count) pair of `speckle_workspace`") from None
    _workspace(name, "workspace[0] (label)", label, B * rows * cols, disp)
    _workspace(name, "workspace[1] (count)", count, B * rows * cols, disp)
    if label.data_ptr() == count.data_ptr():
        raise RuntimeError(f"{name}: workspace[0] and workspace[1] must be two buffers")
    with torch.cuda.device_of(disp):
        _chk(_L().dca_speckle_filter(_ptr(disp), _ptr(mask), _ptr(res.get("disp")), _ptr(res["valid"]), _ptr(res.get("size")),
                                     _ptr(label), _ptr(count), B, Hc, Wc, y0, rows, cols, int(max_size), max_diff, mask_min,
                                     fill, _stream()), "dca_speckle_filter")
    return res


def median_filter(disp, ksize, mask=None, mask_min=0.5, window=None, out=None):
    """Masked ksize x ksize median (ksize 3 or 5) of disparity maps (Hc,Wc) / (B,Hc,Wc) / (B,1,Hc,Wc) over the window
    (y0, rows, cols), one launch (definitions: include/dca_hip.h, dca_median_filter).  For an active centre (finite, and
    mask is None or mask >= mask_min) the candidates are the active pixels of the neighbourhood inside the window -- no
    border replication -- and the result is the one of rank (n - 1) // 2, the lower median for even n, an input value bit
    for bit (-0.0 < +0.0); an inactive centre is copied unchanged.  Returns float32 (rows,cols) per image; out: a buffer
    of that shape to write into (not the input)."""
    name = "median_filter"
    B, Hc, Wc, y0, rows, cols, mask_min, shape = _pf_frame(name, disp, mask, mask_min, window)
    if isinstance(ksize, bool) or ksize not in (3, 5):
        raise RuntimeError(f"{name}: ksize is 3 or 5, got {ksize!r}")
    out = _out(name, "out", out, torch.float32, shape, disp, alias=(disp,))
    with torch.cuda.device_of(disp):
        _chk(_L().dca_median_filter(_ptr(disp), _ptr(mask), _ptr(out), B, Hc, Wc, y0, rows, cols, int(ksize), mask_min,
                                    _stream()), "dca_median_filter")
    return out


# ------------------------------------------------------------------------------------------------
# Pictures of a disparity map (csrc/visualize.hip): the KITTI error map of a prediction against the
# ground truth (utils/visualization.py:31-55) and the colour-coded disparity map, uint8 RGB on the device.  No launch
# synchronises; definitions: include/dca_hip.h.
# ------------------------------------------------------------------------------------------------
CMAPS = {"gray": _C["DCA_CMAP_GRAY"], "kitti": _C["DCA_CMAP_KITTI"]}


def disp_error_image(pred, gt, abs_thres=3.0, rel_thres=0.05, legend=True, f32=True, u8=False, out_f32=None, out_u8=None):
    """The KITTI error map of a (padded) prediction against the ground truth in one launch (the reference's
    disp_error_image_func.forward, utils/visualization.py:31-55): pred (B,Hp,Wp) or (B,1,Hp,Wp) with Hp >= H, Wp >= W (rows
    padded on top, columns on the right, cropped by addressing as in `disp_metrics`), gt (B,H,W).  Returns (float32 planar
    (B,3,H,W) in [0,1] -- the reference's result -- or None, uint8 interleaved (B,H,W,3) or None); out_f32 / out_u8: buffers
    of those shapes to write into.  legend: the colour key in the top-left corner (the reference always draws it)."""
    name = "disp_error_image"
    pred, gt, B, H, W, Hp, Wp = _pred_over_gt(name, pred, gt)
    if gt.numel() == 0 or B * Hp * Wp >= 1 << 31:
        raise RuntimeError(f"{name}: the ground truth must not be empty and B * Hp * Wp must stay below 2^31")
    abs_thres, rel_thres = float(abs_thres), float(rel_thres)
    if not (0.0 < abs_thres < math.inf and 0.0 < rel_thres < math.inf):
        raise RuntimeError(f"{name}: abs_thres and rel_thres must be positive and finite, got {abs_thres} and {rel_thres}")
    if not (f32 or u8):
        raise RuntimeError(f"{name}: nothing to compute (f32 and u8 are both off)")
    of = _out(name, "out_f32", out_f32, torch.float32, (B, 3, H, W), gt) if f32 else None
    ou = _out(name, "out_u8", out_u8, torch.uint8, (B, H, W, 3), gt) if u8 else None
    with torch.cuda.device_of(gt):
        _chk(_L().dca_disp_error_image(_ptr(pred), _ptr(gt), _ptr(of), _ptr(ou), B, H, W, Hp - H, Wp - W, abs_thres, rel_thres,
                                       1 if legend else 0, _stream()), "dca_disp_error_image")
    return of, ou


def disp_range(disp, window=None, mask=None, mask_min=0.5):
    """(lo, hi) of the valid pixels of the window (y0, rows, cols) (default: everything) of every map of disp (Hc,Wc) /
    (B,Hc,Wc) / (B,1,Hc,Wc): finite, > 0 and, with a float32 mask shaped like disp, mask >= mask_min.  Returns (B,2)
    float32 on the device, (0, 0) for a map without a valid pixel; two launches, nothing is read back; bitwise
    reproducible."""
    name = "disp_range"
    B, Hc, Wc = _maps(name, disp, mask, True, 65535)
    if B * Hc * Wc >= 1 << 31:
        raise RuntimeError(f"{name}: the maps must have fewer than 2^31 pixels together")
    y0, rows, cols = _window(name, Hc, Wc, window, "map")
    mask_min = _mask_min(name, mask_min, mask is not None)
    out = torch.empty((B, 2), device=disp.device, dtype=torch.float32)
    with torch.cuda.device_of(disp):
        ws = torch.empty(_L().dca_disp_range_workspace(B, rows, cols), device=disp.device, dtype=torch.uint8)
        _chk(_L().dca_disp_range(_ptr(disp), _ptr(mask), _ptr(out), _ptr(ws), B, Hc, Wc, y0, rows, cols, mask_min, _stream()),
             "dca_disp_range")
    return out


def disp_colorize(disp, y0, rows, cols, max_disp=None, range=None, cmap="kitti", mask=None, mask_min=0.5, out=None):
    """The rows x cols window at row y0, column 0 of ONE map (Hc,Wc) / (1,1,Hc,Wc) as a colour image, one launch: uint8
    (rows,cols,3) on the device.  Exactly one of max_disp (a host number: t = min(d / max_disp, 1), the KITTI devkit's
    scaling) and range (the (1,2) / (2,) device tensor (lo, hi) of `disp_range`: auto-ranging without a read-back) must be
    given.  cmap: "kitti" (the devkit's disp_to_color) or "gray".  Pixels that are not finite, not > 0 or, with a float32 mask
    shaped like disp, below mask_min are black.  out: a (rows,cols,3) uint8 buffer to write into."""
    name = "disp_colorize"
    if cmap not in CMAPS:
        raise ValueError(f"{name}: cmap is one of {sorted(CMAPS)}, got {cmap!r}")
    _, Hc, Wc = _maps(name, disp, mask, False)
    y0, rows, cols = _window(name, Hc, Wc, (y0, rows, cols), "map")
    if (max_disp is None) == (range is None):
        raise RuntimeError(f"{name}: give exactly one of max_disp and range")
    if range is not None:
        _req_dev(range, name, "range", torch.float32, like=disp)
        if range.numel() != 2:
            raise RuntimeError(f"{name}: range must hold (lo, hi), got {tuple(range.shape)}")
        max_disp = 0.0
    elif not 0.0 < float(max_disp) < math.inf:
        raise RuntimeError(f"{name}: max_disp must be positive and finite, got {max_disp}")
    mask_min = _mask_min(name, mask_min, mask is not None)
    out = _out(name, "out", out, torch.uint8, (rows, cols, 3), disp)
    with torch.cuda.device_of(disp):
        _chk(_L().dca_disp_colorize(_ptr(disp), _ptr(mask), _ptr(range), _ptr(out), Hc, Wc, y0, rows, cols, float(max_disp),
                                    mask_min, CMAPS[cmap], _stream()), "dca_disp_colorize")
    return out
