"""The evaluation step of the reference's training script (main_dca.py:143-246 `mytest`, run over the whole test set
after every epoch) without a host round trip per frame: pad -> 2D networks -> hot path -> up-sampler, then three small
HIP launches (csrc/eval_metrics.hip) that turn the prediction, the ground truth and the three DCA region volumes into
the reference's per-batch values and add them to a run state on the device.  Nothing is read back before `result()`.

The reference's `forward` hands out ONE region volume while its `mytest` scores three (`pred_au[0..2]`,
main_dca.py:211-213): the three `cva` heads are meant, and `hot_path(aux_volumes=True)` makes them reachable.

Two quirks of the reference are reproduced, not fixed: a batch whose mask is empty contributes 0 to all ten values and
still counts (main_dca.py:177-195); `mytest` never resets its SegmentationMetric between the heads, so mpa1 / mIoU1 are
computed from CM0 + CM1 and mpa2 / mIoU2 from CM0 + CM1 + CM2 (main_dca.py:215-232).  The per-head matrices of the run
are kept next to them, so `result()` also reports every head on its own over the whole data set."""
from __future__ import annotations

import contextlib

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib, ops
from .graph import GraphedHotPath

# state layout: include/dca_hip.h (DCA_EVAL_*)
BATCHES, SUMS, IMG_KEPT, IMG_EPE, IMG_D1, IMG_THRES, IMG_SEEN, PIXELS = (
    _lib.CONSTANTS[f"DCA_EVAL_{n}"] for n in ("BATCHES", "SUMS", "IMG_KEPT", "IMG_EPE", "IMG_D1", "IMG_THRES", "IMG_SEEN", "PIXELS"))
STATE_HEAD = ops.EVAL_STATE_HEAD
KEYS = ("loss", "epe", "1px", "3px", "mpa0", "mpa1", "mpa2", "mIoU0", "mIoU1", "mIoU2")


class SegmentationMetric:
    """main_dca.py:66-120: pixel accuracy / IoU from a confusion matrix (rows = label, columns = prediction); host math.
    `addBatch` takes label maps like the reference, `addMatrix` a matrix counted elsewhere (ops.region_confusion)."""

    def __init__(self, numClass):
        self.numClass = numClass
        self.reset()

    def reset(self):
        self.confusionMatrix = np.zeros((self.numClass, self.numClass))

    def pixelAccuracy(self):
        return np.diag(self.confusionMatrix).sum() / self.confusionMatrix.sum()

    def classPixelAccuracy(self):
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.diag(self.confusionMatrix) / self.confusionMatrix.sum(axis=1)

    def meanPixelAccuracy(self):
        return np.nanmean(self.classPixelAccuracy())           # classes without a label pixel (0/0) are left out

    def _iou(self):
        cm = self.confusionMatrix
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.diag(cm) / (cm.sum(axis=1) + cm.sum(axis=0) - np.diag(cm))

    def meanIntersectionOverUnion(self):
        return np.nanmean(self._iou())

    def Frequency_Weighted_Intersection_over_Union(self):
        freq = self.confusionMatrix.sum(axis=1) / self.confusionMatrix.sum()
        iu = self._iou()
        return (freq[freq > 0] * iu[freq > 0]).sum()

    def genConfusionMatrix(self, imgPredict, imgLabel):
        keep = (imgLabel >= 0) & (imgLabel < self.numClass)     # labels outside the classes are not scored
        idx = self.numClass * imgLabel[keep].astype("int64") + imgPredict[keep]
        return np.bincount(idx, minlength=self.numClass ** 2).reshape(self.numClass, self.numClass)

    def addBatch(self, imgPredict, imgLabel):
        assert imgPredict.shape == imgLabel.shape
        self.confusionMatrix += self.genConfusionMatrix(imgPredict, imgLabel)

    def addMatrix(self, confusionMatrix):
        self.confusionMatrix += np.asarray(confusionMatrix, dtype=np.float64)


def batch_values(rec, cms):
    """The ten values `mytest` returns for one batch, from the per-image records (B,8) and the per-head confusion
    matrices (3,C,C) of that batch: host restatement of dca_eval_accumulate (fp64), used by `result()`'s tests and by
    anyone who has the matrices on the host."""
    rec, cms = np.asarray(rec, dtype=np.float64), np.asarray(cms)
    n = rec[:, 0].sum()
    if n == 0:
        return dict.fromkeys(KEYS, 0.0)
    out = {"loss": rec[:, 3].sum() / n, "epe": rec[:, 2].sum() / n, "1px": rec[:, 4].sum() / n, "3px": rec[:, 6].sum() / n}
    metric = SegmentationMetric(cms.shape[-1])
    for k in range(3):
        if k < cms.shape[0]:
            metric.addMatrix(cms[k])                            # not reset between the heads, as in the reference
        out[f"mpa{k}"], out[f"mIoU{k}"] = metric.meanPixelAccuracy(), metric.meanIntersectionOverUnion()
    return out


def state_result(state):
    """Run state (host copy, float64) -> the averages main_dca.py:325-335 prints (mean over batches of the ten values)
    plus every head on its own over the run and the per-image metrics of utils/metrics.py."""
    s = np.asarray(state, dtype=np.float64)
    C = int(round(((s.size - STATE_HEAD) / 3) ** 0.5))
    assert s.size == STATE_HEAD + 3 * C * C, "not an evaluation state"
    nb, kept = s[BATCHES], s[IMG_KEPT]
    res = {k: (s[SUMS + i] / nb if nb else 0.0) for i, k in enumerate(KEYS)}
    cms = s[STATE_HEAD:].reshape(3, C, C)
    res["confusion"] = cms.astype(np.int64)
    res["head_mpa"], res["head_mIoU"] = [], []
    for k in range(3):
        metric = SegmentationMetric(C)
        metric.addMatrix(cms[k])
        with np.errstate(invalid="ignore"), _quiet():
            res["head_mpa"].append(metric.meanPixelAccuracy())
            res["head_mIoU"].append(metric.meanIntersectionOverUnion())
    for name, idx in (("image_epe", IMG_EPE), ("image_d1", IMG_D1), ("image_thres1", IMG_THRES),
                      ("image_thres2", IMG_THRES + 1), ("image_thres3", IMG_THRES + 2)):
        res[name] = s[idx] / kept if kept else 0.0              # utils/metrics.py: 0 when no image passes the 10 % rule
    res["batches"], res["images"], res["images_kept"], res["pixels"] = int(nb), int(s[IMG_SEEN]), int(kept), int(s[PIXELS])
    return res


@contextlib.contextmanager
def _quiet():
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)         # np.nanmean of an all-NaN vector (a head without labels)
        yield


def pad16(imgL, imgR):
    """main_dca.py:153-166: zero rows on TOP and zero columns on the RIGHT up to the next multiple of 16.
    Returns (imgL, imgR, top_pad, right_pad)."""
    H, W = imgL.shape[2], imgL.shape[3]
    top_pad, right_pad = -H % 16, -W % 16
    if top_pad or right_pad:
        imgL, imgR = F.pad(imgL, (0, right_pad, top_pad, 0)), F.pad(imgR, (0, right_pad, top_pad, 0))
    return imgL, imgR, top_pad, right_pad


def all_reduce_state(state, group=None):
    """Sums the run state over the ranks of `group` in place (every entry is a sum or a count, and counts stay exact in
    fp64): evaluating shards of the test set on several ranks then equals one process evaluating all the batches."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        dist.all_reduce(state, op=dist.ReduceOp.SUM, group=group)
    return state


def risk_coverage(state):
    """Host arithmetic of `ConfidenceCurve.result()`: state (nbins,3) int64 of ops.conf_histogram -- per confidence bin
    the pixel count, the sum of |pred - gt| in units of 2^-20 pixels and the count of |pred - gt| > 3 -- -> dict with
      counts                 (nbins,) int64, the pixels per bin
      threshold, coverage, epe, bad3    one entry per NON-EMPTY bin, from the most confident bin downwards: keeping the
                             pixels with confidence >= threshold[i] keeps the fraction coverage[i] of all pixels, with mean
                             error epe[i] and the fraction bad3[i] of errors > 3; coverage ends at 1 and epe[-1] is the
                             EPE over all pixels
      aurc_epe               the trapezoid area under epe over coverage in [0, 1], the curve held at epe[0] below
                             coverage[0] (a confidence that says nothing about the error gives the EPE itself; lower is
                             better)
      pixels                 the total count.
    All sums are exact integers until the final divisions.  An empty state gives empty curves and aurc_epe 0."""
    st = np.asarray(state)
    assert st.ndim == 2 and st.shape[1] == 3 and st.dtype.kind in "iu", "not a confidence state"
    st = st.astype(np.int64)
    nbins = st.shape[0]
    counts = st[:, 0].copy()
    keep = np.nonzero(counts[::-1])[0]                      # descending confidence, empty bins left out
    desc = st[::-1][keep]
    n, err, bad = (np.cumsum(desc[:, k]) for k in range(3))
    total = int(counts.sum())
    nf = n.astype(np.float64)
    coverage = nf / float(total) if total else nf
    epe = err.astype(np.float64) / float(ops.CONF_ERR_SCALE) / nf
    bad3 = bad.astype(np.float64) / nf
    aurc = 0.0
    if total:
        c, e = np.concatenate([[0.0], coverage]), np.concatenate([epe[:1], epe])
        aurc = float(((c[1:] - c[:-1]) * (e[1:] + e[:-1])).sum() * 0.5)
    return {"counts": counts, "threshold": (nbins - 1 - keep).astype(np.float64) / nbins, "coverage": coverage, "epe": epe,
            "bad3": bad3, "aurc_epe": aurc, "pixels": total}


class ConfidenceCurve:
    """Scores a confidence map against the ground truth over a run: `cc = ConfidenceCurve(); for frame:
    cc.add(conf, pred, gt); print(cc.result()["aurc_epe"])`.  `add` is one launch (ops.conf_histogram) into an int64
    state on the device and reads nothing back; `result()` reads the state once (`risk_coverage`).  Pixels with
    0 < gt < maxdisp count; conf, pred, gt: float32 tensors of one shape on the device.  Bitwise reproducible.
    Across ranks: `all_reduce_state(cc.state)` accepts this state unchanged (every entry is an integer sum)."""

    def __init__(self, nbins=64, maxdisp=192, device="cuda"):
        if not 2 <= int(nbins) <= ops.CONF_MAX_BINS:
            raise ValueError(f"2 <= nbins <= {ops.CONF_MAX_BINS}")
        self.maxdisp = maxdisp
        self.state = torch.zeros((int(nbins), 3), device=device, dtype=torch.int64)

    def reset(self):
        self.state.zero_()

    def add(self, conf, pred, gt):
        ops.conf_histogram(conf, pred, gt, self.state, self.maxdisp)

    def result(self):
        return risk_coverage(self.state.cpu().numpy())


class _HotPathWithConfusion:
    """`hot_path`-shaped callable for GraphedHotPath: the hot path with its three region volumes, then
    dca_region_confusion against the ground truth, so that one hipGraph holds both."""

    def __init__(self, net):
        self.net = net

    @property
    def training(self):
        return self.net.training

    def hot_path(self, gt, *features):
        r = self.net.hot_path(*features, aux_volumes=True)
        vols = [r["prob_volume1"], r["prob_volume2"], r["prob_volume3"]]
        return {"pred4_q": r["pred4_q"], "cm": ops.region_confusion(vols, gt), "volumes": vols}


class EvalStep:
    """`ev = EvalStep(model); for batch: ev.step(imgL, imgR, disp_true); print(ev.result())` -- main_dca.py:296-335.

    `model`: a GwcNet (or its nn.DataParallel wrapper) on the GPU.  `step` enqueues the whole batch and returns without
    a host synchronisation; `result()` reads the state once.  graph=True: the 2D networks stay eager (MIOpen), the hot
    path with dca_region_confusion at its tail replays as one hipGraph per (frame shape, ground-truth shape);
    dca_disp_metrics and dca_eval_accumulate follow the up-sampler as plain launches on the same stream.
    dtype: None (fp32) or torch.float16 / torch.bfloat16 (ops.reduced_precision; the region volumes stay fp32).
    The metric launches are bitwise reproducible; whole steps repeat bit for bit when the 2D networks' MIOpen
    convolutions do (torch.backends.cudnn.deterministic = True).
    error_images=True: one more launch per step (`ops.disp_error_image` behind `ops.disp_metrics`, same stream, same pred, gt
    and pads; a plain launch with graph=True too) leaves the batch's KITTI error maps in `last["error_image"]`, (B,H,W,3) uint8
    with the colour key; nothing is read back and the run state is bitwise the same with or without."""

    def __init__(self, model, maxdisp=192, graph=False, dtype=None, error_images=False):
        self.net = model.module if isinstance(model, torch.nn.DataParallel) else model
        self.net.eval()
        self.maxdisp, self.graph, self.dtype = maxdisp, graph, dtype
        self.error_images = bool(error_images)
        self._tail = _HotPathWithConfusion(self.net)
        self._graphed = {}
        self.state = ops.eval_state(self.net.maxdisp // 8, next(self.net.parameters()).device)
        self.last = None    # tensors of the last step (prediction, records, matrices); static buffers when graph=True

    def reset(self):
        self.state.zero_()

    @torch.no_grad()
    def step(self, imgL, imgR, disp_true):
        net = self.net
        gt = disp_true[:, 0] if disp_true.dim() == 4 else disp_true
        gt = gt.to(self.state.device, torch.float32).contiguous()
        left, right, top_pad, right_pad = pad16(imgL, imgR)
        fl, fr = net.feature_extraction(left), net.feature_extraction(right)
        guidance = net.guidance(left)["g"]
        args = [gt, fl["gwc_segments"], fr["gwc_segments"]]
        if net.use_concat_volume:
            args += [fl["concat_feature"], fr["concat_feature"]]
        ctx = ops.reduced_precision(self.dtype) if self.dtype is not None else contextlib.nullcontext()
        with ctx:      # (a replay needs no context: the captured launches are already the reduced-precision kernels)
            if self.graph:
                key = (tuple(left.shape), tuple(gt.shape))
                if key not in self._graphed:
                    self._graphed[key] = GraphedHotPath(self._tail, *args)
                r = self._graphed[key](*args)
            else:
                r = self._tail.hot_path(*args)
        pred = net.prop(guidance, r["pred4_q"])
        rec = ops.disp_metrics(pred, gt, self.maxdisp)     # crop [:, top_pad:, :W] fused into the addressing
        ops.eval_accumulate(self.state, rec, r["cm"], gt.shape)
        self.last = {"pred": pred, "rec": rec, "cm": r["cm"], "volumes": r["volumes"], "top_pad": top_pad,
                     "right_pad": right_pad}
        if self.error_images:
            self.last["error_image"] = ops.disp_error_image(pred, gt, f32=False, u8=True)[1]

    def result(self):
        """one device -> host copy; across ranks call `all_reduce_state(ev.state)` first"""
        return state_result(self.state.cpu().numpy())


def mytest(model, imgL, imgR, disp_true, maxdisp=192):
    """Drop-in for main_dca.py:143-246: one batch -> (loss, metrics, mpa, mIoU) with the reference's keys and types
    (loss: 0-dim fp32 tensor on the device, plain 0 for an empty mask; metrics: floats; mpa / mIoU: numpy floats), one
    host synchronisation at the end."""
    dev = next(model.parameters()).device
    ev = EvalStep(model, maxdisp)
    ev.step(imgL.to(dev, torch.float32), imgR.to(dev, torch.float32), disp_true.to(dev))
    loss = ev.state[SUMS].to(torch.float32)                      # enqueued; no synchronisation
    s = ev.state.cpu().numpy()
    if s[PIXELS] == 0:
        return 0, {"epe": 0, "1px": 0, "3px": 0}, {"mpa0": 0, "mpa1": 0, "mpa2": 0}, {"mIoU0": 0, "mIoU1": 0, "mIoU2": 0}
    v = {k: s[SUMS + i] for i, k in enumerate(KEYS)}
    return (loss, {k: float(v[k]) for k in ("epe", "1px", "3px")}, {k: v[k] for k in ("mpa0", "mpa1", "mpa2")},
            {k: v[k] for k in ("mIoU0", "mIoU1", "mIoU2")})
