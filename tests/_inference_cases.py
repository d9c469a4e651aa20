"""What the GPU tests of the inference wrappers share: the seeded model, random uint8 pairs, a left-right threshold that
splits a pair, rectification maps for the 32 x 64 frame, and the wrapper cases of test_gpu_inference_trace.py."""
import collections

import numpy as np
import torch

import _rectify_reference as REF
from oracle import dcanet_oracle as O

DEV = "cuda"
FRAME = dict(crop_height=32, crop_width=64)
RAW, RECT = (36, 70), (30, 60)          # rectify=: raw pairs of 36 x 70 become 30 x 60 images, which fit the 32 x 64 frame
_MODEL = []


def model():
    """one seeded GwcNet(32) for the whole module, never modified (eval mode, no grad)"""
    if not _MODEL:
        from dcanet_amd.models.gwcnet_dca_g import GwcNet
        m = GwcNet(32, use_concat_volume=False)
        m.load_state_dict(O.seeded_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}), strict=True)
        _MODEL.append(m.to(DEV).eval())
    return _MODEL[0]


def pairs(rng, sizes):
    return [(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
            for h, w in sizes]


def lr_tau(plain, left_rgb, right_rgb):
    """a threshold under which most in-view pixels of this pair pass the cross-check: the 60th percentile of the
    differences of the whole window (out-of-view pixels are +inf), so that the MEDIAN of the validity map is 1"""
    from dcanet_amd import ops
    from dcanet_amd.inference import placement
    h, w = left_rgb.shape[:2]
    l8, r8 = torch.from_numpy(left_rgb).to(DEV), torch.from_numpy(right_rgb).to(DEV)
    with torch.no_grad():
        lut, _ = ops.frame_lut(ops.frame_histogram(l8, r8), h * w)
        fl, fr = ops.frame_apply(l8, r8, lut, (32, 64), *placement(h, w, 32, 64))
        disp = plain.forward_frame(fl, fr).clone()
        disp_m = plain.forward_frame(*ops.mirror_pair(fl.contiguous(), fr.contiguous())).clone()
        diff = ops.lr_consistency(disp, disp_m, 0.0, w, outputs=("diff",))["diff"]
    diff = np.sort(diff[0, 0, 32 - h:, :w].cpu().numpy().reshape(-1))
    tau = float(diff[int(0.6 * diff.size)])
    assert np.isfinite(tau), f"only {int(np.isfinite(diff).sum())} of {diff.size} pixels are in view"
    return tau


def rectify_maps(raw=RAW, rect=RECT):
    from dcanet_amd.geometry import RectifyMaps
    return RectifyMaps.from_matrices(*REF.smooth_matrices(raw, rect), raw, rect)


# model: False for a class that takes none (and so no frame and no graph=); items: None, or (rng, sizes) -> the third item of
# every frame (a hint map, a pose), one per pair
Case = collections.namedtuple("Case", "id cls ctor call sizes model items", defaults=(True, None))


def hint_maps(rng, sizes, device=False):
    """sparse float32 hint maps of the images: one pixel in eight carries a disparity in [1, 24), the others +0.0"""
    maps = [np.where(rng.random((h, w)) < 0.125, rng.uniform(1.0, 24.0, (h, w)), 0.0).astype(np.float32) for h, w in sizes]
    return [torch.from_numpy(m).to(DEV) for m in maps] if device else maps


def poses(rng, sizes):
    """the camera moves 2 cm forward per frame"""
    pose = np.tile(np.eye(4), (len(sizes), 1, 1))
    pose[:, 2, 3] = 0.02 * np.arange(len(sizes))
    return list(pose)


def wrapper_cases():
    """Case(id, class name, constructor keywords, call keywords, sizes of the three pairs[, model, items]): the smallest set
    that reaches every branch of the glue around the network in inference.py.  Every case runs eagerly (graph=False) in the
    32 x 64 frame: a full frame, an image smaller than the frame, the full frame again -- but small, full, full for
    KittiInferenceTemporal, whose state drops when the window changes: the last call then reprojects and fuses."""
    from dcanet_amd.geometry import StereoCalib
    sizes, hr_sizes, raw_sizes = [(32, 64), (28, 50), (32, 64)], [(64, 128), (55, 99), (64, 128)], [RAW] * 3
    dev_io, u16 = dict(device_io=True), dict(as_uint16=True)
    # every positive disparity has a depth: the vertex count is the mask's own
    geo = dict(calib=StereoCalib(40.0, 0.5, 31.5, 15.5), min_disp=0.0, max_depth=1e30, device_io=True)
    post = dict(speckle=(20, 1.0), median=3)
    out = [("plain/host", "KittiInference", {}, {}, sizes),
           ("plain/device", "KittiInference", dev_io, {}, sizes),
           ("plain/device_u16", "KittiInference", dev_io, u16, sizes),
           ("plain/device_rectify", "KittiInference", dict(device_io=True, rectify=rectify_maps()), {}, raw_sizes),
           ("confidence/device", "KittiInferenceWithConfidence", dict(radius=2, device_io=True), {}, sizes),
           ("confidence/device_u16", "KittiInferenceWithConfidence", dict(radius=2, device_io=True), u16, sizes),
           ("lr/host", "KittiInferenceLR", dict(tau=1.0), {}, sizes),
           ("lr/device", "KittiInferenceLR", dict(tau=1.0, device_io=True), {}, sizes),
           ("filtered/none", "KittiInferenceFiltered", dict(mask=None), {}, sizes),
           ("filtered/none_median3_only", "KittiInferenceFiltered", dict(mask=None, median=3, speckle=None), {}, sizes),
           ("filtered/confidence_median5", "KittiInferenceFiltered", dict(mask="confidence", median=5), {}, sizes),
           ("filtered/lr", "KittiInferenceFiltered", dict(mask="lr"), {}, sizes)]
    out += [(f"highres/{m or 'none'}", "HighResInference", dict(scale=2, mask=m), {}, hr_sizes) for m in (None, "confidence", "lr")]
    out += [(f"3d/{m or 'none'}", "KittiInference3D", dict(mask=m, **geo), {}, sizes) for m in (None, "confidence", "lr")]
    out += [("3d/none_speckle_median3", "KittiInference3D", dict(mask=None, **post, **geo), {}, sizes),
            ("3d/stride2", "KittiInference3D", dict(stride=2, **geo), {}, sizes),
            ("3d/rectify", "KittiInference3D", dict(rectify=rectify_maps(), min_disp=0.0, max_depth=1e30, device_io=True), {}, raw_sizes)]
    out += [(f"color/{m or 'none'}", "KittiInferenceColor", dict(mask=m), {}, sizes) for m in (None, "confidence", "lr")]
    out += [("color/auto", "KittiInferenceColor", dict(max_disp="auto"), {}, sizes),
            ("color/gray", "KittiInferenceColor", dict(cmap="gray"), {}, sizes),
            ("color/post_mask_min0", "KittiInferenceColor", dict(mask_min=0.0, **post), {}, sizes),
            ("color/post_mask_min05", "KittiInferenceColor", dict(mask_min=0.5, **post), {}, sizes)]
    out = [Case(*c) for c in out]
    # the wrappers that came after the record of the cases above (see "added_on" in the golden file)
    device_hints = lambda rng, sz: hint_maps(rng, sz, device=True)      # noqa: E731
    ground = dict(calib=geo["calib"], grid=(0.5, 4.0, 16.0), plane=dict(min_votes=4, min_inliers=8), segment=dict(min_run=2))
    seq = dict(calib=StereoCalib(40.0, 0.5, 24.5, 13.5), q=0.01, meas_var=1.0, gate=4.0)
    seq_sizes = [sizes[1], sizes[0], sizes[0]]
    post6 = dict(median=3, speckle=(6, 1.0))
    out += [Case("guided/numpy", "KittiInferenceGuided", {}, {}, sizes, items=hint_maps),
            Case("guided/device", "KittiInferenceGuided", {}, {}, sizes, items=device_hints),
            Case("guided/sgm", "KittiInferenceGuided", dict(sgm=dict(max_disp=16)), {}, sizes),
            Case("ground/none", "KittiInferenceGround", dict(mask=None, **ground), {}, sizes),
            Case("ground/confidence_post", "KittiInferenceGround", dict(mask="confidence", **post, **ground), {}, sizes),
            Case("ground/rectify", "KittiInferenceGround", dict(rectify=rectify_maps(), **{**ground, "calib": None}), {}, raw_sizes),
            Case("stixels/defaults", "KittiInferenceStixels", dict(calib=geo["calib"]), {}, sizes),
            Case("temporal/none_guide", "KittiInferenceTemporal", dict(mask=None, guide=(10.0, 1.0), **seq), {}, seq_sizes, items=poses),
            Case("temporal/confidence", "KittiInferenceTemporal", dict(mask="confidence", **seq), {}, seq_sizes, items=poses),
            Case("sgm/none", "SGMInference", dict(max_disp=16, lr_tau=None), {}, sizes, model=False),
            Case("sgm/lr_post", "SGMInference", dict(max_disp=16, lr_tau=1.0, **post6), {}, sizes, model=False)]
    return out
