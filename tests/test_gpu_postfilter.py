"""Disparity post-filter on the MI355X (csrc/postfilter.hip): the speckle filter and the median bit for bit against the numpy
restatements of dcanet_amd/postfilter.py on the cases of tests/_postfilter_cases.py, the workspace under hipGraph replay,
and the way through inference.KittiInferenceFiltered and the `speckle=` / `median=` keywords of KittiInference3D.

Why bitwise, without any tolerance: the only floating-point operation is |a - b| <= max_diff, one IEEE fp32 subtraction
in numpy and in the kernel alike; everything after it is integer arithmetic or a copy of an input value, and a component's
size does not depend on the order in which its pixels were united."""
import numpy as np
import pytest
import torch

from _inference_cases import lr_tau as _lr_tau, model as _model, pairs as _pairs
from _postfilter_cases import flipped, median_cases, speckle_cases
from dcanet_amd.postfilter import median_filter_host, speckle_filter_host

pytestmark = pytest.mark.gpu
DEV = "cuda"


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)         # (a copy: the cases are read-only)


def same_bits(got, want, name):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
    bits = np.uint32 if got.dtype == np.float32 else got.dtype
    bad = np.nonzero(got.view(bits) != want.view(bits))
    assert len(bad[0]) == 0, f"{name}: {len(bad[0])} pixels differ, first at {[int(i[0]) for i in bad]}: " \
                             f"{got[bad][0]} != {want[bad][0]}"


_REF = {}


def _speckle_ref(case, batch):
    """the restatement of a case, computed once for the module and never modified"""
    if (case.name, batch) not in _REF:
        d, mask = (flipped(case.d), flipped(case.mask)) if batch == 2 else (case.d, case.mask)
        _REF[case.name, batch] = (d, mask, speckle_filter_host(d, case.max_size, case.max_diff, mask=mask, window=case.window))
    return _REF[case.name, batch]


@pytest.mark.parametrize("batch", [1, 2])
@pytest.mark.parametrize("case", speckle_cases(), ids=lambda c: c.name)
def test_speckle_filter_is_the_restatement_bit_for_bit(case, batch):
    from dcanet_amd import ops
    d, mask, ref = _speckle_ref(case, batch)
    got = ops.speckle_filter(dev(d), case.max_size, case.max_diff, mask=dev(mask), window=case.window)
    assert set(got) == {"disp", "valid", "size"}
    print(case.name, batch, ref["valid"].shape, "kept", int(ref["valid"].sum()), "largest", int(ref["size"].max()))
    for k in ("size", "valid", "disp"):
        same_bits(got[k], ref[k], f"{case.name} B={batch} {k}")
    again = ops.speckle_filter(dev(d), case.max_size, case.max_diff, mask=dev(mask), window=case.window)
    assert all(torch.equal(again[k], got[k]) for k in ("size", "valid")), "two runs differ"
    assert torch.equal(again["disp"].view(torch.int32), got["disp"].view(torch.int32))
    if batch == 1:               # (1,1,Hc,Wc) in, (1,1,rows,cols) out; another fill value
        four = ops.speckle_filter(dev(d)[None, None], case.max_size, case.max_diff, window=case.window, fill=-1.0,
                                  mask=None if mask is None else dev(mask)[None, None])
        assert four["size"].shape == (1, 1) + ref["size"].shape and torch.equal(four["size"][0, 0], got["size"])
        want = np.where(ref["valid"] == 1, ref["disp"], np.float32(-1))
        same_bits(four["disp"][0, 0], want, f"{case.name} fill")


@pytest.mark.parametrize("ksize", [3, 5])
@pytest.mark.parametrize("case", median_cases(), ids=lambda c: c[0])
def test_median_filter_is_the_restatement_bit_for_bit(case, ksize):
    from dcanet_amd import ops
    name, d, mask, window = case
    same_bits(ops.median_filter(dev(d), ksize, mask=dev(mask), window=window),
              median_filter_host(d, ksize, mask=mask, window=window), f"{name} k={ksize}")
    d2, m2 = flipped(d), flipped(mask)
    want = median_filter_host(d2, ksize, mask=m2, window=window)
    same_bits(ops.median_filter(dev(d2), ksize, mask=dev(m2), window=window), want, f"{name} k={ksize} B=2")
    out = torch.full(want.shape, 7.0, device=DEV)
    assert ops.median_filter(dev(d2), ksize, mask=dev(m2), window=window, out=out) is out
    same_bits(out, want, f"{name} k={ksize} out=")


def test_speckle_filter_outputs_valid_only_writes_only_that():
    from dcanet_amd import ops
    case = speckle_cases()[0]
    d, mask, ref = _speckle_ref(case, 1)
    disp = torch.full(d.shape, 123.0, device=DEV)
    size = torch.full(d.shape, -5, device=DEV, dtype=torch.int32)
    valid = torch.full(d.shape, 9.0, device=DEV)
    got = ops.speckle_filter(dev(d), case.max_size, case.max_diff, mask=dev(mask), outputs=("valid",),
                             out={"disp": disp, "size": size, "valid": valid})
    assert set(got) == {"valid"} and got["valid"] is valid
    same_bits(valid, ref["valid"], "valid only")
    assert (disp == 123.0).all() and (size == -5).all()
    part = ops.speckle_filter(dev(d), case.max_size, case.max_diff, mask=dev(mask), outputs=("size",))
    assert set(part) == {"valid", "size"}
    same_bits(part["size"], ref["size"], "size only")


def test_speckle_filter_under_graph_replay_reinitialises_its_workspace():
    """`out=` and `workspace=`: nothing is allocated, so the four launches are captured (a linear graph) and replayed on two
    inputs copied into the static buffer, the second with FEWER and other components than the first -- what a call leaves in
    the workspace must not reach the next one.  The workspace starts out as garbage."""
    from dcanet_amd import ops
    by = {c.name: c for c in speckle_cases()}
    first, second = by["scene 70x150"], by["checkerboard, identity"]
    H, W = first.d.shape
    inputs = [first.d, np.full((H, W), 3.0, np.float32)]
    inputs[1][:second.d.shape[0], :second.d.shape[1]] = second.d
    static = torch.empty((H, W), device=DEV)
    out = {"disp": torch.empty((H, W), device=DEV), "valid": torch.empty((H, W), device=DEV),
           "size": torch.empty((H, W), device=DEV, dtype=torch.int32)}
    ws = ops.speckle_workspace(H, W, DEV)
    ws[0].fill_(5), ws[1].fill_(-3)
    static.copy_(dev(inputs[1]))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.speckle_filter(static, 50, 1.0, out=out, workspace=ws)                       # warm-up, outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = ops.speckle_filter(static, 50, 1.0, out=out, workspace=ws)
    assert all(res[k] is out[k] for k in out)
    for d in inputs + inputs[:1]:
        static.copy_(dev(d))
        graph.replay()
        torch.cuda.synchronize()
        ref = speckle_filter_host(d, 50, 1.0)
        for k in ("size", "valid", "disp"):
            same_bits(out[k], ref[k], f"replay {k}")
    with pytest.raises(RuntimeError):
        ops.speckle_filter(static, 50, 1.0, workspace=(ws[0][:10], ws[1]))
    with pytest.raises(RuntimeError):
        ops.speckle_filter(static, 50, 1.0, workspace=(ws[0], ws[0]))


def test_postfilter_operators_refuse_what_they_cannot_do():
    from dcanet_amd import ops
    a = torch.zeros(2, 1, 4, 8, device=DEV)
    for bad in (dict(max_size=-1), dict(max_size=2.5), dict(max_diff=-1.0), dict(max_diff=float("nan")),
                dict(max_diff=float("inf")), dict(window=(0, 5, 8)), dict(window=(1, 4, 8)), dict(window=(0, 4, 9)),
                dict(window=(0, 0, 8)), dict(outputs=("nope",)), dict(mask=a[:1]), dict(mask=a, mask_min=float("nan")),
                dict(mask=a.double()), dict(out={"nope": a}), dict(out={"disp": a[0]}), dict(out={"size": a})):
        kw = dict(max_size=10, max_diff=1.0)
        kw.update(bad)
        with pytest.raises(RuntimeError):
            ops.speckle_filter(a, **kw)
    for t in (a.double(), a[..., ::2], a.expand(2, 3, 4, 8).contiguous(), a.clone().requires_grad_()):
        with pytest.raises(RuntimeError):
            ops.speckle_filter(t, 10, 1.0)
        with pytest.raises(RuntimeError):
            ops.median_filter(t, 3)
    for bad in (dict(ksize=4), dict(ksize=1), dict(ksize=3, window=(0, 5, 8)), dict(ksize=3, mask=a[:1]),
                dict(ksize=3, out=a), dict(ksize=5, out=torch.empty(2, 1, 4, 7, device=DEV))):
        with pytest.raises(RuntimeError):
            ops.median_filter(a, **bad)
    with torch.no_grad():
        assert set(ops.speckle_filter(a.clone().requires_grad_(), 10, 1.0)) == {"disp", "valid", "size"}


# ---- through the wrappers ---------------------------------------------------------------------------------------------------
WRAP = dict(crop_height=32, crop_width=64, graph=True, device_io=True)


def _split(disp, mask, mask_min, median):
    """(max_size, max_diff) that split THIS map: max_diff the median difference of horizontal neighbours (about half of the
    pairs join), max_size the median component size over the active pixels (the pixels above it stay, the others go)"""
    from dcanet_amd import ops
    d = dev(disp)
    if median:
        d = ops.median_filter(d, median, mask=dev(mask), mask_min=mask_min)
    max_diff = float(np.median(np.abs(np.diff(d.cpu().numpy(), axis=1))))
    size = ops.speckle_filter(d, 0, max_diff, mask=dev(mask), mask_min=mask_min, outputs=("size",))["size"].cpu().numpy()
    return int(np.median(size[size > 0])), max_diff


def _want(disp, mask, mask_min, median, speckle):
    from dcanet_amd import ops
    d = dev(disp)
    if median:
        d = ops.median_filter(d, median, mask=dev(mask), mask_min=mask_min)
    r = ops.speckle_filter(d, *speckle, mask=dev(mask), mask_min=mask_min)
    return r["disp"].cpu().numpy(), r["valid"].cpu().numpy()


@pytest.mark.parametrize("mode,median", [(None, 0), (None, 3), ("confidence", 5), ("lr", 0)])
def test_kitti_inference_filtered(mode, median, monkeypatch):
    """a full-frame image and a 28 x 50 one in the 32 x 64 frame: the result is ops.median_filter, then ops.speckle_filter, of
    the disparity (and the mask) that the EXISTING class of that mode hands out for the frame; stream() gives the same bytes"""
    from dcanet_amd.inference import KittiInference, KittiInferenceFiltered, KittiInferenceLR, KittiInferenceWithConfidence
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    model = _model()
    pairs = _pairs(np.random.default_rng(23), [(32, 64), (28, 50)])
    plain = KittiInference(model, **WRAP)
    tau = 1.0
    if mode == "confidence":
        own = [KittiInferenceWithConfidence(model, **WRAP)(l, r) for l, r in pairs]
    elif mode == "lr":
        tau = _lr_tau(plain, *pairs[0])
        lr = KittiInferenceLR(model, tau=tau, **WRAP)
        own = [(plain(l, r), lr(l, r)[1]) for l, r in pairs]                 # the UNFILLED disparity, the check's validity
    else:
        own = [(plain(l, r), None) for l, r in pairs]
    mask_min = 0.5 if mode != "confidence" else float(np.median(own[0][1]))
    speckle = _split(own[0][0], own[0][1], mask_min, median)
    infer = KittiInferenceFiltered(model, median=median, speckle=speckle, mask=mode, mask_min=mask_min, tau=tau, **WRAP)
    single = []
    for i, ((l, r), (disp, mask)) in enumerate(zip(pairs, own)):
        h, w = l.shape[:2]
        want_d, want_v = _want(disp, mask, mask_min, median, speckle)
        got_d, got_v = infer(l, r)
        single.append((got_d, got_v))
        print(f"mode={mode} median={median} image {h}x{w} speckle={speckle}: kept {int(want_v.sum())} of {h * w}")
        assert got_d.shape == got_v.shape == (h, w) and got_d.dtype == got_v.dtype == np.float32
        assert got_v.tobytes() == want_v.tobytes(), f"image {i}: valid"
        assert got_d.tobytes() == want_d.tobytes(), f"image {i}: disp"
        if i == 0:
            assert 0 < want_v.sum() < want_v.size
    streamed = list(infer.stream(iter(pairs + pairs[:1]), depth=2))
    assert len(streamed) == 3
    for (gd, gv), (sd, sv) in zip(streamed, single + single[:1]):
        assert gd.tobytes() == sd.tobytes() and gv.tobytes() == sv.tobytes()
    if mode is None and median == 0:             # without a speckle filter: valid = active, the disparity unchanged there
        off = KittiInferenceFiltered(model, speckle=None, **WRAP)(*pairs[1])
        assert off[0].tobytes() == np.ascontiguousarray(own[1][0]).tobytes() and (off[1] == 1).all()


@pytest.mark.parametrize("mode", [None, "confidence"])
def test_kitti_inference_3d_with_the_speckle_filter(mode, monkeypatch):
    """depth == 0 exactly where the filter's valid is 0 (all other filters passing everything), one vertex per pixel that passes
    the mask and the filters, the disparity handed out is the filtered one; without the keywords the Frame3D is today's"""
    from dcanet_amd.geometry import StereoCalib
    from dcanet_amd.inference import KittiInference, KittiInference3D, KittiInferenceWithConfidence
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    model = _model()
    calib = StereoCalib(40.0, 0.5, 31.5, 15.5)
    pairs = _pairs(np.random.default_rng(29), [(32, 64), (28, 50)])
    if mode == "confidence":
        own = [KittiInferenceWithConfidence(model, **WRAP)(l, r) for l, r in pairs]
    else:
        own = [(KittiInference(model, **WRAP)(l, r), None) for l, r in pairs]
    mask_min = 0.5 if mode is None else float(np.median(own[0][1]))
    kw = dict(mask=mode, mask_min=mask_min, min_disp=0.0, max_depth=1e30)          # every positive disparity has a depth
    speckle = _split(own[0][0], own[0][1], mask_min, 0)
    today = KittiInference3D(model, calib, **kw, **WRAP)
    default = KittiInference3D(model, calib, speckle=None, median=0, **kw, **WRAP)
    infer = KittiInference3D(model, calib, speckle=speckle, **kw, **WRAP)
    for i, ((l, r), (disp, mask)) in enumerate(zip(pairs, own)):
        h, w = l.shape[:2]
        want_d, want_v = _want(disp, mask, mask_min, 0, speckle)
        got = infer(l, r)
        assert got.disp.tobytes() == want_d.tobytes(), f"image {i}: the disparity handed out is the filtered one"
        keep = (want_v == 1) & (want_d > 0)          # (an active pixel already passed the mask; a disparity of 0 has no depth)
        print(f"mode={mode} image {h}x{w} speckle={speckle}: kept {int(keep.sum())}, disparities <= 0: {int((disp <= 0).sum())}")
        assert np.array_equal(got.depth == 0, ~keep), f"image {i}: depth is 0 exactly where the filter's valid is 0"
        assert len(got.vertices) == int(keep.sum())
        want_z = (np.float32(calib.fb) / (want_d[keep] + np.float32(calib.doffs))).astype(np.float32)
        assert np.array_equal(got.depth[keep], want_z) and np.array_equal(got.vertices["z"], want_z)
        if mode is not None:
            assert got.mask.tobytes() == np.ascontiguousarray(mask).tobytes()
        if i == 0:
            assert 0 < keep.sum() < keep.size
        a, b = today(l, r), default(l, r)
        assert a.disp.tobytes() == b.disp.tobytes() == np.ascontiguousarray(disp).tobytes()
        assert a.depth.tobytes() == b.depth.tobytes() and a.vertices.tobytes() == b.vertices.tobytes()
        assert (a.mask is None and b.mask is None) or a.mask.tobytes() == b.mask.tobytes()
    with pytest.raises(ValueError):
        KittiInference3D(model, calib, speckle=speckle, mask_min=0.0, **WRAP)


def test_kitti_inference_color_with_the_speckle_filter(monkeypatch):
    """the disparity handed out is the filtered one and a removed pixel is black; without the keywords the pair is today's"""
    from dcanet_amd import ops
    from dcanet_amd.inference import KittiInference, KittiInferenceColor
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    model = _model()
    pairs = _pairs(np.random.default_rng(31), [(32, 64), (28, 50)])
    own = [KittiInference(model, **WRAP)(l, r) for l, r in pairs]
    speckle = _split(own[0], None, 0.5, 3)
    today, default = KittiInferenceColor(model, **WRAP), KittiInferenceColor(model, speckle=None, median=0, **WRAP)
    infer = KittiInferenceColor(model, speckle=speckle, median=3, **WRAP)
    for i, ((l, r), disp) in enumerate(zip(pairs, own)):
        h, w = l.shape[:2]
        want_d, want_v = _want(disp, None, 0.5, 3, speckle)
        got_d, got_rgb = infer(l, r)
        assert got_d.tobytes() == want_d.tobytes(), f"image {i}: the disparity handed out is the filtered one"
        want_rgb = ops.disp_colorize(dev(want_d), 0, h, w, max_disp=float(model.maxdisp)).cpu().numpy()
        assert got_rgb.shape == (h, w, 3) and got_rgb.tobytes() == want_rgb.tobytes()
        assert not got_rgb[want_v == 0].any() and (i > 0 or 0 < want_v.sum() < want_v.size)
        (ad, argb), (bd, brgb) = today(l, r), default(l, r)
        assert ad.tobytes() == bd.tobytes() == np.ascontiguousarray(disp).tobytes() and argb.tobytes() == brgb.tobytes()
