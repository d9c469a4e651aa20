"""Left-right consistency on the MI355X (csrc/lr_consistency.hip): both kernels bit for bit against the numpy restatement of
include/dca_hip.h in tests/_lr_reference.py, and the way through GwcNet.predict_lr and inference.KittiInferenceLR.

Why bitwise: on the restatement's scene every value is a multiple of 1/16 below 2^11, so x - d, the interpolation weight,
both products and their sum are exact in fp32 (tests/test_lr_cpu.py checks float32 numpy against float64); everything
after the comparison with tau is integer arithmetic or a copy of an input value.  No pixel is left out, +inf included."""
import numpy as np
import pytest
import torch

from _inference_cases import pairs as _pairs
from _lr_reference import SHAPES, lr_reference, scene
from oracle import dcanet_oracle as O
from oracle.seeded import seeded_tensor

pytestmark = pytest.mark.gpu
DEV = "cuda"
MAPS = ("diff", "valid", "filled", "disp_right")


def run_kernel(dl, drm, tau, cols=None, **kw):
    from dcanet_amd import ops
    out = ops.lr_consistency(torch.from_numpy(dl).to(DEV), torch.from_numpy(drm).to(DEV), tau, cols, **kw)
    return {k: v.cpu().numpy() for k, v in out.items()}


def same_bits(got, ref, name):
    for k in MAPS:
        assert got[k].shape == ref[k].shape and got[k].dtype == np.float32, (name, k)
        bad = np.nonzero(got[k].view(np.uint32) != ref[k].view(np.uint32))
        assert len(bad[0]) == 0, f"{name} {k}: {len(bad[0])} pixels differ, first at {[int(i[0]) for i in bad]}: " \
                                 f"{got[k][bad][0]} != {ref[k][bad][0]}"


_REF = {}


def _scene_ref(shape, cols=None):
    """scene and restatement of a shape, computed once for the module and never modified"""
    if (shape, cols) not in _REF:
        dl, drm = scene(shape)
        _REF[shape, cols] = (dl, drm, lr_reference(dl, drm, 1.0, cols))
    return _REF[shape, cols]


@pytest.mark.parametrize("shape", SHAPES)
def test_lr_consistency_is_the_restatement_bit_for_bit(shape):
    dl, drm, ref = _scene_ref(shape)
    got = run_kernel(dl, drm, 1.0)
    print(shape, ref["categories"], "diff == tau:", ref["diff_eq_tau"], "valid:", int(ref["valid"].sum()), "of", dl.size)
    same_bits(got, ref, f"{shape}")
    assert np.array_equal(np.isinf(got["diff"]), np.isinf(ref["diff"])) and not np.isnan(got["diff"]).any()
    again = run_kernel(dl, drm, 1.0)
    for k in MAPS:
        assert again[k].tobytes() == got[k].tobytes(), f"two runs differ in {k}"
    # (B,1,H,W) in, (B,1,H,W) out; a subset of the outputs leaves the others uncomputed and the rest unchanged
    four = run_kernel(dl[:, None], drm[:, None], 1.0)
    assert all(four[k].shape == (shape[0], 1) + shape[1:] and four[k].tobytes() == got[k].tobytes() for k in MAPS)
    part = run_kernel(dl, drm, 1.0, outputs=("filled",))
    assert set(part) == {"valid", "filled"} and all(part[k].tobytes() == got[k].tobytes() for k in part)
    only = run_kernel(dl, drm, 1.0, outputs=())
    assert set(only) == {"valid"} and only["valid"].tobytes() == got["valid"].tobytes()


@pytest.mark.parametrize("shape,cols", [((2, 4, 301), 250), ((1, 5, 67), 1)])
def test_lr_consistency_active_width(shape, cols):
    """cols < W: nothing at or beyond cols is a match target or a fill source -- poisoning those columns of either map
    changes nothing inside, and outside the maps are valid = 0, diff = +inf, filled = dl, disp_right = the un-mirrored drm"""
    dl, drm, ref = _scene_ref(shape, cols)
    got = run_kernel(dl, drm, 1.0, cols)
    same_bits(got, ref, f"{shape} cols={cols}")
    assert not got["valid"][..., cols:].any() and np.isposinf(got["diff"][..., cols:]).all()
    dl2, drm2 = dl.copy(), drm.copy()
    dl2[..., cols:] = 2.0                       # would be valid fill sources if they took part
    drm2[..., :shape[2] - cols] = 2.0           # right-image columns >= cols
    poisoned = run_kernel(dl2, drm2, 1.0, cols)
    same_bits(poisoned, lr_reference(dl2, drm2, 1.0, cols), f"{shape} cols={cols} poisoned")
    for k in ("diff", "valid"):
        assert poisoned[k].tobytes() == got[k].tobytes()
    assert poisoned["filled"][..., :cols].tobytes() == got["filled"][..., :cols].tobytes()


def test_lr_consistency_at_the_widest_row():
    """W = 8192: runs of 32 columns (every bit of a thread's mask), and the 64 KB of LDS that need the launch attribute"""
    shape = (1, 2, 8192)
    dl, drm = scene(shape)
    ref = lr_reference(dl, drm, 1.0)
    same_bits(run_kernel(dl, drm, 1.0), ref, "8192")
    assert 0 < ref["valid"].sum() < ref["valid"].size
    ref = lr_reference(dl, drm, 1.0, 7937)      # 32 columns per run, the last thread's run empty
    same_bits(run_kernel(dl, drm, 1.0, 7937), ref, "8192 cols=7937")


def test_lr_consistency_nan_and_non_positive_disparities():
    """a NaN never becomes valid and is never a fill source: diff is +inf where d is NaN (not in view) and NaN where the
    matched right disparity is NaN; d <= 0 is not in view"""
    shape = (1, 5, 67)
    dl, drm = (a.copy() for a in scene(shape)[:2])
    W = shape[2]
    dl[0, 1, 30] = np.nan
    dl[0, 1, 31] = 0.0
    dl[0, 1, 32] = -2.0
    dl[0, 2, 40] = 3.5
    drm[0, 2, W - 1 - 36] = np.nan                  # dR(36), the left neighbour of 40 - 3.5
    drm[0, 2, W - 1 - 37] = np.nan                  # dR(37)
    dl[0, 3, 20] = np.inf
    ref = lr_reference(dl, drm, 1.0)
    got = run_kernel(dl, drm, 1.0)
    assert np.isposinf(got["diff"][0, 1, 30:33]).all() and not got["valid"][0, 1, 30:33].any()
    assert np.isnan(got["diff"][0, 2, 40]) and got["valid"][0, 2, 40] == 0
    assert np.isposinf(got["diff"][0, 3, 20]) and got["valid"][0, 3, 20] == 0
    assert np.array_equal(np.isnan(got["diff"]), np.isnan(ref["diff"]))
    keep = ~np.isnan(ref["diff"])                   # a NaN has no one bit pattern: position only
    assert np.array_equal(got["diff"][keep].view(np.uint32), ref["diff"][keep].view(np.uint32))
    for k in ("valid", "filled", "disp_right"):     # copies of input values: NaN payloads included
        assert got[k].tobytes() == ref[k].tobytes(), k
    assert not np.isnan(got["filled"][0, 1]).any()  # the NaN pixel was filled from its valid neighbours


@pytest.mark.parametrize("shape", [(3, 5, 67), (1, 1, 1), (2, 3, 9, 130)])
def test_mirror_pair_is_flip_with_the_pair_swapped(shape):
    from dcanet_amd import ops
    left, right = seeded_tensor(f"lr.l{shape}", shape).to(DEV), seeded_tensor(f"lr.r{shape}", shape).to(DEV)
    left.view(-1)[0] = float("nan")                 # bit copies
    ml, mr = ops.mirror_pair(left, right)
    assert ml.shape == mr.shape == left.shape and ml.is_contiguous() and mr.is_contiguous()
    assert torch.equal(ml.view(torch.int32), torch.flip(right, [-1]).view(torch.int32))
    assert torch.equal(mr.view(torch.int32), torch.flip(left, [-1]).view(torch.int32))
    out = torch.empty((2,) + shape, device=DEV)
    a, b = ops.mirror_pair(left, right, out=out)
    assert a.data_ptr() == out[0].data_ptr() and b.data_ptr() == out[1].data_ptr()
    assert torch.equal(a.view(torch.int32), ml.view(torch.int32)) and torch.equal(b.view(torch.int32), mr.view(torch.int32))
    # twice gives the pair back
    bl, br = ops.mirror_pair(ml, mr)
    assert torch.equal(bl.view(torch.int32), left.view(torch.int32)) and torch.equal(br.view(torch.int32), right.view(torch.int32))


def test_lr_operators_refuse_what_they_cannot_do():
    from dcanet_amd import ops
    a, b = torch.zeros(2, 1, 4, 8, device=DEV), torch.zeros(2, 1, 4, 8, device=DEV)
    for bad in (dict(tau=-1.0), dict(tau=float("nan")), dict(cols=0), dict(cols=9), dict(outputs=("nope",))):
        with pytest.raises(RuntimeError):
            ops.lr_consistency(a, b, **bad)
    with pytest.raises(RuntimeError):
        ops.lr_consistency(a.cpu(), b.cpu())
    with pytest.raises(RuntimeError):
        ops.lr_consistency(a.double(), b.double())
    with pytest.raises(RuntimeError):
        ops.lr_consistency(a[..., ::2], b[..., ::2])                       # not contiguous
    with pytest.raises(RuntimeError):
        ops.lr_consistency(a, b[:1])
    with pytest.raises(RuntimeError):
        ops.lr_consistency(a.expand(2, 3, 4, 8).contiguous(), b.expand(2, 3, 4, 8).contiguous())      # (B,3,H,W)
    with pytest.raises(RuntimeError):
        ops.lr_consistency(a.clone().requires_grad_(), b)
    with pytest.raises(RuntimeError):
        ops.lr_consistency(torch.zeros(1, 1, 8200, device=DEV), torch.zeros(1, 1, 8200, device=DEV))  # W > 8192
    with torch.no_grad():
        assert set(ops.lr_consistency(a.clone().requires_grad_(), b)) == set(MAPS)
    for bad in ((a.cpu(), b.cpu()), (a.half(), b.half()), (a[..., ::2], b[..., ::2]), (a, b[:1]),
                (a.clone().requires_grad_(), b)):
        with pytest.raises(RuntimeError):
            ops.mirror_pair(*bad)
    with pytest.raises(RuntimeError):
        ops.mirror_pair(a, b, out=torch.empty(2, 2, 1, 4, 7, device=DEV))
    both = torch.zeros(2, 2, 1, 4, 8, device=DEV)
    with pytest.raises(RuntimeError):
        ops.mirror_pair(both[0], both[1], out=both)                        # in place


# ---- through the model -----------------------------------------------------------------------------------------------------
_MODELS = {}


def _model(concat):
    """one seeded GwcNet(32) per volume mode for the whole module, never modified (eval mode, no grad)"""
    if concat not in _MODELS:
        from dcanet_amd.models.gwcnet_dca_g import GwcNet
        m = GwcNet(32, use_concat_volume=concat)
        m.load_state_dict(O.seeded_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}), strict=True)
        _MODELS[concat] = m.to(DEV).eval()
    return _MODELS[concat]


def _images():
    return seeded_tensor("smoke.left", (1, 3, 32, 64)).to(DEV), seeded_tensor("smoke.right", (1, 3, 32, 64)).to(DEV)


def _median_tau(dl, drm, cols=None):
    """a threshold that splits the in-view pixels of a network output: the median of the restatement's finite differences"""
    diff = lr_reference(dl, drm, 0.0, cols, dtype=np.float32)["diff"]
    fin = diff[np.isfinite(diff)]
    return float(np.float32(np.median(fin))) if len(fin) else 1.0


@pytest.mark.parametrize("concat", [False, True])
def test_predict_lr(concat, monkeypatch):
    from dcanet_amd import ops
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)      # MIOpen convolutions of the 2D networks
    model = _model(concat)
    left, right = _images()
    with torch.no_grad():
        pred4 = model(left, right)[0]
        mirrored = model(*ops.mirror_pair(left, right))[0]
    taus = (1.0, _median_tau(pred4[:, 0].cpu().numpy(), mirrored[:, 0].cpu().numpy()))
    for tau in taus:
        out = model.predict_lr(left, right, tau=tau)                      # grad mode on: the method turns it off itself
        assert not model.training
        assert set(out) == {"disp", "disp_filled", "valid", "lr_diff", "disp_right"}
        assert all(v.shape == (1, 1, 32, 64) and v.dtype == torch.float32 and not v.requires_grad for v in out.values())
        assert torch.equal(out["disp"], pred4), "predict_lr()['disp'] is not bitwise forward()[0]"
        with torch.no_grad():
            want = ops.lr_consistency(pred4, mirrored, tau)
        for name, key in (("disp_filled", "filled"), ("valid", "valid"), ("lr_diff", "diff"), ("disp_right", "disp_right")):
            assert torch.equal(out[name].view(torch.int32), want[key].view(torch.int32)), (name, tau)
        assert torch.equal(out["disp_right"], torch.flip(mirrored, [-1]))
        print(f"concat={concat} tau={tau:.4f}: {int(out['valid'].sum().item())} of {out['valid'].numel()} pixels valid")
    assert 0 < out["valid"].sum().item() < out["valid"].numel()           # at the median threshold both kinds occur
    model.train()
    try:
        model.predict_lr(left, right)
        assert model.training, "the training flag was not restored"
    finally:
        model.eval()
    with pytest.raises(RuntimeError):
        model.predict_lr(left.clone().requires_grad_(), right)
    assert not model.training


# ---- through the wrapper ---------------------------------------------------------------------------------------------------
def _frames(plain, left_rgb, right_rgb):
    """the float32 frames KittiInference hands its network, built the way it builds them"""
    from dcanet_amd import ops
    from dcanet_amd.inference import normalize_pair, pad_or_crop, placement
    Hc, Wc = plain.crop_height, plain.crop_width
    h, w = left_rgb.shape[:2]
    if not plain.device_io:
        fl, fr, _, _ = pad_or_crop(normalize_pair(left_rgb, right_rgb), Hc, Wc)
        return fl.to(DEV), fr.to(DEV)
    l8, r8 = torch.from_numpy(left_rgb).to(DEV), torch.from_numpy(right_rgb).to(DEV)
    lut, _ = ops.frame_lut(ops.frame_histogram(l8, r8), h * w)
    return ops.frame_apply(l8, r8, lut, (Hc, Wc), *placement(h, w, Hc, Wc))


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("device_io", [False, True])
def test_kitti_inference_lr(device_io, graph, monkeypatch):
    """a full-frame image and a 28 x 50 one in the 32 x 64 frame: the first map is the restatement's fill of KittiInference's
    own disparity with cols = the image's width, the second its validity; uint16: trunc(d * 256) and 0 / 65535.  Afterwards
    the two existing classes give what they gave before."""
    from dcanet_amd.inference import KittiInference, KittiInferenceLR, KittiInferenceWithConfidence
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    model = _model(False)
    kw = dict(crop_height=32, crop_width=64, graph=graph, device_io=device_io)
    plain, conf = KittiInference(model, **kw), KittiInferenceWithConfidence(model, **kw)
    pairs = _pairs(np.random.default_rng(11), [(32, 64), (28, 50)])
    before = [(plain(l, r), conf(l, r)) for l, r in pairs]
    refs, tau = [], None
    for (l, r), (own, _) in zip(pairs, before):
        h, w = l.shape[:2]
        with torch.no_grad():
            fl, fr = (t.clone() for t in _frames(plain, l, r))
            disp = plain.forward_frame(fl, fr).clone()
            disp_m = plain.forward_frame(torch.flip(fr, [-1]).contiguous(), torch.flip(fl, [-1]).contiguous()).clone()
        dl, drm = disp[:, 0].cpu().numpy(), disp_m[:, 0].cpu().numpy()
        assert dl[0, 32 - h:, :w].tobytes() == np.ascontiguousarray(own).tobytes(), "not KittiInference's own disparity"
        tau = _median_tau(dl, drm, w) if tau is None else tau
        # a network's output is not exact in fp32: the restatement in float32, the kernel's own operations in its order
        refs.append(lr_reference(dl, drm, tau, w, dtype=np.float32))
    infer = KittiInferenceLR(model, tau=tau, **kw)
    for i, ((l, r), ref) in enumerate(zip(pairs, refs)):
        h, w = l.shape[:2]
        want_f = np.ascontiguousarray(ref["filled"][0, 32 - h:, :w])
        want_v = np.ascontiguousarray(ref["valid"][0, 32 - h:, :w])
        filled, valid = infer(l, r)
        assert filled.shape == valid.shape == (h, w) and filled.dtype == valid.dtype == np.float32
        print(f"device_io={device_io} graph={graph} image {h}x{w} tau={tau:.4f}: {int(want_v.sum())} of {h * w} valid")
        assert np.ascontiguousarray(filled).tobytes() == want_f.tobytes(), f"image {i}: filled"
        assert np.ascontiguousarray(valid).tobytes() == want_v.tobytes(), f"image {i}: valid"
        if i == 0:
            assert 0 < want_v.sum() < want_v.size
        f16, v16 = infer(l, r, as_uint16=True)
        assert f16.dtype == v16.dtype == np.uint16 and f16.shape == v16.shape == (h, w)
        assert np.array_equal(f16, np.trunc(want_f * np.float32(256)).astype(np.uint16))       # 0 <= d < 32
        assert set(np.unique(v16)) <= {0, 65535} and np.array_equal(v16, want_v.astype(np.uint16) * 65535)
    for (l, r), (own, (cd, cc)) in zip(pairs, before):
        assert np.ascontiguousarray(plain(l, r)).tobytes() == np.ascontiguousarray(own).tobytes()
        d2, c2 = conf(l, r)
        assert np.ascontiguousarray(d2).tobytes() == np.ascontiguousarray(cd).tobytes()
        assert np.ascontiguousarray(c2).tobytes() == np.ascontiguousarray(cc).tobytes()


def test_lr_stream_equals_one_at_a_time_calls(monkeypatch):
    from dcanet_amd.inference import KittiInferenceLR
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    infer = KittiInferenceLR(_model(False), crop_height=32, crop_width=64, graph=True, device_io=True, tau=1.0)
    pairs = _pairs(np.random.default_rng(13), [(28, 50), (32, 64), (28, 50), (32, 64), (30, 64)])
    single = [infer(l, r) for l, r in pairs]
    assert single[0][0].tobytes() != single[2][0].tobytes()                                # same size, different content
    got = list(infer.stream(iter(pairs), depth=2))
    assert len(got) == 5
    for i, (g, s) in enumerate(zip(got, single)):
        assert isinstance(g, tuple) and len(g) == 2
        for a, b in zip(g, s):
            assert a.shape == b.shape and a.tobytes() == b.tobytes(), f"frame {i} differs"
    for (f16, v16), (f, v) in zip(infer.stream(pairs, depth=2, as_uint16=True), single):
        assert np.array_equal(f16, np.trunc(f * np.float32(256)).astype(np.uint16))
        assert np.array_equal(v16, v.astype(np.uint16) * 65535)
