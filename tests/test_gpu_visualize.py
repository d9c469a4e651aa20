"""GPU checks of the picture stage (csrc/visualize.hip).  Every comparison is BITWISE against the numpy
restatement tests/_vis_reference.py (include/dca_hip.h pins each operation in fp32), the error image also against the
REFERENCE's recorded result (tests/golden/vis_error_image.npz).  Outputs are written into sentinel-filled buffers whose tail
must stay untouched.  Shapes: widths that are and are not multiples of 4 (16-byte loads / scalar tail, dword / byte stores),
a padded prediction, windows with y0 > 0 and cols < Wc, more than one workgroup."""
import numpy as np
import pytest
import torch

import _vis_reference as REF

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 4096


def guarded(shape, dtype):
    """(whole buffer, its leading view of `shape`): sentinel bytes everywhere, GUARD bytes behind the view"""
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    whole = torch.full((n + GUARD,), 0xA5, device=DEV, dtype=torch.uint8)
    return whole, whole[:n].view(dtype).view(shape)


def tail_untouched(whole):
    return bool((whole[-GUARD:] == 0xA5).all())


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- error image -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,top_pad,right_pad,legend", [(0, 0, 0, True), (1, 0, 0, True), (2, 0, 0, True), (0, 3, 5, True),
                                                           (0, 0, 0, False), (2, 4, 0, False)])
def test_error_image(golden, case, top_pad, right_pad, legend):
    from dcanet_amd import ops
    fx = golden("vis_error_image")
    est, gt, image = fx[f"est{case}"], fx[f"gt{case}"], fx[f"image{case}"]
    B, H, W = gt.shape
    pred = np.full((B, H + top_pad, W + right_pad), np.nan, dtype=np.float32)       # a pad that is read shows up as black
    pred[:, top_pad:, :W] = est
    want_f, want_u = REF.error_image(pred, gt, legend=legend, top_pad=top_pad)
    if legend:
        assert want_f.tobytes() == image.tobytes()
    wf, of = guarded((B, 3, H, W), torch.float32)
    wu, ou = guarded((B, H, W, 3), torch.uint8)
    got_f, got_u = ops.disp_error_image(dev(pred), dev(gt), legend=legend, u8=True, out_f32=of, out_u8=ou)
    assert got_f is of and got_u is ou
    assert got_f.cpu().numpy().tobytes() == want_f.tobytes() and np.array_equal(got_u.cpu().numpy(), want_u)
    assert tail_untouched(wf) and tail_untouched(wu)
    # each output on its own, allocated by the operator; (B,1,Hp,Wp) as the network hands it out
    only_f, none = ops.disp_error_image(dev(pred)[:, None], dev(gt), legend=legend)
    none2, only_u = ops.disp_error_image(dev(pred), dev(gt), legend=legend, f32=False, u8=True)
    assert none is None and none2 is None and torch.equal(only_f, got_f) and torch.equal(only_u, got_u)


def test_error_image_through_the_reference_surface(golden):
    from dcanet_amd.utils import disp_error_image_func
    fx = golden("vis_error_image")
    got = disp_error_image_func.forward(None, dev(fx["est2"]), dev(fx["gt2"]))
    assert got.is_cuda and got.dtype == torch.float32 and got.cpu().numpy().tobytes() == fx["image2"].tobytes()


# ---- range -------------------------------------------------------------------------------------------------------------------
def maps(seed, B, Hc, Wc):
    """disparities in (0, 100) with NaN, +-inf, 0 and negative pixels, and a mask in [0, 1]"""
    rs = np.random.RandomState(seed)
    d = (100 * rs.rand(B, Hc, Wc)).astype(np.float32)
    kind = rs.randint(0, 40, (B, Hc, Wc))
    for k, v in enumerate((np.nan, np.inf, -np.inf, 0.0, -3.0)):
        d[kind == k] = v
    m = rs.rand(B, Hc, Wc).astype(np.float32)
    d[:, 0, -1], m[:, 0, -1] = 150.0, 0.25                     # the maximum: outside every window below, and masked out
    d[:, 4, 1], m[:, 4, 1] = 120.0, 0.25                       # the maximum of every window below, masked out
    return d, m


@pytest.mark.parametrize("B,Hc,Wc,window", [(2, 9, 37, None), (1, 16, 64, None), (2, 9, 37, (2, 6, 30)), (1, 16, 64, (3, 13, 50)),
                                            (2, 70, 100, None)])
def test_disp_range(B, Hc, Wc, window):
    from dcanet_amd import ops
    d, m = maps(Hc + Wc, B, Hc, Wc)
    if B > 1:
        d[1][d[1] > 0] = 0.0                                      # an image without a valid pixel
    for mask in (None, m):
        want = REF.disp_range(d, window, mask, 0.5)
        got = ops.disp_range(dev(d), window, None if mask is None else dev(mask), 0.5)
        assert got.shape == (B, 2) and got.dtype == torch.float32
        assert got.cpu().numpy().tobytes() == want.tobytes(), (got, want)
        assert 0 < want[0, 0] < want[0, 1] and (B == 1 or want[1].tolist() == [0.0, 0.0])
    everything = REF.disp_range(d, None, None)
    assert window is None or (REF.disp_range(d, window, None) != everything).any(), "the window must matter"
    assert (REF.disp_range(d, window, m, 0.5) != REF.disp_range(d, window, None)).any(), "the mask must matter"
    one = ops.disp_range(dev(d[0]))                               # a single (Hc,Wc) map
    assert one.shape == (1, 2) and one.cpu().numpy().tobytes() == everything[:1].tobytes()


# ---- colour-coded map -----------------------------------------------------------------------------------------------------------
def ramp(Hc, Wc, max_disp):
    """a map whose disparities pass through every segment boundary of the KITTI map (and beyond max_disp), with the boundaries
    themselves and one pixel of every invalid kind"""
    n = Hc * Wc
    d = (np.arange(n, dtype=np.float64) / (n - 1) * 1.1 * max_disp).astype(np.float32).reshape(Hc, Wc)
    d[-1, :8] = (REF.KITTI_C.astype(np.float64) / 1000 * max_disp).astype(np.float32)
    d[4, :5] = np.nan, np.inf, -np.inf, 0.0, -2.0
    t = d[np.isfinite(d) & (d > 0)] / np.float32(max_disp) * np.float32(1000)
    assert all(((t > lo) & (t < hi)).any() for lo, hi in zip(REF.KITTI_C[:-1], REF.KITTI_C[1:])) and (t > 1000).any()
    return d


@pytest.mark.parametrize("cmap", ["kitti", "gray"])
@pytest.mark.parametrize("Hc,Wc,y0,rows,cols", [(12, 37, 0, 12, 37), (12, 64, 0, 12, 64), (12, 37, 3, 9, 30), (43, 64, 3, 40, 64),
                                                (43, 64, 3, 40, 61)])
def test_disp_colorize(cmap, Hc, Wc, y0, rows, cols):
    from dcanet_amd import ops
    max_disp = 64.0
    d = ramp(Hc, Wc, max_disp)
    m = np.random.RandomState(Hc + Wc).rand(Hc, Wc).astype(np.float32)
    dd, dm = dev(d), dev(m)
    for mask, dmask in ((None, None), (m, dm)):
        # the fixed range
        want = REF.colorize(d, y0, rows, cols, 0.0, max_disp, cmap, mask, 0.5)
        whole, out = guarded((rows, cols, 3), torch.uint8)
        got = ops.disp_colorize(dd, y0, rows, cols, max_disp=max_disp, cmap=cmap, mask=dmask, out=out)
        assert got is out and np.array_equal(got.cpu().numpy(), want) and tail_untouched(whole)
        # the range disp_range left on the device
        rng = ops.disp_range(dd, (y0, rows, cols), dmask, 0.5)
        lo, hi = REF.disp_range(d[None], (y0, rows, cols), None if mask is None else mask[None], 0.5)[0]
        assert rng.cpu().numpy().tobytes() == np.array([[lo, hi]], dtype=np.float32).tobytes()
        want = REF.colorize(d, y0, rows, cols, lo, hi, cmap, mask, 0.5)
        got = ops.disp_colorize(dd.view(1, 1, Hc, Wc), y0, rows, cols, range=rng, cmap=cmap,
                                mask=None if dmask is None else dmask.view(1, 1, Hc, Wc))
        assert got.shape == (rows, cols, 3) and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)
    if y0 <= 4 < y0 + rows:
        assert not want[4 - y0, :5].any(), "NaN, inf, -inf, 0 and negative pixels are black"
    assert want.any() and (mask is None or not want[m[y0:y0 + rows, :cols] < 0.5].any())
    with pytest.raises(RuntimeError):
        ops.disp_colorize(dd, y0, rows, cols)                     # neither max_disp nor range
    with pytest.raises(RuntimeError):
        ops.disp_colorize(dd, y0, Hc + 1, cols, max_disp=max_disp)    # the window leaves the map


# ---- EvalStep ------------------------------------------------------------------------------------------------------------------
def test_eval_step_error_images(monkeypatch):
    from test_gpu_eval import frames, seeded_model
    from dcanet_amd import evaluation as E
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    m = seeded_model()
    L, R, gt = frames("eval")
    on, off = E.EvalStep(m, maxdisp=64, error_images=True), E.EvalStep(m, maxdisp=64)
    on.step(L, R, gt)
    off.step(L, R, gt)
    assert "error_image" not in off.last and torch.equal(on.last["pred"], off.last["pred"])
    img = on.last["error_image"]
    assert img.shape == (2, 60, 120, 3) and img.dtype == torch.uint8 and img.is_cuda
    assert (on.last["top_pad"], on.last["right_pad"]) == (4, 8)
    want = REF.error_image(on.last["pred"][:, 0].cpu().numpy(), gt.cpu().numpy(), top_pad=4)[1]
    assert np.array_equal(img.cpu().numpy(), want)
    assert len(np.unique(want.reshape(-1, 3), axis=0)) > 5, "degenerate test data"
    assert torch.equal(on.state, off.state), "the switch must not change the run state"
    graphed = E.EvalStep(m, maxdisp=64, graph=True, error_images=True)
    graphed.step(L, R, gt)
    assert torch.equal(graphed.last["error_image"], img) and torch.equal(graphed.state, off.state)


# ---- KittiInferenceColor ---------------------------------------------------------------------------------------------------------
def test_kitti_inference_color(monkeypatch):
    from test_gpu_eval import seeded_model
    from dcanet_amd.inference import KittiInference, KittiInferenceColor, KittiInferenceLR
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    m = seeded_model()
    kw = dict(crop_height=32, crop_width=64, graph=False, device_io=True)
    rng = np.random.default_rng(17)
    h, w = 28, 50                                                 # smaller than the frame: the window starts at row 4
    pairs = [(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), rng.integers(0, 256, (h, w, 3), dtype=np.uint8)) for _ in range(3)]
    plain, color = KittiInference(m, **kw), KittiInferenceColor(m, **kw)
    assert color.max_disp == 64.0
    singles = []
    for left, right in pairs:
        d0 = plain(left, right)
        d, rgb = color(left, right)
        assert d.dtype == np.float32 and d.shape == (h, w) and d.tobytes() == d0.tobytes()
        assert rgb.dtype == np.uint8 and rgb.shape == (h, w, 3)
        assert np.array_equal(rgb, REF.colorize(d0, 0, h, w, 0.0, 64.0, "kitti")) and rgb.any()
        singles.append((d, rgb))
    streamed = list(color.stream(pairs))
    assert len(streamed) == 3
    for (d, rgb), (sd, srgb) in zip(singles, streamed):
        assert d.tobytes() == sd.tobytes() and rgb.tobytes() == srgb.tobytes()
    assert singles[0][1].tobytes() != singles[1][1].tobytes()
    left, right = pairs[0]
    d0 = singles[0][0]
    # every frame ranged over its own valid pixels, on the device
    d, rgb = KittiInferenceColor(m, cmap="gray", max_disp="auto", **kw)(left, right)
    lo, hi = REF.disp_range(d0[None])[0]
    assert d.tobytes() == d0.tobytes() and np.array_equal(rgb, REF.colorize(d0, 0, h, w, lo, hi, "gray"))
    assert rgb.min() == 0 and rgb.max() == 255
    # the left-right check as the mask: the UNFILLED disparity, invalid pixels black
    _, valid = KittiInferenceLR(m, tau=1.0, **kw)(left, right)
    d, rgb = KittiInferenceColor(m, mask="lr", tau=1.0, **kw)(left, right)
    assert d.tobytes() == d0.tobytes() and 0 < (valid == 0).mean() < 1
    assert not rgb[valid == 0].any() and np.array_equal(rgb, REF.colorize(d0, 0, h, w, 0.0, 64.0, "kitti", valid, 0.5))
