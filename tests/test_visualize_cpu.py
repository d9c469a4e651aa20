"""The picture stage (csrc/visualize.hip, dcanet_amd.utils.visualization) without a GPU: the numpy
restatement the GPU tests compare against (tests/_vis_reference.py) and the package's own host path against the REFERENCE's
recorded error maps (tests/golden/vis_error_image.npz, tools/make_vis_golden.py) bit for bit, the fp32 definition of the KITTI
colour map against the devkit formula in float64, the bindings, and the keywords of the classes that use the stage."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import _vis_reference as REF


def cases(golden):
    fx = golden("vis_error_image")
    return [(fx[f"est{i}"], fx[f"gt{i}"], fx[f"image{i}"]) for i in range(len(fx["cases"]))]


# ---- error image -------------------------------------------------------------------------------------------------------------
def test_fixture_holds_the_cases_the_kernel_can_get_wrong(golden):
    fx = golden("vis_error_image")
    assert [tuple(c[1:]) for c in fx["cases"].tolist()] == [(2, 13, 47), (1, 7, 230), (1, 12, 200)]
    for est, gt, image in cases(golden):
        assert image.dtype == np.float32 and image.shape == (gt.shape[0], 3) + gt.shape[1:]
        assert 0.2 < (gt == 0).mean() < 0.4 and (gt < 0).any()
        seen = gt > 0
        for bad in (np.isnan(est), est == np.inf, est == -np.inf):
            assert (bad & seen).any()
        with np.errstate(all="ignore"):
            e = np.abs(gt - est)
            on_edge = {float(v) for v in (e / np.float32(3))[seen & (gt <= 60)].tolist()}
            assert {2.0 ** k for k in range(-4, 5)} <= on_edge
            assert (seen & np.isfinite(e) & ((e / gt) / np.float32(0.05) < e / np.float32(3))).any()      # the relative branch
        bins = REF.error_bins(est, gt, legend=False)
        assert set(bins.ravel().tolist()) == set(range(-1, 10)), "ten of the ten bins, and black"


def test_restatements_equal_the_reference_bitwise(golden):
    from dcanet_amd.utils import disp_error_image, disp_error_image_func, error_colormap, gen_error_colormap
    from dcanet_amd.utils.visualization import _error_image_host
    assert error_colormap.dtype == np.float32 and error_colormap.shape == (10, 5)
    assert np.array_equal(error_colormap, gen_error_colormap())
    assert np.array_equal(error_colormap[:, 0], REF.ERR_EDGES[:-1]) and np.array_equal(error_colormap[:, 1], REF.ERR_EDGES[1:])
    assert np.array_equal(error_colormap[:, 2:], REF.ERR_BYTES.astype(np.float32) / np.float32(255))
    for est, gt, image in cases(golden):
        f32, u8 = REF.error_image(est, gt)
        assert f32.dtype == np.float32 and f32.tobytes() == image.tobytes()
        te, tg = torch.from_numpy(est), torch.from_numpy(gt)
        for got in (disp_error_image_func.forward(None, te, tg), disp_error_image_func()(te, tg),
                    disp_error_image_func.apply(te, tg, 3., 0.05), disp_error_image(te, tg)):
            assert torch.is_tensor(got) and got.dtype == torch.float32 and not got.is_cuda
            assert got.numpy().tobytes() == image.tobytes()
        # the uint8 form: rint(float * 255), and that is the byte table
        assert u8.dtype == np.uint8 and u8.shape == gt.shape + (3,)
        assert np.array_equal(u8, np.rint(image * np.float32(255)).astype(np.uint8).transpose(0, 2, 3, 1))
        bins = REF.error_bins(est, gt)
        assert np.array_equal(u8[bins >= 0], REF.ERR_BYTES[bins[bins >= 0]]) and not u8[bins < 0].any()
        # without the legend, other thresholds: the two restatements against each other
        for kw in (dict(legend=False), dict(abs_thres=1.0, rel_thres=0.1, legend=False)):
            want = REF.error_image(est, gt, **kw)[0]
            assert _error_image_host(est, gt, kw.get("abs_thres", 3.0), kw.get("rel_thres", 0.05), False).tobytes() == want.tobytes()
    assert disp_error_image_func().backward(None) is None
    with pytest.raises(ValueError):
        disp_error_image(torch.zeros(1, 4, 5), torch.zeros(1, 4, 6))


def test_padded_prediction_is_cropped_by_the_restatement(golden):
    est, gt, image = cases(golden)[0]
    padded = np.full((2, 16, 52), np.nan, dtype=np.float32)
    padded[:, 3:, :47] = est
    assert REF.error_image(padded, gt, top_pad=3)[0].tobytes() == image.tobytes()


# ---- KITTI map ---------------------------------------------------------------------------------------------------------------
def test_kitti_map_anchors_and_devkit_formula():
    from dcanet_amd.utils import disp_to_color
    anchors = np.array([0, .114, .299, .413, .587, .701, .886, 1], dtype=np.float32)
    got = REF.kitti_bytes(anchors).astype(np.int64)
    assert np.abs(got - 255 * REF.KITTI_CORNERS.astype(np.int64)).max() <= 1, got
    t = (np.arange(100001, dtype=np.float64) / 100000).astype(np.float32)
    a = REF.kitti_bytes(t).astype(np.int64)
    b = np.rint(REF.devkit_f64(t.astype(np.float64)) * 255).astype(np.int64)
    diff = np.abs(a - b).max(-1)
    print(f"fp32 definition vs devkit formula in float64: max {diff.max()} byte, {100 * (diff > 0).mean():.4f} % of the points differ")
    assert diff.max() <= 1 and (diff > 0).mean() <= 1e-3
    assert len({tuple(c) for c in a.tolist()}) > 1000 and (a.max(0) == 255).all() and (a.min(0) == 0).all()
    # the package's restatement (t = d / max_disp) against this one, on a map with every kind of invalid pixel
    d = (t[1:100001].reshape(250, 400) * np.float32(96)).copy()
    d[0, :4] = np.nan, np.inf, -1.0, 0.0
    d[1, :2] = 200.0, -np.inf
    for cmap in ("kitti", "gray"):
        want = REF.colorize(d, 0, 250, 400, 0.0, 64.0, cmap)
        got = disp_to_color(torch.from_numpy(d), 64.0, cmap)
        assert got.dtype == np.uint8 and got.shape == (250, 400, 3) and np.array_equal(got, want)
        assert not want[0, :4].any() and not want[1, 1].any() and want[1, 0].any()
    g = REF.gray_bytes(np.array([0, 0.5, 1], dtype=np.float32))
    assert g.tolist() == [[0, 0, 0], [128, 128, 128], [255, 255, 255]]      # rint: 127.5 -> 128 (ties to even)
    with pytest.raises(ValueError):
        disp_to_color(d, 64.0, "jet")
    with pytest.raises(ValueError):
        disp_to_color(d, 0.0)


def test_range_restatement():
    d = np.array([[[np.nan, 3.0, 0.0], [-2.0, np.inf, 7.5]], [[0.0, -1.0, np.nan], [0.0, 0.0, -np.inf]]], dtype=np.float32)
    assert REF.disp_range(d).tolist() == [[3.0, 7.5], [0.0, 0.0]]
    m = np.array([[[1, 0.4, 1], [1, 1, 0.5]]] * 2, dtype=np.float32)
    assert REF.disp_range(d, mask=m).tolist() == [[7.5, 7.5], [0.0, 0.0]]
    assert REF.disp_range(d, window=(0, 1, 2)).tolist() == [[3.0, 3.0], [0.0, 0.0]]


# ---- bindings ----------------------------------------------------------------------------------------------------------------
def test_launchers_are_bound_and_refuse_bad_arguments_without_a_device():
    from dcanet_amd import _lib
    i, f, p, lg = ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_long
    assert _lib.ABI_VERSION == 21
    assert _lib.SIGNATURES["dca_disp_error_image"] == (i, [p] * 4 + [i] * 5 + [f, f, i, p])
    assert _lib.SIGNATURES["dca_disp_range"] == (i, [p] * 4 + [i] * 6 + [f, p])
    assert _lib.SIGNATURES["dca_disp_range_workspace"] == (lg, [i] * 3)
    assert _lib.SIGNATURES["dca_disp_colorize"] == (i, [p] * 4 + [i] * 5 + [f, f, i, p])
    C = _lib.CONSTANTS
    assert [C[f"DCA_ERRMAP_RGB_{k}"] for k in range(C["DCA_ERRMAP_BINS"])] == \
        [(int(r) << 16) | (int(g) << 8) | int(b) for r, g, b in REF.ERR_BYTES]
    assert (C["DCA_ERRMAP_LEGEND_ROWS"], C["DCA_ERRMAP_LEGEND_STEP"]) == (REF.LEGEND_ROWS, REF.LEGEND_STEP)
    assert [C[f"DCA_KITTI_EDGE_{k}"] for k in range(8)] == REF.KITTI_C.astype(int).tolist()
    assert np.array_equal(np.diff(REF.KITTI_C), REF.KITTI_W)
    corners = [[(C["DCA_KITTI_CORNERS"] >> (4 * k + s)) & 1 for s in (2, 1, 0)] for k in range(8)]
    assert corners == REF.KITTI_CORNERS.astype(int).tolist()
    assert (C["DCA_CMAP_GRAY"], C["DCA_CMAP_KITTI"]) == (0, 1)
    lib = _lib.load()
    assert lib.dca_abi_version() == 21
    x = ctypes.c_void_p(4096)        # a non-NULL address that is never dereferenced: every call below is refused before a launch
    err, rng, col = lib.dca_disp_error_image, lib.dca_disp_range, lib.dca_disp_colorize
    assert err(x, x, None, None, 1, 4, 4, 0, 0, 3.0, 0.05, 1, None) != 0                  # no output
    assert err(None, x, x, x, 1, 4, 4, 0, 0, 3.0, 0.05, 1, None) != 0
    for B, H, W, tp, rp in ((0, 4, 4, 0, 0), (1, 0, 4, 0, 0), (1, 4, -1, 0, 0), (1, 4, 4, -1, 0), (1, 4, 4, 0, -1),
                            (2, 1 << 15, 1 << 15, 0, 0)):
        assert err(x, x, x, x, B, H, W, tp, rp, 3.0, 0.05, 1, None) != 0
    for a, r in ((0.0, 0.05), (3.0, -1.0), (float("nan"), 0.05), (3.0, float("inf"))):
        assert err(x, x, x, x, 1, 4, 4, 0, 0, a, r, 1, None) != 0
    assert err(x, x, x, x, 1, 4, 4, 0, 0, 3.0, 0.05, 2, None) != 0
    assert lib.dca_disp_range_workspace(0, 4, 4) == 0 and lib.dca_disp_range_workspace(1, 0, 4) == 0
    assert lib.dca_disp_range_workspace(2, 9, 37) == 2 * 8 and lib.dca_disp_range_workspace(1, 384, 1248) > 8
    assert rng(x, None, None, x, 1, 8, 8, 0, 8, 8, 0.5, None) != 0 and rng(x, None, x, None, 1, 8, 8, 0, 8, 8, 0.5, None) != 0
    for B, Hc, Wc, y0, rows, cols in ((0, 8, 8, 0, 8, 8), (1, 0, 8, 0, 8, 8), (1, 8, 8, 0, 0, 8), (1, 8, 8, 0, 8, -1),
                                      (1, 8, 8, 1, 8, 8), (1, 8, 8, 0, 8, 9), (1, 8, 8, -1, 4, 4), (70000, 8, 8, 0, 8, 8)):
        assert rng(x, None, x, x, B, Hc, Wc, y0, rows, cols, 0.5, None) != 0
    assert rng(x, x, x, x, 1, 8, 8, 0, 8, 8, float("nan"), None) != 0
    assert col(x, None, None, None, 8, 8, 0, 8, 8, 64.0, 0.5, 1, None) != 0                 # no output
    for Hc, Wc, y0, rows, cols in ((0, 8, 0, 8, 8), (8, 8, 0, 0, 8), (8, 8, 1, 8, 8), (8, 8, 0, 8, 9), (8, 8, -1, 4, 4)):
        assert col(x, None, None, x, Hc, Wc, y0, rows, cols, 64.0, 0.5, 1, None) != 0
    for max_disp in (0.0, -1.0, float("nan"), float("inf")):                               # no range and no usable scalar
        assert col(x, None, None, x, 8, 8, 0, 8, 8, max_disp, 0.5, 1, None) != 0
    assert col(x, None, None, x, 8, 8, 0, 8, 8, 64.0, 0.5, 2, None) != 0                    # no such map
    assert col(x, x, None, x, 8, 8, 0, 8, 8, 64.0, float("nan"), 1, None) != 0


def test_operators_refuse_cpu_tensors_and_bad_arguments():
    from dcanet_amd import ops
    assert ops.CMAPS == {"gray": 0, "kitti": 1}
    z = torch.zeros(1, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.disp_error_image(z, z)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.disp_range(z)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.disp_colorize(z[0], 0, 8, 8, max_disp=64.0)
    with pytest.raises(ValueError, match="cmap"):
        ops.disp_colorize(z[0], 0, 8, 8, max_disp=64.0, cmap="jet")
    sig = inspect.signature(ops.disp_error_image)
    assert [(k, v.default) for k, v in sig.parameters.items()][2:] == [
        ("abs_thres", 3.0), ("rel_thres", 0.05), ("legend", True), ("f32", True), ("u8", False), ("out_f32", None), ("out_u8", None)]
    assert list(inspect.signature(ops.disp_range).parameters) == ["disp", "window", "mask", "mask_min"]
    assert list(inspect.signature(ops.disp_colorize).parameters) == ["disp", "y0", "rows", "cols", "max_disp", "range", "cmap",
                                                                     "mask", "mask_min", "out"]


# ---- the classes that use the stage ----------------------------------------------------------------------------------------------
def test_inference_color_and_eval_step_keywords_without_a_device(tmp_path):
    from dcanet_amd.evaluation import EvalStep
    from dcanet_amd.inference import KittiInference, KittiInferenceColor, color_png
    net = torch.nn.Linear(1, 1)
    net.maxdisp = 64
    a = KittiInferenceColor(net, 64, 128, graph=False)
    assert isinstance(a, KittiInference) and a.device_io and a.nmaps == 1 and a.confidence is False
    assert (a.cmap, a.max_disp, a.mask_mode, a.mask_min) == ("kitti", 64.0, None, 0.5) and (a.crop_height, a.crop_width) == (64, 128)
    b = KittiInferenceColor(net, cmap="gray", max_disp="auto", mask="confidence", mask_min=0.7, radius=2)
    assert (b.cmap, b.max_disp, b.nmaps, b.confidence, b.radius, b.mask_min) == ("gray", "auto", 2, True, 2, 0.7)
    c = KittiInferenceColor(net, max_disp=192, mask="lr", tau=2.0, dtype=torch.float16)
    assert (c.max_disp, c.nmaps, c.confidence, c.tau, c.dtype) == (192.0, 2, False, 2.0, torch.float16)
    for bad in (dict(cmap="jet"), dict(mask="conf"), dict(max_disp=0), dict(max_disp=float("inf")), dict(max_disp="full"),
                dict(radius=-1), dict(tau=-1.0), dict(mask_min=float("nan")), dict(device_io=False)):
        with pytest.raises(ValueError):
            KittiInferenceColor(net, **bad)
    with pytest.raises(ValueError, match="max_disp"):
        KittiInferenceColor(torch.nn.Linear(1, 1))          # no `maxdisp` to fall back on
    with pytest.raises(ValueError, match="device_io"):
        KittiInferenceColor(net, 64, 128, True, None, False)
    sig = inspect.signature(EvalStep.__init__)
    assert list(sig.parameters)[1:] == ["model", "maxdisp", "graph", "dtype", "error_images"]
    assert sig.parameters["error_images"].default is False
    ev = EvalStep(net, maxdisp=64, error_images=True)      # the state is a plain zero tensor on the model's device
    assert ev.error_images is True and EvalStep(net, maxdisp=64).error_images is False and ev.last is None
    rgb = REF.kitti_bytes(np.linspace(0, 1, 35 * 20, dtype=np.float32).reshape(20, 35))
    color_png(str(tmp_path / "c.png"), rgb)
    from PIL import Image
    assert np.array_equal(np.asarray(Image.open(str(tmp_path / "c.png"))), rgb)
    with pytest.raises(ValueError):
        color_png(str(tmp_path / "d.png"), rgb.astype(np.float32))
