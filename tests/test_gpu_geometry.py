"""Geometry from calibrated disparity on the MI355X (csrc/geometry.hip): `ops.disp_to_depth` and `ops.point_cloud` bit for
bit against the numpy float32 restatement of include/dca_hip.h in tests/_geometry_reference.py -- records, their ORDER,
`count`, `tile_offsets` and both depth outputs -- and the way through inference.KittiInference3D.

Why bitwise: every operation of the formulas is one IEEE fp32 operation rounded on its own, in numpy's float32 arithmetic
and in the kernels alike (no contraction, IEEE division); the compaction is integer arithmetic.  tests/test_geometry_cpu.py
checks that the scene populates every rejection category and both kept classes on every shape used here."""
import numpy as np
import pytest
import torch

from _geometry_reference import (CALIB, MASK_MIN, MAX_DEPTH, MIN_DISP, SHAPES, TILE, V0, VERTEX, Y0, Calib,
                                 geometry_reference, scene)
from _inference_cases import lr_tau as _lr_tau, model as _model, pairs as _pairs

pytestmark = pytest.mark.gpu
DEV = "cuda"
FILTERS = dict(mask_min=MASK_MIN, min_disp=MIN_DISP, max_depth=MAX_DEPTH)
SENTINEL = 0x5A


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def records(vertices, n):
    """the first n rows of the (cap,4) float32 tensor as VERTEX records"""
    return vertices[:n].cpu().numpy().view(VERTEX).reshape(-1)


def same_records(got, want, name):
    assert got.shape == want.shape, f"{name}: {got.shape[0]} records, expected {want.shape[0]}"
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    bad = np.nonzero((got.view(np.uint32).reshape(-1, 4) != want.view(np.uint32).reshape(-1, 4)).any(1))[0]
    assert len(bad) == 0, f"{name}: {len(bad)} records differ, first at {int(bad[0])}: {got[bad[0]]} != {want[bad[0]]}"


def same_map(got, want, name):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype, name
    bad = np.nonzero(got.view(np.uint8) != want.view(np.uint8))
    assert len(bad[0]) == 0, f"{name}: differs first at {[int(i[0]) for i in bad]}"


def run_cloud(pred, mask, rgb, window, stride=1, v0=V0, calib=CALIB, **kw):
    from dcanet_amd import ops
    vert, count, offs = ops.point_cloud(dev(pred), calib, dev(rgb), dev(mask), window, v0=v0, stride=stride,
                                        **{**FILTERS, **kw})
    return vert, count.cpu().numpy(), offs.cpu().numpy()


def check_cloud(pred, mask, rgb, window, stride, name):
    ref = geometry_reference(pred, CALIB, window, V0, stride, mask, rgb=rgb)
    vert, count, offs = run_cloud(pred, mask, rgb, window, stride)
    worst = -(-window[1] // stride) * -(-window[2] // stride)
    assert tuple(vert.shape) == (worst, 4) and vert.dtype == torch.float32, name
    assert count.dtype == np.int64 and count.tolist() == [ref["count"], ref["count"]], (name, count, ref["count"])
    assert offs.dtype == np.int32 and np.array_equal(offs, ref["tile_offsets"]), name
    same_records(records(vert, int(count[1])), ref["vertices"], name)
    return ref


_SCENES = {}


def _scene(rows, cols, channels):
    """the scene of a shape, computed once for the module and never modified"""
    if (rows, cols, channels) not in _SCENES:
        _SCENES[rows, cols, channels] = scene(rows, cols, channels=channels)
    return _SCENES[rows, cols, channels]


@pytest.mark.parametrize("shape", SHAPES)
def test_point_cloud_and_depth_are_the_restatement_bit_for_bit(shape):
    """a window at frame row Y0 > 0 / image row V0 > 0 of a larger frame; stride 1, 2, 3; mask given and NULL; rgb NULL,
    C = 3, C = 4"""
    from dcanet_amd import ops
    rows, cols = shape
    window = (Y0, rows, cols)
    for channels in (None, 3, 4):
        pred, mask, rgb = _scene(rows, cols, channels or 3)
        rgb = rgb if channels else None
        for use_mask in (True, False):
            m = mask if use_mask else None
            for stride in (1, 2, 3):
                ref = check_cloud(pred, m, rgb, window, stride, f"{shape} C={channels} mask={use_mask} stride={stride}")
            if channels == 3:
                print(shape, "mask" if use_mask else "no mask", ref["reasons"])
                f32, u16 = ops.disp_to_depth(dev(pred), CALIB, window, dev(m), f32=True, u16=True, **FILTERS)
                same_map(f32, ref["depth"], f"{shape} depth")                        # (ref: stride 3; the depth ignores it)
                same_map(u16, ref["depth_u16"], f"{shape} depth uint16")
                only_f, none = ops.disp_to_depth(dev(pred), CALIB, window, dev(m), **FILTERS)
                assert none is None and torch.equal(only_f, f32)
                none, only_u = ops.disp_to_depth(dev(pred), CALIB, window, dev(m), f32=False, u16=True, **FILTERS)
                assert none is None and torch.equal(only_u, u16)
    # the (1,1,Hc,Wc) form of a network output is the same frame
    pred, mask, rgb = _scene(rows, cols, 3)
    want = geometry_reference(pred, CALIB, window, V0, 1, mask, rgb=rgb)
    vert, count, _ = run_cloud(pred[None, None], mask[None, None], rgb, window)
    same_records(records(vert, int(count[1])), want["vertices"], f"{shape} (1,1,Hc,Wc)")


@pytest.mark.parametrize("kept", ["all", "scene"])
def test_point_cloud_scan_carry(kept):
    """1100 x 1000: 1075 tiles, more than the scan workgroup has threads -- the carry between its steps"""
    rows, cols = 1100, 1000
    assert -(-rows * cols // TILE) > 1024
    pred, mask, rgb = _scene(rows, cols, 3)
    if kept == "all":
        pred, mask = np.full_like(pred, 16.0), None
    window = (Y0, rows, cols)
    ref = geometry_reference(pred, CALIB, window, V0, 1, mask, rgb=rgb)
    vert, count, offs = run_cloud(pred, mask, rgb, window)
    want = rows * cols if kept == "all" else rows * cols // 4
    assert ref["count"] == want and count.tolist() == [want, want]
    assert np.array_equal(offs, ref["tile_offsets"])
    same_records(records(vert, want)[-100:], ref["vertices"][-100:], f"carry {kept}: the last 100 records")
    same_records(records(vert, want)[::997], ref["vertices"][::997], f"carry {kept}: every 997th record")


def test_point_cloud_capacity_and_reproducibility():
    from dcanet_amd import ops
    rows, cols = 9, 1301
    pred, mask, rgb = _scene(rows, cols, 3)
    window = (Y0, rows, cols)
    ref = geometry_reference(pred, CALIB, window, V0, 1, mask, rgb=rgb)
    total = ref["count"]
    assert total > 2 * TILE
    p, m, c = dev(pred), dev(mask), dev(rgb)
    for cap in (total, total - 1, 1, 0):
        buf = torch.full((total + 4, 4), 0, device=DEV, dtype=torch.float32)
        buf.view(torch.uint8).fill_(SENTINEL)
        vert, count, offs = ops.point_cloud(p, CALIB, c, m, window, v0=V0, cap=cap, out=buf, **FILTERS)
        assert tuple(vert.shape) == (cap, 4) and (cap == 0 or vert.data_ptr() == buf.data_ptr())
        assert count.cpu().tolist() == [total, min(total, cap)], cap
        assert np.array_equal(offs.cpu().numpy(), ref["tile_offsets"])                # the offsets do not depend on cap
        same_records(records(buf, cap), ref["vertices"][:cap], f"cap={cap}")
        assert (buf[cap:].view(torch.uint8) == SENTINEL).all(), f"cap={cap}: written at or beyond record cap"
        if cap == 0:
            _, count0, _ = ops.point_cloud(p, CALIB, c, m, window, v0=V0, cap=0, **FILTERS)      # no buffer at all
            assert count0.cpu().tolist() == [total, 0]
    # a buffer smaller than the worst case bounds cap by itself
    small = torch.empty((7, 4), device=DEV)
    vert, count, _ = ops.point_cloud(p, CALIB, c, m, window, v0=V0, out=small, **FILTERS)
    assert tuple(vert.shape) == (7, 4) and count.cpu().tolist() == [total, 7]
    same_records(records(vert, 7), ref["vertices"][:7], "out of 7 records")
    # two calls, identical bytes -- records, count, offsets
    a = ops.point_cloud(p, CALIB, c, m, window, v0=V0, **FILTERS)
    b = ops.point_cloud(p, CALIB, c, m, window, v0=V0, **FILTERS)
    n = int(a[1][1])
    for x, y in zip((a[0][:n], a[1], a[2]), (b[0][:n], b[1], b[2])):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()


def test_point_cloud_degenerate_inputs():
    from dcanet_amd import ops
    rows, cols = 5, 67
    _, _, rgb = _scene(rows, cols, 3)
    window = (Y0, rows, cols)
    shape = (rows + Y0 + 2, cols + 3)
    for name, fill, want in (("all rejected", 0.25, 0), ("a frame of NaN", np.nan, 0), ("all kept", 16.0, rows * cols)):
        pred = np.full(shape, fill, np.float32)
        ref = geometry_reference(pred, CALIB, window, V0, 1, None, rgb=rgb)
        assert ref["count"] == want
        vert, count, offs = run_cloud(pred, None, rgb, window)
        assert count.tolist() == [want, want], name
        assert np.array_equal(offs, ref["tile_offsets"]) and offs[-1] == want
        same_records(records(vert, want), ref["vertices"], name)
        f32, u16 = ops.disp_to_depth(dev(pred), CALIB, window, f32=True, u16=True, **FILTERS)
        same_map(f32, ref["depth"], name)
        same_map(u16, ref["depth_u16"], name)
        assert (f32 > 0).sum().item() == want


def test_depth_uint16_truncates_and_saturates():
    """uint16(Z * scale): fp32 product, truncated toward zero, saturated at 65535, rejected -> 0"""
    from dcanet_amd import ops
    calib = Calib(100.0, 64.0, 0.0, 0.0, 0.0)
    # Z = 64 / d:  0.25   32.5   255.99.. (65534.9 / 256)   256   1024 == max_depth   then rejected: d < min_disp, NaN, Z > max_depth
    d = np.array([[256.0, 64.0 / 32.5, 0.250004, 0.25, 0.0625, 0.005, np.nan, 0.03125]], np.float32)
    kw = dict(min_disp=0.01, max_depth=1024.0, mask_min=0.5)
    ref = geometry_reference(d, calib, None, 0, 1, None, **kw, scale=256.0)
    f32, u16 = ops.disp_to_depth(dev(d), calib, f32=True, u16=True, scale=256.0, **kw)
    same_map(f32, ref["depth"], "depth")
    same_map(u16, ref["depth_u16"], "depth uint16")
    got = u16.cpu().numpy()[0].tolist()
    assert got[0] == 64 and got[3] == 65535 and got[4] == 65535 and got[5:] == [0, 0, 0]
    assert got[1] == int(np.trunc(ref["depth"][0, 1] * np.float32(256))) and got[2] == 65534          # not rounded up
    # another scale; a fractional product is truncated, not rounded
    ref = geometry_reference(d, calib, None, 0, 1, None, **kw, scale=3.0)
    _, u16 = ops.disp_to_depth(dev(d), calib, f32=False, u16=True, scale=3.0, **kw)
    same_map(u16, ref["depth_u16"], "depth uint16, scale 3")
    assert u16.cpu().numpy()[0, :2].tolist() == [0, 97]                             # 0.75 -> 0; 97.5 -> 97


def test_geometry_operators_refuse_what_they_cannot_do():
    from dcanet_amd import ops
    pred, mask = torch.ones(8, 16, device=DEV), torch.ones(8, 16, device=DEV)
    rgb = torch.zeros(8, 16, 3, device=DEV, dtype=torch.uint8)
    for op in (ops.disp_to_depth, ops.point_cloud):
        assert op(pred, CALIB, mask=mask, **FILTERS) is not None
        for bad in (dict(min_disp=-1.0), dict(min_disp=float("inf")), dict(max_depth=0.0), dict(max_depth=float("nan")),
                    dict(mask_min=float("nan")), dict(window=(0, 9, 16)), dict(window=(1, 8, 16)), dict(window=(0, 8, 17)),
                    dict(window=(-1, 4, 4)), dict(window=(0, 0, 4)), dict(mask=mask[:4]), dict(mask=mask.double()),
                    dict(mask=mask.cpu()), dict(mask=mask.t()), dict(mask=mask.clone().requires_grad_())):
            with pytest.raises(RuntimeError):
                op(pred, CALIB, **{**dict(mask=mask), **FILTERS, **bad})
        for bad_pred in (pred.cpu(), pred.double(), pred.t(), pred.clone().requires_grad_(), pred.expand(2, 8, 16).contiguous()):
            with pytest.raises(RuntimeError):
                op(bad_pred, CALIB, **FILTERS)
        for bad_calib in (Calib(0.0, 64.0, 0.0, 0.0, 0.0), Calib(100.0, float("inf"), 0.0, 0.0, 0.0),
                          Calib(100.0, 64.0, float("nan"), 0.0, 0.0), Calib(100.0, -64.0, 0.0, 0.0, 0.0), None):
            with pytest.raises(RuntimeError):
                op(pred, bad_calib, **FILTERS)
        with torch.no_grad():
            assert op(pred.clone().requires_grad_(), CALIB, **FILTERS) is not None
    for bad in (dict(f32=False, u16=False), dict(u16=True, scale=0.0), dict(out_f32=torch.empty(8, 15, device=DEV)),
                dict(u16=True, out_u16=torch.empty(8, 16, device=DEV, dtype=torch.int16))):
        with pytest.raises(RuntimeError):
            ops.disp_to_depth(pred, CALIB, **bad)
    big = torch.empty(129, 4, device=DEV)
    for bad in (dict(stride=0), dict(v0=-1), dict(cap=-1), dict(rgb=rgb.cpu()), dict(rgb=rgb[..., :2].contiguous()),
                dict(rgb=rgb.float()), dict(rgb=rgb[:, :15].contiguous()), dict(rgb=rgb, v0=1),
                dict(out=torch.empty(128, 3, device=DEV)), dict(out=torch.empty(128, 4, device=DEV, dtype=torch.float64)),
                dict(out=big.view(-1)[1:513].view(128, 4)), dict(out=big, cap=130),
                dict(workspace=(torch.empty(1, device=DEV, dtype=torch.int32), torch.empty(2, device=DEV, dtype=torch.int64))),
                dict(workspace=(torch.empty(2, device=DEV, dtype=torch.int64), torch.empty(2, device=DEV, dtype=torch.int64))),
                dict(workspace=(torch.empty(2, device=DEV, dtype=torch.int32), torch.empty(2, device=DEV, dtype=torch.int32)))):
        with pytest.raises(RuntimeError):
            ops.point_cloud(pred, CALIB, **bad)


def test_geometry_replays_from_a_hipgraph():
    """with out= and workspace= nothing is allocated and the host never waits: both operators captured as ONE linear chain
    on a side stream, replayed twice with changed inputs, equal eager"""
    from dcanet_amd import ops
    rows, cols = 9, 1301
    window = (Y0, rows, cols)
    scenes = [_scene(rows, cols, 3)]
    for k in (1, 2):                                    # changed inputs: the scene shifted along the window, other colours
        p, m, c = (a.copy() for a in scenes[0])
        p[Y0:Y0 + rows, :cols] = np.roll(p[Y0:Y0 + rows, :cols].reshape(-1), 3 * k).reshape(rows, cols)
        m[Y0:Y0 + rows, :cols] = np.roll(m[Y0:Y0 + rows, :cols].reshape(-1), 3 * k).reshape(rows, cols)
        scenes.append((p, m, (c + 40 * k).astype(np.uint8)))
    P, M, C = (dev(a).clone() for a in scenes[0])
    vert = torch.empty((rows * cols, 4), device=DEV)
    ws = ops.point_cloud_workspace(rows, cols, DEV)
    of, ou = torch.empty((rows, cols), device=DEV), torch.empty((rows, cols), device=DEV, dtype=torch.uint16)

    def run():
        ops.disp_to_depth(P, CALIB, window, M, f32=True, u16=True, out_f32=of, out_u16=ou, **FILTERS)
        return ops.point_cloud(P, CALIB, C, M, window, v0=V0, out=vert, workspace=ws, **FILTERS)

    run()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        v_g, count_g, offs_g = run()
    assert v_g.data_ptr() == vert.data_ptr() and count_g.data_ptr() == ws[1].data_ptr()
    counts = []
    for p, m, c in scenes[1:]:
        P.copy_(dev(p)), M.copy_(dev(m)), C.copy_(dev(c))
        for t in (vert, of):
            t.fill_(-1.0)
        g.replay()
        got = [t.clone() for t in (vert, ws[1], offs_g, of, ou)]
        n = int(got[1][1])
        ref = geometry_reference(p, CALIB, window, V0, 1, m, rgb=c)
        same_records(records(got[0], n), ref["vertices"], "replay")
        assert got[1].cpu().tolist() == [ref["count"]] * 2
        vert.fill_(-1.0)
        run()
        for a, b in zip(got, (vert, ws[1], offs_g, of, ou)):
            assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
        counts.append(got[0].cpu().numpy().tobytes())
    assert counts[0] != counts[1]       # the inputs did change what the graph computed


# ---- through the wrapper ---------------------------------------------------------------------------------------------------
WRAP_CALIB = Calib(40.0, float(np.float32(40.0 * 0.5)), 31.5, 15.5, 0.0)
WRAP = dict(crop_height=32, crop_width=64, graph=True, device_io=True)


@pytest.mark.parametrize("mode", [None, "confidence", "lr"])
def test_kitti_inference_3d(mode, monkeypatch):
    """a full-frame image and a 28 x 50 one in the 32 x 64 frame.  The network's output is not exact, so the want is the
    float32 restatement applied to the disparity and the mask that the EXISTING class of that mode hands out; mask_min is the
    median of the mask inside the window.  Afterwards the three existing classes give what they gave before."""
    from dcanet_amd.geometry import PLY_VERTEX
    from dcanet_amd.inference import (Frame3D, KittiInference, KittiInference3D, KittiInferenceLR,
                                      KittiInferenceWithConfidence)
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    model = _model()
    pairs = _pairs(np.random.default_rng(17), [(32, 64), (28, 50)])
    plain, conf = KittiInference(model, **WRAP), KittiInferenceWithConfidence(model, **WRAP)
    tau = _lr_tau(plain, *pairs[0]) if mode == "lr" else 1.0
    lr = KittiInferenceLR(model, tau=tau, **WRAP)
    before = [(plain(l, r), conf(l, r), lr(l, r)) for l, r in pairs]
    # the disparity and the mask of the mode, from the existing classes
    own = [(b[0], None) if mode is None else b[1] if mode == "confidence" else (b[0], b[2][1]) for b in before]
    mask_min = 0.5 if mode is None else float(np.median(own[0][1]))
    kw = dict(mask_min=mask_min, min_disp=0.25, max_depth=60.0)
    if mode is None:             # no mask to split the pixels: the depth of the median disparity does
        kw["max_depth"] = float(np.float32(WRAP_CALIB.fb) / np.float32(np.median(own[0][0])))
    infer = KittiInference3D(model, WRAP_CALIB, mask=mode, tau=tau, **kw, **WRAP)
    for i, ((l, r), (disp, mask)) in enumerate(zip(pairs, own)):
        h, w = l.shape[:2]
        ref = geometry_reference(disp, WRAP_CALIB, None, 0, 1, mask, rgb=l, **kw)
        got = infer(l, r)
        assert isinstance(got, Frame3D) and got.disp.shape == got.depth.shape == (h, w)
        assert got.disp.tobytes() == np.ascontiguousarray(disp).tobytes(), f"image {i}: not the class's own disparity"
        if mode is None:
            assert got.mask is None
        else:
            assert got.mask.tobytes() == np.ascontiguousarray(mask).tobytes(), f"image {i}: not the class's own mask"
        print(f"mode={mode} image {h}x{w} mask_min={mask_min:.4f} tau={tau:.4f}: {ref['reasons']}")
        assert got.depth.dtype == np.float32 and got.depth.tobytes() == ref["depth"].tobytes(), f"image {i}: depth"
        assert got.vertices.dtype == PLY_VERTEX and got.vertices.ndim == 1
        same_records(got.vertices, ref["vertices"], f"mode={mode} image {i}")
        rr, cc = np.nonzero(ref["keep"])
        for j, name in enumerate(("red", "green", "blue")):
            assert np.array_equal(got.vertices[name], l[rr, cc, j]), name
        if i == 0:
            assert 0 < ref["count"] < h * w, ref["reasons"]
            if mode is not None:
                assert ref["reasons"]["mask"] > 0
    for (l, r), (p0, (cd, cc), (lf, lv)) in zip(pairs, before):
        assert np.ascontiguousarray(plain(l, r)).tobytes() == np.ascontiguousarray(p0).tobytes()
        for a, b in zip(conf(l, r) + lr(l, r), (cd, cc, lf, lv)):
            assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def test_kitti_inference_3d_stream_equals_one_at_a_time_calls(monkeypatch):
    from dcanet_amd.inference import KittiInference3D
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    infer = KittiInference3D(_model(), WRAP_CALIB, mask="confidence", mask_min=0.3, min_disp=0.25, max_depth=60.0, stride=2,
                             **WRAP)
    pairs = _pairs(np.random.default_rng(19), [(28, 50), (32, 64), (28, 50), (32, 64), (30, 64)])
    single = [infer(l, r) for l, r in pairs]
    assert single[0].vertices.tobytes() != single[2].vertices.tobytes()                    # same size, different content
    assert all(len(s.vertices) > 0 for s in single)
    got = list(infer.stream(iter(pairs), depth=2))
    assert len(got) == 5
    for i, (g, s) in enumerate(zip(got, single)):
        assert type(g) is type(s) and g._fields == ("disp", "mask", "depth", "vertices")
        for a, b in zip(g, s):
            assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), f"frame {i} differs"
    again = list(infer.stream(pairs, depth=3))
    assert all(a.vertices.tobytes() == s.vertices.tobytes() for a, s in zip(again, single))


def test_kitti_inference_3d_needs_device_io():
    from dcanet_amd.inference import KittiInference3D
    for bad in (dict(device_io=False), dict()):
        with pytest.raises(ValueError):
            KittiInference3D(_model(), WRAP_CALIB, crop_height=32, crop_width=64, **bad)
