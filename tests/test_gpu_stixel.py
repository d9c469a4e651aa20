"""Stixels on the MI355X (csrc/stixel.hip): `ops.stixels` bit for bit against the numpy restatement of dcanet_amd/stixel.py on
the cases of tests/_stixel_cases.py, a second call on the same buffers, selective outputs, the workspace under hipGraph replay
behind `ops.ground_plane`, the operator's refusals, and the way through inference.KittiInferenceStixels.

Why bitwise, without any tolerance: the cells' medians are order statistics of integers, the energy is integer arithmetic
(no atomic of any kind: one wave per column, minima of packed keys), and the one fp32 formula -- the road's disparity at a
cell's centre -- is rounded one operation at a time in numpy and in the kernel alike; seg_disp is one exact fp32 division by 16."""
import numpy as np
import pytest
import torch

import _ground_cases as GC
import _stixel_cases as C
from _inference_cases import lr_tau as _lr_tau, model as _model, pairs as _pairs
from dcanet_amd import ground as G
from dcanet_amd import stixel as S

pytestmark = pytest.mark.gpu
DEV = "cuda"


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)         # (a copy: the cases are read-only)


def same_bits(got, want, name):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
    bits = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize] if got.dtype.kind == "f" else got.dtype
    bad = np.nonzero(got.view(bits) != want.view(bits))
    assert len(bad[0]) == 0, f"{name}: {len(bad[0])} elements differ, first at {[int(i[0]) for i in bad]}: " \
                             f"{got[bad][0]!r} != {want[bad][0]!r}"


_REF = {}


def _ref(case):
    """the restatement of a case, computed once for the module and never modified"""
    if case.name not in _REF:
        _REF[case.name] = S.stixels_host(case.d, case.plane, mask=case.mask, **case.kw)
    return _REF[case.name]


@pytest.mark.parametrize("case", C.cases(), ids=lambda c: c.name)
def test_stixels_are_the_restatement_bit_for_bit(case):
    from dcanet_amd import ops
    ref = _ref(case)
    d, plane, mask = dev(case.d), dev(case.plane), dev(case.mask)
    got = ops.stixels(d, plane, mask=mask, **case.kw)
    assert tuple(got) == S.STIXEL_OUTPUTS
    print(case.name, "cells", ref["cells"].shape[-3:-1], "segments per column", ref["count"].reshape(-1).tolist()[:12],
          "classes", np.bincount(ref["seg_class"].ravel(), minlength=3)[:3].tolist())
    for k in S.STIXEL_OUTPUTS:
        same_bits(got[k], ref[k], k)
    # a second call on the same buffers, poisoned in between; without `cells` the pair (q, g) goes through a workspace of garbage
    for t in got.values():
        t.fill_(77)
    ws = ops.stixel_workspace(*case.d.shape[-2:], DEV, case.kw["width"], case.kw.get("row_step", 1), batch=max(1, case.d.size // (case.d.shape[-1] * case.d.shape[-2])))
    ws.fill_(-3)
    names = S.STIXEL_OUTPUTS[1:]
    again = ops.stixels(d, plane, mask=mask, outputs=names, out={k: got[k] for k in names}, workspace=ws, **case.kw)
    assert set(again) == set(names) and all(again[k] is got[k] for k in names)
    for k in names:
        same_bits(again[k], ref[k], k + " (second call, through the workspace)")
    assert bool((got["cells"] == 77).all()), "cells was not asked for"
    win = case.kw.get("window")
    rows, cols = (win[1], win[2]) if win else case.d.shape[-2:]
    H, CS = ref["cells"].shape[-3:-1]
    same_bits(ws.view(-1)[:ref["cells"].size].view(ref["cells"].shape), ref["cells"], "the workspace holds the cells")
    assert (H, CS) == (rows // case.kw.get("row_step", 1), cols // case.kw["width"])


def test_stixels_selective_outputs_write_only_those():
    from dcanet_amd import ops
    case = C.cases()[1]
    ref = _ref(case)
    d, plane = dev(case.d), dev(case.plane)
    poison = {k: torch.full(ref[k].shape, 9, device=DEV, dtype=S._STIXEL_KINDS[k]) for k in S.STIXEL_OUTPUTS}
    got = ops.stixels(d, plane, outputs=("count",), out=poison, **case.kw)
    assert set(got) == {"count"} and got["count"] is poison["count"]
    same_bits(got["count"], ref["count"], "count only")
    assert all(bool((poison[k] == 9).all()) for k in S.STIXEL_OUTPUTS if k != "count"), "the others stay poisoned"
    got = ops.stixels(d, plane, outputs=("cells",), out={"cells": poison["cells"]}, **case.kw)
    assert set(got) == {"cells"}
    same_bits(got["cells"], ref["cells"], "cells only: one launch")
    assert all(bool((poison[k] == 9).all()) for k in ("seg_class", "seg_disp", "stixels", "energy"))
    got = ops.stixels(d, plane, outputs=("energy", "seg_disp"), **case.kw)
    assert set(got) == {"energy", "seg_disp"}
    same_bits(got["energy"], ref["energy"], "energy"), same_bits(got["seg_disp"], ref["seg_disp"], "seg_disp")


def test_stixels_under_graph_replay_behind_the_plane_fit():
    """`out=` and `workspace=`: nothing is allocated, so the launches of `ops.ground_plane` and `ops.stixels` are captured on
    one stream and replayed on inputs copied into the static buffer -- a scene, an all-wall frame (status 1: count 0), another
    scene, the first again.  The stixel workspace starts as garbage; what a replay leaves anywhere must not reach the next."""
    from dcanet_amd import ops
    case = GC.cases()[0]
    H, W = case.d.shape
    inputs = [case.d, np.full((H, W), 10.0, np.float32), GC._scene_a(5).d]
    kw = dict(max_disp=32, calib=case.calib, min_rise=4, min_votes=1000)
    skw = dict(max_disp=32, width=5, max_segments=6)
    static = torch.empty((H, W), device=DEV)
    ws = ops.ground_workspace(H, W, 32, DEV)
    ws.fill_(123)
    sws = ops.stixel_workspace(H, W, DEV, 5, 1)
    sws.fill_(-12345)
    out_p = {"plane": torch.full((G.PLANE_LEN,), 9.0, device=DEV, dtype=torch.float64),
             "vdisp": torch.full((H, 32), 77, device=DEV, dtype=torch.int32)}
    names = S.STIXEL_OUTPUTS[1:]
    shapes = {"seg_class": (H, W // 5), "seg_disp": (H, W // 5), "count": (W // 5,), "stixels": (W // 5, 6, 4), "energy": (W // 5,)}
    out_s = {k: torch.full(shapes[k], 9, device=DEV, dtype=S._STIXEL_KINDS[k]) for k in names}

    def run():
        p = ops.ground_plane(static, workspace=ws, out=out_p, **kw)
        return p, ops.stixels(static, p["plane"], outputs=names, out=out_s, workspace=sws, **skw)

    static.copy_(dev(inputs[2]))
    run()                                                # warm-up, outside the capture, on the same stream
    torch.cuda.synchronize()
    sws.fill_(-12345)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        p, s = run()
    assert all(p[k] is out_p[k] for k in out_p) and all(s[k] is out_s[k] for k in out_s)
    counts = []
    for d in inputs + inputs[:1]:
        static.copy_(dev(d))
        graph.replay()
        torch.cuda.synchronize()
        ref = G.ground_plane_host(d, **kw)
        ref_s = S.stixels_host(d, ref["plane"], **skw)
        counts.append(int(ref_s["count"].max()))
        same_bits(out_p["plane"], ref["plane"], "replay plane")
        for k in names:
            same_bits(out_s[k], ref_s[k], "replay " + k)
        same_bits(sws.view(ref_s["cells"].shape), ref_s["cells"], "replay cells")
    assert counts[1] == 0 and min(counts[0], counts[2], counts[3]) >= 2 and counts[0] == counts[3]


def test_stixels_refuse_what_they_cannot_do():
    from dcanet_amd import ops
    a = torch.full((2, 1, 48, 80), 5.0, device=DEV)
    plane = torch.zeros((2, 1, 16), device=DEV, dtype=torch.float64)
    nan = float("nan")
    for bad in (dict(max_disp=7), dict(max_disp=1025), dict(width=0), dict(width=17), dict(row_step=9), dict(row_step=25),
                dict(min_valid=0), dict(min_valid=6), dict(max_segments=0), dict(max_segments=65), dict(min_disp=-1.0), dict(min_disp=nan),
                dict(params=dict(Tg=-1)), dict(params=dict(T=((0, 0), (0, 0)))), dict(params=dict(nope=1)), dict(window=(0, 49, 80)),
                dict(window=(0, 1, 80)), dict(window=(0, 48, 4)), dict(mask=a[:1]), dict(mask=a, mask_min=nan), dict(outputs=("nope",)),
                dict(outputs=()), dict(plane=plane[0]), dict(plane=plane.float()), dict(plane=plane.cpu()),
                dict(out={"count": torch.empty((2, 1, 15), device=DEV, dtype=torch.int32)}), dict(out={"nope": a}),
                dict(out={"energy": torch.empty((2, 1, 16), device=DEV, dtype=torch.int32)}),
                dict(outputs=("count",), workspace=torch.empty(100, device=DEV, dtype=torch.int16)),
                dict(outputs=("count",), workspace=torch.empty((2, 48, 16, 2), device=DEV, dtype=torch.int32))):
        kw = {**dict(plane=plane, max_disp=32), **bad}
        with pytest.raises(RuntimeError, match="stixels"):
            ops.stixels(a, kw.pop("plane"), **kw)
    for t in (a.double(), a[..., ::2], a.expand(2, 3, 48, 80).contiguous(), a.clone().requires_grad_()):
        with pytest.raises(RuntimeError, match="stixels"):
            ops.stixels(t, plane, 32)
    with torch.no_grad():
        r = ops.stixels(a.clone().requires_grad_(), plane, 32)
    assert r["count"].shape == (2, 1, 16) and r["stixels"].shape == (2, 1, 16, 16, 4) and int(r["count"].abs().sum()) == 0


# ---- through the wrapper ----------------------------------------------------------------------------------------------------
WRAP = dict(crop_height=32, crop_width=64, graph=False)
STAGE = dict(plane=dict(min_votes=4, min_inliers=8), stixel=dict(min_valid=2))
GRID = dict(width=4, row_step=2, max_segments=5)


@pytest.mark.parametrize("mode,post", [(None, False), ("lr", False), (None, True), ("lr", True)])
def test_kitti_inference_stixels(mode, post, monkeypatch):
    """a full-frame image and a 28 x 50 one in the 32 x 64 frame: the record is ops.ground_plane and ops.stixels of the disparity
    (and the mask) that the EXISTING classes hand out for the frame -- after ops.median_filter and ops.speckle_filter with
    `median=` / `speckle=` -- in ONE read-back per frame of exactly the record's bytes; stream() gives the same bytes"""
    from dcanet_amd import ops
    from dcanet_amd.geometry import StereoCalib
    from dcanet_amd.inference import FrameStixels, KittiInference, KittiInferenceLR, KittiInferenceStixels
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    model = _model()
    calib = StereoCalib(40.0, 0.5, 31.5, 15.5)
    pairs = _pairs(np.random.default_rng(37), [(32, 64), (28, 50)])
    plain = KittiInference(model, device_io=True, **WRAP)
    tau = 1.0
    if mode == "lr":
        tau = _lr_tau(plain, *pairs[0])
        lr = KittiInferenceLR(model, tau=tau, device_io=True, **WRAP)
        own = [(plain(l, r), lr(l, r)[1]) for l, r in pairs]                 # the UNFILLED disparity, the check's validity
    else:
        own = [(plain(l, r), None) for l, r in pairs]
    speckle = (6, 1.0) if post else None
    infer = KittiInferenceStixels(model, calib, mask=mode, tau=tau, speckle=speckle, median=3 if post else 0, **GRID, **STAGE, **WRAP)
    assert infer._rest.__func__ is KittiInference._rest, "nothing follows the record"
    copies = []
    readback = infer._readback
    monkeypatch.setattr(infer, "_readback", lambda s, copy: (copies.append(s.out_bytes), readback(s, copy))[1])
    single = []
    for i, ((l, r), (disp, mask)) in enumerate(zip(pairs, own)):
        h, w = l.shape[:2]
        d, m = dev(disp), dev(mask)
        if post:
            d = ops.median_filter(d, 3, mask=m)
            f = ops.speckle_filter(d, *speckle, mask=m)
            d, m = f["disp"], f["valid"] if m is None else m * f["valid"]
        p = ops.ground_plane(d, model.maxdisp, calib, mask=m, **STAGE["plane"])
        s = ops.stixels(d, p["plane"], model.maxdisp, mask=m, **GRID, **STAGE["stixel"])
        before = len(copies)
        got = infer(l, r)
        assert len(copies) == before + 1, "one read-back per frame"
        single.append(got)
        CS = w // 4
        assert isinstance(got, FrameStixels) and got.disp.shape == (h, w) and got.stixels.shape == (CS, 5, 4) and got.count.shape == (CS,)
        print(f"mode={mode} post={post} image {h}x{w}: status {int(got.plane[5])}, segments per column {got.count.tolist()}")
        assert got.disp.tobytes() == d.cpu().numpy().tobytes(), f"image {i}: the disparity the stage read"
        assert got.plane.dtype == np.float64 and got.plane.tobytes() == p["plane"].cpu().numpy().tobytes(), f"image {i}: plane"
        for k in ("count", "stixels", "energy"):
            assert getattr(got, k).dtype == s[k].cpu().numpy().dtype and getattr(got, k).tobytes() == s[k].cpu().numpy().tobytes(), (i, k)
        assert copies[-1] == 128 + 8 * CS + 4 * h * w + 4 * CS + 4 * CS * 5 * 4, "the record's bytes, no more"
    streamed = list(infer.stream(iter(pairs + pairs[:1]), depth=2))
    assert len(streamed) == 3
    for a, b in zip(streamed, single + single[:1]):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
