"""Ground plane, obstacles and free space on the MI355X (csrc/ground.hip): `ops.ground_plane` and `ops.ground_segment` bit for
bit against the numpy restatements of dcanet_amd/ground.py on the cases of tests/_ground_cases.py, the workspace and the grid
under hipGraph replay, selective outputs, the operators' refusals, and the way through inference.KittiInferenceGround.

Why bitwise, without any tolerance: the v-disparity, the votes and the ten sums are integer counts and integer sums (LDS and
integer atomics: any order gives the same number); the inlier tests and the labels are single fp32 operations rounded one
at a time in numpy and in the kernel alike; the plane is one fp64 solve over exactly representable sums in one written order
of + - x / sqrt (csrc/ground_math.h), each correctly rounded on the device and on the host."""
import numpy as np
import pytest
import torch

import _ground_cases as C
from _inference_cases import lr_tau as _lr_tau, model as _model, pairs as _pairs
from dcanet_amd import ground as G

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


def ulps(got, want):
    """distance in units of the last place between two float64 arrays of one sign pattern"""
    g, w = got.view(np.int64).astype(np.float64), want.view(np.int64).astype(np.float64)
    return np.abs(g - w)


_REF = {}


def _ref(case):
    """the restatement of a case, computed once for the module and never modified"""
    if case.name not in _REF:
        r = G.ground_plane_host(case.d, **C.plane_kwargs(case))
        _REF[case.name] = (r, G.ground_segment_host(case.d, r["plane"], case.calib, **C.segment_kwargs(case)))
    return _REF[case.name]


def _dev_kwargs(kw):
    return {k: dev(v) if k == "mask" else v for k, v in kw.items()}


@pytest.mark.parametrize("case", C.cases(), ids=lambda c: c.name)
def test_ground_plane_and_segment_are_the_restatement_bit_for_bit(case):
    from dcanet_amd import ops
    ref, ref_seg = _ref(case)
    d = dev(case.d)
    lead = case.d.shape[:-2]
    B = int(np.prod(lead, dtype=np.int64))
    ws = ops.ground_workspace(case.d.shape[-2], case.d.shape[-1], case.max_disp, DEV, batch=B)
    ws.fill_(-7)                                         # the first launch clears it
    got = ops.ground_plane(d, workspace=ws, **_dev_kwargs(C.plane_kwargs(case)))
    assert set(got) == {"plane", "vdisp"}
    plane, want = got["plane"].cpu().numpy(), ref["plane"]
    P, W = plane.reshape(B, G.PLANE_LEN), want.reshape(B, G.PLANE_LEN)
    print(case.name, "status", W[:, 5].tolist(), "line", W[:, 6:9].tolist(), "inliers", W[:, 3].tolist(), "rounds", W[:, 15].tolist())
    # (i) the integers: histogram, Hough triple, the ten sums of every round, inlier count, status, rounds
    same_bits(got["vdisp"], ref["vdisp"], "vdisp")
    assert P[:, 6:9].tolist() == W[:, 6:9].tolist(), "the Hough line and its vote"
    sums = ws.cpu().numpy().reshape(B, G.WS_LEN)[:, ops.GROUND_SUMS_AT:ops.GROUND_SUMS_AT + 10 * G.MAX_REFINE]
    same_bits(sums.reshape(lead + (G.MAX_REFINE, 10)), ref["sums"], "the ten sums")
    assert P[:, [3, 5, 13, 14, 15]].tolist() == W[:, [3, 5, 13, 14, 15]].tolist(), "inliers, status, centre, rounds"
    # (ii) the fp64 results: a, b, c, rms, hs, normal -- which field, how many ulps
    dist = ulps(P, W)
    for b, k in zip(*np.nonzero(dist)):
        print(f"  image {b} {G.PLANE_FIELDS[k]}: device {P[b, k]!r} restatement {W[b, k]!r}: {dist[b, k]:.0f} ulp")
    same_bits(plane, want, "the plane record")
    # the segmentation under the DEVICE's record
    seg = ops.ground_segment(d, got["plane"], case.calib, **_dev_kwargs(C.segment_kwargs(case)))
    assert tuple(seg) == G.SEGMENT_OUTPUTS
    for k in G.SEGMENT_OUTPUTS:
        same_bits(seg[k], ref_seg[k], k)
    # a second call: the same bits, whatever the first left in the workspace and in the grid
    again = ops.ground_plane(d, workspace=ws, **_dev_kwargs(C.plane_kwargs(case)))
    assert torch.equal(again["plane"].view(torch.int64), got["plane"].view(torch.int64)) and torch.equal(again["vdisp"], got["vdisp"])
    seg2 = ops.ground_segment(d, again["plane"], case.calib, out={"bev": seg["bev"]}, **_dev_kwargs(C.segment_kwargs(case)))
    assert seg2["bev"] is seg["bev"]
    for k in G.SEGMENT_OUTPUTS:
        same_bits(seg2[k], ref_seg[k], k + " (second call)")


def test_ground_under_graph_replay_clears_its_counts():
    """`out=` and `workspace=`: nothing is allocated, so the launches of both operators are captured on one stream (a linear
    graph) and replayed on inputs copied into the static buffer -- a scene, an all-wall frame (status 1: no sums, no grid), the
    scene again.  What a replay leaves in the workspace, the histogram and the grid must not reach the next one."""
    from dcanet_amd import ops
    case = C.cases()[0]
    H, W = case.d.shape
    inputs = [case.d, np.full((H, W), 10.0, np.float32), C._scene_a(5).d]
    kw = dict(max_disp=32, calib=case.calib, min_rise=4, min_votes=1000)      # (an all-wall frame: at most 12 rows x 75 votes)
    grid = (0.5, 3.0, 12.0)
    static = torch.empty((H, W), device=DEV)
    ws = ops.ground_workspace(H, W, 32, DEV)
    ws.fill_(123)
    out_p = {"plane": torch.full((G.PLANE_LEN,), 9.0, device=DEV, dtype=torch.float64),
             "vdisp": torch.full((H, 32), 77, device=DEV, dtype=torch.int32)}
    out_s = {"label": torch.full((H, W), 9, device=DEV, dtype=torch.uint8), "height": torch.full((H, W), 9.0, device=DEV),
             "free_row": torch.full((W,), 9, device=DEV, dtype=torch.int32), "free_disp": torch.full((W,), 9.0, device=DEV),
             "bev": torch.full((2, 24, 12), 1000, device=DEV, dtype=torch.int32)}

    def run():
        p = ops.ground_plane(static, workspace=ws, out=out_p, **kw)
        return p, ops.ground_segment(static, p["plane"], case.calib, 32, grid=grid, out=out_s)

    static.copy_(dev(inputs[2]))
    run()                                                # warm-up, outside the capture, on the same stream
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        p, s = run()
    assert all(p[k] is out_p[k] for k in out_p) and all(s[k] is out_s[k] for k in out_s)
    statuses = []
    for d in inputs + inputs[:1]:
        static.copy_(dev(d))
        graph.replay()
        torch.cuda.synchronize()
        ref = G.ground_plane_host(d, **kw)
        ref_seg = G.ground_segment_host(d, ref["plane"], case.calib, 32, grid=grid)
        statuses.append(int(ref["plane"][5]))
        same_bits(out_p["vdisp"], ref["vdisp"], "replay vdisp")
        same_bits(out_p["plane"], ref["plane"], "replay plane")
        same_bits(ws.cpu().numpy()[0, 8:48].reshape(4, 10), ref["sums"], "replay sums")
        for k in G.SEGMENT_OUTPUTS:
            same_bits(out_s[k], ref_seg[k], "replay " + k)
        static.copy_(dev(d))                             # ... and the eager call gives what the replay gave
        eager_p = ops.ground_plane(static, **kw)
        eager_s = ops.ground_segment(static, eager_p["plane"], case.calib, 32, grid=grid)
        assert torch.equal(eager_p["plane"].view(torch.int64), out_p["plane"].view(torch.int64))
        assert all(torch.equal(eager_s[k].view(torch.uint8), out_s[k].view(torch.uint8)) for k in G.SEGMENT_OUTPUTS)
    assert statuses == [0, 1, 0, 0]
    with pytest.raises(RuntimeError, match="ground_plane"):
        ops.ground_plane(static, workspace=ws.view(-1)[:10], **kw)
    with pytest.raises(RuntimeError, match="ground_plane"):
        ops.ground_plane(static, workspace=ws.int(), **kw)


def test_ground_segment_selective_outputs_write_only_those():
    from dcanet_amd import ops
    case = C.cases()[0]
    ref, ref_seg = _ref(case)
    d, plane = dev(case.d), dev(ref["plane"])
    H, W = case.d.shape
    kw = _dev_kwargs(C.segment_kwargs(case))
    poison = {"label": torch.full((H, W), 9, device=DEV, dtype=torch.uint8), "height": torch.full((H, W), 9.0, device=DEV),
              "free_row": torch.full((W,), 9, device=DEV, dtype=torch.int32), "free_disp": torch.full((W,), 9.0, device=DEV),
              "bev": torch.full((2, 24, 12), 9, device=DEV, dtype=torch.int32)}
    got = ops.ground_segment(d, plane, case.calib, outputs=("label",), out=poison, **kw)
    assert set(got) == {"label"} and got["label"] is poison["label"]
    same_bits(got["label"], ref_seg["label"], "label only")
    assert all(bool((poison[k] == 9).all()) for k in ("height", "free_row", "free_disp", "bev")), "the others stay poisoned"
    got = ops.ground_segment(d, plane, case.calib, outputs=("free_row",), **kw)
    assert set(got) == {"free_row", "free_disp"}
    same_bits(got["free_row"], ref_seg["free_row"], "free_row only"), same_bits(got["free_disp"], ref_seg["free_disp"], "free_disp")
    got = ops.ground_segment(d, plane, case.calib, outputs=("bev",), out={"bev": poison["bev"]}, **kw)
    assert set(got) == {"bev"}
    same_bits(got["bev"], ref_seg["bev"], "bev only: cleared, then counted")
    got = ops.ground_segment(d, plane, case.calib, outputs=("height", "bev"), **kw)
    same_bits(got["height"], ref_seg["height"], "height"), same_bits(got["bev"], ref_seg["bev"], "bev")
    assert bool((poison["label"].cpu() == torch.from_numpy(ref_seg["label"])).all()) and bool((poison["height"] == 9).all())


def test_ground_operators_refuse_what_they_cannot_do():
    from dcanet_amd import ops
    from dcanet_amd.geometry import StereoCalib
    a = torch.full((2, 1, 48, 80), 5.0, device=DEV)
    cal = StereoCalib(60.0, 0.5, 37.0, -7.0)
    nan, inf = float("nan"), float("inf")
    for bad in (dict(max_disp=7), dict(max_disp=1025), dict(max_disp=32.5), dict(fit_rows=(24, 49)), dict(fit_rows=(30, 30)),
                dict(fit_rows=(-1, 10)), dict(min_rise=0), dict(min_rise=33), dict(min_votes=0), dict(refine=-1), dict(refine=5),
                dict(min_inliers=2), dict(min_disp=-0.5), dict(min_disp=nan), dict(tol=-1.0), dict(tol=inf), dict(window=(0, 49, 80)),
                dict(window=(1, 48, 80)), dict(window=(0, 48, 81)), dict(window=(0, 1, 80)), dict(mask=a[:1]),
                dict(mask=a, mask_min=nan), dict(mask=a.double()), dict(calib=object()), dict(calib=cal, v0=nan),
                dict(workspace=torch.empty((1, 48), device=DEV, dtype=torch.int64)), dict(out={"nope": a}),
                dict(out={"plane": torch.empty((2, 1, 16), device=DEV)}), dict(out={"vdisp": torch.empty((2, 1, 48, 31), device=DEV, dtype=torch.int32)})):
        with pytest.raises(RuntimeError, match="ground_plane"):
            ops.ground_plane(a, **{**dict(max_disp=32), **bad})
    plane = torch.zeros((2, 1, 16), device=DEV, dtype=torch.float64)
    for bad in (dict(max_disp=7), dict(min_disp=-1.0), dict(tol_d=-1.0), dict(tol_d=nan), dict(h_ground=-0.1), dict(h_max=inf),
                dict(min_run=0), dict(min_run=1.5), dict(grid=(0.0, 3.0, 12.0)), dict(grid=(0.5, 3.0)), dict(grid=(1e-4, 3.0, 12.0)),
                dict(outputs=("nope",)), dict(outputs=()), dict(plane=plane[0]), dict(plane=plane.float()), dict(plane=plane.cpu()),
                dict(calib=None), dict(window=(0, 49, 80)), dict(mask=a[:1]), dict(mask=a, mask_min=nan), dict(out={"label": a}),
                dict(out={"bev": torch.empty((2, 1, 2, 24, 11), device=DEV, dtype=torch.int32)})):
        kw = {**dict(plane=plane, calib=cal, max_disp=32, grid=(0.5, 3.0, 12.0)), **bad}
        with pytest.raises(RuntimeError, match="ground_segment"):
            ops.ground_segment(a, kw.pop("plane"), kw.pop("calib"), **kw)
    for t in (a.double(), a[..., ::2], a.expand(2, 3, 48, 80).contiguous(), a.clone().requires_grad_()):
        with pytest.raises(RuntimeError, match="ground_plane"):
            ops.ground_plane(t, 32)
        with pytest.raises(RuntimeError, match="ground_segment"):
            ops.ground_segment(t, plane, cal, 32)
    with torch.no_grad():
        r = ops.ground_plane(a.clone().requires_grad_(), 32)
    assert r["plane"].shape == (2, 1, 16) and r["vdisp"].shape == (2, 1, 48, 32) and r["plane"][:, 0, 5].tolist() == [0.0, 0.0]


# ---- through the wrapper ----------------------------------------------------------------------------------------------------
WRAP = dict(crop_height=32, crop_width=64, graph=False)
GROUND = dict(grid=(0.5, 4.0, 16.0), plane=dict(min_votes=4, min_inliers=8), segment=dict(min_run=2))


@pytest.mark.parametrize("mode,post", [(None, False), ("lr", False), (None, True), ("lr", True)])
def test_kitti_inference_ground(mode, post, monkeypatch):
    """a full-frame image and a 28 x 50 one in the 32 x 64 frame: the record is ops.ground_plane and ops.ground_segment of the
    disparity (and the mask) that the EXISTING classes hand out for the frame -- after ops.median_filter and ops.speckle_filter
    with `median=` / `speckle=` -- in ONE read-back per frame; stream() gives the same bytes"""
    from dcanet_amd import ops
    from dcanet_amd.geometry import StereoCalib
    from dcanet_amd.inference import FrameGround, KittiInference, KittiInferenceGround, KittiInferenceLR
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
    infer = KittiInferenceGround(model, calib, mask=mode, tau=tau, speckle=speckle, median=3 if post else 0, **GROUND, **WRAP)
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
        p = ops.ground_plane(d, model.maxdisp, calib, mask=m, **GROUND["plane"])
        s = ops.ground_segment(d, p["plane"], calib, model.maxdisp, mask=m, grid=GROUND["grid"], **GROUND["segment"])
        before = len(copies)
        got = infer(l, r)
        assert len(copies) == before + 1, "one read-back per frame"
        single.append(got)
        assert isinstance(got, FrameGround) and got.disp.shape == got.label.shape == (h, w) and got.bev.shape == (2, 32, 16)
        lab = s["label"].cpu().numpy()
        print(f"mode={mode} post={post} image {h}x{w}: status {int(got.plane[5])}, line {got.plane[6:9].tolist()}, inliers "
              f"{int(got.plane[3])}, labels {np.bincount(lab.ravel(), minlength=5).tolist()}, free columns {int((got.free_row >= 0).sum())}")
        assert got.disp.tobytes() == d.cpu().numpy().tobytes(), f"image {i}: the disparity the stage read"
        assert got.plane.dtype == np.float64 and got.plane.tobytes() == p["plane"].cpu().numpy().tobytes(), f"image {i}: plane"
        for k in ("label", "free_row", "free_disp", "bev"):
            assert getattr(got, k).tobytes() == s[k].cpu().numpy().tobytes(), f"image {i}: {k}"
        assert copies[-1] == 128 + 4 * h * w + 8 * w + 4 * 2 * 32 * 16 + h * w, "the record's bytes, no more"
    streamed = list(infer.stream(iter(pairs + pairs[:1]), depth=2))
    assert len(streamed) == 3
    for a, b in zip(streamed, single + single[:1]):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
