"""Semi-global matching on the MI355X (csrc/sgm.hip): `ops.sgm_census` and every output of `ops.sgm_disparity` bit for bit
against the numpy restatement of dcanet_amd/sgm.py on the cases of tests/_sgm_cases.py, a second call into poisoned buffers
through a workspace of garbage, selective outputs, the launches under hipGraph replay, the operators' refusals, and the ways
through inference.SGMInference and inference.KittiInferenceGuided(sgm=).

Why bitwise, without any tolerance: census, Hamming cost, path recursion, sum, winner, uniqueness test and sub-pixel step are
integer arithmetic (no atomic of any kind: one wave per scanline, the paths summed by launches the stream orders), and the one
fp32 operation is the exact division of an integer below 2^13 by 16."""
import numpy as np
import pytest
import torch

import _sgm_cases as C
from _inference_cases import model as _model, pairs as _pairs
from dcanet_amd import sgm as S

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


def poisoned(H, W, names=S.SGM_OUTPUTS):
    return {k: torch.full((H, W), 77, device=DEV, dtype=S._SGM_KINDS[k]) for k in names}


@pytest.mark.parametrize("case", C.cases(), ids=lambda c: c.name)
def test_sgm_is_the_restatement_bit_for_bit(case):
    from dcanet_amd import ops
    ref = C.expected(case.name)
    left, right = dev(case.left), dev(case.right)
    H, W = case.left.shape[:2]
    census = ops.sgm_census(left, right)
    assert census.dtype == torch.int64 and census.shape == (2, H, W)
    same_bits(census.cpu().numpy().view(np.uint64), ref["census"], "census")
    got = ops.sgm_disparity(left, right, outputs=S.SGM_OUTPUTS, **case.kw)
    assert tuple(got) == S.SGM_OUTPUTS
    print(case.name, (H, W), case.kw, "valid", float(ref["valid"].mean()), "largest cost", int(ref["cost"].max()))
    for k in S.SGM_OUTPUTS:
        same_bits(got[k], ref[k], k)
    # a second call into the same buffers, poisoned in between, through a workspace of garbage
    for t in got.values():
        t.fill_(77)
    ws = ops.sgm_workspace(H, W, case.kw["max_disp"], DEV)
    ws.fill_(0xA5)
    again = ops.sgm_disparity(left, right, outputs=S.SGM_OUTPUTS, out=got, workspace=ws, **case.kw)
    assert all(again[k] is got[k] for k in S.SGM_OUTPUTS)
    for k in S.SGM_OUTPUTS:
        same_bits(again[k], ref[k], k + " (second call)")
    same_bits(ws[:16 * H * W].view(torch.int64).view(2, H, W).cpu().numpy().view(np.uint64), ref["census"],
              "the workspace starts with the census")
    default = ops.sgm_disparity(left, right, **case.kw)
    assert tuple(default) == S.SGM_OUTPUTS[:3]
    census.fill_(-1)
    assert ops.sgm_census(left, right, out=census) is census
    same_bits(census.cpu().numpy().view(np.uint64), ref["census"], "census into out=")


def test_sgm_selective_outputs_write_only_those():
    from dcanet_amd import ops
    case = C.case("plane")
    ref = C.expected("plane")
    left, right = dev(case.left), dev(case.right)
    H, W = case.left.shape[:2]
    for names in (("cost",), ("disp_right_mirrored",), ("valid", "disp_right"), ("disp",)):
        out = poisoned(H, W)
        got = ops.sgm_disparity(left, right, outputs=names, out=out, **case.kw)
        assert set(got) == set(names) and all(got[k] is out[k] for k in names)
        for k in names:
            same_bits(got[k], ref[k], f"{k} of {names}")
        assert all(bool((out[k] == 77).all()) for k in S.SGM_OUTPUTS if k not in names), f"{names}: the others stay poisoned"
    got = ops.sgm_disparity(left, right, outputs=("disp_right",), **case.kw)
    assert set(got) == {"disp_right"}
    same_bits(got["disp_right"], ref["disp_right"], "disp_right alone, allocated")


def test_sgm_under_graph_replay():
    """`out=` and `workspace=`: nothing is allocated, so census, the eight paths and both winner-take-all launches are captured
    once on one stream behind static uint8 inputs and replayed on three different pairs and then the first again.  The
    workspace starts as garbage; what a replay leaves anywhere must not reach the next."""
    from dcanet_amd import ops
    H, W, D = 23, 67, 24
    rng = np.random.default_rng(11)
    inputs = [C.shifted_pair(rng, H, W, d, 3, noise=n) for d, n in ((9, 0), (3, 5), (15, 2))]
    kw = dict(max_disp=D, paths=8, P1=7, P2=90, uniqueness=10, min_disp=2)
    sl, sr = (torch.empty((H, W, 3), device=DEV, dtype=torch.uint8) for _ in range(2))
    ws = ops.sgm_workspace(H, W, D, DEV)
    out = poisoned(H, W)

    def run():
        return ops.sgm_disparity(sl, sr, outputs=S.SGM_OUTPUTS, out=out, workspace=ws, **kw)

    sl.copy_(dev(inputs[2][0])), sr.copy_(dev(inputs[2][1]))
    run()                                                # warm-up, outside the capture, on the same stream
    torch.cuda.synchronize()
    ws.fill_(0x5A)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = run()
    assert all(got[k] is out[k] for k in out)
    seen = []
    for left, right in inputs + inputs[:1]:
        sl.copy_(dev(left)), sr.copy_(dev(right))
        graph.replay()
        torch.cuda.synchronize()
        ref = S.sgm_host(left, right, outputs=S.SGM_OUTPUTS, **kw)
        for k in S.SGM_OUTPUTS:
            same_bits(out[k], ref[k], "replay " + k)
        seen.append(int(round(float(np.median(ref["disp"][ref["valid"] > 0])))))
    assert seen == [9, 3, 15, 9], f"the pairs differ: {seen}"


def test_sgm_refuses_what_it_cannot_do():
    from dcanet_amd import ops
    a = torch.zeros((12, 40, 3), device=DEV, dtype=torch.uint8)
    g = torch.zeros((12, 40), device=DEV, dtype=torch.uint8)
    f32 = lambda *s: torch.empty(s, device=DEV)
    for bad in (dict(max_disp=7), dict(max_disp=257), dict(max_disp=16.5), dict(max_disp="x"), dict(P1=0), dict(P1=11, P2=10),
                dict(P2=4096), dict(uniqueness=100), dict(uniqueness=-1), dict(paths=5), dict(paths=0), dict(min_disp=-1),
                dict(min_disp=16), dict(outputs=("nope",)), dict(outputs=()), dict(out={"nope": f32(12, 40)}),
                dict(out={"disp": f32(12, 41)}), dict(out={"cost": f32(12, 40)}), dict(out={"disp": f32(12, 40).cpu()}),
                dict(out={"valid": f32(12, 80)[:, ::2]}), dict(workspace=torch.empty(100, device=DEV, dtype=torch.uint8)),
                dict(workspace=torch.empty(S.sgm_workspace_bytes(12, 40, 16), device=DEV, dtype=torch.int8)),
                dict(workspace=torch.empty(S.sgm_workspace_bytes(12, 40, 16) + 8, device=DEV, dtype=torch.uint8)[1:]),
                dict(workspace=torch.empty(S.sgm_workspace_bytes(12, 40, 16), dtype=torch.uint8))):
        with pytest.raises(RuntimeError, match="sgm_disparity"):
            ops.sgm_disparity(a, a, **{**dict(max_disp=16), **bad})
    for left, right in ((a, a[:, :39].contiguous()), (a, g), (g, a), (a.float(), a.float()), (a[:, ::2], a[:, ::2]), (a, a.cpu()),
                        (a.cpu(), a), (a[:, :, :2].contiguous(),) * 2, (a[:6], a[:6]), (a[:, :6].contiguous(),) * 2,
                        (g[:, ::2], g[:, ::2]), (a[None], a[None])):
        for call in (lambda: ops.sgm_disparity(left, right, 16), lambda: ops.sgm_census(left, right)):
            with pytest.raises(RuntimeError, match="sgm_(disparity|census)"):
                call()
    for bad in (torch.empty((2, 12, 40), device=DEV, dtype=torch.int32), torch.empty((2, 12, 41), device=DEV, dtype=torch.int64),
                torch.empty((2, 12, 40), dtype=torch.int64)):
        with pytest.raises(RuntimeError, match="sgm_census"):
            ops.sgm_census(a, a, out=bad)
    r = ops.sgm_disparity(g, g, 16)
    assert float(r["valid"].sum()) == 0.0 and int(r["cost"].abs().sum()) == 0, "a flat pair: d* = 0 everywhere"


# ---- through the wrappers ---------------------------------------------------------------------------------------------------
def _by_hand(left, right, kw, lr_tau, median, speckle):
    """the operators applied one by one to the uint8 frame: what SGMInference documents"""
    from dcanet_amd import ops
    r = ops.sgm_disparity(dev(left), dev(right), outputs=("disp", "valid", "disp_right_mirrored"), **kw)
    d, v = r["disp"], r["valid"]
    if lr_tau is not None:
        v = v * ops.lr_consistency(d[None], r["disp_right_mirrored"][None], lr_tau, outputs=("valid",))["valid"][0]
        d = d * v
    if median:
        d = ops.median_filter(d, median, mask=v)
    if median or speckle is not None:
        f = ops.speckle_filter(d, *(speckle or (0, 0.0)), mask=v)
        d, v = f["disp"], f["valid"]
    return d.cpu().numpy(), v.cpu().numpy()


@pytest.mark.parametrize("lr_tau,median,speckle", [(None, 0, None), (1.0, 0, None), (None, 3, (6, 1.0)), (1.0, 3, (6, 1.0)), (1.0, 5, None)])
def test_sgm_inference(lr_tau, median, speckle, monkeypatch):
    """three pairs of different sizes, the last the largest (the buffers grow): the record is the operators applied by hand to the
    same uint8 frame, in ONE read-back per frame of exactly the record's bytes; stream() gives the same bytes"""
    from dcanet_amd.inference import SGMInference
    rng = np.random.default_rng(41)
    pairs = [C.shifted_pair(rng, 30, 70, 6, 3, noise=3), C.shifted_pair(rng, 24, 50, 4, 3, noise=2), C.shifted_pair(rng, 36, 80, 9, 4)]
    kw = dict(max_disp=16, paths=8, P1=8, P2=100, uniqueness=10)
    infer = SGMInference(lr_tau=lr_tau, median=median, speckle=speckle, **kw)
    copies = []
    readback = infer._readback
    monkeypatch.setattr(infer, "_readback", lambda s, copy: (copies.append(s.out_bytes), readback(s, copy))[1])
    single = []
    for i, (l, r) in enumerate(pairs):
        h, w = l.shape[:2]
        want_d, want_v = _by_hand(l, r, {**kw, "min_disp": 1}, lr_tau, median, speckle)
        before = len(copies)
        disp, valid = infer(l, r)
        assert len(copies) == before + 1 and copies[-1] == 8 * h * w, "one read-back per frame, of the record's bytes and no more"
        single.append((disp, valid))
        print(f"lr_tau={lr_tau} median={median} speckle={speckle} image {h}x{w}: {valid.mean():.3f} valid, median disparity "
              f"{np.median(disp[valid > 0])}")
        same_bits(disp, want_d, f"image {i}: disp"), same_bits(valid, want_v, f"image {i}: valid")
        assert valid.mean() > 0.5 and abs(np.median(disp[valid > 0]) - (6, 4, 9)[i]) <= 0.5, "the shift is found"
        assert (disp[valid == 0].view(np.uint32) == 0).all()
    streamed = list(infer.stream(iter(pairs + pairs[:1]), depth=2))
    assert len(streamed) == 4
    for a, b in zip(streamed, single + single[:1]):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_sgm_inference_rectifies_first():
    from dcanet_amd import ops
    from dcanet_amd.inference import SGMInference
    from _inference_cases import RAW, RECT, rectify_maps
    maps = rectify_maps()
    l, r = _pairs(np.random.default_rng(5), [RAW])[0]
    infer = SGMInference(max_disp=16, lr_tau=None, rectify=maps)
    disp, valid = infer(l, r)
    rl, rr = ops.rectify_pair(dev(l), dev(r), maps)
    want_d, want_v = _by_hand(rl.cpu().numpy(), rr.cpu().numpy(), dict(max_disp=16), None, 0, None)
    assert disp.shape == RECT
    same_bits(disp, want_d, "disp of the rectified pair"), same_bits(valid, want_v, "valid of the rectified pair")


def test_kitti_inference_guided_by_sgm(monkeypatch):
    """KittiInferenceGuided(model, sgm=...)(l, r) is KittiInferenceGuided(model)(l, r, hints) with the hints computed by hand from
    the same pair: a full 32 x 64 frame and a 28 x 50 image inside it; stream() takes pairs alone and gives the same bytes"""
    from dcanet_amd.inference import KittiInferenceGuided
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    model = _model()
    wrap = dict(crop_height=32, crop_width=64, graph=False)
    rng = np.random.default_rng(43)
    pairs = [C.shifted_pair(rng, 32, 64, 5, 3, noise=2), C.shifted_pair(rng, 28, 50, 3, 3, noise=2)]
    for opts in (dict(max_disp=16, lr_tau=1.0), dict(max_disp=24, paths=4, uniqueness=0, lr_tau=None)):
        auto, manual = KittiInferenceGuided(model, sgm=opts, **wrap), KittiInferenceGuided(model, **wrap)
        kw = {k: v for k, v in opts.items() if k != "lr_tau"}
        single = []
        for l, r in pairs:
            hints, v = _by_hand(l, r, kw, opts["lr_tau"], 0, None)
            assert (hints > 0).mean() > 0.5 and (hints[v == 0] == 0).all(), "the hints are a real map"
            got, want = auto(l, r), manual(l, r, hints)
            same_bits(got, want, f"{opts}: guided by its own hints")
            single.append(got)
        for a, b in zip(auto.stream(iter(pairs)), single):
            assert a.tobytes() == b.tobytes()
        with pytest.raises(TypeError, match="sgm="):
            auto(*pairs[0], np.zeros((32, 64), np.float32))
        with pytest.raises(TypeError, match="sgm="):
            manual(*pairs[0])
