"""Per-pixel confidence on the MI355X (csrc/confidence.hip): the three kernels against fp64 / int64 restatements of
include/dca_hip.h written here in plain torch / numpy, their bitwise ties to the existing soft-argmin and convex
up-sampler, and the way through GwcNet.predict, GraphedHotPath, KittiInference and ConfidenceCurve."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import dcanet_oracle as O
from oracle.seeded import seeded_tensor

pytestmark = pytest.mark.gpu
DEV = "cuda"
GATE = 2e-6          # the project's soft-argmin forward gate; fp32-vs-fp64 of the same formulas on the CPU: <= 2.3e-7
UP_GATE = 1e-6       # test_convex_upsample_vs_oracle's gate


def close(a, b, tol=2e-5, name=""):
    a, b = torch.as_tensor(a).detach().cpu().double(), torch.as_tensor(b).detach().cpu().double()
    assert a.shape == b.shape, (name, a.shape, b.shape)
    err = (a - b).abs().max().item()
    scale = max(1.0, b.abs().max().item())
    print(f"{name}: max err {err:.3e} (scale {scale:.3e}, gate {tol * scale:.3e})")
    assert err <= tol * scale, f"{name}: max err {err:.3e} (scale {scale:.3e})"


PLANES = ("disp", "duni", "mass", "ent", "std")


def stats_ref(logits, radius):
    """include/dca_hip.h, dca_softargmin_stats, in fp64: (B,K,h,w) fp32 -> (B,5,h,w) fp64"""
    x = logits.detach().cpu().double()
    K = x.shape[1]
    k = torch.arange(K, dtype=torch.float64).view(1, K, 1, 1)
    m = x.max(1, keepdim=True).values
    kstar = torch.where(x == m, k, torch.full_like(x, float(K))).min(1, keepdim=True).values     # lowest index of the maximum
    e = torch.exp(x - m)
    s = e.sum(1, keepdim=True)
    d = (e * k).sum(1, keepdim=True) / s
    win = ((k - kstar).abs() <= radius).double()
    ws = (e * win).sum(1, keepdim=True)
    duni = (e * win * k).sum(1, keepdim=True) / ws
    ent = (torch.log(s) - (e * (x - m)).sum(1, keepdim=True) / s) / math.log(K) if K > 1 else torch.zeros_like(s)
    std = ((e * (k - d) ** 2).sum(1, keepdim=True) / s).sqrt()
    return torch.cat([d, duni, ws / s, ent, std], 1)


def check_stats(logits, radius, name):
    from dcanet_amd import ops
    got = ops.softargmin_stats(logits.to(DEV), radius)
    ref = stats_ref(logits, radius)
    assert got.shape == ref.shape and got.dtype == torch.float32
    assert not torch.isnan(got).any(), name
    for i, plane in enumerate(PLANES):
        close(got[:, i], ref[:, i], GATE, f"{name} r={radius} {plane}")
    return got, ref


@pytest.mark.parametrize("shape", [(2, 48, 5, 9), (1, 8, 1, 1), (2, 12, 3, 67), (1, 2, 4, 5), (1, 1, 2, 3)])
def test_softargmin_stats_vs_fp64(shape):
    """Spread (s = 2), sharp (8) and saturated (40: the entropy underflows to ~1e-32) distributions and an all-zero map,
    radii 0, 1, 3 and one beyond K.  All five planes at the soft-argmin forward gate 2e-6: the same formulas in fp32 on the
    CPU differ from fp64 by at most 2.3e-7 in this measure on these inputs, so the gate leaves ~9x."""
    from dcanet_amd import ops
    B, K, h, w = shape
    for s in (2, 8, 40):
        logits = seeded_tensor(f"conf.x{shape}", shape) * s
        plain = ops.softargmin(logits.to(DEV))
        for radius in (0, 1, 3, K + 5):
            got, _ = check_stats(logits, radius, f"{shape} s={s}")
            assert torch.equal(got[:, :1], plain), "plane 0 is not bitwise ops.softargmin"
            if radius >= K:
                close(got[:, 1], got[:, 0], GATE, "whole-range duni == disp")
                close(got[:, 2], torch.ones_like(got[:, 2]), GATE, "whole-range mass == 1")
    zero = torch.zeros(shape)
    for radius in (0, 1, 3, K + 5):
        got, _ = check_stats(zero, radius, f"{shape} zeros")
        assert torch.equal(got[:, :1], ops.softargmin(zero.to(DEV)))
        # ties go to k* = 0: the window is [0, radius]; the distribution is uniform
        close(got[:, 2], torch.full_like(got[:, 2], min(radius + 1, K) / K), GATE, "uniform mass")
        if K > 1:
            assert torch.equal(got[:, 3], torch.ones_like(got[:, 3])), "entropy of a uniform distribution is exactly 1"
        else:
            assert torch.equal(got[:, 3], torch.zeros_like(got[:, 3]))


@pytest.mark.parametrize("peak", ["first", "last"])
def test_softargmin_stats_window_is_clipped(peak):
    """the peak forced to k = 0 and to k = K - 1: the window loses the bins outside [0, K-1]"""
    shape = (2, 12, 3, 67)
    logits = seeded_tensor("conf.clip", shape) * 2
    kp = 0 if peak == "first" else shape[1] - 1
    logits[:, kp] = logits.amax(1) + 1.5
    for radius in (0, 1, 3):
        got, ref = check_stats(logits, radius, f"peak {peak}")
        close(got[:, 1], ref[:, 1], GATE, "duni"); close(got[:, 2], ref[:, 2], GATE, "mass")
        # the soft-argmin of a one-sided window lies inside it
        lo, hi = max(kp - radius, 0), min(kp + radius, shape[1] - 1)
        assert got[:, 1].min().item() >= lo - 1e-5 and got[:, 1].max().item() <= hi + 1e-5


def test_softargmin_stats_refuses_what_it_cannot_do():
    from dcanet_amd import ops
    x = torch.zeros(1, 4, 2, 2, device=DEV)
    with pytest.raises(RuntimeError):
        ops.softargmin_stats(x, -1)
    with pytest.raises(RuntimeError):
        ops.softargmin_stats(x.cpu(), 1)
    with pytest.raises(RuntimeError):
        ops.softargmin_stats(x.clone().requires_grad_(), 1)
    with pytest.raises(RuntimeError):
        ops.convex_upsample4_planes(torch.zeros(1, 144, 2, 2, device=DEV).requires_grad_(), x, [1.0] * 4)


# ---- convex up-sampling of several planes ----------------------------------------------------------------------------------
def convex_ref(mask, planes, scales):
    """include/dca_hip.h, dca_convex_up4_planes, in fp64 as the reference writes it (F.unfold, soft-max, pixel shuffle)"""
    mask, planes = mask.detach().cpu().double(), planes.detach().cpu().double()
    B, P, h, w = planes.shape
    wgt = mask.view(B, 1, 9, 4, 4, h, w).softmax(2)
    x = planes * torch.tensor(scales, dtype=torch.float64).view(1, P, 1, 1)
    nb = F.unfold(x, [3, 3], padding=1).view(B, P, 9, 1, 1, h, w)
    return (wgt * nb).sum(2).permute(0, 1, 4, 2, 5, 3).reshape(B, P, 4 * h, 4 * w)


@pytest.mark.parametrize("P", [1, 5, 8])
@pytest.mark.parametrize("shape", [(2, 6, 10), (1, 1, 1), (3, 5, 67), (1, 34, 60)])
def test_convex_upsample4_planes(shape, P):
    """the shapes of test_convex_upsample_vs_oracle (a single cell: all eight neighbours padded; a width that is no multiple
    of the workgroup), scales a mix of 1 and 4; a plane with scale 4 is bitwise the single-plane operator"""
    from dcanet_amd import ops
    B, h, w = shape
    mask = seeded_tensor(f"cvxp.m{shape}", (B, 144, h, w)) * 2
    planes = seeded_tensor(f"cvxp.p{shape}{P}", (B, P, h, w)) * 3 + 10
    scales = [(4.0, 1.0, 1.0, 4.0, 1.0, 4.0, 4.0, 1.0)[p] for p in range(P)]
    got = ops.convex_upsample4_planes(mask.to(DEV), planes.to(DEV), scales)
    close(got, convex_ref(mask, planes, scales), UP_GATE, f"planes {shape} P={P}")
    for p in range(P):
        if scales[p] == 4.0:
            one = ops.convex_upsample4(mask.to(DEV), planes[:, p:p + 1].to(DEV))
            assert torch.equal(got[:, p:p + 1], one), f"plane {p} is not bitwise ops.convex_upsample4"


def test_convex_upsample4_planes_refuses_bad_plane_counts():
    from dcanet_amd import ops
    mask = torch.zeros(1, 144, 3, 4, device=DEV)
    for P in (0, 9):
        with pytest.raises(RuntimeError):
            ops.convex_upsample4_planes(mask, torch.zeros(1, P, 3, 4, device=DEV), [1.0] * P)
    with pytest.raises(RuntimeError):
        ops.convex_upsample4_planes(mask, torch.zeros(1, 2, 3, 4, device=DEV), [1.0])            # one scale short
    with pytest.raises(RuntimeError):
        ops.convex_upsample4_planes(mask[:, :143], torch.zeros(1, 2, 3, 4, device=DEV), [1.0, 1.0])


def test_convex_upsample4_planes_border_rule():
    """constant planes of 1.0 under a random mask: the weights sum to 1, so interior outputs are `scale`; cells along the
    border see zero-padded neighbours and are pulled towards 0, for a confidence plane as for the disparity.  Both bounds
    are relative to `scale` (close()'s measure): interior within 1e-6 * scale of scale, and no output above
    scale * (1 + 1e-6), because a rounded convex sum of equal values may exceed them by an ulp"""
    from dcanet_amd import ops
    scales = [1.0, 4.0, 1.0]
    mask = seeded_tensor("cvxp.border", (2, 144, 5, 67)).to(DEV) * 2
    up = ops.convex_upsample4_planes(mask, torch.ones(2, 3, 5, 67, device=DEV), scales)
    for p, s in enumerate(scales):
        assert (up[:, p, 4:-4, 4:-4] - s).abs().max().item() <= 1e-6 * s
        assert up[:, p].max().item() <= s * (1 + 1e-6) and up[:, p].min().item() >= 0.0
        border = torch.cat([up[:, p, :4].flatten(), up[:, p, -4:].flatten(), up[:, p, :, :4].flatten(),
                            up[:, p, :, -4:].flatten()])
        assert border.max().item() <= s * (1 + 1e-6) and border.min().item() < s * 0.99        # pulled towards 0 somewhere


# ---- risk-coverage histogram ---------------------------------------------------------------------------------------------
def hist_ref(conf, pred, gt, nbins, maxdisp):
    """include/dca_hip.h, dca_conf_histogram, in numpy: fp32 products, int64 sums"""
    c, p, g = (np.asarray(a, np.float32).ravel() for a in (conf, pred, gt))
    valid = (g > 0) & (g < np.float32(maxdisp)) & (c == c)
    c = np.where(valid, c, np.float32(0))
    raw = (np.clip(c, np.float32(0), np.float32(1)) * np.float32(nbins)).astype(np.int64)
    bins = np.minimum(raw, nbins - 1)[valid]
    err = np.abs(p - g)[valid]
    assert err.dtype == np.float32
    st = np.zeros((nbins, 3), np.int64)
    np.add.at(st[:, 0], bins, 1)
    np.add.at(st[:, 1], bins, (err * np.float32(1048576)).astype(np.int64))
    np.add.at(st[:, 2], bins, (err > np.float32(3)).astype(np.int64))
    return st, int(valid.sum())


def _hist_inputs(B, HW, seed, maxdisp):
    rs = np.random.RandomState(seed)
    n = B * HW
    conf = rs.uniform(-0.05, 1.05, n).astype(np.float32)
    conf[::7] = (rs.randint(0, 65, len(conf[::7])) / 64).astype(np.float32)        # exact bin edges i/64, incl. 0.0 and 1.0
    conf[1::31] = np.nan
    conf[2::53] = np.float32(1.0)
    conf[3::59] = np.float32(0.0)
    conf[4::61] = np.float32(np.inf)
    gt = rs.uniform(0.5, maxdisp - 0.5, n).astype(np.float32)
    gt[::5] = 0.0
    gt[1::11] = np.float32(maxdisp)
    gt[2::13] = np.float32(maxdisp + 7.25)
    gt[3::17] = -3.0
    pred = (gt + rs.standard_normal(n).astype(np.float32) * rs.choice([0.3, 2.0, 9.0], n).astype(np.float32)).astype(np.float32)
    return tuple(a.reshape(B, HW) for a in (conf, pred, gt))


@pytest.mark.parametrize("B,HW,nbins", [(2, 37 * 53, 7), (2, 37 * 53, 64), (1, 300, 1024)])
def test_conf_histogram_is_exact(B, HW, nbins):
    """bin edges, confidences outside [0,1], NaN, invalid ground truth; two calls into one state; the same sequence twice"""
    from dcanet_amd.evaluation import ConfidenceCurve, risk_coverage
    maxdisp = 48
    a, b = _hist_inputs(B, HW, 100 + nbins, maxdisp), _hist_inputs(B, HW, 200 + nbins, maxdisp)
    want, counted = hist_ref(*(np.concatenate([x, y]) for x, y in zip(a, b)), nbins, maxdisp)
    assert counted * 2 >= 2 * B * HW, "fewer than half of the pixels count"
    assert want[:, 0].sum() == counted and (want[:, 0] > 0).sum() >= min(nbins, 7) // 2
    states = []
    for _ in range(2):
        cc = ConfidenceCurve(nbins=nbins, maxdisp=maxdisp, device=DEV)
        for conf, pred, gt in (a, b):
            cc.add(*(torch.from_numpy(t).to(DEV) for t in (conf, pred, gt)))
        states.append(cc.state.cpu().numpy())
    assert states[0].dtype == np.int64 and np.array_equal(states[0], want)
    assert states[0].tobytes() == states[1].tobytes()
    res = cc.result()
    assert res["pixels"] == counted and np.array_equal(res["counts"], want[:, 0])
    host = risk_coverage(want)
    assert set(res) == set(host) and all(np.array_equal(res[k], host[k]) for k in res)
    assert res["coverage"][-1] == 1.0 and res["aurc_epe"] > 0
    cc.reset()
    assert not cc.state.any().item()
    with pytest.raises(RuntimeError):
        from dcanet_amd import ops
        ops.conf_histogram(torch.zeros(4, device=DEV), torch.zeros(4, device=DEV), torch.zeros(5, device=DEV), cc.state, 48)


# ---- through the model -----------------------------------------------------------------------------------------------------
def load_seeded(module):
    shapes = {k: tuple(v.shape) for k, v in module.state_dict().items()}
    module.load_state_dict(O.seeded_state_dict(shapes), strict=True)
    return module


_MODELS = {}


def _model(concat):
    """one seeded GwcNet(32) per volume mode for the whole module, never modified (eval mode, no grad)"""
    if concat not in _MODELS:
        from dcanet_amd.models.gwcnet_dca_g import GwcNet
        _MODELS[concat] = load_seeded(GwcNet(32, use_concat_volume=concat)).to(DEV).eval()
    return _MODELS[concat]


def _images():
    return seeded_tensor("smoke.left", (1, 3, 32, 64)).to(DEV), seeded_tensor("smoke.right", (1, 3, 32, 64)).to(DEV)


def _hot_args(model, left, right):
    fl, fr = model.feature_extraction(left), model.feature_extraction(right)
    args = [fl["gwc_segments"], fr["gwc_segments"]]
    if model.use_concat_volume:
        args += [fl["concat_feature"], fr["concat_feature"]]
    return args


@pytest.mark.parametrize("concat", [False, True])
def test_predict_against_the_models_own_logits(concat, monkeypatch):
    """predict()["disp"] is forward()[0] bit for bit; the other maps are the fp64 restatements applied to the model's own
    logits3 and mask logits, recomputed here by calling the sub-modules (no hook in the model)"""
    from dcanet_amd import ops
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)      # MIOpen convolutions of the 2D networks
    model, radius = _model(concat), 1
    left, right = _images()
    with torch.no_grad():
        pred4, _ = model(left, right)
        out = model.predict(left, right, radius=radius)
        assert not model.training
        assert set(out) == {"disp", "disp_unimodal", "confidence", "entropy", "std"}
        assert all(v.shape == (1, 1, 32, 64) and v.dtype == torch.float32 for v in out.values())
        assert torch.equal(out["disp"], pred4), "predict()['disp'] is not bitwise forward()[0]"
        # the model's own logits: GwcNet._hot_path's eval branch, module by module
        args = _hot_args(model, left, right)
        volume = ops.cost_volume(args[0], args[1], model.maxdisp // 4, model.num_groups, *(args[2:] or [None, None]))
        cost0 = model.dres1(model.dres0(volume))
        _, out1 = model.cva1(cost0, res_post=cost0)
        _, out2 = model.cva2(out1)
        _, out3 = model.cva3(out2)
        logits3 = model.classif3(out3).squeeze(1)
        mask = model.prop.conv(model.guidance(left)["g"])
        hot = model.hot_path(*args)
        assert torch.equal(ops.softargmin(logits3), hot["pred4_q"]), "the recomputed logits are not the model's"
    ref = convex_ref(mask, stats_ref(logits3, radius).float(), [4.0, 4.0, 1.0, 1.0, 4.0])
    # the up-sampler's inputs in the restatement are the fp64 statistics rounded to fp32; the kernel's are its own fp32
    # statistics, within GATE of them, and a convex combination does not amplify that: GATE + UP_GATE
    for i, name in enumerate(("disp", "disp_unimodal", "confidence", "entropy", "std")):
        close(out[name], ref[:, i:i + 1], GATE + UP_GATE, f"predict {name} (concat={concat})")
    assert 0.0 <= out["confidence"].min().item() and out["confidence"].max().item() <= 1.0 + 1e-6
    assert out["confidence"].std().item() > 1e-3, "a constant confidence map says nothing"


def test_hot_path_confidence_argument(monkeypatch):
    from dcanet_amd import ops
    from dcanet_amd.graph import GraphedHotPath
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    model = _model(False)
    left, right = _images()
    with torch.no_grad():
        args = _hot_args(model, left, right)
        plain = model.hot_path(*args)
        assert set(plain) == {"pred4_q", "prob_volume2"}                                   # exactly today's keys
        eager = model.hot_path(*args, confidence=1)
        assert set(eager) == {"pred4_q", "prob_volume2", "stats4_q"}
        assert eager["stats4_q"].shape == (1, 5, 8, 16) and eager["pred4_q"].shape == (1, 1, 8, 16)
        assert torch.equal(eager["pred4_q"], plain["pred4_q"]) and torch.equal(eager["stats4_q"][:, :1], plain["pred4_q"])
        assert torch.equal(eager["prob_volume2"], plain["prob_volume2"])
        graphed = GraphedHotPath(model, *args, confidence=1)
        replay = graphed(*args)
        assert set(replay) == set(eager)
        for k in eager:
            assert torch.equal(replay[k], eager[k]), f"replay differs from eager in {k}"
        assert set(GraphedHotPath(model, *args)(*args)) == {"pred4_q", "prob_volume2"}     # the default stays as it is
        # reduced precision: plane 0 is still that path's soft-argmin
        with ops.reduced_precision(torch.float16):
            lp_plain = model.hot_path(*args)
            lp = model.hot_path(*args, confidence=1)
        assert torch.equal(lp["stats4_q"][:, :1], lp["pred4_q"]) and torch.equal(lp["pred4_q"], lp_plain["pred4_q"])
        assert not torch.isnan(lp["stats4_q"]).any()
    with torch.no_grad():
        model.train()
        try:
            with pytest.raises(RuntimeError):
                model.hot_path(*args, confidence=1)
        finally:
            model.eval()
    with pytest.raises(RuntimeError):                                                      # eval mode, but grad enabled
        model.hot_path(*args, confidence=1)


def _pairs(rng, sizes):
    return [(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
            for h, w in sizes]


def test_kitti_inference_with_confidence(monkeypatch):
    """a 27 x 61 image in a 32 x 64 frame; device_io x graph: the disparity is bitwise the one without confidence, the
    confidence is a cropped map in [0,1], the same wherever the disparity is, and its uint16 form is trunc(conf * 65535)"""
    from dcanet_amd.inference import KittiInference, KittiInferenceWithConfidence
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    model = _model(False)
    (left, right), = _pairs(np.random.default_rng(7), [(27, 61)])
    results = {}
    for device_io in (False, True):
        for graph in (False, True):
            plain = KittiInference(model, crop_height=32, crop_width=64, graph=graph, device_io=device_io)
            infer = KittiInferenceWithConfidence(model, crop_height=32, crop_width=64, graph=graph, device_io=device_io,
                                                 radius=1)
            want = plain(left, right)
            assert isinstance(want, np.ndarray)                                            # off: nothing changes
            disp, conf = infer(left, right)
            assert disp.shape == conf.shape == (27, 61) and disp.dtype == conf.dtype == np.float32
            assert np.ascontiguousarray(disp).tobytes() == np.ascontiguousarray(want).tobytes(), (device_io, graph)
            assert conf.min() >= 0.0 and conf.max() <= 1.0 and conf.std() > 1e-3
            d16, c16 = infer(left, right, as_uint16=True)
            assert d16.dtype == c16.dtype == np.uint16 and c16.shape == (27, 61)
            assert np.array_equal(d16, plain(left, right, as_uint16=True))
            assert np.array_equal(c16, np.trunc(conf * np.float32(65535)).astype(np.uint16))
            results[device_io, graph] = (np.ascontiguousarray(disp), np.ascontiguousarray(conf))
    base_disp, base_conf = results[False, False]
    same = 0
    for key, (disp, conf) in results.items():
        if disp.tobytes() == base_disp.tobytes():
            same += 1
            assert conf.tobytes() == base_conf.tobytes(), f"equal disparity, other confidence: {key}"
    for device_io in (False, True):       # a replay is bitwise the eager path, so each pair must have been compared
        assert results[device_io, True][0].tobytes() == results[device_io, False][0].tobytes()
        assert results[device_io, True][1].tobytes() == results[device_io, False][1].tobytes()
    print(f"{same} of 4 configurations give the host path's eager disparity bit for bit")


@pytest.mark.parametrize("graph", [True, False])
def test_stream_with_confidence_equals_one_at_a_time_calls(graph, monkeypatch):
    from dcanet_amd.inference import KittiInferenceWithConfidence
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    infer = KittiInferenceWithConfidence(_model(False), crop_height=32, crop_width=64, graph=graph, device_io=True)
    pairs = _pairs(np.random.default_rng(9), [(27, 61), (32, 64), (27, 61)])
    single = [infer(l, r) for l, r in pairs]
    assert not np.array_equal(single[0][1], single[2][1])                                  # same size, different content
    got = list(infer.stream(iter(pairs), depth=2))
    assert len(got) == 3
    for i, (g, s) in enumerate(zip(got, single)):
        assert isinstance(g, tuple) and len(g) == 2
        for a, b in zip(g, s):
            assert a.shape == b.shape and a.tobytes() == b.tobytes(), f"frame {i} differs"
    for (d16, c16), (d, c) in zip(infer.stream(pairs, depth=2, as_uint16=True), single):
        assert np.array_equal(d16, (d * 256).astype("uint16"))
        assert np.array_equal(c16, np.trunc(c * np.float32(65535)).astype(np.uint16))
