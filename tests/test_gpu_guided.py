"""Guided stereo on the MI355X (csrc/guided.hip, the GUIDED instantiations of csrc/volume_fused.hip, ops.hints_to_quarter,
ops.volume_modulate, ops.cost_volume(hints4=), GwcNet(hints=), GraphedHotPath(hints4=), KittiInferenceGuided; DESIGN.md
section 6n).

Downsample: bit for bit the numpy restatement.  Stand-alone pass and fused builder: the fp64 gate of
tests/test_gpu_volume_fp64.py -- truth in float64 (the oracle's builders times the float64 factor), yardstick the same
arithmetic in float32 on the CPU (the oracle's builders in float32 times guided.guide_factor_host), metric
max |a - ref| / max(1, max |ref|), pass at max(4 x yardstick, 2^-22) and, for the gradients, at the siblings' 1e-5 (gwc) and
1e-6 (concat).  The per-row maxima the guided builder emits are those of the products.  The fp32 fused volume is BITWISE
the unguided fused volume followed by the stand-alone pass: one definition of the factor (csrc/guided_math.h), and
correlation sums that the GUIDED instantiation forms as the unguided one does (csrc/volume_fused.hip);
on it rest the two model tests hints = zeros and the composition of the public ops.

Measured on one MI355X, as printed by the tests before they assert: over the 38 gated outputs and gradients the float32
yardsticks lie between 7.3e-08 and 1.9e-07, the kernels' errors are at most 1.8e-07, and the error
closest to its gate stands at 0.28 of it."""
import numpy as np
import pytest
import torch

import _volume_cases as V
from oracle import dcanet_oracle as O
from oracle.seeded import seeded_tensor

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUIDE = (10.0, 1.0)
GUARD, SENTINEL = 4096, -1024.0
MAXDISP = 48

def _ops():
    from dcanet_amd import ops
    return ops


def _flags(monkeypatch, ops):
    for flag in ("CONV_X3", "CONV_X2", "PACK", "AMAX_EMIT"):
        monkeypatch.setattr(ops, flag, True)


def factor64(D, h4, guide=GUIDE):
    """m(d, h4) in float64 from the float32 hints: (..., H, W) -> (..., D, H, W)"""
    k, c = guide
    d = torch.arange(D, dtype=torch.float64).view(D, 1, 1)
    h = torch.as_tensor(h4).double().unsqueeze(-3)
    return torch.where(h > 0, k * torch.exp(-((d - h) ** 2) / (2 * c * c)), torch.ones((), dtype=torch.float64))


def factor32(D, h4, guide=GUIDE):
    from dcanet_amd.guided import guide_factor_host
    return torch.from_numpy(guide_factor_host(D, np.asarray(h4), guide))


def factor(D, h4, dtype):
    return factor64(D, h4) if dtype == torch.float64 else factor32(D, h4)


def hint_map(B, H, W, D, variant, seed=3):
    """hints in bins.  "rows": image row 0 has a hint in every cell, the last row none, the rows between are mixed; "mixed":
    every row is mixed.  A mixed row has hints at 0.25, at D - 1 and at a fractional value, seeded ones and a run without."""
    rng = np.random.default_rng(seed)
    h4 = (rng.random((B, H, W)) * (D - 1) + 0.25).astype(np.float32)
    mixed = h4.copy()
    mixed[rng.random((B, H, W)) < 0.5] = 0
    mixed[:, :, W // 2:W // 2 + max(5, W // 4)] = 0            # a run of cells without a hint, across x quads
    mixed[:, :, 0], mixed[:, :, 1], mixed[:, :, 2], mixed[:, :, 3] = 0.25, D - 1, 2.6875, 0
    mixed[:, :, W - 1] = D - 1
    if variant == "mixed":
        return mixed
    h4[:, :, 0], h4[:, :, 1], h4[:, :, 2] = 0.25, D - 1, 2.6875
    out = mixed
    out[:, 0] = h4[:, 0]
    out[:, H - 1] = 0
    return out


# ---- downsample ------------------------------------------------------------------------------------------------------------
def _special_image():
    from test_guided_cpu import special_image
    return special_image()


@pytest.mark.parametrize("name", ["placed-13x22-in-16x24", "frame-2x32x64"])
def test_hints_to_quarter_is_the_host_restatement(name):
    from dcanet_amd.guided import hints_to_quarter_host
    from dcanet_amd.inference import placement
    ops = _ops()
    if name.startswith("placed"):
        src, frame, place = _special_image(), (16, 24), placement(13, 22, 16, 24)
        assert place == (0, 3, 13, 22)
    else:
        rng = np.random.default_rng(4)
        src = (rng.random((2, 32, 64)) * 60 - 6).astype(np.float32)             # some <= 0, some >= maxdisp
        src[rng.random(src.shape) < 0.8] = 0
        src[0, 5, 7], src[1, 31, 63], src[1, 0, 0] = np.nan, np.inf, MAXDISP
        frame, place = (32, 64), None
    want, n = hints_to_quarter_host(src, frame, place, MAXDISP, count=True)
    shape = want.shape
    out = torch.full(shape, float("nan"), device=DEV)
    cnt = torch.full((1,), -7, device=DEV, dtype=torch.int64)
    got, c = ops.hints_to_quarter(torch.from_numpy(src).to(DEV), frame, place, MAXDISP, out=out, count=cnt)
    torch.cuda.synchronize()
    assert got is out and c is cnt
    assert not torch.isnan(out).any(), "a cell of the NaN-prefilled out was not written"
    assert out.cpu().numpy().tobytes() == want.tobytes(), "not bit for bit the host restatement"
    assert int(cnt.item()) == n and 0 < n < want.size
    fresh = ops.hints_to_quarter(torch.from_numpy(src).to(DEV), frame, place, MAXDISP)
    assert torch.equal(fresh, out)
    with pytest.raises(RuntimeError, match="hints_to_quarter"):
        ops.hints_to_quarter(torch.from_numpy(src).to(DEV), (frame[0] + 2, frame[1]), place, MAXDISP)
    with pytest.raises(RuntimeError, match="hints_to_quarter"):
        ops.hints_to_quarter(torch.from_numpy(src).to(DEV), frame, place, MAXDISP, out=torch.zeros(1, device=DEV))


# ---- the stand-alone pass --------------------------------------------------------------------------------------------------
MOD_SHAPES = [(1, 3, 5, 6, 19), (2, 4, 6, 5, 20), (1, 40, 12, 2, 240)]


def _guarded(n, fill):
    big = torch.full((n + 2 * GUARD,), SENTINEL, device=DEV, dtype=torch.float32)
    view = big[GUARD:GUARD + n]
    view.fill_(fill)
    assert view.data_ptr() % 16 == 0
    return big, view


@pytest.mark.parametrize("shape", MOD_SHAPES, ids=["x".join(map(str, s)) for s in MOD_SHAPES])
def test_volume_modulate(shape):
    """scalar path (odd W), vector path, and the training row width: fp64 gate of the forward and of the gradient, in place,
    and the C entry into a NaN-filled buffer between guard bands"""
    ops = _ops()
    B, C, D, H, W = shape
    tag = "gd.mod." + "x".join(map(str, shape))
    vol, seed = seeded_tensor(tag + ".v", shape), seeded_tensor(tag + ".g", shape)
    h4 = torch.from_numpy(hint_map(B, H, W, D, "rows"))
    m64, m32 = factor64(D, h4)[:, None], factor32(D, h4)[:, None]
    truth = {"fwd": vol.double() * m64, "d vol": seed.double() * m64}
    yard = {"fwd": V.error(vol * m32, truth["fwd"]), "d vol": V.error(seed * m32, truth["d vol"])}
    v = vol.to(DEV).requires_grad_()
    out = ops.volume_modulate(v, h4.to(DEV), *GUIDE)
    assert type(out.grad_fn).__name__ == "_VolumeModulateBackward"
    g, = torch.autograd.grad((out * seed.to(DEV)).sum(), v)
    got = {"fwd": out.detach(), "d vol": g}
    for name in truth:
        e = V.error(got[name], truth[name])
        print(f"  {tag} {name}: yardstick {yard[name]:.2e}  error {e:.2e}  gate {V.gate(yard[name]):.2e}")
        assert e <= V.gate(yard[name]), (name, e, yard[name])
    none = (h4 <= 0)[:, None, None].expand(shape)
    assert torch.equal(out.detach().cpu()[none], vol[none]), "a cell without a hint must leave its column bit-identical"
    with torch.no_grad():
        inplace = vol.to(DEV)
        r = ops.volume_modulate(inplace, h4.to(DEV), *GUIDE, out=inplace)
        assert r.data_ptr() == inplace.data_ptr() and torch.equal(inplace, out.detach()), "in place differs from out of place"
        other = torch.full(shape, float("nan"), device=DEV)
        assert ops.volume_modulate(vol.to(DEV), h4.to(DEV), *GUIDE, out=other) is other and torch.equal(other, out.detach())
    n = vol.numel()
    big, view = _guarded(n, float("nan"))
    src, hd = vol.to(DEV), h4.to(DEV)
    ops._chk(ops._L().dca_volume_modulate(ops._ptr(src), ops._ptr(hd), ops._ptr(view), B, C, D, H, W, GUIDE[0],
                                          1.0 / (2 * GUIDE[1] ** 2), ops._stream()), "dca_volume_modulate")
    torch.cuda.synchronize()
    assert int(torch.isnan(view).sum()) == 0, "an element was not written"
    assert bool((big[:GUARD] == SENTINEL).all()) and bool((big[GUARD + n:] == SENTINEL).all()), "wrote outside the volume"
    assert torch.equal(view.view(shape), out.detach()), "the C entry differs from the op"


def test_volume_modulate_misaligned_takes_the_scalar_path():
    """W % 4 == 0 but the volume 4 bytes off alignment (C ABI only: `_req` clones such tensors): same bits"""
    ops = _ops()
    shape = B, C, D, H, W = (2, 4, 6, 5, 20)
    vol = seeded_tensor("gd.mod.mis", shape).to(DEV)
    h4 = torch.from_numpy(hint_map(B, H, W, D, "mixed")).to(DEV)
    want = ops.volume_modulate(vol, h4)
    buf = torch.full((vol.numel() + 8,), SENTINEL, device=DEV)
    v = buf[1:1 + vol.numel()]
    v.copy_(vol.view(-1))
    assert v.data_ptr() % 16 == 4
    ops._chk(ops._L().dca_volume_modulate(ops._ptr(v), ops._ptr(h4), ops._ptr(v), B, C, D, H, W, 10.0, 0.5, ops._stream()),
             "dca_volume_modulate")
    torch.cuda.synchronize()
    assert torch.equal(v.view(shape), want) and buf[0].item() == SENTINEL and bool((buf[1 + vol.numel():] == SENTINEL).all())


def test_volume_modulate_refuses():
    ops = _ops()
    vol, h4 = torch.zeros(1, 2, 4, 3, 8, device=DEV), torch.zeros(1, 3, 8, device=DEV)
    for bad in (lambda: ops.volume_modulate(vol, h4[:, :2]), lambda: ops.volume_modulate(vol, h4.double()),
                lambda: ops.volume_modulate(vol, h4, k=-1.0), lambda: ops.volume_modulate(vol, h4, c=0.0),
                lambda: ops.volume_modulate(vol, h4, k=float("inf")), lambda: ops.volume_modulate(vol, h4.requires_grad_()),
                lambda: ops.volume_modulate(vol, h4.detach(), out=torch.zeros(1, device=DEV)),
                lambda: ops.volume_modulate(vol, h4.detach().cpu())):
        with pytest.raises(RuntimeError, match="volume_modulate"):
            bad()


# ---- the fused builder ---------------------------------------------------------------------------------------------------
def guided_reference(h4):
    def call(case, t):
        vol = V.reference(case, t)
        return vol * factor(vol.shape[2], h4, vol.dtype)[:, None]
    return call


def guided_op(ops, h4dev):
    def call(case, t):
        G, D = case.shape[2], case.shape[5]
        one = len(t["L"]) == 1
        cl, cr = (t["cl"][0], t["cr"][0]) if "cl" in t else (None, None)
        dtype = torch.float32 if V.has_grads(case) else V.LP[case.p["dtype"]][0]
        return ops.cost_volume(t["L"][0] if one else tuple(t["L"]), t["R"][0] if one else tuple(t["R"]), D, G, cl, cr,
                               out_dtype=dtype, hints4=h4dev, guide=GUIDE)
    return call


FUSED = [(c, v) for c in V.FUSED for v in ("rows", "mixed")]


def _report_bits(cid, what, a, b):
    """prints how far two fp32 tensors that should be equal bit for bit are apart: elements that differ, the largest
    difference over max(1, max |b|) and in units of the last place of b"""
    a, b = a.detach().double().flatten(), b.detach().double().flatten()
    diff = (a - b).abs()
    ulp = torch.ldexp(torch.ones_like(b), torch.frexp(b.abs().clamp_min(2.0 ** -126))[1] - 24)
    n = int((diff > 0).sum())
    print(f"  {cid}: {what}: {n} of {a.numel()} elements differ, max {diff.max().item() / max(1.0, b.abs().max().item()):.2e} "
          f"relative to the maximum, {(diff / ulp).max().item():.1f} ulp")


def _zero_half_plane(cid, vol):
    D, W = vol.shape[2], vol.shape[4]
    for d in range(1, D):
        assert not bool(vol[:, :, d, :, :min(d, W)].any()), f"{cid}: x < d must be exactly 0 (d = {d})"


@pytest.mark.parametrize("case,variant", FUSED, ids=[f"{c.id}-{v}" for c, v in FUSED])
def test_cost_volume_guided_fused(case, variant, monkeypatch):
    """the four fused rows under two hint maps: x < d exactly 0, the fp64 gate of the forward and of every gradient (2-byte
    volumes: element by element beyond half an ulp of the storage type), the per-row maxima of the products, and -- last,
    after everything else has been checked -- bit for bit the unguided fused volume followed by `ops.volume_modulate`.

    That last comparison bites: with the factor multiplied straight onto the sums the compiler fused other products of the
    correlation sums than in the unguided kernel, and 50 018 of 921 600 elements of the CPG 8 rows differed (1.7e-7 of the
    maximum), 34 369 of them in cells without a hint."""
    ops = _ops()
    _flags(monkeypatch, ops)
    B, C, G, H, W, D = case.shape
    cid = f"{case.id}-{variant}"
    h4 = torch.from_numpy(hint_map(B, H, W, D, variant))
    assert bool((h4[:, 0] > 0).all()) == (variant == "rows") and bool((h4 == 0.25).any()) and bool((h4 == D - 1).any())
    h4dev = h4.to(DEV)
    ref = V.evaluate(case, torch.float64, call=guided_reference(h4))[0]
    f32 = V.evaluate(case, torch.float32, call=guided_reference(h4))[0]
    yard = {k: V.error(f32[k], ref[k]) for k in ref}
    got, out = V.evaluate(case, torch.float32, DEV, guided_op(ops, h4dev))
    torch.cuda.synchronize()
    print(f"{cid}: {case.branch}")
    _zero_half_plane(cid, out.detach())
    if not V.has_grads(case):
        lp, half_ulp = V.LP[case.p["dtype"]]
        assert out.dtype == lp and out.shape == (B, G, D, H, W)
        want, v = ref["fwd"], out.detach().cpu().double()
        assert torch.isfinite(v).all()
        tol = V.gate(yard["fwd"])
        excess = (v - want).abs() - half_ulp * want.abs()
        e = max(0.0, excess.max().item()) / max(1.0, want.abs().max().item())
        print(f"  fwd: yardstick {yard['fwd']:.2e}  error beyond half an ulp of {case.p['dtype']} {e:.2e}  gate {tol:.2e}")
        assert e <= tol, (cid, e, tol)
        return
    assert type(out.grad_fn).__name__ == "_CostVolumeBackward", "not on the fused builder"
    sib = {"fwd": None, "concat": None, "d L": 1e-5, "d R": 1e-5, "d cl": 1e-6, "d cr": 1e-6}
    failures = []
    for name, want in ref.items():
        assert got[name].dtype == torch.float32 and got[name].shape == want.shape and torch.isfinite(got[name]).all(), name
        e, tol = V.error(got[name], want), V.gate(yard[name])
        print(f"  {name}: |ref|max {want.abs().max().item():.3e}  yardstick {yard[name]:.2e}  error {e:.2e}  gate {tol:.2e}")
        if e > tol:
            failures.append(f"{name}: {e:.3e} > max(4 x {yard[name]:.3e}, 2^-22)")
        if sib[name] is not None and e > sib[name]:
            failures.append(f"{name}: {e:.3e} > the sibling's {sib[name]:.0e}")
    assert not failures, f"{cid}: " + "; ".join(failures)
    # ONE definition of the factor: bit for bit the unguided fused volume followed by the stand-alone pass
    with torch.no_grad():
        t, _ = V.inputs(case)
        t = {k: [x.to(DEV) for x in v] for k, v in t.items()}
        plain = V.public_op(ops)(case, t)
        assert type(plain.grad_fn).__name__ != "_VolumeModulateBackward"
        two = ops.volume_modulate(plain, h4dev, *GUIDE)
    none = (h4 <= 0)[:, None, None].expand(out.shape)
    if case.p["Cc"] == 0:
        tag = ops._tag_ok(out, "_dca_cmax")
        assert tag is not None, f"{cid}: no valid _dca_cmax on the guided volume"
        slots, nslots, _ = tag
        assert nslots == B * H
        s = slots.view(torch.float32).view(G, ops.CSLOTS)[:, :nslots]
        want = out.detach().abs().amax((2, 4)).permute(1, 0, 2).reshape(G, B * H)
        bad = (s != want).nonzero().tolist()
        assert not bad, f"{cid}: emitted row maxima differ from max |guided volume| at (g, b * H + y) = {bad[:6]}"
        unguided = plain.abs().amax((2, 4)).permute(1, 0, 2).reshape(G, B * H)
        assert bool((want != unguided).any()), "the hints do not move any row maximum: the vmax check says nothing"
    _report_bits(cid, "fused vs unguided + volume_modulate", out.detach(), two)
    _report_bits(cid, "cells without a hint vs the unguided volume", out.detach()[none.to(DEV)], plain[none.to(DEV)])
    assert torch.equal(two, out.detach()), f"{cid}: the fused route differs from unguided + volume_modulate"
    assert torch.equal(out.detach()[none.to(DEV)], plain[none.to(DEV)])


def test_guided_fused_two_calls_are_bit_identical(monkeypatch):
    ops = _ops()
    _flags(monkeypatch, ops)
    case = max(V.FUSED, key=V.volume_numel)
    B, C, G, H, W, D = case.shape
    h4dev = torch.from_numpy(hint_map(B, H, W, D, "rows")).to(DEV)
    (a, _), (b, _) = (V.evaluate(case, torch.float32, DEV, guided_op(ops, h4dev)) for _ in range(2))
    assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)


FALLBACK = [(2, 32, 4, 5, 18, 6), (1, 8, 2, 3, 16, 6)]          # W % 4 != 0; fp32 with D % 4 != 0


@pytest.mark.parametrize("shape", FALLBACK, ids=["W18", "D6"])
def test_fallback_routing(shape):
    """the shapes the fused builder does not take: `_GwcVolume` (+ `_ConcatVolume`) and the stand-alone pass, same gate"""
    ops = _ops()
    B, C, G, H, W, D = shape
    Cc = 2
    tag = "gd.fb." + "x".join(map(str, shape))
    cpu = {k: seeded_tensor(f"{tag}.{k}", (B, C if k in "LR" else Cc, H, W)) for k in ("L", "R", "cl", "cr")}
    seed = seeded_tensor(tag + ".g", (B, G + 2 * Cc, D, H, W)) * float(C // G)
    h4 = torch.from_numpy(hint_map(B, H, W, D, "rows"))

    def run(dtype):
        t = {k: v.to(dtype).requires_grad_() for k, v in cpu.items()}
        vol = torch.cat((O.build_gwc_volume(t["L"], t["R"], D, G), O.build_concat_volume(t["cl"], t["cr"], D)), 1)
        vol = vol * factor(D, h4, dtype)[:, None]
        grads = torch.autograd.grad((vol * seed.to(dtype)).sum(), list(t.values()))
        return {"fwd": vol.detach(), **{f"d {k}": g for k, g in zip(t, grads)}}

    ref, f32 = run(torch.float64), run(torch.float32)
    t = {k: v.to(DEV).requires_grad_() for k, v in cpu.items()}
    out = ops.cost_volume(t["L"], t["R"], D, G, t["cl"], t["cr"], hints4=h4.to(DEV), guide=GUIDE)
    assert type(out.grad_fn).__name__ == "_VolumeModulateBackward", type(out.grad_fn).__name__
    grads = torch.autograd.grad((out * seed.to(DEV)).sum(), list(t.values()))
    got = {"fwd": out.detach(), **{f"d {k}": g for k, g in zip(t, grads)}}
    _zero_half_plane(tag, out.detach())
    sib = {"fwd": None, "d L": 1e-5, "d R": 1e-5, "d cl": 1e-6, "d cr": 1e-6}
    for name, want in ref.items():
        y, e = V.error(f32[name], want), V.error(got[name], want)
        print(f"  {tag} {name}: yardstick {y:.2e}  error {e:.2e}  gate {V.gate(y):.2e}")
        assert e <= V.gate(y) and (sib[name] is None or e <= sib[name]), (name, e, y)


def test_reduced_precision_guided_needs_w_multiple_of_4():
    ops = _ops()
    f = torch.zeros(1, 8, 3, 18, device=DEV)
    with pytest.raises(RuntimeError, match="reduced-precision volume needs W % 4 == 0"):
        ops.cost_volume(f, f, 8, 2, out_dtype=torch.float16, hints4=torch.zeros(1, 3, 18, device=DEV))
    with pytest.raises(RuntimeError, match="cost_volume: hints4 must be"):
        ops.cost_volume(f, f, 8, 2, hints4=torch.zeros(1, 3, 16, device=DEV))


# ---- the model -----------------------------------------------------------------------------------------------------------
_MODELS = {}


def _model(concat):
    """one seeded GwcNet(32) per volume mode for the whole module (eval mode unless a test says otherwise and puts it back)"""
    if concat not in _MODELS:
        from dcanet_amd.models.gwcnet_dca_g import GwcNet
        m = GwcNet(32, use_concat_volume=concat)
        m.load_state_dict(O.seeded_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}), strict=True)
        _MODELS[concat] = m.to(DEV).eval()
    return _MODELS[concat]


def _images(hw=(32, 64)):
    return seeded_tensor("smoke.left", (1, 3) + hw).to(DEV), seeded_tensor("smoke.right", (1, 3) + hw).to(DEV)


def _full_hints(hw, seed, share=0.3, maxdisp=32):
    rng = np.random.default_rng(seed)
    h = (rng.random((1,) + hw) * (maxdisp - 1) + 0.5).astype(np.float32)
    h[rng.random(h.shape) > share] = 0
    return torch.from_numpy(h).to(DEV)


def _hot_args(model, left, right):
    fl, fr = model.feature_extraction(left), model.feature_extraction(right)
    args = [fl["gwc_segments"], fr["gwc_segments"]]
    if model.use_concat_volume:
        args += [fl["concat_feature"], fr["concat_feature"]]
    return args


@pytest.mark.parametrize("concat", [False, True])
def test_model_forward_with_hints(concat, monkeypatch):
    ops = _ops()
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)      # MIOpen convolutions of the 2D networks
    model = _model(concat)
    left, right = _images()
    hints = _full_hints((32, 64), 1)
    with torch.no_grad():
        plain, prob = model(left, right)
        guided, _ = model(left, right, hints=hints)
        assert guided.shape == plain.shape and torch.isfinite(guided).all()
        assert not torch.equal(guided, plain), "the hints change nothing"
        assert torch.equal(model.predict(left, right, hints=hints)["disp"], guided), "predict(hints=) is not forward(hints=)"
        assert torch.equal(model.predict(left, right)["disp"], plain)
        args = _hot_args(model, left, right)
        hints4 = ops.hints_to_quarter(hints, (32, 64), maxdisp=model.maxdisp)
        assert hints4.shape == (1, 8, 16) and int((hints4 > 0).sum()) > 8
        hot = model.hot_path(*args, hints4=hints4)
        assert torch.equal(model.prop(model.guidance(left)["g"], hot["pred4_q"]), guided)
    with pytest.raises(RuntimeError, match="hints must be"):
        model(left, right, hints=torch.zeros(1, 32, 60, device=DEV))


@pytest.mark.parametrize("concat", [False, True])
def test_model_zero_hints_are_no_hints(concat, monkeypatch):
    """forward(left, right, hints=zeros) is forward(left, right) bit for bit: every factor is exactly 1.

    Bites on the correlation sums: a GUIDED instantiation that rounded them at other places than the unguided one gave 1292
    of 2048 pixels off by up to 3.6e-7 of the maximum (G), 1851 by 1.3e-6 (GC); see test_cost_volume_guided_fused."""
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    model = _model(concat)
    left, right = _images()
    with torch.no_grad():
        plain, prob = model(left, right)
        zero, prob0 = model(left, right, hints=torch.zeros(1, 32, 64, device=DEV))
    _report_bits(f"concat={concat}", "forward(hints=zeros) vs forward()", zero, plain)
    assert torch.equal(zero, plain) and torch.equal(prob0, prob), "hints = zeros is not forward(left, right) bit for bit"


@pytest.mark.parametrize("concat", [False, True])
def test_model_is_the_composition_of_the_public_ops(concat, monkeypatch):
    """hot_path(hints4=) against the composition through public ops, bit for bit: the unguided volume, then the stand-alone
    pass, then the network module by module.  (`ops.volume_modulate` hands on no per-row maxima; the first convolution then
    takes them in a read pass of its own, and a maximum does not depend on the order it is taken in.)

    Replay against eager: test_graphed_hot_path_with_hints."""
    ops = _ops()
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    model = _model(concat)
    left, right = _images()
    hints = _full_hints((32, 64), 1)
    with torch.no_grad():
        args = _hot_args(model, left, right)
        hints4 = ops.hints_to_quarter(hints, (32, 64), maxdisp=model.maxdisp)
        hot = model.hot_path(*args, hints4=hints4)
        volume = ops.cost_volume(args[0], args[1], model.maxdisp // 4, model.num_groups, *(args[2:] or [None, None]))
        volume = ops.volume_modulate(volume, hints4, *GUIDE)
        cost0 = model.dres1(model.dres0(volume))
        _, out1 = model.cva1(cost0, res_post=cost0)
        _, out2 = model.cva2(out1)
        _, out3 = model.cva3(out2)
        composed = ops.softargmin(model.classif3(out3).squeeze(1))
    _report_bits(f"concat={concat}", "hot_path(hints4=) vs the composition", hot["pred4_q"], composed)
    assert torch.equal(composed, hot["pred4_q"]), "hot_path(hints4=) is not the composition of the public ops"


@pytest.mark.parametrize("concat", [False, True])
def test_model_trains_through_the_guided_volume(concat, monkeypatch):
    from dcanet_amd.models.gwcnet_dca_g import GwcNet
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    model = GwcNet(32, use_concat_volume=concat)
    model.load_state_dict(O.seeded_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}), strict=True)
    model = model.to(DEV).train()
    left, right = _images()
    hints = _full_hints((32, 64), 2)
    aux, (pred3, pred4) = model(left, right, hints=hints)
    (pred4.sum() + pred3.mean() + sum(a.square().mean() for a in aux)).backward()
    torch.cuda.synchronize()
    assert not hints.requires_grad and hints.grad is None
    missing = [n for n, p in model.named_parameters() if p.grad is None or not torch.isfinite(p.grad).all()]
    assert not missing, f"no finite gradient for {missing[:5]}"
    fe = model.feature_extraction.firstconv[0][0].weight.grad if hasattr(model.feature_extraction, "firstconv") else None
    assert fe is None or fe.abs().sum() > 0, "no gradient reached the feature extractor"


def test_launches_without_hints_are_what_they_were(monkeypatch):
    """hints=None: the launch list is forward(left, right)'s, entry by entry, and names none of the guided entry points; with
    hints it is that list with the builder's call replaced and one dca_hints_to_quarter in front"""
    from dcanet_amd import guided, ops
    from _recorder import Recorder
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    model = _model(False)
    left, right = _images()
    hints = _full_hints((32, 64), 1)

    def record(**kw):
        rec = Recorder(real=ops._L())
        with monkeypatch.context() as mp:
            mp.setattr(ops, "_L", lambda: rec)
            mp.setattr(guided, "_L", lambda: rec)
            with torch.no_grad():
                model(left, right, **kw)
        return rec.calls

    base, none, guided = record(), record(hints=None), record(hints=hints)
    assert base == none
    names = [c[0] for c in base]
    assert not {"dca_hints_to_quarter", "dca_volume_modulate", "dca_cost_volume_guided_fwd"} & set(names)
    assert names.count("dca_cost_volume_fwd") == 1
    gnames = [c[0] for c in guided]
    assert gnames[0] == "dca_hints_to_quarter"
    assert gnames[1:] == ["dca_cost_volume_guided_fwd" if n == "dca_cost_volume_fwd" else n for n in names]
    i = names.index("dca_cost_volume_fwd")
    assert guided[1 + i][1] == base[i][1][:-1] + [1, 10.0, 0.5, base[i][1][-1]]


# ---- graph and wrapper -----------------------------------------------------------------------------------------------------
def test_graphed_hot_path_with_hints(monkeypatch):
    from dcanet_amd.graph import GraphedHotPath
    ops = _ops()
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    model = _model(False)
    left, right = _images()
    with torch.no_grad():
        args = _hot_args(model, left, right)
        maps = [ops.hints_to_quarter(_full_hints((32, 64), s), (32, 64), maxdisp=32) for s in (5, 6)]
        assert not torch.equal(maps[0], maps[1])
        eager = [{k: v.clone() for k, v in model.hot_path(*args, hints4=m).items()} for m in maps]
        assert not torch.equal(eager[0]["pred4_q"], eager[1]["pred4_q"])
        graphed = GraphedHotPath(model, *args, hints4=maps[0])
        for m, want in zip(maps + maps[:1], eager + eager[:1]):      # the second replay must not see the first map
            got = graphed(*args, hints4=m)
            assert set(got) == set(want)
            for k in want:
                assert torch.equal(got[k], want[k]), f"replay differs from eager in {k}"
        with pytest.raises(AssertionError):
            graphed(*args)
        with pytest.raises(AssertionError):
            GraphedHotPath(model, *args)(*args, hints4=maps[0])


def _frame_case(seed):
    rng = np.random.default_rng(seed)
    left, right = (rng.integers(0, 256, (100, 300, 3), dtype=np.uint8) for _ in range(2))
    hints = (rng.random((100, 300)) * 30 + 0.5).astype(np.float32)
    hints[rng.random(hints.shape) > 0.05] = 0
    return left, right, hints


def test_kitti_inference_guided(monkeypatch):
    """a 100 x 300 image in a 128 x 320 frame (bottom-left, dst_y0 = 28): graph and eager agree bit for bit and equal
    model.forward on the hand-padded inputs with the hand-placed hint map; stream over three triples = three calls"""
    from dcanet_amd.inference import KittiInference, KittiInferenceGuided, normalize_pair, pad_or_crop, placement
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    model = _model(False)
    triples = [_frame_case(s) for s in (21, 22, 23)]
    left, right, hints = triples[0]
    assert placement(100, 300, 128, 320) == (0, 28, 100, 300)
    res = {}
    for graph in (True, False):
        infer = KittiInferenceGuided(model, crop_height=128, crop_width=320, graph=graph)
        res[graph] = infer(left, right, hints)
        assert res[graph].shape == (100, 300) and res[graph].dtype == np.float32
        dev_hints = infer(left, right, torch.from_numpy(hints).to(DEV))
        assert dev_hints.tobytes() == res[graph].tobytes(), "a device hint map gives another frame than the numpy one"
        if graph:
            single = [infer(*t) for t in triples]
            assert not np.array_equal(single[0], single[1])
            got = list(infer.stream(iter(triples), depth=2))
            assert len(got) == 3 and all(g.tobytes() == s.tobytes() for g, s in zip(got, single)), "stream != single calls"
    assert res[True].tobytes() == res[False].tobytes(), "graph and eager differ"
    plain = KittiInference(model, crop_height=128, crop_width=320, graph=False, device_io=True)(left, right)
    assert not np.array_equal(plain, res[False]), "the hints change nothing"
    # by hand: the device frames are what the plain wrapper builds; here the host's normalisation, which the existing tests
    # show equal on these images or not -- so take the frames from the wrapper itself
    infer = KittiInferenceGuided(model, crop_height=128, crop_width=320, graph=False)
    infer(left, right, hints)
    fl, fr = infer._frames[0:1].clone(), infer._frames[1:2].clone()
    L, R, h, w = pad_or_crop(normalize_pair(left, right), 128, 320)
    assert (h, w) == (100, 300) and L.shape == fl.shape
    placed = torch.zeros(1, 128, 320)
    placed[0, 28:, :300] = torch.from_numpy(hints)
    with torch.no_grad():
        want = model(fl, fr, hints=placed.to(DEV))[0]
    assert want[0, 0, 28:, :300].cpu().numpy().tobytes() == res[False].tobytes(), "not model.forward on the hand-placed hints"


def test_kitti_inference_guided_from_a_scan(monkeypatch):
    """lidar=: the route fed with a 200-point scan equals the route fed with ops.lidar_disparity's map"""
    import _lidar_reference as LR
    from dcanet_amd.inference import KittiInferenceGuided
    ops = _ops()
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    model = _model(False)
    left, right, _ = _frame_case(31)
    calib = LR.calib_for((100, 300))
    scan = LR.random_points(calib, 200, seed=5, zrange=(12.0, 60.0))
    disp = ops.lidar_disparity(torch.from_numpy(scan).to(DEV), calib)["disp"]
    assert disp.shape == (100, 300) and int(((disp > 0) & (disp < model.maxdisp)).sum()) > 20, "the scan gives too few hints"
    for graph in (False, True):
        by_map = KittiInferenceGuided(model, crop_height=128, crop_width=320, graph=graph)(left, right, disp)
        by_scan = KittiInferenceGuided(model, crop_height=128, crop_width=320, graph=graph, lidar=calib)(left, right, scan)
        assert by_scan.tobytes() == by_map.tobytes(), f"graph={graph}: the scan route differs from the map route"
