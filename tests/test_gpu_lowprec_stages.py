"""The reduced-precision inference path (ops.reduced_precision(bf16 | fp16)) stage by stage against fp64, teacher-forced.

A free-running fp64 reference of this path cannot be sharp: a 1e-7 difference in summation order flips one 2-byte
rounding and the flip travels through forty layers.  So every stage -- one stored tensor of the path -- is compared with
an fp64 evaluation of that stage alone, fed the GPU's OWN input tensors for it, each operand rounded where the GPU path
rounds it (tests/_lp_reference.py).  Then only the summation order and the final store differ, and the kernel-level gates
the project already uses apply.  The reference takes weights, BatchNorm buffers, slopes and residuals from the state dict
along oracle/dcanet_oracle.py, never from what the GPU code handed to its kernels: a wrong affine, slope, residual or
operand order fails the stage it belongs to (tests/test_lp_reference_cpu.py shows that each such mistake misses its gate
by at least 10x, and that the restatement without rounding equals the oracle's hot path to 1e-10).

Stages, in order (2 = stored in the 2-byte type, 4 = fp32):
    volume 2, dres0.a 2, dres0 2, dres1.a 2, cost0 2,
    cva{1,2,3}.: pooled 4, cost_down 4, h 4, prob 4, aug_down 4, aug 2, fused 2, c1 4, c2 4, skip 2, out 2,
    classif3.h 2, logits3 4, pred4_q 4.
Capture: one m.eval().hot_path(...) under torch.no_grad() and ops.reduced_precision(lp); forward hooks on the ConvBn3d,
_Classify, slc_net, cva, _Dres0 and _Dres1 modules, recording wrappers around the ops.*_lp functions that cva._forward_lp
calls directly and around ops.context_inject (k*).  Every stage must be captured exactly once, in its listed type.

Gates, per element, scale = max(1, |ref|max), ulp(bf16) = 2^-8, ulp(fp16) = 2^-11 (tests/test_gpu_lowprec.py):
    fp32 result of a convolution stage     2e-5 x scale                        test_gpu_lowprec.py (test_conv3d_s2_lp)
    2-byte result of a convolution stage   2e-5 x scale + ulp x |ref|          test_gpu_lowprec.py (test_conv3d_lp)
    pooled                                 1e-6 x scale                        test_gpu_parity.py test_avgpool
    aug                                    2e-6 x scale + ulp x |ref|          test_gpu_parity.py test_trilinear
    aug_down                               2e-5 x scale, and k* equal          test_gpu_parity.py test_golden_attention_block
    pred4_q                                2e-6 x scale                        test_gpu_parity.py test_softargmin
    volume                                 2e-6 x scale + ulp x |ref|          test_gpu_parity.py test_gwc_volume (the 2-byte
                                           volume is the fp32 one rounded: test_cost_volume_fused_reduced_precision)

Cases (tests/_lp_reference.py CASES; W4 % 4 == 0 and a 1/8-res voxel count divisible by 4, which the path requires):
    A-g    features (2, 320, 16, 32), maxdisp 32: 1/8-res 4 x 8 x 16, the shape of the hot_path goldens
    B-g    features (1, 320, 10, 24), maxdisp 40: 1/8-res 5 x 5 x 12, odd depth and height, partial tiles
    B-gc   the same with 12 concat channels: dres0 reads 64 channels
Seed tags: A-g "a0", B-g and B-gc "b0" (seeded_tensor("lpst.<tag>.fL" / ".fR")); the arg-max margin of these seeds is
checked in tests/test_lp_reference_cpu.py.

Free-running context (printed, NOT gated: rounding flips make it a statistic): max |pred4_q_gpu - pred4_q_ref| with the
restatement free-running in the same type, measured on an MI355X:
    case    bf16        fp16
    A-g     2.895e-02   5.532e-03
    B-g     3.246e-02   5.654e-03
    B-gc    9.343e-02   1.114e-02
(1/4-res pixels, on a disparity range of 0..7 / 0..9: about a hundred and ten times the unit roundoff of the type, which
is what forty layers of rounding flips add up to and why only the teacher-forced stages are gated.)
"""
import numpy as np
import pytest
import torch

from _lp_reference import CASES, LP_STORED, STAGES, case_inputs, gate, hot_path_lp, kstar

pytestmark = pytest.mark.gpu
DEV = "cuda"
LPS = [torch.bfloat16, torch.float16]


def _capture(m, ops, monkeypatch, lp, args):
    """run the reduced-precision hot path once; {stage: tensor}, {block: k*}, names captured more than once"""
    from dcanet_amd.models.augment.cva import cva as Cva
    got, ks, twice, state, handles = {}, {}, [], {"blk": None}, []

    def rec(name, t):
        assert isinstance(t, torch.Tensor), (name, type(t))
        if name in got:
            twice.append(name)
        got[name] = t.detach().clone()

    def hook(mod, fn):
        handles.append(mod.register_forward_hook(fn, with_kwargs=True))

    first = lambda o: o[0] if isinstance(o, tuple) else o          # alias=True returns (z, x)
    hook(m.dres0, lambda mod, a, kw, o: (rec("volume", a[0]), rec("dres0", o)) and None)
    hook(m.dres0[0], lambda mod, a, kw, o: rec("dres0.a", first(o)))
    hook(m.dres1[0], lambda mod, a, kw, o: rec("dres1.a", first(o)))
    hook(m.dres1, lambda mod, a, kw, o: rec("cost0", o))
    hook(m.classif3[0], lambda mod, a, kw, o: rec("classif3.h", first(o)))
    hook(m.classif3, lambda mod, a, kw, o: rec("logits3", o))
    for b in ("cva1", "cva2", "cva3"):
        blk = getattr(m, b)
        assert isinstance(blk, Cva)
        handles.append(blk.register_forward_pre_hook(lambda mod, a, b=b: state.update(blk=b)))
        hook(blk, lambda mod, a, kw, o, b=b: (rec(f"{b}.out", o[1]), state.update(blk=None)) and None)
        hook(blk.downsample[1], lambda mod, a, kw, o, b=b: rec(f"{b}.cost_down", o))
        hook(blk.classify[0], lambda mod, a, kw, o, b=b: rec(f"{b}.h", first(o)))
        hook(blk.classify, lambda mod, a, kw, o, b=b: rec(f"{b}.prob", o))
        hook(blk.slc_net, lambda mod, a, kw, o, b=b: rec(f"{b}.aug_down", o))
        hook(blk.cost_agg.conv2[0], lambda mod, a, kw, o, b=b: rec(f"{b}.c2", o))

    def wrap(name, stage_of):
        real = getattr(ops, name)

        def wrapper(*a, **kw):
            out = real(*a, **kw)
            stage = stage_of(a, kw)
            if state["blk"] is not None and stage is not None:      # outside a block: classif3's tap expansion
                rec(f"{state['blk']}.{stage}", out)
            return out
        monkeypatch.setattr(ops, name, wrapper)

    wrap("avg_pool3d_lp", lambda a, kw: "pooled")
    wrap("trilinear_up2_lp", lambda a, kw: "aug")
    wrap("conv1x1_lp", lambda a, kw: "skip" if kw.get("x2", a[3] if len(a) > 3 else None) is None else "fused")
    wrap("conv3d_s2_lp", lambda a, kw: "c1")
    real_inject = ops.context_inject

    def inject(x, preds):
        key, k = real_inject(x, preds)
        assert state["blk"] not in ks
        ks[state["blk"]] = k.detach().clone()
        return key, k
    monkeypatch.setattr(ops, "context_inject", inject)
    try:
        with torch.no_grad(), ops.reduced_precision(lp):
            rec("pred4_q", m.hot_path(*args)["pred4_q"])
        torch.cuda.synchronize()
    finally:
        for h in handles:
            h.remove()
    return got, ks, twice


@pytest.mark.parametrize("lp", LPS, ids=["bf16", "fp16"])
@pytest.mark.parametrize("cid", list(CASES))
def test_reduced_precision_stages_teacher_forced(cid, lp, monkeypatch, capsys):
    from dcanet_amd import ops
    from dcanet_amd.models.gwcnet_dca_g import GwcNet
    from oracle import dcanet_oracle as O
    sd, fL, fR, cL, cR, maxdisp = case_inputs(cid)
    m = GwcNet(maxdisp, use_concat_volume=CASES[cid][2])
    m.load_state_dict(O.seeded_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}), strict=True)
    m = m.to(DEV).eval()
    for k, v in sd.items():          # the reference's weights are the model's, key by key
        assert torch.equal(m.state_dict()[k].cpu(), v), k
    args = tuple(t.to(DEV) for t in (fL, fR, cL, cR) if t is not None)
    got, ks, twice = _capture(m, ops, monkeypatch, lp, args)
    assert not twice, f"captured more than once: {twice}"
    assert sorted(got) == sorted(STAGES), (sorted(set(STAGES) - set(got)), sorted(set(got) - set(STAGES)))
    assert sorted(ks) == ["cva1", "cva2", "cva3"], sorted(ks, key=str)
    for s in STAGES:
        assert got[s].dtype == (lp if s in LP_STORED else torch.float32), (s, got[s].dtype)
    forced = {s: t.cpu() for s, t in got.items()}
    with torch.no_grad():
        ref = hot_path_lp(sd, fL, fR, maxdisp, lp, cL, cR, forced=forced)
        freerun = hot_path_lp(sd, fL, fR, maxdisp, lp, cL, cR)
    dev = (forced["pred4_q"].double() - freerun["pred4_q"]).abs().max().item()
    rows, bad = [], []
    for s in STAGES:
        r, g = ref[s], forced[s].double()
        assert g.shape == r.shape, (s, g.shape, r.shape)
        err, lim = (g - r).abs(), gate(s, r, lp)
        i = int((err / lim).argmax())
        idx = tuple(int(v) for v in np.unravel_index(i, tuple(r.shape)))
        rows.append(f"   {s:16s} worst err/gate {(err / lim).flatten()[i].item():.3f}  (err {err.flatten()[i].item():.3e}, "
                    f"|ref| {r.abs().flatten()[i].item():.3e}, |ref|max {r.abs().max().item():.3e})")
        if not bool((err <= lim).all()):
            blk, _, name = s.rpartition(".")
            bad.append(f"stage {name} of block {blk or 'top level'}: err {err.flatten()[i].item():.3e} > gate "
                       f"{lim.flatten()[i].item():.3e} at {idx} (gpu {g.flatten()[i].item():.6e}, ref {r.flatten()[i].item():.6e})")
    for b in ("cva1", "cva2", "cva3"):
        kr = kstar(forced[f"{b}.prob"])
        kg = ks[b].cpu().view(kr.shape).long()
        if not torch.equal(kg, kr):
            bad.append(f"stage aug_down of block {b}: k* differs at {(kg != kr).sum().item()} of {kr.numel()} pixels")
    with capsys.disabled():
        print(f"\n[lp stages {cid} {str(lp)[6:]}] free-running max|pred4_q_gpu - pred4_q_ref| = {dev:.3e}")
        print("\n".join(rows))
    assert ref["pred4_q"].std() > 0.1, "degenerate case: flat disparity map"
    assert not bad, "\n".join(bad)
