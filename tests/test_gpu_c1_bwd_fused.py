"""Backward of a 1x1x1 convolution + BatchNorm as one launch (csrc/conv1_bwd_fused.hip, ops._c1_bwd_route) against fp64.

The fp64 reference is F.conv3d + F.batch_norm + F.leaky_relu on the CPU, differentiated by autograd.  Every case asserts
the route first (a spy on the entry point dca_conv1_bwd_fused; no ops._conv_sliced / ops._wgrad call with ksize 1 in the
backward), then compares dx, dx2, dw, dgamma, dbeta.  Gates are the unfused siblings' (tests/test_gpu_parity.py,
test_conv1x1_two_inputs / test_bn_act): close 2e-5 x scale for tensors, close_l2 1e-5 for dw.  Every case also runs the
split route (ops.C1_BWD_FUSE off: BatchNorm apply pass, backward-data, weight gradient) against the same reference and
prints both errors; where the split route itself exceeds a sibling gate, the gate of that quantity is twice the split
route's measured error.  The fused kernel keeps the split route's tiles, summation order and products (fp32 MFMA for dw,
the bf16x3 product of conv1_x3.hip for dx), so every gradient is also asserted bit-identical to the split route's."""
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle.seeded import seeded_tensor

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAMES = ("dx", "dx2", "dw", "dgamma", "dbeta")


def _ops():
    from dcanet_amd import ops
    return ops


def _max_err(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return (a - b).abs().max().item(), max(1.0, b.abs().max().item())


def _l2_err(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def gpu(t, grad=False):
    return t.detach().float().to(DEV).requires_grad_(grad)


# name: (C1, C2, Cout, slope, training, N, dims)
CASES = {
    "c32_full_and_partial_tile": (32, 0, 32, 1.0, True, 2, (4, 6, 12)),     # S = 288: one full and one partial tile per sample
    "two_inputs_partial_tile": (32, 32, 32, 1.0, True, 2, (3, 5, 12)),      # S = 180: a partial tile only
    "proj_leaky": (32, 0, 32, 0.1, True, 1, (4, 6, 10)),                    # a _ProjLayer: slope 0.1
    "eval_bn": (32, 0, 32, 1.0, False, 2, (4, 6, 12)),                      # eval-mode BatchNorm with grad enabled
    "pipeline": (32, 0, 32, 1.0, True, 3, (12, 34, 120)),                   # 576 tiles for at most 512 workgroups
    "pipeline_deep": (32, 0, 32, 1.0, True, 9, (12, 34, 120)),              # 1728 tiles: at least three per workgroup
    "pipeline_deep_two_inputs": (32, 32, 32, 1.0, True, 9, (12, 34, 120)),
}
FALLBACKS = {
    "s_not_multiple_of_4": (32, 0, 32, 1.0, True, 2, (3, 5, 9)),
    "c1_64": (64, 0, 32, 1.0, True, 2, (4, 6, 12)),
}


@functools.lru_cache(maxsize=None)
def _ref(name, with_pre=False):
    """inputs (fp32, CPU) and the fp64 gradients of loss = (act(BN(conv(x [, x2])) [+ res_pre]) * gz).sum()"""
    C1, C2, Cout, slope, training, N, dims = {**CASES, **FALLBACKS}[name]
    Cin = C1 + C2
    x = seeded_tensor(f"c1b.x.{name}", (N, C1) + dims)
    x2 = seeded_tensor(f"c1b.x2.{name}", (N, C2) + dims) if C2 else None
    w = seeded_tensor(f"c1b.w.{name}", (Cout, Cin, 1, 1, 1)) * (1.0 / Cin ** 0.5)
    gamma = torch.rand(Cout, generator=torch.Generator().manual_seed(11)) + 0.5
    beta = seeded_tensor(f"c1b.beta.{name}", (Cout,)) * 0.3        # u = gamma xhat + beta: both signs well populated
    rm = seeded_tensor(f"c1b.rm.{name}", (Cout,)) * 0.1
    rv = torch.rand(Cout, generator=torch.Generator().manual_seed(12)) + 0.5
    gz = seeded_tensor(f"c1b.gz.{name}", (N, Cout) + dims)
    rp = seeded_tensor(f"c1b.rp.{name}", (N, Cout) + dims) if with_pre else None
    xd, wd, gd, bd = (t.double().requires_grad_() for t in (x, w, gamma, beta))
    x2d = x2.double().requires_grad_() if C2 else None
    y = F.conv3d(xd if x2d is None else torch.cat([xd, x2d], 1), wd)
    u = F.batch_norm(y, rm.double().clone(), rv.double().clone(), gd, bd, training, 0.1, 1e-5)
    if with_pre:
        u = u + rp.double()
    z = F.leaky_relu(u, slope) if slope != 1.0 else u
    wrt = [xd] + ([x2d] if C2 else []) + [wd, gd, bd]
    grads = list(torch.autograd.grad((z * gz.double()).sum(), wrt))
    if not C2:
        grads.insert(1, None)
    return {"x": x, "x2": x2, "w": w, "gamma": gamma, "beta": beta, "rm": rm, "rv": rv, "gz": gz, "rp": rp,
            "grads": dict(zip(NAMES, grads)), "neg_share": (u < 0).double().mean().item()}


class _Spies:
    """counts the launches of the fused entry point and the 1x1x1 calls of the split route's two helpers"""

    def __init__(self, monkeypatch, ops):
        self.fused, self.sliced1, self.wgrad1 = [], [], []
        lib = ops._L()
        real_f, real_s, real_w = lib.dca_conv1_bwd_fused, ops._conv_sliced, ops._wgrad

        def spy_f(*args):
            self.fused.append((args[15], args[16], args[17], args[19]))      # N, C1, C2, S
            return real_f(*args)

        def spy_s(x, x2, w_src, A, B, K, src_ab, flip, ksize, *args, **kw):
            if ksize == 1:
                self.sliced1.append((A, B))
            return real_s(x, x2, w_src, A, B, K, src_ab, flip, ksize, *args, **kw)

        def spy_w(x, dy, dw, off, Cx, Cy, ksize, *args, **kw):
            if ksize == 1:
                self.wgrad1.append((Cx, Cy, off))
            return real_w(x, dy, dw, off, Cx, Cy, ksize, *args, **kw)
        monkeypatch.setattr(lib, "dca_conv1_bwd_fused", spy_f)
        monkeypatch.setattr(ops, "_conv_sliced", spy_s)
        monkeypatch.setattr(ops, "_wgrad", spy_w)

    def reset(self):
        del self.fused[:], self.sliced1[:], self.wgrad1[:]


def _modules(ref, name):
    C1, C2, Cout, slope, training, N, dims = {**CASES, **FALLBACKS}[name]
    conv = nn.Conv3d(C1 + C2, Cout, 1, bias=False).to(DEV)
    bn = nn.BatchNorm3d(Cout).to(DEV)
    with torch.no_grad():
        conv.weight.copy_(ref["w"])
        bn.weight.copy_(ref["gamma"]); bn.bias.copy_(ref["beta"])
        bn.running_mean.copy_(ref["rm"]); bn.running_var.copy_(ref["rv"])
    bn.train(training)
    return conv, bn


def _run(ops, ref, name, spies, with_pre=False):
    """one forward + backward through ops.convbn3d; returns the five gradients (dx2 None for one input) and the spy counts
    of the backward alone"""
    C1, C2, Cout, slope, training, N, dims = {**CASES, **FALLBACKS}[name]
    conv, bn = _modules(ref, name)
    xg = gpu(ref["x"], True)
    x2g = gpu(ref["x2"], True) if C2 else None
    rpg = gpu(ref["rp"]) if with_pre else None
    z = ops.convbn3d(xg, conv, bn, slope, res_pre=rpg, x2=x2g)
    spies.reset()
    wrt = [xg] + ([x2g] if C2 else []) + [conv.weight, bn.weight, bn.bias]
    grads = list(torch.autograd.grad((z * ref["gz"].to(DEV)).sum(), wrt))
    torch.cuda.synchronize()
    if not C2:
        grads.insert(1, None)
    counts = (list(spies.fused), list(spies.sliced1), list(spies.wgrad1))
    return dict(zip(NAMES, grads)), counts


def _errors(got, want):
    out = {}
    for nm in NAMES:
        if want[nm] is None:
            assert got[nm] is None
            continue
        out[nm] = (_l2_err(got[nm], want[nm]), 1e-5) if nm == "dw" else _max_err(got[nm], want[nm])
    return out


def _gate(nm, split_err):
    """the sibling's gate; twice the split route's error where the parent's code itself is over it"""
    if nm == "dw":
        sib = 1e-5
        return sib if split_err[nm][0] <= sib else 2 * split_err[nm][0]
    err, scale = split_err[nm]
    return 2e-5 * scale if err <= 2e-5 * scale else 2 * err


def _both_routes(name, monkeypatch, with_pre=False):
    ops = _ops()
    monkeypatch.setattr(ops, "_X3_MIN_WORKGROUPS", 1)
    ref = _ref(name, with_pre)
    spies = _Spies(monkeypatch, ops)
    monkeypatch.setattr(ops, "C1_BWD_FUSE", False)
    split, split_counts = _run(ops, ref, name, spies, with_pre)
    monkeypatch.setattr(ops, "C1_BWD_FUSE", True)
    fused, fused_counts = _run(ops, ref, name, spies, with_pre)
    return ops, ref, split, split_counts, fused, fused_counts


@pytest.mark.parametrize("name", list(CASES))
def test_fused_route_against_fp64(name, monkeypatch):
    C1, C2, Cout, slope, training, N, dims = CASES[name]
    S = dims[0] * dims[1] * dims[2]
    ops, ref, split, split_counts, fused, fused_counts = _both_routes(name, monkeypatch)
    # ---- routes
    assert split_counts[0] == [] and len(split_counts[1]) == (2 if C2 else 1) and len(split_counts[2]) == (2 if C2 else 1), split_counts
    assert fused_counts == ([(N, C1, C2, S)], [], []), fused_counts
    if slope != 1.0:
        assert 0.2 <= ref["neg_share"] <= 0.8, ref["neg_share"]
    # ---- values
    e_split, e_fused = _errors(split, ref["grads"]), _errors(fused, ref["grads"])
    for nm in e_fused:
        gate = _gate(nm, e_split)
        print(f"    {name} {nm}: fused {e_fused[nm][0]:.3e}, split {e_split[nm][0]:.3e}, gate {gate:.3e}")
    for nm in e_fused:
        assert e_fused[nm][0] <= _gate(nm, e_split), (name, nm, e_fused[nm][0], e_split[nm][0])
    # the BatchNorm's reduction is the same launch on both routes, dy the same expression: same bits, and the weight
    # gradient's tile-to-workgroup assignment and summation order are the split kernel's
    assert torch.equal(fused["dgamma"], split["dgamma"]) and torch.equal(fused["dbeta"], split["dbeta"])
    assert torch.equal(fused["dw"], split["dw"]), (fused["dw"] - split["dw"]).abs().max().item()
    # dx: the bf16x3 product of the backward-data launch it replaces, term for term
    assert torch.equal(fused["dx"], split["dx"]), (fused["dx"] - split["dx"]).abs().max().item()
    if C2:
        assert torch.equal(fused["dx2"], split["dx2"]), (fused["dx2"] - split["dx2"]).abs().max().item()
    if C2:      # both halves of dw at their offsets, both input gradients
        assert fused["dw"].shape == (Cout, C1 + C2, 1, 1, 1) and fused["dx2"].shape == ref["x2"].shape
        for lo, hi, nm in ((0, C1, "dw[:, :C1]"), (C1, C1 + C2, "dw[:, C1:]")):
            e = _l2_err(fused["dw"][:, lo:hi], ref["grads"]["dw"][:, lo:hi])
            print(f"    {name} {nm}: rel L2 {e:.3e}")
            assert e <= max(1e-5, 2 * _l2_err(split["dw"][:, lo:hi], ref["grads"]["dw"][:, lo:hi]))


def test_two_identical_calls_are_bit_identical(monkeypatch):
    ops = _ops()
    spies = _Spies(monkeypatch, ops)
    for name in ("c32_full_and_partial_tile", "two_inputs_partial_tile"):
        ref = _ref(name)
        a, ca = _run(ops, ref, name, spies)
        b, cb = _run(ops, ref, name, spies)
        assert len(ca[0]) == 1 and len(cb[0]) == 1
        for nm in NAMES:
            if a[nm] is not None:
                assert torch.equal(a[nm], b[nm]), (name, nm)


@pytest.mark.parametrize("name", list(FALLBACKS) + ["res_pre"])
def test_fallbacks_keep_the_split_route(name, monkeypatch):
    """shapes the fused kernel does not take, and a BatchNorm with res_pre: the split route, with the values it gives when
    the switch is off"""
    with_pre = name == "res_pre"
    case = "c32_full_and_partial_tile" if with_pre else name
    ops, ref, split, split_counts, fused, fused_counts = _both_routes(case, monkeypatch, with_pre)
    assert fused_counts[0] == [] and fused_counts == split_counts and len(fused_counts[2]) >= 1, fused_counts
    for nm in NAMES:
        if split[nm] is not None:
            assert torch.equal(fused[nm], split[nm]), (name, nm)
    e = _errors(fused, ref["grads"])
    for nm in e:
        print(f"    {name} {nm}: {e[nm][0]:.3e}")
        assert e[nm][0] <= (1e-5 if nm == "dw" else 2e-5 * e[nm][1]), (name, nm, e[nm])


def test_bn_act_on_a_leaf_is_unchanged(monkeypatch):
    """ops.bn_act called directly: its backward writes dy itself, whatever the switch says"""
    ops = _ops()
    spies = _Spies(monkeypatch, ops)
    ref = _ref("c32_full_and_partial_tile")
    y = seeded_tensor("c1b.leaf.y", ref["gz"].shape) * 1.7 + 0.3
    yd, gd, bd = (t.double().requires_grad_() for t in (y, ref["gamma"], ref["beta"]))
    zr = F.batch_norm(yd, None, None, gd, bd, True, 0.1, 1e-5)
    want = torch.autograd.grad((zr * ref["gz"].double()).sum(), [yd, gd, bd])
    got = {}
    for on in (False, True):
        monkeypatch.setattr(ops, "C1_BWD_FUSE", on)
        _, bn = _modules(ref, "c32_full_and_partial_tile")
        yg = gpu(y, True)
        z = ops.bn_act(yg, bn, 1.0)
        got[on] = torch.autograd.grad((z * ref["gz"].to(DEV)).sum(), [yg, bn.weight, bn.bias])
        assert not hasattr(got[on][0], "_dca_lazy")
    assert spies.fused == []
    for a, b, w, nm in zip(got[True], got[False], want, ("dy", "dgamma", "dbeta")):
        assert torch.equal(a, b), nm
        err, scale = _max_err(a, w)
        print(f"    leaf {nm}: {err:.3e}")
        assert err <= 2e-5 * scale, (nm, err)


def test_conv_pair_fused_second_branch(monkeypatch):
    """ops.convbn3d_pair (cost_agg.conv1 + cost_agg.redir): the fused launch serves the 1x1x1 branch, its dx enters the
    stride-2 branch's backward-data launch as res_post, and the shared input's gradient is fp64's sum of both branches"""
    ops = _ops()
    monkeypatch.setattr(ops, "_X3_MIN_WORKGROUPS", 1)
    monkeypatch.setattr(ops, "PAIR_FUSE", True)
    N, C, dims = 2, 32, (4, 8, 16)
    x = seeded_tensor("c1b.pair.x", (N, C) + dims)
    wa = seeded_tensor("c1b.pair.wa", (64, C, 3, 3, 3)) * (1.0 / (C * 27) ** 0.5)
    wb = seeded_tensor("c1b.pair.wb", (32, C, 1, 1, 1)) * (1.0 / C ** 0.5)
    ga, gb = torch.rand(64, generator=torch.Generator().manual_seed(21)) + 0.5, torch.rand(32, generator=torch.Generator().manual_seed(22)) + 0.5
    ba, bb = seeded_tensor("c1b.pair.ba", (64,)) * 0.3, seeded_tensor("c1b.pair.bb", (32,)) * 0.3
    xd, wad, wbd, gad, gbd, bad, bbd = (t.double().requires_grad_() for t in (x, wa, wb, ga, gb, ba, bb))
    za = F.relu(F.batch_norm(F.conv3d(xd, wad, None, 2, 1), None, None, gad, bad, True, 0.1, 1e-5))
    zb = F.batch_norm(F.conv3d(xd, wbd), None, None, gbd, bbd, True, 0.1, 1e-5)
    gza, gzb = seeded_tensor("c1b.pair.gza", za.shape), seeded_tensor("c1b.pair.gzb", zb.shape)
    want = torch.autograd.grad((za * gza.double()).sum() + (zb * gzb.double()).sum(), [xd, wad, wbd, gbd, bbd])
    spies = _Spies(monkeypatch, ops)
    res = {}
    for on in (False, True):
        monkeypatch.setattr(ops, "C1_BWD_FUSE", on)
        conv_a, conv_b = nn.Conv3d(C, 64, 3, 2, 1, bias=False).to(DEV), nn.Conv3d(C, 32, 1, bias=False).to(DEV)
        bn_a, bn_b = nn.BatchNorm3d(64).to(DEV).train(), nn.BatchNorm3d(32).to(DEV).train()
        with torch.no_grad():
            conv_a.weight.copy_(wa); conv_b.weight.copy_(wb)
            bn_a.weight.copy_(ga); bn_a.bias.copy_(ba); bn_b.weight.copy_(gb); bn_b.bias.copy_(bb)
        xg = gpu(x, True)
        ya, yb = ops.convbn3d_pair(xg, conv_a, bn_a, 0.0, conv_b, bn_b, 1.0)
        assert type(yb.grad_fn).__name__ == "_BnActBackward" and type(ya.grad_fn).__name__ == "_BnActBackward"
        spies.reset()
        res[on] = torch.autograd.grad((ya * gza.to(DEV)).sum() + (yb * gzb.to(DEV)).sum(),
                                      [xg, conv_a.weight, conv_b.weight, bn_b.weight, bn_b.bias])
        torch.cuda.synchronize()
        if on:
            assert spies.fused == [(N, 32, 0, dims[0] * dims[1] * dims[2])] and spies.sliced1 == [] and spies.wgrad1 == []
        else:
            assert spies.fused == [] and len(spies.sliced1) == 1 and len(spies.wgrad1) == 1
    for i, nm in enumerate(("dx", "dwa", "dwb", "dgamma_b", "dbeta_b")):
        if nm in ("dwa", "dwb"):
            es, ef, sib = _l2_err(res[False][i], want[i]), _l2_err(res[True][i], want[i]), 1e-5
        else:
            (es, scale), (ef, _) = _max_err(res[False][i], want[i]), _max_err(res[True][i], want[i])
            sib = 2e-5 * scale
        gate = sib if es <= sib else 2 * es
        print(f"    pair {nm}: fused {ef:.3e}, split {es:.3e}, gate {gate:.3e}")
        assert ef <= gate, (nm, ef, es)
    for i, nm in enumerate(("dx", "dwa", "dwb", "dgamma_b", "dbeta_b")):
        assert torch.equal(res[True][i], res[False][i]), f"{nm}: same tiles, same order, same products, same bits"
