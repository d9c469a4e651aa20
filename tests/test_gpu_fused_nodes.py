"""The fused autograd nodes and the fused cost-volume builder against fp64.

tests/test_gpu_parity.py gates every kernel through its UNFUSED op; the launches the shipped training / eval path takes at
its fused seams are gated here, each at the tolerance of its unfused sibling (the fusion adds one fp32 addition):

  fused form                                                    sibling (unfused)        gates
  ops._Conv3d(alias=True), ops.convbn3d(alias=True)             test_conv3d              close 1e-5 y / dx; dw close_l2 1e-5, close 2e-5
  ops._ConvPair, ops.convbn3d_pair, Multi_Aggregation           test_conv3d              the same
  ops._PoolFork, ops.avg_pool3d_fork                            test_avgpool             close 1e-6
  ops.cost_volume / ops._CostVolume (csrc/volume_fused.hip)     test_gwc_volume          2e-6 forward, 1e-5 gradients
                                                                test_concat_volume       exact forward, 1e-6 gradients

Every reference is a float64 PyTorch graph on the CPU in which the shared tensor really has several consumers, differentiated
by autograd.  Every case asserts the kernel route it is on (the eligibility predicates of ops.py, the gradient object a
_GradProbe / a spy on ops._conv_sliced sees, the autograd node that built the result) before it compares, and prints its
measured errors."""
import ctypes
import functools
import itertools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import dcanet_oracle as O
from oracle.seeded import seeded_tensor

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _ops():
    from dcanet_amd import ops
    return ops


def _err(a, b):
    a, b = torch.as_tensor(a).detach().cpu().double(), torch.as_tensor(b).detach().cpu().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return a, b


def close(a, b, tol=2e-5, name=""):
    a, b = _err(a, b)
    err = (a - b).abs().max().item()
    scale = max(1.0, b.abs().max().item())
    print(f"    {name}: max err {err:.3e} (scale {scale:.3e}, gate {tol * scale:.3e})")
    assert err <= tol * scale, f"{name}: max err {err:.3e} (scale {scale:.3e})"


def close_l2(a, b, rel=1e-4, name=""):
    a, b = _err(a, b)
    err = ((a - b).norm() / b.norm().clamp_min(1e-30)).item()
    print(f"    {name}: rel L2 err {err:.3e} (gate {rel:.3e})")
    assert err <= rel, f"{name}: rel L2 err {err:.3e}"


def rel_l2(a, b):
    a, b = _err(a, b)
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def gpu(t, grad=False):
    return t.detach().float().to(DEV).requires_grad_(grad)


def _family(monkeypatch, ops, fam):
    """conv kernel family: fp32mfma = fp32 MFMA kernels everywhere; bf16x3 = the three-term bf16 split kernels;
    f16x2 (shipped default) = the two-term f16 split kernels for the 3x3x3 stride-1 convolution, its weight gradient and
    the stride-2 / transposed weight gradient, bf16x3 for the transposed / 1x1x1 forward members"""
    monkeypatch.setattr(ops, "CONV_X3", fam != "fp32mfma")
    monkeypatch.setattr(ops, "CONV_X2", fam == "f16x2")
    monkeypatch.setattr(ops, "DECONV_X3", True)
    monkeypatch.setattr(ops, "PAIR_FUSE", True)
    monkeypatch.setattr(ops, "_X3_MIN_WORKGROUPS", 1)


class _GradProbe(torch.autograd.Function):
    """identity whose backward records the gradient OBJECT it receives (with its Python attributes: the way
    ops._Conv3d.backward receives the gradient the node behind it produced)"""
    seen = {}

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        _GradProbe.seen["g"] = g
        return g


def _spy_res_post(monkeypatch, ops):
    """records every ops._conv_sliced launch that carries `res_post` -- the backward-data launches that also sum another
    consumer's gradient -- with the operand object it was given: (dy, A, B, ksize, stride, transposed)"""
    calls = []
    real = ops._conv_sliced

    def spy(x, x2, w_src, A, B, K, src_ab, flip, ksize, stride, transposed, *args, **kw):
        res_post = kw.get("res_post", args[4] if len(args) > 4 else None)
        if res_post is not None:
            calls.append((x, A, B, ksize, stride, transposed))
        return real(x, x2, w_src, A, B, K, src_ab, flip, ksize, stride, transposed, *args, **kw)
    monkeypatch.setattr(ops, "_conv_sliced", spy)
    return calls


def _same_storage(a, b):
    return a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr() and a.data_ptr() == b.data_ptr()


# ------------------------------------------------------------------------------------- 1. alias output of the 3x3x3 convolution
ALIAS_CASES = [
    # cin, cout, dims, N
    (32, 32, (5, 9, 20), 2),      # partial tile in d, h and w of the 4 x 8 x 32 tile
    (40, 32, (4, 6, 36), 1),      # dx has 40 channels: the second 32-block is partial (okc masks the res_post loads); two w tiles
    (64, 64, (4, 8, 40), 1),
    (32, 32, (3, 9, 17), 2),      # W % 4 != 0: the non-VEC form of the `+ res_post` epilogue
    (16, 33, (5, 9, 17), 2),
]


@functools.lru_cache(maxsize=None)
def _alias_ref(case):
    """fp64: y = conv(x); loss = (y * gy).sum() + (x * ga).sum() -- x has two consumers"""
    cin, cout, dims, N = case
    x = seeded_tensor(f"fa.x{case}", (N, cin) + dims)
    w = seeded_tensor(f"fa.w{case}", (cout, cin, 3, 3, 3)) * (1.0 / (cin * 27) ** 0.5)
    gy = seeded_tensor(f"fa.gy{case}", (N, cout) + dims)
    ga = seeded_tensor(f"fa.ga{case}", (N, cin) + dims)
    xd, wd = x.double().requires_grad_(), w.double().requires_grad_()
    y = F.conv3d(xd, wd, None, 1, 1)
    both = torch.autograd.grad((y * gy.double()).sum() + (xd * ga.double()).sum(), [xd, wd], retain_graph=True)
    only_y = torch.autograd.grad((y * gy.double()).sum(), [xd, wd])
    return {"x": x, "w": w, "gy": gy, "ga": ga, "y": y.detach(), "both": both, "only_y": only_y}


@pytest.mark.parametrize("stats", [False, True], ids=["plain", "stats"])
@pytest.mark.parametrize("fam", ["fp32mfma", "bf16x3", "f16x2"])
@pytest.mark.parametrize("case", ALIAS_CASES, ids=[str(c) for c in ALIAS_CASES])
def test_conv3d_alias_node(case, fam, stats, monkeypatch):
    """ops._Conv3d with the alias output, raw: y, and for the three ways its two outputs can be used -- both (backward-data
    with the `+ res_post` epilogue: EPI 2 of conv3_f16x2_kernel, the bf16x3 / fp32 MFMA kernels' res_post), only y (no
    alias gradient, plain backward-data), only the alias (nothing flows through the convolution) -- dx and dw"""
    ops = _ops()
    _family(monkeypatch, ops, fam)
    cin, cout, dims, N = case
    ref = _alias_ref(case)
    split = fam != "fp32mfma"
    xg, wg = gpu(ref["x"], True), gpu(ref["w"], True)
    gy, ga = ref["gy"].to(DEV), ref["ga"].to(DEV)
    assert ops._x3_eligible(xg, None, 3, 1, False, cin, cout) == split
    calls = _spy_res_post(monkeypatch, ops)
    out = ops._Conv3d.apply(xg, None, wg, 1, False, stats, True, False)
    assert len(out) == (3 if stats else 2)
    y, xa = out[0], out[-1]
    if stats:      # the split kernels emit the BatchNorm partials, the fp32 MFMA kernel has no such form
        assert (out[1].numel() > 0) == split
    assert torch.equal(xa, xg) and _same_storage(xa, xg), "the alias output is x itself"
    close(y, ref["y"], 1e-5, "y")
    yp = _GradProbe.apply(y)

    def check(gx, gw, want, tag):
        close(gx, want[0], 1e-5, f"dx[{tag}]")
        close_l2(gw, want[1], 1e-5, f"dw[{tag}]"); close(gw, want[1], 2e-5, f"dw[{tag}]")

    # both outputs used: one backward-data launch that adds the alias gradient
    gx, gw = torch.autograd.grad((yp * gy).sum() + (xa * ga).sum(), [xg, wg], retain_graph=True)
    dy = _GradProbe.seen.pop("g")
    assert not ops._is_packed(dy)
    assert ops._x3_eligible(dy, None, 3, 1, False, cout, cin) == split
    assert len(calls) == 1 and calls[0][1:] == (cout, cin, 3, 1, False), calls
    check(gx, gw, ref["both"], "both")
    # only y used: no alias gradient, no epilogue
    del calls[:]
    gx, gw = torch.autograd.grad((yp * gy).sum(), [xg, wg], retain_graph=True)
    assert not calls
    check(gx, gw, ref["only_y"], "y only")
    # only the alias used: dx is the alias gradient itself, the weight gets none
    gx, gw = torch.autograd.grad((xa * ga).sum(), [xg, wg], allow_unused=True)
    assert not calls
    assert gw is None and torch.equal(gx, ga)


def _dres1_modules(tag):
    c1 = nn.Conv3d(32, 32, 3, 1, 1, bias=False).to(DEV); b1 = nn.BatchNorm3d(32).to(DEV)
    c2 = nn.Conv3d(32, 32, 3, 1, 1, bias=False).to(DEV); b2 = nn.BatchNorm3d(32).to(DEV)
    with torch.no_grad():
        for i, c in enumerate((c1, c2)):
            c.weight.copy_(seeded_tensor(f"{tag}.w{i}", c.weight.shape) * (1.5 / (27 * 32)) ** 0.5)
        for i, b in enumerate((b1, b2)):
            b.weight.copy_(seeded_tensor(f"{tag}.bw{i}", (32,)).abs() + 0.5); b.bias.copy_(seeded_tensor(f"{tag}.bb{i}", (32,)) * 0.3)
    return c1, b1, c2, b2


@pytest.mark.parametrize("leaf_grad", [True, False], ids=["x-needs-grad", "x-no-grad"])
@pytest.mark.parametrize("W", [24, 22])
def test_dres1_layer_alias_chain(W, leaf_grad, monkeypatch):
    """exactly _Dres1.forward -- convbn3d(x, alias=True, pack_out=True), then convbn3d(h, res_post=x', pack_out="both") --
    in training mode against the fp64 chain conv -> BN(batch statistics) -> ReLU -> conv -> BN + x, at the gates of
    test_packed_training_chain_matches_fp32_chain / test_packed_training_chain_unaligned_width: the packed chain within
    2x (+2e-6) of the fp32-operand chain's own error, that one within 1e-4.  At W = 24 the first convolution's dy arrives
    packed (the packed `+ res_post` instantiation), at W = 22 as fp32 (the non-VEC one).  x-no-grad: the input needs no
    gradient, convbn3d returns (z, x) without the fused node; the parameters' gradients must still match."""
    ops = _ops()
    _family(monkeypatch, ops, "f16x2")
    c1, b1, c2, b2 = _dres1_modules("fd1")
    x = seeded_tensor("fd1.x", (2, 32, 6, 10, W))
    gz = seeded_tensor("fd1.g", (2, 32, 6, 10, W)) * 1e-3
    params = [c1.weight, c2.weight, b1.weight, b1.bias, b2.weight, b2.bias]
    names = ["z"] + (["dx"] if leaf_grad else []) + ["dw1", "dw2", "dgamma1", "dbeta1", "dgamma2", "dbeta2"]
    calls = _spy_res_post(monkeypatch, ops)
    res = {}
    for pack in (True, False):
        monkeypatch.setattr(ops, "PACK", pack)
        for b in (b1, b2):
            b.reset_running_stats()
        del calls[:]
        xx = gpu(x, leaf_grad)
        h, xa = ops.convbn3d(xx, c1, b1, 0.0, alias=True, pack_out=True)
        if leaf_grad:
            assert xa is not xx and torch.equal(xa, xx) and _same_storage(xa, xx)
            assert ops._is_packed(h) == pack
        else:
            assert xa is xx
        z = ops.convbn3d(h, c2, b2, 1.0, res_post=xa, pack_out="both")
        assert not ops._is_packed(z) and (ops._twin_of(z) is not None) == pack
        g = torch.autograd.grad((z * gz.to(DEV)).sum(), ([xx] if leaf_grad else []) + params)
        if leaf_grad:      # one `+ res_post` launch: the first convolution's backward-data, on the f16x2 kernel
            assert len(calls) == 1 and calls[0][1:] == (32, 32, 3, 1, False), calls
            dy = calls[0][0]
            assert ops._x3_eligible(dy, None, 3, 1, False, 32, 32)
            assert ops._is_packed(dy) == (pack and W % 4 == 0)
        else:
            assert not calls
        res[pack] = [z.detach()] + [t.detach() for t in g]
    m = nn.Sequential(nn.Conv3d(32, 32, 3, 1, 1, bias=False), nn.BatchNorm3d(32), nn.ReLU(), nn.Conv3d(32, 32, 3, 1, 1, bias=False),
                      nn.BatchNorm3d(32)).double()
    with torch.no_grad():
        m[0].weight.copy_(c1.weight.cpu()); m[3].weight.copy_(c2.weight.cpu())
        for dst, src in ((m[1], b1), (m[4], b2)):
            dst.weight.copy_(src.weight.cpu()); dst.bias.copy_(src.bias.cpu())
    xr = x.double().requires_grad_()
    zr = m(xr) + xr
    gr = torch.autograd.grad((zr * gz.double()).sum(), ([xr] if leaf_grad else []) +
                             [m[0].weight, m[3].weight, m[1].weight, m[1].bias, m[4].weight, m[4].bias])
    for name, a, b, want in zip(names, res[True], res[False], [zr] + list(gr)):
        ea, eb = rel_l2(a, want), rel_l2(b, want)
        print(f"    {name}: rel L2 packed {ea:.3e}, fp32 operands {eb:.3e}")
        assert ea <= 2.0 * eb + 2e-6, (name, ea, eb)
        assert eb <= 1e-4, (name, eb)


# ------------------------------------------------------------------------------------- 2. _ConvPair / convbn3d_pair
PAIR_CASES = [
    # cin, ca, cb, fine dims, N, backward-data launch on deconv3d_x3.hip?
    (32, 64, 32, (4, 6, 8), 2, True),
    (32, 64, 32, (8, 10, 72), 1, True),      # coarse W 36 > 32: two w tiles
    (32, 64, 32, (4, 6, 10), 2, False),      # coarse W 5
    (32, 64, 32, (6, 8, 20), 1, False),      # coarse W 10
    (64, 128, 64, (4, 4, 8), 1, False),      # 64 > 32 output channels of the transposed launch: generic, channel-sliced
]


@functools.lru_cache(maxsize=None)
def _pair_ref(case):
    """fp64: ya = conv3d(x, wa, stride 2, pad 1), yb = conv3d(x, wb) of ONE leaf x"""
    cin, ca, cb, dims, N, _ = case
    x = seeded_tensor(f"fp.x{case}", (N, cin) + dims)
    wa = seeded_tensor(f"fp.wa{case}", (ca, cin, 3, 3, 3)) * (1.0 / (cin * 27) ** 0.5)
    wb = seeded_tensor(f"fp.wb{case}", (cb, cin, 1, 1, 1)) * (1.0 / cin ** 0.5)
    xd, wad, wbd = (t.double().requires_grad_() for t in (x, wa, wb))
    ya, yb = F.conv3d(xd, wad, None, 2, 1), F.conv3d(xd, wbd)
    gya, gyb = seeded_tensor(f"fp.ga{case}", ya.shape), seeded_tensor(f"fp.gb{case}", yb.shape)
    both = torch.autograd.grad((ya * gya.double()).sum() + (yb * gyb.double()).sum(), [xd, wad, wbd], retain_graph=True)
    only_b = torch.autograd.grad((yb * gyb.double()).sum(), [xd, wbd])
    return {"x": x, "wa": wa, "wb": wb, "gya": gya, "gyb": gyb, "ya": ya.detach(), "yb": yb.detach(), "both": both,
            "only_b": only_b}


def _check_pair_route(ops, calls, case):
    cin, ca, cb, dims, N, dx3 = case
    assert len(calls) == 1 and calls[0][1:] == (ca, cin, 3, 2, True), calls      # A^T dya + res_post (= B^T dyb)
    assert ops._dx3_eligible(calls[0][0], None, 3, 2, True, ca, cin) == dx3


@pytest.mark.parametrize("stats", [False, True], ids=["plain", "stats"])
@pytest.mark.parametrize("case", PAIR_CASES, ids=[str(c) for c in PAIR_CASES])
def test_conv_pair_node(case, stats, monkeypatch):
    """ops._ConvPair raw: ya, yb, dx (formed inside the transposed launch's `+ res_post`), dwa, dwb against fp64 at the gates
    of test_conv3d; with stats, the partials it returns give the fp64 batch mean / variance through bn_act at the gates of
    test_conv3d_stats_fused"""
    ops = _ops()
    _family(monkeypatch, ops, "f16x2")
    cin, ca, cb, dims, N, dx3 = case
    ref = _pair_ref(case)
    xg, wag, wbg = gpu(ref["x"], True), gpu(ref["wa"], True), gpu(ref["wb"], True)
    calls = _spy_res_post(monkeypatch, ops)
    ya, pa, yb, pb = ops._ConvPair.apply(xg, wag, wbg, stats)
    assert not calls
    close(ya, ref["ya"], 1e-5, "ya"); close(yb, ref["yb"], 1e-5, "yb")
    gx, gwa, gwb = torch.autograd.grad((ya * ref["gya"].to(DEV)).sum() + (yb * ref["gyb"].to(DEV)).sum(), [xg, wag, wbg])
    _check_pair_route(ops, calls, case)
    close(gx, ref["both"][0], 1e-5, "dx")
    for got, want, name in ((gwa, ref["both"][1], "dwa"), (gwb, ref["both"][2], "dwb")):
        close_l2(got, want, 1e-5, name); close(got, want, 2e-5, name)
    if not stats:
        assert pa.numel() == 0 and pb.numel() == 0
        return
    assert pb.numel() > 0, "the 1x1x1 bf16x3 kernel emits the statistics of these shapes"
    for y, part, yr, name in ((ya, pa, ref["ya"], "a"), (yb, pb, ref["yb"], "b")):
        C = y.shape[1]
        part = part if part.numel() else None
        mean_ref, var_ref = yr.mean(dim=(0, 2, 3, 4)), yr.var(dim=(0, 2, 3, 4), unbiased=False)
        cnt = float(yr.numel() // C)
        bn = nn.BatchNorm3d(C).to(DEV).train()
        ops.bn_act(y.detach(), bn, 1.0, stats_part=part)
        e_rm = (bn.running_mean.cpu().double() - 0.1 * mean_ref).abs().max().item()
        unb = var_ref * cnt / (cnt - 1)
        e_rv = ((bn.running_var.cpu().double() - (0.9 + 0.1 * unb)).abs() / (0.9 + 0.1 * unb)).max().item()
        bn2 = nn.BatchNorm3d(C).to(DEV)
        st = ops.bn_stats_vector(y.detach(), bn2.weight, bn2.bias, bn2.running_mean, bn2.running_var, True, 0.1, 1e-5, part)
        e_m = (st[:C].cpu().double() - mean_ref).abs().max().item()
        inv_ref = 1.0 / torch.sqrt(var_ref + 1e-5)
        e_i = ((st[C:2 * C].cpu().double() - inv_ref).abs() / inv_ref).max().item()
        print(f"    stats {name}: mean {e_m:.3e}, invstd rel {e_i:.3e}, running_mean {e_rm:.3e}, running_var rel {e_rv:.3e}")
        assert e_m <= 2e-6 * mean_ref.abs().max().item() + 1e-6
        assert e_i <= 2e-6
        assert e_rm <= 1e-6 * (1 + mean_ref.abs().max().item())
        assert e_rv <= 2e-6


@pytest.mark.parametrize("case", [PAIR_CASES[0], PAIR_CASES[2]], ids=[str(c) for c in (PAIR_CASES[0], PAIR_CASES[2])])
def test_conv_pair_only_second_output_used(case, monkeypatch):
    """only yb is consumed: dya arrives as zeros, so dx = B^T dyb and the stride-2 weight gets an exactly zero gradient"""
    ops = _ops()
    _family(monkeypatch, ops, "f16x2")
    ref = _pair_ref(case)
    xg, wag, wbg = gpu(ref["x"], True), gpu(ref["wa"], True), gpu(ref["wb"], True)
    calls = _spy_res_post(monkeypatch, ops)
    ya, pa, yb, pb = ops._ConvPair.apply(xg, wag, wbg, False)
    gx, gwa, gwb = torch.autograd.grad((yb * ref["gyb"].to(DEV)).sum(), [xg, wag, wbg])
    _check_pair_route(ops, calls, case)
    assert not bool(calls[0][0].any()), "dya is all zeros"
    close(gx, ref["only_b"][0], 1e-5, "dx")
    close_l2(gwb, ref["only_b"][1], 1e-5, "dwb"); close(gwb, ref["only_b"][1], 2e-5, "dwb")
    assert torch.equal(gwa, torch.zeros_like(gwa)), "dwa"


def _load_seeded(module):
    module.load_state_dict(O.seeded_state_dict({k: tuple(v.shape) for k, v in module.state_dict().items()}), strict=True)
    return module


def _multi_agg_fp64(m, x):
    """Multi_Aggregation (train mode) from torch.nn.functional ops in fp64: conv s2 -> conv -> deconv s2, the 1x1x1 skip,
    ReLU of the sum; returns (y, leaf weights of conv1, conv2, conv3, redir)"""
    def bn(t, mod):
        return F.batch_norm(t, None, None, mod.weight.detach().cpu().double(), mod.bias.detach().cpu().double(), True, 0.1, mod.eps)
    w1, w2, w3, wr = (p.detach().cpu().double().requires_grad_()
                      for p in (m.conv1[0][0].weight, m.conv2[0][0].weight, m.conv3[0].weight, m.redir[0].weight))
    c1 = F.relu(bn(F.conv3d(x, w1, None, 2, 1), m.conv1[0][1]))
    c2 = F.relu(bn(F.conv3d(c1, w2, None, 1, 1), m.conv2[0][1]))
    c3 = bn(F.conv_transpose3d(c2, w3, None, 2, 1, 1), m.conv3[1])
    r = bn(F.conv3d(x, wr), m.redir[1])
    return F.relu(c3 + r), [w1, w2, w3, wr]


@pytest.mark.parametrize("shape", [(2, 32, 4, 6, 8), (1, 32, 8, 10, 24)], ids=str)
def test_multi_aggregation_aligned_pair_route(shape, monkeypatch):
    """Multi_Aggregation(32) in train mode at coarse widths 4 and 12 (the golden shape's coarse width 5 keeps the pair's
    backward-data off deconv3d_x3.hip): y at close 2e-5, gx and the four convolution weights' gradients at close_l2 1e-4
    against fp64"""
    ops = _ops()
    _family(monkeypatch, ops, "f16x2")
    from dcanet_amd.models.augment.cva import Multi_Aggregation
    m = _load_seeded(Multi_Aggregation(32)).to(DEV).train()
    x = seeded_tensor(f"fma.x{shape}", shape)
    gy = seeded_tensor(f"fma.g{shape}", shape)
    xg = gpu(x, True)
    calls = _spy_res_post(monkeypatch, ops)
    y = m(xg)
    ws = [m.conv1[0][0].weight, m.conv2[0][0].weight, m.conv3[0].weight, m.redir[0].weight]
    g = torch.autograd.grad((y * gy.to(DEV)).sum(), [xg] + ws)
    assert len(calls) == 1 and calls[0][1:] == (64, 32, 3, 2, True), calls
    assert ops._dx3_eligible(calls[0][0], None, 3, 2, True, 64, 32)
    xr = x.double().requires_grad_()
    yr, wr = _multi_agg_fp64(m, xr)
    gr = torch.autograd.grad((yr * gy.double()).sum(), [xr] + wr)
    close(y, yr, 2e-5, "y")
    for got, want, name in zip(g, gr, ["gx", "g_w1", "g_w2", "g_w3", "g_wr"]):
        close_l2(got, want, 1e-4, name)


# ------------------------------------------------------------------------------------- 3. _PoolFork
POOL_DIMS = [(4, 6, 10), (5, 7, 9), (8, 8, 16), (6, 18, 68), (5, 17, 72)]      # W % 4 == 0: the 16-byte-store kernel
POOL_USES = [(third, use) for third in (False, True)
             for use in itertools.product((False, True), repeat=3 if third else 2) if any(use)]


def _pool_inputs(dims):
    x = seeded_tensor("fpl.x", (2, 3) + dims)
    gy = seeded_tensor("fpl.gy", (2, 3) + tuple((d + 1) // 2 for d in dims))
    return x, gy, seeded_tensor("fpl.g2", x.shape), seeded_tensor("fpl.g3", x.shape)


def _pool_ref(x, grads):
    """fp64: avg_pool3d(x), x and x consumed separately; grads = (gy, g2[, g3]) with None for an unused output"""
    xd = x.double().requires_grad_()
    outs = [F.avg_pool3d(xd, (3, 3, 3), stride=2, padding=1), xd, xd]
    loss = sum((o * g.double()).sum() for o, g in zip(outs, grads) if g is not None)
    return torch.autograd.grad(loss, [xd])[0], outs[0].detach()


def _pool_fork(ops, x, third):
    xg = gpu(x, True)
    outs = ops.avg_pool3d_fork(xg, third=third)
    assert len(outs) == (3 if third else 2)
    assert type(outs[0].grad_fn).__name__ == "_PoolForkBackward"
    for o in outs[1:]:
        assert torch.equal(o, xg) and _same_storage(o, xg)
    return xg, outs


@pytest.mark.parametrize("third,use", POOL_USES, ids=["".join("yab"[i] for i, u in enumerate(use) if u) + ("/3" if third else "/2")
                                                      for third, use in POOL_USES])
@pytest.mark.parametrize("dims", POOL_DIMS, ids=str)
def test_pool_fork(dims, third, use, monkeypatch):
    """ops.avg_pool3d_fork: every non-empty subset of its outputs receiving a gradient (`res` / `res2` of both backward
    kernels; gy None with one and two extras; gx2 None while gx3 is given) against the fp64 graph"""
    ops = _ops()
    monkeypatch.setattr(ops, "PAIR_FUSE", True)
    x, *gs = _pool_inputs(dims)
    gs = [g if u else None for g, u in zip(gs, use)]
    want, yr = _pool_ref(x, gs)
    xg, outs = _pool_fork(ops, x, third)
    close(outs[0], yr, 1e-6, "y")
    loss = sum((o * g.to(DEV)).sum() for o, g in zip(outs, gs) if g is not None)
    (gx,) = torch.autograd.grad(loss, [xg])
    close(gx, want, 1e-6, "gx")


@pytest.mark.parametrize("kind", ["transposed-view", "expanded"])
@pytest.mark.parametrize("dims", [(5, 7, 9), (6, 18, 68)], ids=str)
def test_pool_fork_strided_extra_gradient(dims, kind, monkeypatch):
    """an extra gradient that is not contiguous -- a transposed view, or the stride-0 expansion `.sum().backward()` makes --
    is copied on the way in and gives the numbers of its contiguous copy"""
    ops = _ops()
    monkeypatch.setattr(ops, "PAIR_FUSE", True)
    x, gy, g2, _ = _pool_inputs(dims)
    if kind == "expanded":
        g2 = torch.full((), 0.37).expand(x.shape)
    g2g = g2.to(DEV)
    if kind == "transposed-view":
        g2g = g2g.transpose(-1, -2).contiguous().transpose(-1, -2)
    else:
        g2g = torch.full((), 0.37, device=DEV).expand(x.shape)
    assert not g2g.is_contiguous() and torch.equal(g2g.cpu(), g2)
    want, _ = _pool_ref(x, (gy, g2))
    arrived = []       # contiguity of the extra gradient as _PoolFork.backward hands it to _opt
    real_opt = ops._opt
    monkeypatch.setattr(ops, "_opt", lambda t, name: (arrived.append(t is None or t.is_contiguous()), real_opt(t, name))[1])
    got = []
    for extra in (g2g, g2g.contiguous()):
        xg, outs = _pool_fork(ops, x, False)
        (gx,) = torch.autograd.grad(outs, [xg], grad_outputs=[gy.to(DEV), extra])
        got.append(gx)
    assert arrived == [False, True], arrived      # `res` of the strided run, then of the contiguous one
    close(got[0], want, 1e-6, "gx")
    assert torch.equal(got[0], got[1])


# ------------------------------------------------------------------------------------- 4. fused cost-volume builder
VOL_CASES = {
    # name: (segment channels, G, Cc, D, H, W, B)
    "a-model-segments": ((64, 128, 128), 40, 0, 8, 5, 12, 2),        # cpg 8; WQ = 3 does not divide 256: one idle thread
    "a-model-segments+concat": ((64, 128, 128), 40, 12, 8, 5, 12, 2),
    "b-two-segments": ((8, 24), 8, 0, 8, 5, 12, 2),                  # cpg 4
    "c-cpg1": ((4,), 4, 0, 8, 5, 12, 2),
    "c-cpg2": ((8,), 4, 0, 8, 5, 12, 2),
    "c-cpg16": ((64,), 4, 0, 8, 5, 12, 2),
    "d-D>W": ((8, 8, 16), 4, 12, 16, 3, 8, 2),                       # every disparity beyond the width: the zero half-plane
    "e-WQ257": ((2,), 2, 0, 4, 2, 1028, 1),                          # WQ = 257 > 256: threads stride over the row
    "f-lds66048": ((16,), 1, 0, 8, 2, 512, 1),                       # 16 * (1024 + 8) * 4 B of LDS > 64 KiB: the attribute branch
    "g-concat-W256": ((32,), 8, 12, 8, 3, 256, 1),
}
VOL_FALLBACK = {
    "W10": ((8, 24), 8, 12, 8, 5, 10, 2),
    "D6": ((8, 24), 8, 12, 6, 5, 12, 2),
    "W10-no-concat": ((64, 128, 128), 40, 0, 8, 5, 10, 1),
}


@functools.lru_cache(maxsize=None)
def _vol_ref(name):
    """fp64: build_gwc_volume(cat(segments)) concatenated with build_concat_volume, and the gradients of every input"""
    segC, G, Cc, D, H, W, B = {**VOL_CASES, **VOL_FALLBACK}[name]
    L = [seeded_tensor(f"fv.L{i}.{name}", (B, c, H, W)) for i, c in enumerate(segC)]
    R = [seeded_tensor(f"fv.R{i}.{name}", (B, c, H, W)) for i, c in enumerate(segC)]
    cl = seeded_tensor(f"fv.cl.{name}", (B, Cc, H, W)) if Cc else None
    cr = seeded_tensor(f"fv.cr.{name}", (B, Cc, H, W)) if Cc else None
    gv = seeded_tensor(f"fv.gv.{name}", (B, G + 2 * Cc, D, H, W))
    leaves = [t.double().requires_grad_() for t in L + R + ([cl, cr] if Cc else [])]
    n = len(segC)
    vol = O.build_gwc_volume(torch.cat(leaves[:n], 1), torch.cat(leaves[n:2 * n], 1), D, G)
    if Cc:
        vol = torch.cat((vol, O.build_concat_volume(leaves[2 * n], leaves[2 * n + 1], D)), 1)
    grads = torch.autograd.grad((vol * gv.double()).sum(), leaves)
    return {"L": L, "R": R, "cl": cl, "cr": cr, "gv": gv, "vol": vol.detach(), "grads": grads}


def _vol_run(ops, ref, G, D, as_one=False, out_dtype=torch.float32):
    """ops.cost_volume on the case's inputs (segments as a tuple, or as_one: as one concatenated tensor)"""
    L, R = [gpu(t, True) for t in ref["L"]], [gpu(t, True) for t in ref["R"]]
    if as_one:
        L, R = [gpu(torch.cat(ref["L"], 1), True)], [gpu(torch.cat(ref["R"], 1), True)]
    cl = gpu(ref["cl"], True) if ref["cl"] is not None else None
    cr = gpu(ref["cr"], True) if ref["cr"] is not None else None
    one = len(L) == 1
    vol = ops.cost_volume(L[0] if one else tuple(L), R[0] if one else tuple(R), D, G, cl, cr, out_dtype=out_dtype)
    return vol, L + R + ([cl, cr] if cl is not None else [])


def _vol_check(vol, leaves, ref, G, Cc, D, nseg):
    """the bounds of the separate builders' tests, and the exact zero half-plane"""
    close(vol[:, :G], ref["vol"][:, :G], 2e-6, "gwc")
    if Cc:
        assert torch.equal(vol[:, G:].cpu().double(), ref["vol"][:, G:]), "concat part"
    W = vol.shape[-1]
    for d in range(1, D):
        assert not bool(vol[:, :, d, :, :min(d, W)].any()), f"x < d must be exactly 0 (d = {d})"
    grads = torch.autograd.grad((vol * ref["gv"].to(DEV)).sum(), leaves)
    for i, (got, want) in enumerate(zip(grads, ref["grads"])):
        close(got, want, 1e-5 if i < 2 * nseg else 1e-6, f"grad[{i}]")
    return grads


@pytest.mark.parametrize("name", list(VOL_CASES))
def test_cost_volume_fused(name, monkeypatch):
    """ops.cost_volume on the fused builder (gwc_fused_kernel<1..16>, concat_fused_kernel): forward, gradients, the zero
    half-plane, and segments passed as a tuple against the same features as one tensor (bitwise)"""
    ops = _ops()
    _family(monkeypatch, ops, "f16x2")
    segC, G, Cc, D, H, W, B = VOL_CASES[name]
    ref = _vol_ref(name)
    vol, leaves = _vol_run(ops, ref, G, D)
    assert type(vol.grad_fn).__name__ == "_CostVolumeBackward", "not on the fused builder"
    assert vol.shape == (B, G + 2 * Cc, D, H, W) and vol.dtype == torch.float32
    grads = _vol_check(vol, leaves, ref, G, Cc, D, len(segC))
    if len(segC) > 1:
        vol1, leaves1 = _vol_run(ops, ref, G, D, as_one=True)
        assert type(vol1.grad_fn).__name__ == "_CostVolumeBackward"
        assert torch.equal(vol, vol1), "tuple of segments vs one tensor"
        grads1 = torch.autograd.grad((vol1 * ref["gv"].to(DEV)).sum(), leaves1)
        n = len(segC)
        for side in (0, 1):
            for got, want in zip(grads[side * n:(side + 1) * n], grads1[side].split(list(segC), 1)):
                assert torch.equal(got, want), "per-segment gradient vs split of the single-tensor gradient"


@pytest.mark.parametrize("lp", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("name", ["a-model-segments", "a-model-segments+concat", "d-D>W"])
def test_cost_volume_fused_reduced_precision(name, lp, monkeypatch):
    """the 2-byte volume is the fp32 one rounded to nearest even (same template, lp_pack2 of csrc/dca_frag.h)"""
    ops = _ops()
    _family(monkeypatch, ops, "f16x2")
    segC, G, Cc, D, H, W, B = VOL_CASES[name]
    ref = _vol_ref(name)
    v32, _ = _vol_run(ops, ref, G, D)
    vlp, _ = _vol_run(ops, ref, G, D, out_dtype=lp)
    assert type(vlp.grad_fn).__name__ == "_CostVolumeBackward" and vlp.dtype == lp and vlp.shape == v32.shape
    diff = (vlp.detach().float() - v32.detach().to(lp).float()).abs().max().item()
    print(f"    max |lp volume - round(fp32 volume)| = {diff:.3e}")
    assert torch.equal(vlp.detach(), v32.detach().to(lp))


@pytest.mark.parametrize("name", list(VOL_FALLBACK))
def test_cost_volume_fallback(name, monkeypatch):
    """W % 4 != 0 or D % 4 != 0: the separate builders, same bounds.  The reduced-precision request raises before any
    launch at W % 4 != 0; at D % 4 != 0 alone it is served by the fused builder (partial last disparity quad): fp64 on the
    same features at the gwc bound plus the rounding of the store, the concat part and the zero half-plane exact, and
    nothing written outside the volume"""
    ops = _ops()
    _family(monkeypatch, ops, "f16x2")
    segC, G, Cc, D, H, W, B = VOL_FALLBACK[name]
    ref = _vol_ref(name)
    vol, leaves = _vol_run(ops, ref, G, D)
    assert type(vol.grad_fn).__name__ != "_CostVolumeBackward", "expected the fallback"
    _vol_check(vol, leaves, ref, G, Cc, D, len(segC))
    if W % 4 == 0:
        assert D % 4
        want = ref["vol"]
        for lp, half_ulp in ((torch.bfloat16, 2.0 ** -8), (torch.float16, 2.0 ** -11)):
            vlp, srcs = _vol_run(ops, ref, G, D, out_dtype=lp)
            assert type(vlp.grad_fn).__name__ == "_CostVolumeBackward" and vlp.dtype == lp and vlp.shape == want.shape
            got = vlp.detach().cpu().double()
            err = (got - want).abs()
            assert (err <= 2e-6 * max(1.0, want.abs().max().item()) + half_ulp * want.abs()).all(), err.max().item()
            if Cc:
                assert torch.equal(got[:, G:], want[:, G:].to(lp).double()), "concat part"
            for d in range(1, D):
                assert not bool(got[:, :, d, :, :min(d, W)].any()), f"x < d must be exactly 0 (d = {d})"
            # the C entry on a volume inside a sentinel-filled buffer (-1024 is exact in both types)
            n, pad = want.numel(), 4096
            big = torch.full((n + 2 * pad,), -1024.0, device=DEV, dtype=lp)
            nseg = len(segC)
            feats = [t.detach() for t in srcs]
            rp = (ctypes.c_void_p * nseg)(*[t.data_ptr() for t in feats[:nseg]])
            tp = (ctypes.c_void_p * nseg)(*[t.data_ptr() for t in feats[nseg:2 * nseg]])
            sc = (ctypes.c_int * nseg)(*segC)
            cl, cr = (feats[2 * nseg], feats[2 * nseg + 1]) if Cc else (None, None)
            ops._chk(ops._L().dca_cost_volume_fwd(rp, tp, sc, nseg, ops._ptr(cl), ops._ptr(cr), Cc, ops._ptr(big[pad:pad + n]),
                                                  B, H, W, D, G, ops.LP_DTYPES[lp], None, ops._stream()), "dca_cost_volume_fwd")
            assert torch.equal(big[pad:pad + n].view(want.shape), vlp.detach()), "direct C-ABI call differs from the op"
            assert bool((big[:pad] == -1024.0).all()) and bool((big[pad + n:] == -1024.0).all()), "wrote outside the volume"
        return

    def no_launch():
        raise AssertionError("a kernel launch was attempted")
    monkeypatch.setattr(ops, "_L", no_launch)
    with pytest.raises(RuntimeError, match="reduced-precision volume needs"):
        _vol_run(ops, ref, G, D, out_dtype=torch.bfloat16)
