"""Logit heads: the head's backward-data folded into the BatchNorm backward (csrc/conv3d_c1.hip, dca_bn_backward_pack_c1;
ops._c1_head_bwd_route) against fp64.

The layer is a `_Classify` head, ConvBn3d(32,32,3) -> ReLU -> Conv3d(32,1,3), built through ops.convbn3d / ops.conv3d and run
forward and backward with a random gradient of the logits.  The fp64 reference is F.conv3d + F.batch_norm + F.relu +
F.conv3d on the CPU, differentiated by autograd.  The tile of the c1 kernels is 4 x 8 x 32 (d, h, w):

  one-tile    N 1 (4, 8, 32)    exactly one tile, no partial edges
  partial     N 2 (5, 9, 36)    partial tiles in all three dimensions; two samples (descending tile order, per-sample base)
  many-tiles  N 2 (9, 17, 68)   54 tiles; the apply pass' persistent grid is read back from dca_bn_backward_pack_c1_grid and
                                must be smaller than that: every workgroup walks several tiles; the reduce pass has 11 chunks
  scales      N 2 (5, 9, 36)    the channels of y and of the head's input gradient 1e2 .. 1e-6 apart (rows of the 32 -> 32
                                weight and the head's per-channel weights scaled): max |g| and the exponents of the packed dy
  fallback-W     N 1 (6, 10, 22)  W % 4 == 2: the route answers "split", bits of today's route
  fallback-off4  N 1 (4, 8, 32)   x one float off 16-byte alignment: "split", bits of today's route

Every fused case asserts the route (one dca_bn_backward_pack_c1 launch, no dca_conv3d_c1_bwd_data launch), runs the split route
(ops.C1_HEAD_BWD off) on the same inputs, and gates every gradient on the split route's own error against fp64, measured in the
same test: relative L2 and max-abs / max|ref| of the fused route <= 2 x the split route's, with a floor of one fp32 ulp of
max|ref| per element (max-abs: ulp; relative L2: ulp x sqrt(numel) / ||ref||).  The fused route runs twice and must give the
same bits (fixed-order reductions, no atomics).  Beyond that gate the fused route must give the SPLIT route's bits: its reduce
pass keeps the summation order of bn_bwd_reduce_kernel, because the training step's results may not move (a last-bit
difference of a gradient is an lr-sized step after Adam).

MEASURED on one MI355X (256 CUs), relative L2 and max-abs / max|ref| against fp64, the same figures on both routes (the tests
print split / fused per row):

             dx                   dw_conv              dgamma               dbeta                dw_head
one-tile     3.21e-07  5.78e-07   1.73e-07  1.83e-07   3.93e-07  4.17e-07   8.21e-08  7.94e-08   3.42e-07  2.49e-07
partial      3.36e-07  6.49e-07   1.94e-07  2.61e-07   3.40e-07  2.62e-07   7.55e-08  7.91e-08   2.97e-07  2.36e-07
many-tiles   3.43e-07  6.95e-07   2.51e-07  3.59e-07   4.44e-07  5.39e-07   2.58e-07  2.44e-07   3.92e-07  3.90e-07
scales       2.21e-07  3.64e-07   1.78e-07  2.11e-07   2.36e-07  1.99e-07   4.16e-07  4.87e-07   3.64e-07  4.23e-07

(A first version of the reduce pass summed per tile and wave; it met the 2 x gate on every row -- closest dbeta of the one-tile
case, 1.53e-07 against 2 x 7.94e-08 -- and was withdrawn because the benchmark's outputs moved with it.)
"""
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle.seeded import seeded_tensor

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAMES = ("dx", "dw_conv", "dgamma", "dbeta", "dw_head")
ULP = 2.0 ** -23

# name: (N, dims, per-channel scales)
CASES = {
    "one-tile": (1, (4, 8, 32), False),
    "partial": (2, (5, 9, 36), False),
    "many-tiles": (2, (9, 17, 68), False),
    "scales": (2, (5, 9, 36), True),
}
FALLBACKS = {
    "fallback-W": (1, (6, 10, 22), False),
    "fallback-off4": (1, (4, 8, 32), False),
}


def _ops():
    from dcanet_amd import ops
    return ops


@functools.lru_cache(maxsize=None)
def _ref(name):
    """inputs (fp32, CPU) and the fp64 gradients of loss = (head(relu(BN(conv(x)))) * dlogit).sum(); computed once per case"""
    N, dims, scales = {**CASES, **FALLBACKS}[name]
    x = seeded_tensor(f"hbb.x.{name}", (N, 32) + dims)
    wc = seeded_tensor(f"hbb.wc.{name}", (32, 32, 3, 3, 3)) * (1.0 / 864 ** 0.5)
    wh = seeded_tensor(f"hbb.wh.{name}", (1, 32, 3, 3, 3)) * (1.0 / 864 ** 0.5)
    if scales:
        s = 10.0 ** (2.0 - 8.0 * torch.arange(32, dtype=torch.float64) / 31.0)         # 1e2 .. 1e-6
        wc = (wc.double() * s.view(32, 1, 1, 1, 1)).float()                              # channels of y
        wh = (wh.double() * s.flip(0).view(1, 32, 1, 1, 1)).float()                      # channels of the gradient of h
    gamma = torch.rand(32, generator=torch.Generator().manual_seed(21)) + 0.5
    beta = seeded_tensor(f"hbb.beta.{name}", (32,)) * 0.3                                # both signs of u well populated
    dlogit = seeded_tensor(f"hbb.dl.{name}", (N, 1) + dims)
    xd, wcd, gd, bd, whd = (t.double().requires_grad_() for t in (x, wc, gamma, beta, wh))
    y = F.conv3d(xd, wcd, padding=1)
    h = F.relu(F.batch_norm(y, None, None, gd, bd, True, 0.1, 1e-5))
    logit = F.conv3d(h, whd, padding=1)
    grads = torch.autograd.grad((logit * dlogit.double()).sum(), [xd, wcd, gd, bd, whd])
    return {"x": x, "wc": wc, "wh": wh, "gamma": gamma, "beta": beta, "dlogit": dlogit, "grads": dict(zip(NAMES, grads))}


def _layer(r):
    conv = nn.Conv3d(32, 32, 3, padding=1, bias=False)
    bn = nn.BatchNorm3d(32)
    head = nn.Conv3d(32, 1, 3, padding=1, bias=False)
    with torch.no_grad():
        conv.weight.copy_(r["wc"]), bn.weight.copy_(r["gamma"]), bn.bias.copy_(r["beta"]), head.weight.copy_(r["wh"])
    return conv.to(DEV).train(), bn.to(DEV).train(), head.to(DEV).train()


def _input(r, off4=False):
    x = r["x"]
    if not off4:
        return x.to(DEV).requires_grad_()
    buf = torch.empty(x.numel() + 1, device=DEV)
    v = buf[1:].view(x.shape)
    v.copy_(x)
    assert v.data_ptr() % 16 == 4
    return v.detach().requires_grad_()


class _Spies:
    """the answers of the route function and the launches of the two entry points that tell the routes apart"""

    def __init__(self, monkeypatch, ops):
        self.routes, self.fused, self.bwd_data = [], 0, 0
        lib = ops._L()
        real_r, real_f, real_d = ops._c1_head_bwd_route, lib.dca_bn_backward_pack_c1, lib.dca_conv3d_c1_bwd_data

        def route(*a, **k):
            self.routes.append(real_r(*a, **k))
            return self.routes[-1]

        def fused(*a):
            self.fused += 1
            return real_f(*a)

        def bwd_data(*a):
            self.bwd_data += 1
            return real_d(*a)

        monkeypatch.setattr(ops, "_c1_head_bwd_route", route)
        monkeypatch.setattr(lib, "dca_bn_backward_pack_c1", fused)
        monkeypatch.setattr(lib, "dca_conv3d_c1_bwd_data", bwd_data)


def _step(ops, x, conv, bn, head, dlogit):
    h = ops.convbn3d(x, conv, bn, 0.0)
    logit = ops.conv3d(h, head.weight, sole_reader=True)
    logit.backward(dlogit)
    return logit


def _run(ops, monkeypatch, r, flag, off4=False):
    """gradients of one forward + backward with ops.C1_HEAD_BWD = flag, on fresh modules"""
    monkeypatch.setattr(ops, "C1_HEAD_BWD", flag)
    conv, bn, head = _layer(r)
    x = _input(r, off4)
    _step(ops, x, conv, bn, head, r["dlogit"].to(DEV))
    torch.cuda.synchronize()
    return dict(zip(NAMES, (x.grad, conv.weight.grad, bn.weight.grad, bn.bias.grad, head.weight.grad)))


def _errors(got, ref):
    """(relative L2, max-abs / max|ref|, floor of the first, floor of the second)"""
    g, ref = got.detach().cpu().double(), ref.double()
    assert g.shape == ref.shape, (g.shape, ref.shape)
    top, nrm = ref.abs().max().item(), ref.norm().item()
    return (((g - ref).norm() / nrm).item(), ((g - ref).abs().max() / top).item(), ULP * top * ref.numel() ** 0.5 / nrm, ULP)


def _setup(monkeypatch):
    ops = _ops()
    monkeypatch.setattr(ops, "_X3_MIN_WORKGROUPS", 1)
    return ops, _Spies(monkeypatch, ops)


def _tiles(N, dims):
    return N * -(-dims[0] // 4) * -(-dims[1] // 8) * -(-dims[2] // 32)


@pytest.mark.parametrize("name", list(CASES))
def test_fused_against_fp64_and_split(name, monkeypatch, capsys):
    ops, spies = _setup(monkeypatch)
    N, dims, _ = CASES[name]
    r = _ref(name)
    lib = ops._L()
    nwg, tiles = lib.dca_bn_backward_pack_c1_grid(N, *dims), _tiles(N, dims)      # the apply pass' persistent workgroups
    assert 1 <= nwg <= tiles
    assert lib.dca_bn_backward_pack_c1_chunks(N, *dims) == lib.dca_bn_num_chunks(32, dims[0] * dims[1] * dims[2])
    if name == "one-tile":
        assert (nwg, tiles) == (1, 1)
    if name == "many-tiles":
        assert nwg < tiles and tiles == 54, f"{name}: {tiles} tiles on {nwg} workgroups: no workgroup walks several tiles"
        assert lib.dca_bn_backward_pack_c1_chunks(N, *dims) > 1      # and the reduce pass has several chunks per channel
    fused = _run(ops, monkeypatch, r, True)
    assert spies.routes == ["fused"] and (spies.fused, spies.bwd_data) == (1, 0), (spies.routes, spies.fused, spies.bwd_data)
    again = _run(ops, monkeypatch, r, True)
    split = _run(ops, monkeypatch, r, False)
    assert spies.routes == ["fused", "fused", "split"] and (spies.fused, spies.bwd_data) == (2, 1)
    rows, bad = [], []
    for q in NAMES:
        ef, es = _errors(fused[q], r["grads"][q]), _errors(split[q], r["grads"][q])
        rows.append(f"{name:11s} {q:8s} nwg {nwg:3d} tiles {tiles:3d}  rel L2 {es[0]:.2e} / {ef[0]:.2e}   "
                    f"max-abs {es[1]:.2e} / {ef[1]:.2e}")
        if ef[0] > max(2 * es[0], ef[2]) or ef[1] > max(2 * es[1], ef[3]):
            bad.append(rows[-1])
    with capsys.disabled():
        print("\n" + "\n".join(rows))
    assert not bad, "fused route beyond twice the split route's error against fp64:\n" + "\n".join(bad)
    for q in NAMES:
        assert torch.equal(fused[q], again[q]), f"{name}: {q} differs between two runs of the fused route"
        # the reduce pass keeps the split route's summation order and the apply pass its expressions: the training step's
        # results do not move with the route (Adam turns a last-bit difference of a gradient into a visible one)
        assert torch.equal(fused[q], split[q]), f"{name}: {q} of the fused route is not the split route's, bit for bit"


@pytest.mark.parametrize("name", list(FALLBACKS))
def test_fallbacks_keep_todays_bits(name, monkeypatch):
    ops, spies = _setup(monkeypatch)
    r = _ref(name)
    off4 = name == "fallback-off4"
    on = _run(ops, monkeypatch, r, True, off4)
    assert spies.routes == ["split"] and (spies.fused, spies.bwd_data) == (0, 1), (spies.routes, spies.fused, spies.bwd_data)
    off = _run(ops, monkeypatch, r, False, off4)
    for q in NAMES:
        assert torch.equal(on[q], off[q]), f"{name}: {q} changed with the flag although the route is split"
        e = _errors(on[q], r["grads"][q])
        assert e[0] < 1e-4, (name, q, e)          # (the split route itself is gated elsewhere; this guards the reference)


def test_second_reader_raises(monkeypatch):
    """a broken sole_reader promise: the sum of two gradients reaches the BatchNorm without the head's tag"""
    ops, _ = _setup(monkeypatch)
    monkeypatch.setattr(ops, "C1_HEAD_BWD", True)
    r = _ref("one-tile")
    conv, bn, head = _layer(r)
    x = _input(r)
    h = ops.convbn3d(x, conv, bn, 0.0)
    logit = ops.conv3d(h, head.weight, sole_reader=True)
    with pytest.raises(RuntimeError, match="hand-off of the logit head"):
        (logit.sum() + h.sum()).backward()


def test_graph_replay_equals_eager(monkeypatch):
    """forward + backward captured in a hipGraph and replayed: the bits of the eager run (what GraphedTrainStep relies on)"""
    ops, spies = _setup(monkeypatch)
    r = _ref("partial")
    eager = _run(ops, monkeypatch, r, True)
    conv, bn, head = _layer(r)
    x, dlogit = _input(r), r["dlogit"].to(DEV)
    params = (x, conv.weight, bn.weight, bn.bias, head.weight)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _step(ops, x, conv, bn, head, dlogit)                 # warm-up, outside the capture
    torch.cuda.current_stream().wait_stream(side)
    for p in params:
        p.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _step(ops, x, conv, bn, head, dlogit)
    assert spies.routes == ["fused"] * 3 and spies.bwd_data == 0
    for p in params:
        p.grad.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    for q, p in zip(NAMES, params):
        assert torch.equal(p.grad, eager[q]), f"{q}: the replayed graph differs from the eager run"
