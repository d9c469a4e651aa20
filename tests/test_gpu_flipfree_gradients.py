"""Every gradient of the composed train step at the fp32-grade yardstick, on flip-free references, on every route.

tests/test_gpu_unaligned.py holds the train step (`GwcNet.hot_path`, train mode, seven heads, ~150 parameter tensors) to
median <= 3e-3 / every tensor <= 8e-3 only, because its inputs put some (leaky-)ReLU input or arg-max within rounding distance
of its decision boundary, where two fp32-grade implementations branch differently.  Here the inputs are chosen so that the
fp64 reference has NO such decision near its boundary (flip-free: definition, margin rule M = 8 and tracer in
tests/_flipfree_reference.py; the seeds come from tools/flipfree_seed_search.py, which tries the suffixes s0, s1, ... in order
on the CPU and prints the first that passes; tests/test_flipfree_reference_cpu.py re-checks every committed case without a
GPU).  The step is then locally smooth and the project's per-tensor yardstick is the right gate for EVERY gradient tensor:

    heads                 head_tol (the project's forward gates, test_gpu_unaligned.py)
    running statistics    err_gpu <= 4 x err_oracle32 + 1e-5     relative L2 against the fp64 oracle, per buffer
    every gradient        err_gpu <= 4 x err_oracle32 + 1e-5     relative L2 against the fp64 oracle, per tensor
                          (`check_yardstick` of test_gpu_unaligned.py; tensors with |ref| < 1e-6 skipped, <= 5 % of them)

No median gate and no absolute gate: a ~1 % error in any one backward term of any one tensor fails.

Cases (features (B, 320[+12], H4, W4); D4 = maxdisp / 4 = 4) and their references, CPU only (the same rows are the first
half of profiles/flipfree_gradients.txt; margin = min over the sites of min |u64| / max |u32 - u64| for the 40 activation
sites, of top-two gap / (2 max |p32 - p64|) for the three arg-max sites; all must be >= M = 8):

    id     B H4 W4  maxdisp  variant seed  activation inputs  activation margin  arg-max margin
    b1w8   1  4  8  16       g       s0      59 392           19.1                  15328
    b1w8                     gc      s8      59 392           14.6                 234197
    b2w8   2  4  8  16       g       s127   118 784           13.7                  26755
    b2w8                     gc      s15    118 784           16.0                  17865
    b1w10  1  4 10  16       g       s2      74 240           11.5                 160694
    b1w10                    gc      s9      74 240           27.1                  46999
    b1w16  1  4 16  16       g       s8     118 784           12.2                   6258
    b1w16                    gc      s13    118 784           13.3                  12534

(1, 4, 16, 16) did yield seeds, so it is included.  b1w10 is the W4 % 4 == 2 shape.

Routes.  Every case runs on every route a model can train on, `_X3_MIN_WORKGROUPS` = 1 so that these small volumes reach the
split kernels, all at the same gate (which also gives "packed equals unpacked" at the 1e-5 level):

    default    f16x2 family, PACK on, pair / alias nodes, fused 1x1x1 backward, fused statistics (what ships)
    nopack     PACK off: fp32 tensors between the layers
    bf16x3     CONV_X2 off
    fp32       CONV_X2 and CONV_X3 off: the fp32 MFMA kernels everywhere
    nofuse     C1_BWD_FUSE, PAIR_FUSE and BN_FUSE off together; c1split / nopair / nobnfuse: each of them off alone

The test records which kernels ran -- the answers of ops._conv_family / _wgrad_family / _c1_bwd_route, the twins handed out
by ops._twin_of, and every entry point of the library with its packed-operand flags -- prints them, and asserts per route:
  * default, aligned cases: convolution families "x2", "s2x2", "dx3", "c1x3" each launched; weight gradients "x2" (stride 1)
    and "s2x2" (stride 2 and transposed); dca_conv1_bwd_fused launched; a weight gradient with a packed dy; a convolution that
    read a packed twin, and its weight gradient with a packed x.
  * default, b1w10 (fine width 10, coarse width 5): the fallback set of test_gpu_unaligned.py -- the stride-2 convolution, the
    transposed one and their weight gradients on the fp32 MFMA kernels ("mfma"; no "s2x2", no "dx3"), the logit heads' weight
    gradient through dca_conv3d_c1_expand, and a stride-1 f16x2 weight gradient only where BOTH operands are packed
    (`_x2_pairs`).  Not reached at this shape, by its own predicate: the generic 1x1x1 kernels and the split 1x1x1 backward
    -- `_c1x3_eligible` and `_c1_bwd_route` ask for S % 4 == 0, and S = D H W = 4 x 4 x 10 (2 x 2 x 5 at eighth res) is a
    multiple of 4 from D and H alone; test_gpu_unaligned.py covers those at u22 / u26.
  * nopack: no packed operand reaches any kernel, no twin.  bf16x3: no f16x2 entry point, "x3" launched.  fp32: "mfma" only.
    c1split / nofuse: no dca_conv1_bwd_fused.  nobnfuse / nofuse: no *_forward_stats entry point.
Not reached at any of these shapes: the channel-sliced launches (more than 64 output channels: baseline hourglass only).

One graphed variant (b2w8 g, default route): a GraphedTrainStep replay of the same step is bitwise
equal to the eager step gated above.

Measured on an MI355X (median / max over the gradient tensors of err_gpu, err_oracle32 and err_gpu / err_oracle32; the same
table is the second half of profiles/flipfree_gradients.txt):

    case      route     err_gpu                   err_oracle32              ratio
    b1w8 g    default   2.084e-06 / 3.841e-06     1.558e-06 / 3.580e-06     1.37 / 2.84
    b1w8 gc   default   1.958e-06 / 3.796e-06     1.458e-06 / 2.983e-06     1.31 / 2.43
    b2w8 g    default   1.666e-06 / 4.088e-06     1.510e-06 / 3.520e-06     1.12 / 1.97
    b2w8 gc   default   1.553e-06 / 3.730e-06     1.799e-06 / 3.575e-06     0.84 / 1.59
    b1w10 g   default   1.748e-06 / 4.706e-06     1.574e-06 / 3.766e-06     1.12 / 2.42
    b1w10 gc  default   2.043e-06 / 5.211e-06     1.595e-06 / 3.214e-06     1.31 / 2.57
    b1w16 g   default   1.800e-06 / 6.037e-06     1.395e-06 / 3.728e-06     1.32 / 2.36
    b1w16 gc  default   1.601e-06 / 3.629e-06     1.446e-06 / 3.097e-06     1.17 / 2.04

The other seven routes lie in the same range: over all 64 runs the gradients have err_gpu <= 7.078e-06 and err_gpu /
err_oracle32 <= 3.71, the running statistics err_gpu <= 4.194e-07 and a ratio <= 2.72.  default, nopack and c1split give the
same figures to every printed digit although other kernels ran (the route assertions).  The module takes about 35 s.

Would it notice?  Shown once on a scratch copy (not part of the suite), default route:
  * `dgamma / count` x 1.01 in bn_bwd_finalize_kernel: all 8 cases fail here (err_gpu median 4.1e-3 .. 5.8e-3, ratio to the
    fp32 oracle > 2500).  test_train_step_unaligned_width_all_gradients passes 6 of its 8 cases with that library (medians
    2.54e-3 .. 2.96e-3 under its 3e-3 gate) and fails u26 gc (3.01e-3) and u18 g (3.55e-3): at best a marginal signal there.
  * `_Conv3d.backward` without its `res_post=g_alias` term: all 8 cases fail here (err_gpu ~ 1).
"""
import collections
import functools

import pytest
import torch

from oracle.seeded import seeded_tensor
from test_gpu_configs import load_seeded
from test_gpu_unaligned import HEADS, check_yardstick, head_tol, split, summary, yardstick_rows
import _flipfree_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"

SEEDS = {             # (shape id, variant): seed suffix -- the record of tools/flipfree_seed_search.py
    ("b1w8", "g"): "s0", ("b1w8", "gc"): "s8",
    ("b2w8", "g"): "s127", ("b2w8", "gc"): "s15",
    ("b1w10", "g"): "s2", ("b1w10", "gc"): "s9",
    ("b1w16", "g"): "s8", ("b1w16", "gc"): "s13",
}
ALIGNED = ("b1w8", "b2w8", "b1w16")
HOT_MODULES = ("dres0", "dres1", "cva1", "cva2", "cva3", "classif0", "classif1", "classif2", "classif3")

ALL_ON = dict(CONV_X2=True, CONV_X3=True, CONV_S2_X2=True, WGRAD_S2_X2=True, DECONV_X3=True, C1_WGRAD_FUSED=True,
              BN_FUSE=True, PAIR_FUSE=True, C1_BWD_FUSE=True, PACK=True, AMAX_EMIT=True, _X3_MIN_WORKGROUPS=1)
ROUTES = {
    "default": {},
    "nopack": {"PACK": False},
    "bf16x3": {"CONV_X2": False},
    "fp32": {"CONV_X2": False, "CONV_X3": False},
    "nofuse": {"C1_BWD_FUSE": False, "PAIR_FUSE": False, "BN_FUSE": False},
    "c1split": {"C1_BWD_FUSE": False},
    "nopair": {"PAIR_FUSE": False},
    "nobnfuse": {"BN_FUSE": False},
}
X2_ENTRY_POINTS = ("dca_conv3d_x2_forward", "dca_conv3d_x2_forward_stats", "dca_conv3d_s2x2_forward", "dca_conv3d_wgrad_x2",
                   "dca_conv3d_wgrad_s2_x2", "dca_bn_apply_pack", "dca_bn_backward_pack")


class RouteSpy:
    """what the step really ran: answers of the routing functions, twins handed out, library entry points.
    packed: per entry point that takes packed px2 operands, the set of its packed-flag tuples seen -- (x,) for the f16x2
    convolution, (x, dy) for its weight gradient"""

    def __init__(self, setattr_, ops):
        self.conv, self.wgrad, self.c1bwd = (collections.Counter() for _ in range(3))
        self.entry, self.packed, self.twins = collections.Counter(), collections.defaultdict(set), 0
        for name, counter in (("_conv_family", self.conv), ("_wgrad_family", self.wgrad), ("_c1_bwd_route", self.c1bwd)):
            setattr_(ops, name, self._counting(getattr(ops, name), counter))
        twin_of = ops._twin_of

        def spy_twin(t):
            tw = twin_of(t)
            self.twins += tw is not None
            return tw
        setattr_(ops, "_twin_of", spy_twin)
        real, spy = ops._L(), self

        class Lib:
            def __getattr__(self, name):
                fn = getattr(real, name)
                if name.startswith("__"):
                    return fn

                def entry(*args):
                    spy.entry[name] += 1
                    if name in ("dca_conv3d_x2_forward", "dca_conv3d_x2_forward_stats"):
                        spy.packed[name].add((int(args[1]),))
                    if name == "dca_conv3d_wgrad_x2":
                        spy.packed[name].add((int(args[1]), int(args[4])))
                    return fn(*args)
                return entry
        lib = Lib()
        setattr_(ops, "_L", lambda: lib)

    @staticmethod
    def _counting(fn, counter):
        @functools.wraps(fn)
        def wrapped(*a, **k):
            r = fn(*a, **k)
            counter[r] += 1
            return r
        return wrapped

    def report(self):
        fmt = lambda c: " ".join(f"{k}*{v}" for k, v in sorted(c.items()))
        return (f"      conv families   {fmt(self.conv)}\n      wgrad families  {fmt(self.wgrad)}\n"
                f"      1x1x1 backward  {fmt(self.c1bwd)}   twins read {self.twins}\n"
                f"      packed flags    {' '.join(f'{k}:{sorted(v)}' for k, v in sorted(self.packed.items()))}\n"
                f"      entry points    {fmt(self.entry)}")


def check_routes(spy, sid, route):
    """the kernels the route is meant to exercise were launched, and none it excludes (module docstring)"""
    e, flags = spy.entry, ROUTES[route]
    launched = lambda *names: all(e[n] > 0 for n in names)
    x2, x3, pack = flags.get("CONV_X2", True), flags.get("CONV_X3", True), flags.get("PACK", True)
    c1fuse, bnfuse = flags.get("C1_BWD_FUSE", True), flags.get("BN_FUSE", True)
    aligned = sid in ALIGNED
    any_packed = any(any(t) for v in spy.packed.values() for t in v)
    if x2:
        assert spy.conv["x2"] and launched("dca_conv3d_x2_forward"), "no f16x2 3x3x3 stride-1 convolution"
        if aligned or route == "default":       # at W % 4 != 0 only two packed operands pair: PACK and the nodes that pack
            assert launched("dca_conv3d_wgrad_x2") and spy.wgrad["x2"], "no f16x2 stride-1 weight gradient"
        if aligned:
            assert spy.conv["s2x2"] and launched("dca_conv3d_s2x2_forward"), "no f16x2 stride-2 convolution"
            assert spy.conv["dx3"] and (e["dca_deconv3d_x3_forward"] or e["dca_deconv3d_x3_forward_stats"]), "no bf16x3 deconv"
            assert spy.conv["c1x3"] and (e["dca_conv1_x3_forward"] or e["dca_conv1_x3_forward_stats"]), "no bf16x3 1x1x1 conv"
            assert spy.wgrad["s2x2"] and launched("dca_conv3d_wgrad_s2_x2"), "no f16x2 stride-2 weight gradient"
            assert launched("dca_conv3d_c1_wgrad") and not e["dca_conv3d_c1_expand"], "logit heads off the fused weight gradient"
        else:
            assert not spy.conv["s2x2"] and not spy.conv["dx3"] and not spy.wgrad["s2x2"], (spy.conv, spy.wgrad)
            assert not (e["dca_conv3d_s2x2_forward"] or e["dca_deconv3d_x3_forward_stats"] or e["dca_conv3d_wgrad_s2_x2"])
            assert spy.conv["mfma"] and spy.wgrad["mfma"] and launched("dca_conv3d_forward", "dca_conv3d_wgrad")
            assert launched("dca_conv3d_c1_expand") and not e["dca_conv3d_c1_wgrad"], "logit heads: expansion expected"
            assert all(t == (1, 1) for t in spy.packed["dca_conv3d_wgrad_x2"]), spy.packed      # _x2_pairs at W % 4 != 0
        if route == "default":
            assert any(t[1] for t in spy.packed["dca_conv3d_wgrad_x2"]), "no weight gradient read a packed dy"
            assert (1,) in spy.packed["dca_conv3d_x2_forward"], "no backward-data launch read a packed dy"
            assert launched("dca_bn_apply_pack", "dca_bn_backward_pack")
            if aligned:
                assert spy.twins > 0, "no convolution read a packed twin"
                assert (1, 0) in spy.packed["dca_conv3d_wgrad_x2"] or (1, 1) in spy.packed["dca_conv3d_wgrad_x2"]
    else:
        assert not any(e[n] for n in X2_ENTRY_POINTS), {n: e[n] for n in X2_ENTRY_POINTS if e[n]}
        assert not spy.conv["x2"] and not spy.conv["s2x2"] and not spy.wgrad["x2"] and not spy.wgrad["s2x2"]
        if x3:
            assert spy.conv["x3"] and e["dca_conv3d_x3_forward_stats"] and e["dca_conv3d_x3_forward"], "no bf16x3 convolution"
            if aligned:
                assert spy.wgrad["x3"] and launched("dca_conv3d_wgrad_x3"), "no bf16x3 weight gradient"
                assert spy.conv["dx3"] and spy.conv["c1x3"]
        else:
            assert set(spy.conv) == {"mfma"} and set(spy.wgrad) == {"mfma"}, (spy.conv, spy.wgrad)
            assert launched("dca_conv3d_forward", "dca_conv3d_wgrad")
    if not pack or not x2:
        assert not any_packed and spy.twins == 0 and not e["dca_bn_apply_pack"] and not e["dca_bn_backward_pack"], spy.packed
    if c1fuse:
        assert spy.c1bwd["fused"] and launched("dca_conv1_bwd_fused", "dca_bn_backward_reduce"), "no fused 1x1x1 backward"
    else:
        assert set(spy.c1bwd) <= {"split"} and not e["dca_conv1_bwd_fused"] and not e["dca_bn_backward_reduce"], spy.c1bwd
    stats_launches = sum(v for k, v in e.items() if k.endswith("_forward_stats"))
    assert stats_launches > 0 if (bnfuse and x3) else stats_launches == 0, stats_launches


def loss_weights(r, suffix):
    return [seeded_tensor(f"{R.tag_of(suffix)}.g{i}", r[k].shape).to(r[k].device) for i, k in enumerate(HEADS)]


def gpu_step(sid, variant):
    """(model, the step as a closure returning heads + gradients, gradient names)"""
    from dcanet_amd.models.gwcnet_dca_g import GwcNet
    shape, concat, suffix = R.SHAPES[sid], variant == "gc", SEEDS[sid, variant]
    names = R.oracle_train(shape, concat, suffix, torch.float64)["names"]
    m = load_seeded(GwcNet(shape[3], use_concat_volume=concat)).to(DEV).train()
    fL, fR = R.features(shape, concat, suffix)
    ag, bg = fL.to(DEV).requires_grad_(), fR.to(DEV).requires_grad_()
    params = dict(m.named_parameters())
    hot = sorted(k for k in params if k.split(".")[0] in HOT_MODULES)
    assert sorted(names[2:]) == hot, "the oracle and the model disagree about the parameter tensors of the hot path"
    leaves = [ag, bg] + [params[k] for k in names[2:]]
    wts = []

    def step():
        r = m.hot_path(*split(ag, bg, concat))
        if not wts:
            wts.extend(loss_weights(r, suffix))         # the seeded loss of _flipfree_reference.seeded_loss, weights made once
        loss = 0
        for k, g in zip(HEADS, wts):
            loss = loss + (r[k] * g).sum()
        return [r[k] for k in HEADS], list(torch.autograd.grad(loss, leaves))
    return m, step, names


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("case", list(SEEDS), ids=lambda c: f"{c[0]}-{c[1]}")
def test_train_step_flip_free_every_gradient_at_the_yardstick(case, route, monkeypatch, capsys):
    """heads, running statistics and the gradient of both feature maps and of EVERY parameter tensor against the fp64 oracle
    at the gates of the module docstring, on one route; the kernels that ran are printed and asserted"""
    from dcanet_amd import ops
    sid, variant = case
    shape, concat, suffix = R.SHAPES[sid], variant == "gc", SEEDS[case]
    bad = R.flip_free_violations(shape, concat, suffix)
    assert not bad, bad
    r64, r32 = (R.oracle_train(shape, concat, suffix, d) for d in (torch.float64, torch.float32))
    for k, v in {**ALL_ON, **ROUTES[route]}.items():
        monkeypatch.setattr(ops, k, v)
    m, step, names = gpu_step(sid, variant)
    spy = RouteSpy(monkeypatch.setattr, ops)
    heads, got_g = step()
    torch.cuda.synchronize()
    monkeypatch.undo()
    what = f"{sid} {variant} {route}"
    rows = yardstick_rows(names, got_g, r64["grads"], r32["grads"])
    state = m.state_dict()
    snames = sorted(r64["stats"])
    srows = yardstick_rows(snames, [state[k] for k in snames], [r64["stats"][k] for k in snames],
                           [r32["stats"][k] for k in snames])
    with capsys.disabled():
        print(f"\n[{what}] per-tensor gradient rel-L2 vs the fp64 oracle {shape}, seed {suffix}: worst by err_gpu / err_oracle32")
        for n, eg, eo, nr in sorted(rows, key=lambda t: -t[1] / max(t[2], 1e-30))[:6]:
            print(f"   {n:60s} gpu {eg:.3e}   oracle32 {eo:.3e}   |ref| {nr:.3e}")
        print(f"   GRADIENTS {what}: {summary(rows)}")
        print(f"   RUNNING-STATS {what}: {summary(srows)}")
        print(f"   ROUTES {what}:\n{spy.report()}")
    for k, z in zip(HEADS, heads):
        ref = r64["heads"][k]
        err = (z.detach().cpu().double() - ref).abs().max().item()
        assert err <= head_tol(k, ref), f"{what} {k}: max err {err:.3e} > {head_tol(k, ref):.1e}"
    check_yardstick(srows, f"{what} running statistics")
    check_yardstick(rows, f"{what} gradients")
    assert len(rows) == len(r64["names"]) >= 150
    check_routes(spy, sid, route)


def test_graphed_train_step_flip_free_is_bitwise_the_eager_step(monkeypatch):
    """b2w8 g on the default route: the step gated above (it is the same closure), replayed by GraphedTrainStep, gives bitwise
    the heads and gradients of the eager launch"""
    from dcanet_amd import ops
    from dcanet_amd.graph import GraphedTrainStep
    for k, v in ALL_ON.items():
        monkeypatch.setattr(ops, k, v)
    m, step, names = gpu_step("b2w8", "g")
    eager = [t.detach().clone() for part in step() for t in part]
    graphed = GraphedTrainStep(step, lambda: None, restore=list(m.buffers()))
    heads, grads = graphed()
    torch.cuda.synchronize()
    for n, a, b in zip(list(HEADS) + names, eager, list(heads) + list(grads)):
        assert torch.equal(a, b), f"{n}: graph replay differs by {(a - b).abs().max().item():.3e}"


@pytest.mark.parametrize("W", [10, 8])
def test_packed_operand_pairs_with_a_packed_gradient_without_fused_statistics(W, monkeypatch):
    """What the nobnfuse route exposed at b1w10: with BN_FUSE off the alias node still packs its output, and the layer that
    reads it took the plain path, whose gradient is fp32 -- at W % 4 != 0 the weight gradient then had a packed x beside an
    fp32 dy and raised (`_x2_pairs`).  The smallest chain that shows it: convbn3d(alias, pack_out) -> convbn3d(res_post =
    the alias) at (1, 32, 4, 4, W), no activation (smooth: no sign to flip), BN_FUSE off and on, forward and every gradient
    against fp64 at the single-op gates of test_gpu_parity.py (forward 1e-5 of the scale, gradients 1e-4 relative L2)."""
    import torch.nn as nn
    import torch.nn.functional as F
    from dcanet_amd import ops
    from test_gpu_configs import rel_l2
    c = [nn.Conv3d(32, 32, 3, 1, 1, bias=False).to(DEV) for _ in range(2)]
    b = [nn.BatchNorm3d(32).to(DEV) for _ in range(2)]
    with torch.no_grad():
        for i in range(2):
            c[i].weight.copy_(seeded_tensor(f"ffnode.w{i}", c[i].weight.shape) * (1.5 / (27 * 32)) ** 0.5)
            b[i].weight.copy_(seeded_tensor(f"ffnode.g{i}", (32,)).abs() + 0.5)
            b[i].bias.copy_(seeded_tensor(f"ffnode.b{i}", (32,)))
    x = seeded_tensor("ffnode.x", (1, 32, 4, 4, W))
    gz = seeded_tensor("ffnode.gz", (1, 32, 4, 4, W))
    xr = x.double().requires_grad_()
    wr = [t.weight.detach().cpu().double().requires_grad_() for t in c]
    br = [(t.weight.detach().cpu().double().requires_grad_(), t.bias.detach().cpu().double().requires_grad_()) for t in b]
    z1 = F.batch_norm(F.conv3d(xr, wr[0], None, 1, 1), None, None, br[0][0], br[0][1], True)
    zr = F.batch_norm(F.conv3d(z1, wr[1], None, 1, 1), None, None, br[1][0], br[1][1], True) + xr
    ref = [zr.detach()] + list(torch.autograd.grad((zr * gz.double()).sum(), [xr] + wr + [t for p in br for t in p]))
    for k, v in ALL_ON.items():
        monkeypatch.setattr(ops, k, v)
    for fuse in (False, True):
        monkeypatch.setattr(ops, "BN_FUSE", fuse)
        for t in b:
            t.reset_running_stats()
        spy = RouteSpy(monkeypatch.setattr, ops)
        xg = x.to(DEV).requires_grad_()
        y1, xa = ops.convbn3d(xg, c[0], b[0], 1.0, alias=True, pack_out=True)
        assert ops._is_packed(y1)
        z = ops.convbn3d(y1, c[1], b[1], 1.0, res_post=xa)
        leaves = [xg, c[0].weight, c[1].weight, b[0].weight, b[0].bias, b[1].weight, b[1].bias]
        got = [z.detach()] + list(torch.autograd.grad((z * gz.to(DEV)).sum(), leaves))
        torch.cuda.synchronize()
        assert (1, 1) in spy.packed["dca_conv3d_wgrad_x2"], spy.packed       # the second layer: packed x, packed dy
        err = (got[0].cpu().double() - ref[0]).abs().max().item()
        assert err <= 1e-5 * max(1.0, ref[0].abs().max().item()), (fuse, err)
        for name, a, r in zip(("dx", "dw1", "dw2", "dgamma1", "dbeta1", "dgamma2", "dbeta2"), got[1:], ref[1:]):
            assert rel_l2(a, r) <= 1e-4, (fuse, name, rel_l2(a, r))
