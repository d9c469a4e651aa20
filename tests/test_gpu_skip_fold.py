"""The cva skip BatchNorm folded into the block's output BatchNorm (ops._skip_fold_route, ops._BnSkipAct) against the
two-node route it replaces and against fp64.

`Multi_Aggregation(32)` computes relu(BN_d(deconv(c2)) + BN_r(redir(x))) [+ res_post].  On the two-node route BN_r is
applied by a pass of its own that writes `skip`, and its backward sums come from one more pass over (g, y_r); on the folded
route the output BatchNorm's apply / reduce / apply kernels form skip = fma(y_r, scale_r, shift_r) in registers, the
reduce pass carries BN_r's sums, and one read pass over y_r gives the maxima of skip that the packed output's exponents need.  Every case runs the block forward + backward on both routes (the module switch
ops.SKIP_FOLD) and asserts:

 1. bit-identical fp32 output z, every gradient (dx, four convolution weights, four BatchNorms' dgamma / dbeta) and every
    BatchNorm's running statistics; the packed twin of z decodes to z within 2^-22 of the channel maximum on both routes,
    and its per-channel exponents differ by at most 1 between them.  They are in fact equal, and so are the twins, bit for
    bit (asserted too): the folded route takes the maxima of skip from a read pass over y_r (dca_bn_skip_max) instead of
    bounding them analytically, because with |gamma_r| sqrt(count) + |beta_r| in the bound the exponents came out up to TWO
    lower at these BatchNorm weights (case n1: 6 channels equal, 25 one lower, 1 two lower; the bound grows by the factor
    1 + |gamma_r| / |gamma_d| <= 2.67), and the next head's convolution, which reads the twin, then no longer computes what
    it computed;
 2. both routes against an fp64 restatement on the CPU (F.conv3d, F.conv_transpose3d, F.batch_norm, autograd) at the
    fp32-grade gates of tests/test_gpu_c1_bwd_fused.py: max-abs <= 2e-5 max(1, max |ref|) for z, dx, dgamma, dbeta, relative
    L2 <= 1e-5 for the convolution weights' gradients;
 3. launches: the folded route launches no bn_apply_kernel (entry point dca_bn_apply) at the output's shape -- the one it keeps
    is conv2's BatchNorm at 1/8 resolution, which both routes have -- and exactly one bn_bwd_reduce_kernel fewer (entry points
    dca_bn_backward, _reduce, _pack, _skip: one launch each); its node saves two tensors of the output's shape (y_d, y_r) --
    no skip.

Shapes (N, 32, D, H, W), fine dims even (ops._ConvPair), every one multi-chunk with a clipped last chunk in both chunkings
of csrc/pointwise.hip (tests/_bn_cases.chunking; checked below, not assumed):

    pack4      N 2  (4, 12, 24)  S 1152   coarse width 12: the deconvolution emits its statistics (centred finalize)
    n1         N 1  (4, 14, 20)  S 1120   coarse width 10: statistics by dca_bn_stats (plain finalize)
    res_post   N 2  (4, 14, 20)  S 1120   with res_post

(two chunks of 1024 voxels each way, the second clipped: the smallest volumes that have a chunk index above 0)

All three have S % 4 == 0 and take bn_apply_pack4_kernel and the 16-byte forms.  A block shape with S % 4 != 0 does not
exist: three even dims make S a multiple of 8, and the folded route needs the fused 1x1x1 backward, which needs S % 4 == 0
(ops._c1_bwd_route).  The one-voxel pack kernel and the scalar forms of the backward kernels are therefore driven at the
node: test_scalar_forms_at_the_node runs ops.bn_skip_act against the two ops.bn_act nodes on leaf tensors at S = 3990
(5, 21, 38), same assertions, the skip's input gradient compared as what each route hands to the 1x1x1 convolution (g).

Flip-free inputs (the rule of tests/_flipfree_reference.py, M = 8): a ReLU input within rounding distance of 0 makes two
fp32-grade implementations mask differently and costs |dz| at that element, which no fp32-grade gate survives.  The seed
suffix of each case is the first of s0, s1, ... for which the fp64 reference has min |u64| >= 8 max |u32 - u64| at each of
the three ReLU sites (u32: the same restatement in float on the CPU) -- with 12 in place of 8 when searching, so that another
CPU's float rounding does not undo the choice; the test re-checks the rule on the CPU before it looks at the GPU (margins
found: pack4 12.5, n1 26.3, res_post 14.8, scalar 21.5).  Nothing here depends on what the kernels give.

Measured on an MI355X: see DESIGN.md section 5 (skip fold)."""
import collections
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from oracle.seeded import seeded_tensor
from _bn_cases import chunking
from test_gpu_parity import _unpack_px2

pytestmark = pytest.mark.gpu
DEV = "cuda"
C = 32
MARGIN = 8.0

# name: (N, fine dims, res_post, seed suffix)
CASES = {
    "pack4": (2, (4, 12, 24), False, "s13"),
    "n1": (1, (4, 14, 20), False, "s0"),
    "res_post": (2, (4, 14, 20), True, "s1"),
}
SCALAR = (2, (5, 21, 38), "s4")
CONVS = ("conv1", "conv2", "conv3", "redir")
REDUCE_ENTRIES = ("dca_bn_backward", "dca_bn_backward_reduce", "dca_bn_backward_pack", "dca_bn_backward_skip")


def _ops():
    from dcanet_amd import ops
    return ops


def _geometry_ok(dims, vector):
    S = dims[0] * dims[1] * dims[2]
    (pn, pl), (kn, kl) = chunking(S, C), chunking(S, C // 8)
    return pn > 1 and kn > 1 and S % pl != 0 and S % kl != 0 and (S % 4 == 0) == vector


def _bn_params(tag, n):
    """gamma in +-[0.75, 1.25] (every fourth channel negative), beta 0.3 randn"""
    g = torch.rand(n, generator=torch.Generator().manual_seed(sum(map(ord, tag)))) * 0.5 + 0.75
    g = torch.where(torch.arange(n) % 4 == 3, -g, g)
    return g, seeded_tensor(tag + ".beta", (n,)) * 0.3


def _inputs(name, N, dims, post, seed):
    t = f"skipfold.{name}.{seed}"
    p = {"x": seeded_tensor(t + ".x", (N, C) + dims),
         "gz": seeded_tensor(t + ".gz", (N, C) + dims),
         "rq": seeded_tensor(t + ".rq", (N, C) + dims) if post else None,
         "conv1.w": seeded_tensor(t + ".w1", (2 * C, C, 3, 3, 3)) / math.sqrt(27 * C),
         "conv2.w": seeded_tensor(t + ".w2", (2 * C, 2 * C, 3, 3, 3)) / math.sqrt(27 * 2 * C),
         "conv3.w": seeded_tensor(t + ".w3", (2 * C, C, 3, 3, 3)) / math.sqrt(27 * 2 * C / 8),
         "redir.w": seeded_tensor(t + ".wr", (C, C, 1, 1, 1)) / math.sqrt(C)}
    for nm, n in (("conv1", 2 * C), ("conv2", 2 * C), ("conv3", C), ("redir", C)):
        p[nm + ".gamma"], p[nm + ".beta"] = _bn_params(f"{t}.{nm}", n)
    return p


def _restate(p, dtype):
    """the block on the CPU in `dtype`: outputs, gradients of (z * gz).sum(), running statistics, the three ReLU inputs"""
    leaf = lambda t: t.to(dtype).clone().requires_grad_()      # noqa: E731
    x = leaf(p["x"])
    w = {nm: leaf(p[nm + ".w"]) for nm in CONVS}
    g = {nm: leaf(p[nm + ".gamma"]) for nm in CONVS}
    b = {nm: leaf(p[nm + ".beta"]) for nm in CONVS}
    rm = {nm: torch.zeros(g[nm].numel(), dtype=dtype) for nm in CONVS}
    rv = {nm: torch.ones(g[nm].numel(), dtype=dtype) for nm in CONVS}
    bn = lambda y, nm: F.batch_norm(y, rm[nm], rv[nm], g[nm], b[nm], True, 0.1, 1e-5)      # noqa: E731
    u1 = bn(F.conv3d(x, w["conv1"], None, 2, 1), "conv1")
    u2 = bn(F.conv3d(F.relu(u1), w["conv2"], None, 1, 1), "conv2")
    u3 = bn(F.conv_transpose3d(F.relu(u2), w["conv3"], None, 2, 1, 1), "conv3") + bn(F.conv3d(x, w["redir"]), "redir")
    z = F.relu(u3)
    if p["rq"] is not None:
        z = z + p["rq"].to(dtype)
    wrt = [x] + [d[nm] for nm in CONVS for d in (w, g, b)]
    grads = torch.autograd.grad((z * p["gz"].to(dtype)).sum(), wrt)
    out = {"z": z.detach(), "dx": grads[0]}
    for i, nm in enumerate(CONVS):
        out[nm + ".dw"], out[nm + ".dgamma"], out[nm + ".dbeta"] = grads[1 + 3 * i:4 + 3 * i]
        out[nm + ".running_mean"], out[nm + ".running_var"] = rm[nm], rv[nm]
    return out, [u.detach() for u in (u1, u2, u3)]


@functools.lru_cache(maxsize=None)
def _case(name):
    N, dims, post, seed = CASES[name]
    p = _inputs(name, N, dims, post, seed)
    ref, u64 = _restate(p, torch.float64)
    _, u32 = _restate(p, torch.float32)
    margin = min((a.abs().min() / (b.double() - a).abs().max()).item() for a, b in zip(u64, u32))
    return p, ref, margin


def flipfree_seed(name, tries=400):
    """the first suffix s0, s1, ... that passes the margin rule (how the suffixes in CASES were found; CPU only)"""
    N, dims, post, _ = CASES[name]
    for i in range(tries):
        p = _inputs(name, N, dims, post, f"s{i}")
        (_, u64), (_, u32) = _restate(p, torch.float64), _restate(p, torch.float32)
        if min((a.abs().min() / (b.double() - a).abs().max()).item() for a, b in zip(u64, u32)) >= MARGIN:
            return f"s{i}"
    return None


class _Entries:
    """counts the calls of the library's entry points"""

    def __init__(self, monkeypatch, ops):
        self.count = collections.Counter()
        real, spy = ops._L(), self

        class Lib:
            def __getattr__(self, name):
                fn = getattr(real, name)
                if name.startswith("__"):
                    return fn

                def entry(*args):
                    spy.count[name] += 1
                    if name == "dca_bn_apply":
                        spy.count[("dca_bn_apply", int(args[6]), int(args[7]))] += 1      # (C, S)
                    return fn(*args)
                return entry
        lib = Lib()
        monkeypatch.setattr(ops, "_L", lambda: lib)


def _block(p):
    from dcanet_amd.models.augment.cva import Multi_Aggregation
    m = Multi_Aggregation(C).to(DEV).train()
    mods = {"conv1": (m.conv1[0][0], m.conv1[0][1]), "conv2": (m.conv2[0][0], m.conv2[0][1]),
            "conv3": (m.conv3[0], m.conv3[1]), "redir": (m.redir[0], m.redir[1])}
    with torch.no_grad():
        for nm, (conv, bn) in mods.items():
            conv.weight.copy_(p[nm + ".w"]); bn.weight.copy_(p[nm + ".gamma"]); bn.bias.copy_(p[nm + ".beta"])
    return m, mods


def _run(ops, p, fold, monkeypatch, entries):
    monkeypatch.setattr(ops, "SKIP_FOLD", fold)
    m, mods = _block(p)
    x = p["x"].to(DEV).requires_grad_()
    rq = p["rq"].to(DEV).requires_grad_() if p["rq"] is not None else None
    entries.count.clear()
    z = m(x, res_post=rq)
    node = type(z.grad_fn).__name__
    saved = [tuple(t.shape) for t in z.grad_fn.saved_tensors if t is not None and t.dim() == 5]
    twin = ops._twin_of(z)
    assert twin is not None, "no packed twin beside z"
    wrt = [x] + [t for nm in CONVS for t in (mods[nm][0].weight, mods[nm][1].weight, mods[nm][1].bias)] + ([rq] if rq is not None else [])
    grads = torch.autograd.grad((z * p["gz"].to(DEV)).sum(), wrt)
    torch.cuda.synchronize()
    out = {"z": z.detach(), "dx": grads[0]}
    for i, nm in enumerate(CONVS):
        out[nm + ".dw"], out[nm + ".dgamma"], out[nm + ".dbeta"] = grads[1 + 3 * i:4 + 3 * i]
        out[nm + ".running_mean"], out[nm + ".running_var"] = mods[nm][1].running_mean.clone(), mods[nm][1].running_var.clone()
        out[nm + ".batches"] = mods[nm][1].num_batches_tracked.clone()
    if rq is not None:
        out["drq"] = grads[-1]
    return out, {"node": node, "saved": saved, "twin": twin, "exps": twin._dca_px2[0], "entries": dict(entries.count)}


def _check_twin(z, info, label):
    """the packed twin decodes to the fp32 z within 2^-22 of the channel maximum"""
    dec = _unpack_px2(info["twin"], info["exps"])
    zc = z.detach().cpu().double()
    cmax = zc.abs().amax((0, 2, 3, 4))
    err = (dec - zc).abs().amax((0, 2, 3, 4))
    worst = (err / cmax.clamp_min(1e-30)).max().item()
    print(f"    {label}: twin max err / channel max = {worst:.3e} (gate {2.0 ** -22:.3e})")
    assert (err <= 2.0 ** -22 * cmax).all(), (label, worst)


def _check_fp64(got, ref, label):
    worst = {}
    for k, r in ref.items():
        if k.endswith(("running_mean", "running_var")) or k not in got:
            continue
        a, b = got[k].detach().cpu().double(), r.double()
        assert a.shape == b.shape, (k, a.shape, b.shape)
        if k.endswith(".dw"):
            err, gate = ((a - b).norm() / b.norm().clamp_min(1e-30)).item(), 1e-5
        else:
            err, gate = (a - b).abs().max().item(), 2e-5 * max(1.0, b.abs().max().item())
        worst[k] = (err, gate)
        print(f"    {label} {k}: err {err:.3e}, gate {gate:.3e}")
    bad = {k: v for k, v in worst.items() if not v[0] <= v[1]}
    assert not bad, (label, bad)


_RUNS = {}


def _both_routes(name, monkeypatch):
    """the case's block on the two-node and on the folded route, run once and shared by the tests of the case"""
    if name not in _RUNS:
        p, _, _ = _case(name)
        ops = _ops()
        monkeypatch.setattr(ops, "_X3_MIN_WORKGROUPS", 1)
        entries = _Entries(monkeypatch, ops)
        _RUNS[name] = _run(ops, p, False, monkeypatch, entries) + _run(ops, p, True, monkeypatch, entries)
    return _RUNS[name]


@pytest.mark.parametrize("name", list(CASES))
def test_folded_route_against_two_nodes_and_fp64(name, monkeypatch):
    N, dims, post, _ = CASES[name]
    assert _geometry_ok(dims, vector=True) and all(d % 2 == 0 for d in dims), dims
    p, ref, margin = _case(name)
    print(f"    {name}: flip-free margin {margin:.1f}")
    assert margin >= MARGIN, (name, margin)
    old, iold, new, inew = _both_routes(name, monkeypatch)
    # ---- routes and launches
    assert iold["node"] == "_BnActBackward" and inew["node"] == "_BnSkipActBackward", (iold["node"], inew["node"])
    eo, en = iold["entries"], inew["entries"]
    # bn_apply_kernel = dca_bn_apply: conv2's BatchNorm at 1/8 resolution on both routes, the skip's on the two-node route only
    S = dims[0] * dims[1] * dims[2]
    assert eo.get(("dca_bn_apply", C, S), 0) == 1 and en.get(("dca_bn_apply", C, S), 0) == 0, (eo, en)
    assert eo.get("dca_bn_apply", 0) == 2 and en.get("dca_bn_apply", 0) == 1 and en.get(("dca_bn_apply", 2 * C, S // 8), 0) == 1, (eo, en)
    reduces = lambda e: sum(e.get(k, 0) for k in REDUCE_ENTRIES)      # noqa: E731  (one bn_bwd_reduce_kernel launch each)
    assert reduces(en) == reduces(eo) - 1 and en.get("dca_bn_backward_skip", 0) == 1, (eo, en)
    assert en.get("dca_conv1_bwd_fused", 0) == 1 and eo.get("dca_conv1_bwd_fused", 0) == 1, (eo, en)
    assert en.get("dca_bn_skip_max", 0) == 1 and eo.get("dca_bn_skip_max", 0) == 0, (eo, en)       # the read pass over y_r
    shape = (N, C) + dims
    assert inew["saved"] == [shape, shape] and iold["saved"] == [shape, shape], (inew["saved"], iold["saved"])   # (y_d, y_r) / (y_d, skip)
    # ---- 1. same bits
    assert set(old) == set(new)
    for k in old:
        assert torch.equal(old[k], new[k]), (name, k, (old[k].double() - new[k].double()).abs().max().item())
    _check_twin(old["z"], iold, name + " two-node")
    _check_twin(new["z"], inew, name + " folded")
    assert torch.equal(iold["exps"], inew["exps"]) and torch.equal(iold["twin"], inew["twin"]), "the packed twins differ"
    # ---- 2. fp64
    _check_fp64(old, ref, name + " two-node")
    _check_fp64(new, ref, name + " folded")
    for nm in CONVS:
        for k in (nm + ".running_mean", nm + ".running_var"):
            assert (new[k].cpu().double() - ref[k]).abs().max().item() <= 1e-6 * max(1.0, ref[k].abs().max().item()), k
        assert new[nm + ".batches"].item() == 1


@pytest.mark.parametrize("name", list(CASES))
def test_twin_exponents_differ_by_at_most_one(name, monkeypatch):
    """the packed twin's per-channel exponents on the two routes (module docstring, "Exponents")"""
    _, iold, _, inew = _both_routes(name, monkeypatch)
    de = iold["exps"].cpu() - inew["exps"].cpu()
    print(f"    {name}: twin exponents two-node - folded, channels per difference: "
          f"{dict(sorted(collections.Counter(de.tolist()).items()))}")
    assert de.abs().max().item() <= 1, de


def test_scalar_forms_at_the_node(monkeypatch):
    """S % 4 != 0: the one-voxel pack kernel and the scalar forms of the reduce / apply kernels (module docstring)"""
    N, dims, seed = SCALAR
    assert _geometry_ok(dims, vector=False), dims
    ops = _ops()
    t = "skipfold.scalar." + seed
    shape = (N, C) + dims
    y, yr = seeded_tensor(t + ".y", shape) * 1.7 + 0.3, seeded_tensor(t + ".yr", shape) * 0.8 - 0.2
    rq, gz = seeded_tensor(t + ".rq", shape), seeded_tensor(t + ".gz", shape)
    (gd, bd), (gr, br) = _bn_params(t + ".d", C), _bn_params(t + ".r", C)
    # fp64 and the margin rule at the one ReLU site
    us = []
    for dtype in (torch.float64, torch.float32):
        leaf = lambda a: a.to(dtype).clone().requires_grad_()      # noqa: E731
        wrt = [leaf(a) for a in (y, gd, bd, yr, gr, br)]
        u = (F.batch_norm(wrt[0], None, None, wrt[1], wrt[2], True, 0.1, 1e-5)
             + F.batch_norm(wrt[3], None, None, wrt[4], wrt[5], True, 0.1, 1e-5))
        us.append(u.detach())
        if dtype == torch.float64:
            u.retain_grad()
            z64 = F.relu(u) + rq.double()
            g64 = torch.autograd.grad((z64 * gz.double()).sum(), wrt + [u])
    margin = (us[0].abs().min() / (us[1].double() - us[0]).abs().max()).item()
    print(f"    scalar: flip-free margin {margin:.1f}")
    assert margin >= MARGIN, margin
    ref = {"z": z64.detach(), "dy": g64[0], "dgamma": g64[1], "dbeta": g64[2], "g": g64[6], "dgamma_r": g64[4], "dbeta_r": g64[5]}

    def run(fold):
        bnd, bnr = torch.nn.BatchNorm3d(C).to(DEV).train(), torch.nn.BatchNorm3d(C).to(DEV).train()
        with torch.no_grad():
            bnd.weight.copy_(gd); bnd.bias.copy_(bd); bnr.weight.copy_(gr); bnr.bias.copy_(br)
        yg, yrg, rqg = (a.to(DEV).requires_grad_() for a in (y, yr, rq))
        kept = {}
        if fold:
            z = ops.bn_skip_act(yg, bnd, 0.0, ops._SkipBn(yrg, None, bnr, bnd), rqg)
        else:
            skip = ops.bn_act(yrg, bnr, 1.0)
            skip.register_hook(lambda g: kept.setdefault("g", g))
            z = ops.bn_act(yg, bnd, 0.0, res_pre=skip, res_post=rqg, pack_out="both")
        twin = ops._twin_of(z)
        gr_ = torch.autograd.grad((z * gz.to(DEV)).sum(), [yg, bnd.weight, bnd.bias, yrg, bnr.weight, bnr.bias, rqg])
        torch.cuda.synchronize()
        out = {"z": z.detach(), "dy": gr_[0], "dgamma": gr_[1], "dbeta": gr_[2], "g": gr_[3] if fold else kept["g"],
               "dgamma_r": gr_[4], "dbeta_r": gr_[5], "drq": gr_[6]}
        for nm, bn in (("d", bnd), ("r", bnr)):
            out["rm_" + nm], out["rv_" + nm] = bn.running_mean.clone(), bn.running_var.clone()
        if fold:
            assert getattr(gr_[3], "_dca_lazy", None) is not None, "the skip's gradient lost the tag of the fused 1x1x1 backward"
        return out, {"twin": twin, "exps": twin._dca_px2[0]}

    old, iold = run(False)
    new, inew = run(True)
    for k in old:
        assert torch.equal(old[k], new[k]), (k, (old[k].double() - new[k].double()).abs().max().item())
    _check_twin(old["z"], iold, "scalar two-node")
    _check_twin(new["z"], inew, "scalar folded")
    for label, got in (("scalar two-node", old), ("scalar folded", new)):
        for k, r in ref.items():
            err, gate = (got[k].cpu().double() - r).abs().max().item(), 2e-5 * max(1.0, r.abs().max().item())
            print(f"    {label} {k}: err {err:.3e}, gate {gate:.3e}")
            assert err <= gate, (label, k, err, gate)
    de = iold["exps"].cpu() - inew["exps"].cpu()
    print(f"    scalar: twin exponents two-node - folded, channels per difference: "
          f"{dict(sorted(collections.Counter(de.tolist()).items()))}")
    assert de.abs().max().item() <= 1, de


def test_fallbacks_keep_two_nodes(monkeypatch):
    """eval, no_grad, DCA_PACK=0 and the split 1x1x1 backward keep the two-node route, with its values"""
    ops = _ops()
    monkeypatch.setattr(ops, "_X3_MIN_WORKGROUPS", 1)
    p, _, _ = _case("n1")
    entries = _Entries(monkeypatch, ops)
    base, _ = _run(ops, p, False, monkeypatch, entries)
    for flag in ("PACK", "C1_BWD_FUSE"):
        res = {}
        for fold in (False, True):
            monkeypatch.setattr(ops, flag, False)
            monkeypatch.setattr(ops, "SKIP_FOLD", fold)
            m, _ = _block(p)
            x = p["x"].to(DEV).requires_grad_()
            entries.count.clear()
            z = m(x)
            assert type(z.grad_fn).__name__ == "_BnActBackward", flag
            res[fold] = (z.detach(), torch.autograd.grad((z * p["gz"].to(DEV)).sum(), [x])[0])
            assert not entries.count.get("dca_bn_apply_pack_skip") and not entries.count.get("dca_bn_backward_skip")
        monkeypatch.setattr(ops, flag, True)
        assert torch.equal(res[True][0], res[False][0]) and torch.equal(res[True][1], res[False][1]), flag
    monkeypatch.setattr(ops, "SKIP_FOLD", True)
    m, _ = _block(p)
    with torch.no_grad():
        z = m(p["x"].to(DEV))
    assert torch.equal(z, base["z"]), "train-mode forward under no_grad"
    m.eval()
    entries.count.clear()
    with torch.no_grad():
        m(p["x"].to(DEV))
    torch.cuda.synchronize()
    assert not entries.count.get("dca_bn_apply_pack_skip")
