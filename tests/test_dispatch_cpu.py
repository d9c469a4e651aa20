"""Which entry point of libdca_hip.so serves each convolution and weight gradient, pinned without a GPU.

Routing in ops.py reads only shapes, alignment, operand tags and the module flags, so it is observable on CPU tensors:
`ops._L` is replaced by a recorder (tests/_recorder.py) that notes every call as (entry-point name, per argument: the
int / float value, or 1 / 0 for a pointer given / null) and launches nothing.  Its answers to the size queries are fixed:

    *_bytes, *_workspace -> 4096        *_chunks, *_slots -> 4        everything else -> 0 (hipSuccess)

`ops._stream` returns None and `ops._req` passes its tensor through.  tests/golden/dispatch_trace.json holds, per flag
setting and case, the sequence of entry-point names (as indices into its "entry_points" list) and a SHA-256 of the full
(name, arguments) sequence; a setting other than "f16x2" lists only the cases whose trace differs from that of "f16x2" --
which is exactly what the flag moves.  A case that raises ends in "raises <type>: <first words of the message>".  The
hot-path cases (some 800 launches each) keep the hash and, instead of the sequence, the launch count per entry point.

    python tests/test_dispatch_cpu.py --record      rewrites the file from the ops.py that is checked out

The file is a record of behaviour, not a specification: re-record it only in a change that means to move a launch, and
read the diff.  The GPU test at the end runs the `_conv_sliced` / `_wgrad` cases through the real library with the same
recorder and compares the names (the real size queries answer other values than the fake's, so no hashes there)."""
import hashlib
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import dcanet_amd  # noqa: E402,F401
from dcanet_amd import ops  # noqa: E402
from _recorder import Recorder  # noqa: E402

GOLDEN_FILE = os.path.join(ROOT, "tests", "golden", "dispatch_trace.json")

ALL_ON = dict(CONV_X2=True, CONV_X3=True, CONV_S2_X2=True, WGRAD_S2_X2=True, DECONV_X3=True, C1_WGRAD_FUSED=True,
              BN_FUSE=True, PAIR_FUSE=True, PACK=True, AMAX_EMIT=True, _X3_MIN_WORKGROUPS=1)
SETTINGS = {"f16x2": {}, "bf16x3": {"CONV_X2": False}, "fp32": {"CONV_X2": False, "CONV_X3": False},
            "min_workgroups": {"_X3_MIN_WORKGROUPS": 1 << 30}}
SETTINGS.update({"no_" + f: {f: False} for f in ("PACK", "BN_FUSE", "PAIR_FUSE", "CONV_S2_X2", "WGRAD_S2_X2", "DECONV_X3",
                                                 "C1_WGRAD_FUSED")})
WIDTHS = (24, 22)         # quarter-res widths with W % 4 == 0 and 2; the volumes are (1, C, 6, 10, W)


def _summary(calls, raised, counts=False):
    """(entry-point names in call order [+ "raises ..."], SHA-256 of the full (name, arguments) sequence); counts: the
    names as sorted "name*launches" instead"""
    names = [c[0] for c in calls] + (["raises " + raised] if raised else [])
    if counts:
        names = [f"{n}*{names.count(n)}" for n in sorted(set(names))]
    return names, hashlib.sha256(json.dumps([calls, raised]).encode()).hexdigest()


# ---- tensors -----------------------------------------------------------------------------------------------------------
def _t(dev, *shape, grad=False):
    t = torch.zeros(shape, device=dev)
    assert t.data_ptr() % 16 == 0
    return t.requires_grad_() if grad else t


def _unaligned(dev, *shape):
    n = 1
    for s in shape:
        n *= s
    t = torch.zeros(n + 1, device=dev)[1:].view(shape)      # a view one float into a buffer
    assert t.data_ptr() % 16 == 4
    return t


def _packed(dev, *shape, grad=False):
    return ops._tag_px2(_t(dev, *shape, grad=grad), torch.zeros(shape[1], dtype=torch.int32, device=dev))


def _operand(dev, kind, *shape):
    return {"f32": _t, "px2": _packed, "off4": _unaligned}[kind](dev, *shape)


class _PackGrad(torch.autograd.Function):
    """identity whose backward hands its gradient on as a packed px2 operand, the way _BnAct's does under pack_dy"""

    @staticmethod
    def forward(ctx, y):
        return y.view_as(y)

    @staticmethod
    def backward(ctx, g):
        return ops._tag_px2(g.clone(), torch.zeros(g.shape[1], dtype=torch.int32, device=g.device))


# ---- cases: (id, thunk) ------------------------------------------------------------------------------------------------
# geometry of a _conv_sliced call: id -> (C1, C2, B, ksize, stride, transposed, src_ab, flip)
CONV_GEOM = {
    "k3s1_32_32": (32, 0, 32, 3, 1, False, 0, 0),
    "k3s1_40_72": (40, 0, 72, 3, 1, False, 0, 0),
    "k3s1_bwd_data_32_32": (32, 0, 32, 3, 1, False, 1, 1),
    "k3s2_32_64": (32, 0, 64, 3, 2, False, 0, 0),
    "tr_64_32": (64, 0, 32, 3, 2, True, 1, 0),             # its input is the coarse tensor: W = 12 / 11
    "k1_32": (32, 0, 32, 1, 1, False, 0, 0),
    "k1_64": (64, 0, 64, 1, 1, False, 0, 0),
    "k1_32_32": (32, 32, 32, 1, 1, False, 0, 0),
    "k1_40": (40, 0, 32, 1, 1, False, 0, 0),               # a layout conv1_x3.hip is not built for
    "head_gemm_27": (32, 0, 27, 1, 1, False, 1, 0),        # _Conv3dC1.forward: the 27 taps as output channels
}
GPU_CONV = ("k3s1_32_32", "k3s2_32_64", "tr_64_32")
EPILOGUES = ("plain", "stats", "res_post", "bn", "bn_res_pre", "amax")


def _conv_dims(geom, W):
    return (3, 5, W // 2) if CONV_GEOM[geom][5] else (6, 10, W)


def _conv_case(dev, geom, dims, epi, xkind):
    C1, C2, B, ksize, stride, transposed, src_ab, flip = CONV_GEOM[geom]
    A, K = C1 + C2, ksize ** 3
    x = _operand(dev, xkind, 1, C1, *dims)
    x2 = _t(dev, 1, C2, *dims) if C2 else None
    w = _t(dev, A * B * K)
    odims = ops._out_dims(dims, ksize, stride, transposed)
    kw = {}
    if epi == "stats":
        kw["want_stats"] = True
    if epi == "amax":
        kw["emit_amax"] = True
    if epi == "res_post":
        kw["res_post"] = _t(dev, 1, B, *odims)
    if epi in ("bn", "bn_res_pre"):
        kw.update(scale=_t(dev, B), shift=_t(dev, B), slope=0.1)
    if epi == "bn_res_pre":
        kw["res_pre"] = _t(dev, 1, B, *odims)
    ops._conv_sliced(x, x2, w, A, B, K, src_ab, flip, ksize, stride, transposed, **kw)


def conv_cases(dev, geoms=tuple(CONV_GEOM)):
    for geom in geoms:
        for W in WIDTHS:
            dims = _conv_dims(geom, W)
            for epi in EPILOGUES:
                yield f"conv/{geom}/W{dims[2]}/{epi}", lambda g=geom, d=dims, e=epi: _conv_case(dev, g, d, e, "f32")
        dims = _conv_dims(geom, 24)
        yield f"conv/{geom}/W{dims[2]}/off4", lambda g=geom, d=dims: _conv_case(dev, g, d, "plain", "off4")
    for W in WIDTHS:     # packed operand: the f16x2 3x3x3 stride-1 kernel reads it, every other route must raise
        for geom, epi in (("k3s1_32_32", "plain"), ("k3s1_32_32", "stats"), ("k3s1_bwd_data_32_32", "res_post"),
                          ("k3s2_32_64", "plain")):
            if geom in geoms:
                yield f"conv/{geom}/W{W}/{epi}/px2", lambda g=geom, W=W, e=epi: _conv_case(dev, g, (6, 10, W), e, "px2")
    if "k1_32" in geoms:
        yield "conv/k1_32/S990/plain", lambda: _conv_case(dev, "k1_32", (5, 9, 22), "plain", "f32")    # voxels % 4 != 0
        yield "conv/k1_32/S990/stats", lambda: _conv_case(dev, "k1_32", (5, 9, 22), "stats", "f32")


# geometry of a _wgrad call: id -> (Cx, Cy, ksize, stride, dims of x, dims of dy)
def _wgrad_geoms():
    g = {}
    for W in WIDTHS:
        g[f"k3s1_32_32/W{W}"] = (32, 32, 3, 1, (6, 10, W), (6, 10, W))
        g[f"k3s1_40_72/W{W}"] = (40, 72, 3, 1, (6, 10, W), (6, 10, W))
        g[f"k3s2_32_64/W{W}"] = (32, 64, 3, 2, (6, 10, W), (3, 5, W // 2))      # Conv3d(32, 64, 3, stride 2)
        g[f"tr_64_32/W{W}"] = (32, 64, 3, 2, (6, 10, W), (3, 5, W // 2))        # ConvTranspose3d(64, 32): x = the fine gradient
        g[f"k1_32_64/W{W}"] = (32, 64, 1, 1, (6, 10, W), (6, 10, W))
        g[f"head_27/W{W}"] = (32, 27, 1, 1, (6, 10, W), (6, 10, W))
    g["k3s2_32_64/W20"] = (32, 64, 3, 2, (6, 10, 20), (3, 5, 10))               # fine W % 4 == 0, coarse W % 4 != 0
    g["k3s2_32_64/odd"] = (32, 64, 3, 2, (5, 9, 24), (3, 5, 12))                # odd fine dimensions
    g["k3s2_32_64/odd_W23"] = (32, 64, 3, 2, (5, 9, 23), (3, 5, 12))
    return g


WGRAD_GEOM = _wgrad_geoms()
GPU_WGRAD = tuple(f"{g}/W{W}" for g in GPU_CONV for W in WIDTHS)


def _wgrad_case(dev, geom, xkind, ykind):
    Cx, Cy, ksize, stride, xd, yd = WGRAD_GEOM[geom]
    K = ksize ** 3
    x, dy = _operand(dev, xkind, 1, Cx, *xd), _operand(dev, ykind, 1, Cy, *yd)
    gw = _t(dev, Cy * Cx * K)
    if geom.startswith("head"):
        ops._wgrad(x, dy, gw, 0, Cx, Cy, 1, 1, 1, 27)          # dw[ci * 27 + tap]
    else:
        ops._wgrad(x, dy, gw, 0, Cx, Cy, ksize, stride, Cx * K, K)


def wgrad_cases(dev, geoms=tuple(WGRAD_GEOM)):
    for geom in geoms:
        k3s1 = geom.startswith("k3s1")
        kinds = [("f32", "f32"), ("off4", "f32"), ("f32", "off4")]
        if k3s1 or geom in ("k3s2_32_64/W24", "k1_32_64/W24"):       # elsewhere a packed operand must raise
            kinds += [("px2", "f32"), ("f32", "px2"), ("px2", "px2")]
        for xk, yk in kinds:
            yield f"wgrad/{geom}/{xk}_{yk}", lambda g=geom, xk=xk, yk=yk: _wgrad_case(dev, g, xk, yk)


def _conv3d_node(W, xkind, stats, alias, packed_dy, geom="k3s1"):
    """_Conv3d.apply forward + backward"""
    dev = "cpu"
    x2 = None
    if geom == "k3s1":
        x, w, meta = _t(dev, 1, 32, 6, 10, W, grad=True), _t(dev, 32, 32, 3, 3, 3, grad=True), (1, False)
    elif geom == "k3s2":
        x, w, meta = _t(dev, 1, 32, 6, 10, W, grad=True), _t(dev, 64, 32, 3, 3, 3, grad=True), (2, False)
    elif geom == "tr":
        x, w, meta = _t(dev, 1, 64, 3, 5, W // 2, grad=True), _t(dev, 64, 32, 3, 3, 3, grad=True), (2, True)
    else:
        x, w, meta = _t(dev, 1, 32, 6, 10, W, grad=True), _t(dev, 32, 64, 1, 1, 1, grad=True), (1, False)
        x2 = _t(dev, 1, 32, 6, 10, W, grad=True)
    if xkind == "px2":
        ops._tag_px2(x, torch.zeros(32, dtype=torch.int32))
    if xkind == "twin":
        ops._tag_twin(x, _packed(dev, *x.shape))
    out = ops._Conv3d.apply(x, x2, w, meta[0], meta[1], stats, alias, packed_dy)
    out = out if isinstance(out, tuple) else (out,)
    y = _PackGrad.apply(out[0]) if packed_dy else out[0]
    roots, grads = [y], [torch.zeros_like(y)]
    if alias:
        roots.append(out[-1])
        grads.append(torch.zeros_like(out[-1]))
    torch.autograd.backward(roots, grads)


def node_cases():
    for W in WIDTHS:
        for xkind in ("f32", "px2", "twin"):
            for stats in (False, True):
                for alias in (False, True):
                    for pdy in (False, True):
                        if xkind == "px2" and alias:
                            continue                       # raises before any launch
                        yield (f"node/k3s1/W{W}/{xkind}/stats{int(stats)}_alias{int(alias)}_pdy{int(pdy)}",
                               lambda a=(W, xkind, stats, alias, pdy): _conv3d_node(*a))
        for geom in ("k3s2", "tr", "k1x2"):
            for stats in (False, True):
                yield f"node/{geom}/W{W}/stats{int(stats)}", lambda W=W, s=stats, g=geom: _conv3d_node(W, "f32", s, False, False, g)


def _layer(cin, cout, k=3, stride=1, transposed=False):
    if transposed:
        conv = torch.nn.ConvTranspose3d(cin, cout, 3, stride=2, padding=1, output_padding=1, bias=False)
    else:
        conv = torch.nn.Conv3d(cin, cout, k, stride=stride, padding=k // 2, bias=False)
    return conv, torch.nn.BatchNorm3d(cout)


def _chain(W, pack1, pack2, train=True, xkind="f32"):
    """convbn3d(alias=True, pack_out=pack1) -> convbn3d(pack_out=pack2) -> convbn3d, forward and backward"""
    layers = [_layer(32, 32) for _ in range(3)]
    for conv, bn in layers:
        bn.train(train)
    x = _operand("cpu", xkind, 1, 32, 6, 10, W).requires_grad_()
    with torch.set_grad_enabled(train):
        z1, xa = ops.convbn3d(x, *layers[0], slope=0.0, alias=True, pack_out=pack1)
        z2 = ops.convbn3d(z1, *layers[1], slope=0.0, pack_out=pack2)
        z3 = ops.convbn3d(z2, *layers[2], slope=0.0, res_post=xa)
        if pack2 == "both":
            z3 = z3 + ops.convbn3d(z2, *_layer(32, 64, 1), slope=1.0).sum()      # the second consumer of z2
    if train:
        z3.sum().backward()


def _single(W, kind, train, xkind="f32"):
    """one convbn3d of every other geometry, forward (and backward in training)"""
    x = _operand("cpu", xkind, 1, 64 if kind == "tr" else 32, *((3, 5, W // 2) if kind == "tr" else (6, 10, W)))
    x.requires_grad_(train)
    x2 = _t("cpu", 1, 32, 6, 10, W, grad=train) if kind == "k1x2" else None
    conv, bn = {"k3s2": lambda: _layer(32, 64, 3, 2), "tr": lambda: _layer(64, 32, transposed=True),
                "k1x2": lambda: _layer(64, 32, 1), "k3s1": lambda: _layer(32, 32), "head": lambda: _layer(32, 1), "k3_16_1": lambda: _layer(16, 1)}[kind]()
    if kind == "k3_16_1":
        x = _t("cpu", 1, 16, 6, 10, W, grad=train)
    bn.train(train)
    with torch.set_grad_enabled(train):
        z = ops.convbn3d(x, conv, bn, slope=0.0, x2=x2)
    if train:
        z.sum().backward()


def _pair(dims):
    (ca, ba), (cb, bb) = _layer(32, 64, 3, 2), _layer(32, 64, 1)
    x = _t("cpu", 1, 32, *dims, grad=True)
    za, zb = ops.convbn3d_pair(x, ca, ba, 0.0, cb, bb, 1.0, pack_a=True)
    (za.sum() + zb.sum()).backward()


def _head(W, cin):
    x, w = _t("cpu", 1, cin, 6, 10, W, grad=True), _t("cpu", 1, cin, 3, 3, 3, grad=True)
    ops.conv3d(x, w).sum().backward()


def layer_cases():
    for W in WIDTHS:
        for p1 in (False, True):
            for p2 in (False, True, "both"):
                yield f"convbn3d/chain/W{W}/train_{p1}_{p2}", lambda a=(W, p1, p2): _chain(*a)
        yield f"convbn3d/chain/W{W}/eval", lambda W=W: _chain(W, True, "both", train=False)
        for kind in ("k3s2", "tr", "k1x2", "head", "k3_16_1"):
            for train in (True, False):
                yield f"convbn3d/{kind}/W{W}/{'train' if train else 'eval'}", lambda a=(W, kind, train): _single(*a)
        yield f"pair/W{W}", lambda W=W: _pair((6, 10, W))
        yield f"c1/W{W}/32", lambda W=W: _head(W, 32)
        yield f"c1/W{W}/64", lambda W=W: _head(W, 64)
        yield f"c1/W{W}/16_generic", lambda W=W: _head(W, 16)
    yield "pair/odd_dims", lambda: _pair((5, 10, 24))
    # an fp32 input one float off 16-byte alignment: its gradient must stay fp32 (_pack_dy_ok), alias branch and plain one
    yield "convbn3d/chain/W24/train_True_both/off4", lambda: _chain(24, True, "both", xkind="off4")
    yield "convbn3d/k3s1/W24/train", lambda: _single(24, "k3s1", True)
    yield "convbn3d/k3s1/W24/train/off4", lambda: _single(24, "k3s1", True, xkind="off4")


def _hot_path(concat, train, W):
    from dcanet_amd.models.gwcnet_dca_g import GwcNet
    torch.manual_seed(0)
    m = GwcNet(24, use_concat_volume=concat).train(train)
    fl, fr = (_t("cpu", 1, 320, 10, W, grad=train) for _ in range(2))
    cl, cr = ((_t("cpu", 1, 12, 10, W, grad=train) for _ in range(2)) if concat else (None, None))
    with torch.set_grad_enabled(train):
        out = m.hot_path(fl, fr, cl, cr)
    if train:
        sum(v.sum() for v in out.values()).backward()


def hot_path_cases():
    for concat in (False, True):
        for W in WIDTHS:
            for train in (True, False):
                yield (f"hot_path/{'GC' if concat else 'G'}/W{W}/{'train' if train else 'eval'}",
                       lambda a=(concat, train, W): _hot_path(*a))


def cpu_cases(setting):
    yield from conv_cases("cpu")
    yield from wgrad_cases("cpu")
    yield from node_cases()
    yield from layer_cases()
    if setting == "f16x2":
        yield from hot_path_cases()


# ---- running -----------------------------------------------------------------------------------------------------------
def _apply(setattr_, setting):
    for k, v in {**ALL_ON, **SETTINGS[setting]}.items():
        setattr_(ops, k, v)


def _trace(thunk, setattr_, real=None):
    rec = Recorder(real)
    setattr_(ops, "_L", lambda: rec)
    raised = ""
    try:
        thunk()
    except RuntimeError as e:
        raised = type(e).__name__ + ": " + " ".join(str(e).split()[:6])
    return rec.calls, raised


def _cpu_patches(setattr_):
    setattr_(ops, "_stream", lambda: None)
    setattr_(ops, "_req", lambda t, name, packed_ok=False: t)
    setattr_(ops, "AMAX_STATS", {"tagged": 0, "computed": 0, "packed": 0})


def _expected(golden, setting, case):
    own = golden["traces"][setting].get(case)
    idx, sha = (own if own is not None else golden["traces"]["f16x2"][case]).split("#")
    names = [golden["entry_points"][int(i.split("*")[0])] + i[len(i.split("*")[0]):] for i in idx.split()]
    return names, sha


@pytest.fixture(scope="module")
def golden_trace():
    with open(GOLDEN_FILE) as f:
        return json.load(f)


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_dispatch_trace(setting, monkeypatch, golden_trace):
    _apply(monkeypatch.setattr, setting)
    _cpu_patches(monkeypatch.setattr)
    bad, seen = [], set()
    for case, thunk in cpu_cases(setting):
        got = _summary(*_trace(thunk, monkeypatch.setattr), counts=case.startswith("hot_path/"))
        want = _expected(golden_trace, setting, case)
        assert case not in seen, case
        seen.add(case)
        if got != want:
            bad.append(f"{case}:\n    recorded {' '.join(want[0])}\n    now      {' '.join(got[0])}"
                       + ("" if got[0] != want[0] else "\n    (same entry points, other arguments)"))
    assert not bad, f"{len(bad)} launches moved under '{setting}':\n" + "\n".join(bad)
    assert set(golden_trace["traces"][setting]) <= seen, sorted(set(golden_trace["traces"][setting]) - seen)


@pytest.mark.gpu
def test_dispatch_names_on_the_real_library(monkeypatch, golden_trace):
    """the `_conv_sliced` / `_wgrad` cases at (1,32,6,10,24), (1,32,6,10,22), stride 2 and transposed, through the real
    library: the names must be the recorded ones, i.e. the fake's size answers misled no CPU trace (the one place they could
    is `nsl <= CSLOTS` on the stride-2 route)"""
    _apply(monkeypatch.setattr, "f16x2")
    real = ops._L()
    bad = []
    for case, thunk in list(conv_cases("cuda", GPU_CONV)) + list(wgrad_cases("cuda", GPU_WGRAD)):
        if "off4" in case:       # `_req` re-aligns every operand before a kernel sees it: those cases pin host predicates only
            continue
        calls, raised = _trace(thunk, monkeypatch.setattr, real)
        got, want = _summary(calls, raised)[0], _expected(golden_trace, "f16x2", case)[0]
        print(case, "->", " ".join(got))
        if got != want:
            bad.append(f"{case}: recorded {' '.join(want)}, real library {' '.join(got)}")
    torch.cuda.synchronize()
    assert not bad, "\n".join(bad)


def record():
    def set_(obj, name, value):
        setattr(obj, name, value)
    raw = {}
    for setting in SETTINGS:
        _apply(set_, setting)
        _cpu_patches(set_)
        raw[setting] = {case: _summary(*_trace(thunk, set_), counts=case.startswith("hot_path/"))
                        for case, thunk in cpu_cases(setting)}
    table = sorted({n.split("*")[0] for cases in raw.values() for names, _ in cases.values() for n in names})
    token = lambda n: str(table.index(n.split("*")[0])) + n[len(n.split("*")[0]):]
    traces = {setting: {case: " ".join(token(n) for n in names) + "#" + sha
                        for case, (names, sha) in cases.items()
                        if setting == "f16x2" or (names, sha) != raw["f16x2"][case]}
              for setting, cases in raw.items()}
    with open(GOLDEN_FILE, "w") as f:
        json.dump({"entry_points": table, "traces": traces}, f, indent=0, sort_keys=True)
        f.write("\n")
    print({k: len(v) for k, v in traces.items()}, os.path.getsize(GOLDEN_FILE), "bytes")


if __name__ == "__main__":
    if "--record" in sys.argv:
        record()
