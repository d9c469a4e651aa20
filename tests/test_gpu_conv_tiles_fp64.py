"""The persistent forward / backward-data convolution kernels against fp64 beyond one tile per workgroup.

conv3d_f16x2.hip, conv3d_bf16x3.hip, conv3d_s2_f16x2.hip, deconv3d_x3.hip (fp32 grade) and conv3d_lp.hip, conv3d_s2_lp.hip,
deconv3d_lp.hip (reduced precision) share the tile walk of csrc/dca_tiles.h: `min(tiles, CUs / channel blocks)` workgroups,
each looping over its part of its XCD's chunk of the tiles.  The op-level parity tests reach them with at most a few dozen
tiles, one per workgroup on 256 CUs; what is delicate in these kernels -- the pipeline that fetches the next tile's first
chunk while the current tile's last chunk is multiplied, `dca_tile_advance`, the `on` mask behind the last chunk of the last
tile, the BatchNorm sums and per-channel maxima that accumulate over every tile before ONE flush -- runs only from the second
tile on.  Every row of tests/_conv_tile_cases.py sits on one regime of that walk (`mixed`, `deep`, `ragged`, `samples`, `idle`)
and does five things here: (1) computes the grid from the device's CU count, requires the kernel's own size query (where it
has one) to return it and the walk to be in the row's regime -- a row that drifts off its regime fails, it does not skip; (2)
asserts the route (`ops._conv_family`, or the reduced-precision entry point counted at the C ABI); (3) runs the kernel through
`ops` into memory that held NaN; (4) compares with fp64 at the gate of the existing parity test of the SAME kernel, per tile,
so a failure names the worst tile, its owner and its position in that workgroup's walk; (5) launches again and requires
the same bits (output, dx, statistics partials, y_cmax slots).  tests/test_conv_tile_cases_cpu.py checks the table, the
arithmetic and the references without a GPU.

Gates (the project's existing ones, unchanged).  conv3d_f16x2 / conv3d_bf16x3 forward, fused epilogue and dx: max-abs <=
1e-5 max(1, max|ref|) (`test_conv3d_bf16x3_path`, `test_conv3d_bf16x3_fused_epilogue`).  deconv3d_x3: max-abs <= 2e-6
max|ref|, with the fused epilogue <= 2e-6 max|ref_epi| + 2e-6 max|ref| (`test_deconv3d_bf16x3`).  conv3d_s2_f16x2: per
output channel, max-abs / max|ref_c| <= 3e-6 and <= 2 x the fp32 MFMA kernel's on the same data + 2e-7; with the epilogue
max-abs / (max|ref_epi_c| + max|ref_c|) <= 3e-6 (`test_conv3d_s2_f16x2_matches_fp64`).  Statistics: mean within 2e-6
max|mean| + 1e-6, variance and 1 / std within 2e-6 relative, counts exact (`test_conv3d_stats_fused`), against the mean and
biased variance of the fp64 output.  Reduced precision: |err| <= 2e-5 max(1, max|ref|) + ulp |ref| elementwise against the
fp64 evaluation of the rounded operands (tests/test_gpu_lowprec.py).

Not covered: operands above 2 GiB (every launcher refuses a sample whose byte offsets leave 31 bits; N alone can pass 2 GiB
and is not run here); a packed px2 operand with the inference epilogue (the launcher refuses it: the packed operand exists in
training only); `ragged` for the kernels with one grid row (deconv3d_x3, deconv3d_lp, conv3d_s2_lp), whose grid on 256 CUs is
256 or the tile count.

MEASURED on one MI355X (256 CUs); every test prints its row (max-abs error, that error over the gate at the worst
element, relative L2).  Max-abs / gate: conv3d_f16x2 0.04 .. 0.11, conv3d_bf16x3 0.06 .. 0.17, deconv3d_x3 0.20 .. 0.48,
conv3d_s2_f16x2 0.12 .. 0.39, conv3d_s2_lp 0.01 .. 0.02; the 2-byte results of conv3d_lp / deconv3d_lp 0.89 .. 0.98, where the
gate's `ulp |ref|` term is the rounding of the result itself.  Relative L2 1.2e-7 .. 5.8e-7 on the fp32-grade kernels.
Statistics: mean within 6.5e-8, variance within 1.1e-7 and 1 / std within 1.2e-7 relative.  The table per kernel and path is in
DESIGN.md, section 2.

That the gates bite (libraries built from a scratch copy, never committed).  `dca_my_tile_walk` made to drop the last tile
of every workgroup that owns two or more: all 69 rows fail.  Limited to workgroups with three or more tiles: exactly the
30 `deep` rows fail while every existing parity test of these kernels passes.  The statistics sums made to take a workgroup's
first tile only (counts left right): all 16 statistics rows fail, test_conv3d_stats_fused at one shape of eleven."""
import pytest
import torch

import _conv_tile_cases as T
from oracle.seeded import seeded_tensor

pytestmark = pytest.mark.gpu

DEV = "cuda"
LPT = {"bf16": torch.bfloat16, "fp16": torch.float16}
ULP = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11}
SLOPE = 0.1
_TRUTH = {}      # (data key, name) -> fp64 reference tensor
_ROWS = []       # the rows printed so far


def _mods():
    import dcanet_amd  # noqa: F401
    from dcanet_amd import ops
    return ops


def _route(monkeypatch, ops, kernel):
    """the flags that send a convolution to `kernel`'s family"""
    monkeypatch.setattr(ops, "CONV_X3", True)
    monkeypatch.setattr(ops, "CONV_X2", kernel != "x3")
    monkeypatch.setattr(ops, "CONV_S2_X2", True)
    monkeypatch.setattr(ops, "DECONV_X3", True)
    monkeypatch.setattr(ops, "AMAX_EMIT", True)
    monkeypatch.setattr(ops, "_X3_MIN_WORKGROUPS", 1)


def _regime(ops, case):
    """the launch geometry on THIS device; the kernel's size query must give the same grid and the walk must be in every
    regime the row names"""
    ncu = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    g = T.geometry(case, ncu)
    N, A, B, dims = T.launch_of(case)
    lib = ops._L()
    query = {"x2": lambda: lib.dca_conv3d_x2_stats_chunks(N, B, *dims),
             "x3": lambda: lib.dca_conv3d_x3_stats_chunks(N, B, *dims),
             "dx3": lambda: lib.dca_deconv3d_x3_stats_chunks(N, *dims),
             "s2x2": lambda: lib.dca_conv3d_s2x2_out_slots(N, B, *dims)}
    if case.kernel in query:
        got = query[case.kernel]()
        assert got == g.grid, f"{case.id}: the size query gives {got} workgroups, the restated grid rule {g.grid} ({ncu} CUs)"
    for r in case.regimes:
        assert T.REGIMES[r](g) is True, (f"{case.id} is not in its regime on this device: {r} (tiles {g.tiles}, share "
                                         f"{g.share}, grid {g.grid}, {ncu} CUs)")
    return g


def _t(case, name):
    return T.tensor(case, name, seeded_tensor)


def _truth(case, name, build):
    key = (T.data_key(case), name)
    if key not in _TRUTH:
        _TRUTH[key] = build()
    return _TRUTH[key]


def _y_ref(case):
    """fp64 output of the row's operator on its (for the reduced-precision rows: rounded) operands"""
    stride, transposed = T.op_of(case)

    def build():
        x, w = _t(case, "x"), _t(case, "w")
        if case.lp:
            x, w = x.to(LPT[case.lp]), w.to(LPT[case.lp])
        return T.ref_forward(x, w, stride, transposed)
    return _truth(case, "y", build)


def _poison(shape, dtype=torch.float32):
    """fills a block of the output's size with NaN and frees it, so that the caching allocator hands the launch under test
    memory in which a tile that is never written stays NaN"""
    t = torch.full(tuple(shape), float("nan"), device=DEV, dtype=dtype)
    del t


_HEAD = (f"\n{'row':22s} {'grid':>4s} {'tiles':>5s} {'walk':>5s}  {'what':8s} {'max err':>9s} {'/ gate':>6s}  {'rel L2':>9s} "
         f"{'max|ref|':>9s}")


def _gate(capsys, case, g, what, got, ref, lim):
    """prints the row, then requires |got - ref| <= lim (a number or a tensor that broadcasts against ref) everywhere, naming
    the worst tile"""
    gotd = got.detach().cpu().double()
    assert gotd.shape == ref.shape, (case.id, what, gotd.shape, ref.shape)
    err = (gotd - ref).abs()
    ratio = err / lim
    lens = [len(w) for w in g.walk]
    worst = torch.nan_to_num(ratio, nan=float("inf")).max().item()
    el2 = (torch.nan_to_num(err, nan=float("inf")).norm() / ref.norm().clamp_min(1e-300)).item()
    emax = torch.nan_to_num(err, nan=float("inf")).max().item()
    with capsys.disabled():
        if not _ROWS:
            print(_HEAD)
        print(f"{case.id:22s} {g.grid:4d} {g.tiles:5d} {min(lens):2d}..{max(lens):<2d} {what:8s} {emax:9.2e} {worst:6.3f}  "
              f"{el2:9.2e} {ref.abs().max().item():9.2e}")
    _ROWS.append(case.id)
    assert worst <= 1.0, f"{case.id} {what}: max err {emax:.3e}; {T.worst_tile(ratio, g)}"


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same_bits(case, what, a, b):
    assert torch.equal(_bits(a), _bits(b)), f"{case.id} {what}: not bitwise reproducible"


def _check_cmax(ops, case, g, y):
    """the y_cmax slots of the f16x2 epilogues: one slot per (channel, workgroup); their maximum is max |y| of the kernel's
    own output bit for bit (what the exponents of a following f16x2 convolution are derived from), a workgroup without
    tiles writes zero"""
    tag = getattr(y, "_dca_cmax", None)
    assert tag is not None, f"{case.id}: the epilogue did not tag its per-channel maxima"
    slots, nslots, _ = tag
    assert nslots == g.grid, (case.id, nslots, g.grid)
    C = y.shape[1]
    s = slots.view(torch.float32).view(C, ops.CSLOTS)[:, :nslots]
    assert bool(torch.isfinite(s).all()) and bool((s >= 0).all()), f"{case.id}: a y_cmax slot was not written"
    assert torch.equal(s.amax(1), y.abs().amax((0, 2, 3, 4))), f"{case.id}: the slots' maximum is not max |y|"
    idle = [wg for wg, w in enumerate(g.walk) if not w]
    if "idle" in case.regimes:
        assert idle
    for wg in idle:
        assert bool((s[:, wg] == 0).all()), f"{case.id}: workgroup {wg} has no tile, its y_cmax slot is not zero"
    # every workgroup's slot is the maximum over ITS tiles of the kernel's own output: slot index = blockIdx.x in every
    # channel block, so the maximum over the channels of a slot is the maximum over that workgroup's tiles
    per = T.tile_max(y.detach().abs().cpu().double(), g)
    want = torch.tensor([max([per[t].item() for t in w], default=0.0) for w in g.walk], dtype=torch.float64)
    bad = (s.cpu().double().amax(0) != want).nonzero().flatten().tolist()
    assert not bad, f"{case.id}: the y_cmax slots of workgroups {bad[:8]} are not the maxima over their tiles {g.walk[bad[0]]}"
    return s.clone()


def _voxels_per_workgroup(g, odims):
    """output voxels inside the volume of every workgroup's tiles"""
    out = []
    for w in g.walk:
        n = 0
        for t in w:
            _, td, th, tw = T.decode(t, g.N, g.nT)
            ext = [min(e, d - i * e) for e, d, i in zip(g.out_tile, odims, (td, th, tw))]
            n += ext[0] * ext[1] * ext[2]
        out.append(float(n))
    return torch.tensor(out, dtype=torch.float64)


def _check_stats(capsys, ops, case, g, y, part, y_ref):
    """the partials {K, n, s, q} per (channel, workgroup): exact counts per workgroup (a workgroup without tiles flushes
    zeros), mean and biased variance of the fp64 output at the gate of test_conv3d_stats_fused, and the finalize kernel"""
    C = y.shape[1]
    assert part.numel() == C * g.grid * 4, (case.id, part.numel(), C, g.grid)
    p = part.cpu().view(C, g.grid, 4)
    assert bool(torch.isfinite(p).all()), f"{case.id}: a statistics partial was not written"
    want_n = _voxels_per_workgroup(g, tuple(y.shape[2:]))
    bad = (p[..., 1] != want_n.view(1, -1)).any(0).nonzero().flatten().tolist()
    assert not bad, (f"{case.id}: workgroups {bad[:8]} count {p[0, bad[0], 1].item():.0f} voxels, their tiles "
                     f"{g.walk[bad[0]]} hold {want_n[bad[0]].item():.0f}")
    for wg, w in enumerate(g.walk):
        if not w:
            assert bool((p[:, wg, 1:] == 0).all()), f"{case.id}: workgroup {wg} has no tile, its partial is not zero"
    if "idle" in case.regimes:
        assert any(not w for w in g.walk)
    cnt, mean, var = T.fold_partials(part, C)
    mean_ref, var_ref = T.ref_stats(y_ref)
    assert bool((cnt == float(y_ref.numel() // C)).all())
    e_mean = (mean - mean_ref).abs().max().item()
    e_var = ((var - var_ref).abs() / var_ref).max().item()
    assert e_mean <= 2e-6 * mean_ref.abs().max().item() + 1e-6, \
        f"{case.id}: mean off by {e_mean:.3e} (variance by {e_var:.3e} relative)"
    assert e_var <= 2e-6, f"{case.id}: variance off by {e_var:.3e} relative"
    bn = torch.nn.BatchNorm3d(C).to(DEV)
    stats = ops.bn_stats_vector(y, bn.weight, bn.bias, bn.running_mean, bn.running_var, True, 0.1, 1e-5, part)
    assert (stats[:C].double().cpu() - mean_ref).abs().max().item() <= 2e-6 * mean_ref.abs().max().item() + 1e-6
    inv_ref = 1.0 / torch.sqrt(var_ref + 1e-5)
    e_inv = ((stats[C:2 * C].double().cpu() - inv_ref).abs() / inv_ref).max().item()
    assert e_inv <= 2e-6, f"{case.id}: 1 / std off by {e_inv:.3e} relative"
    with capsys.disabled():
        print(f"{'':40s} statistics: mean {e_mean:.2e} (max|mean| {mean_ref.abs().max().item():.2e}), variance {e_var:.2e} "
              f"and 1 / std {e_inv:.2e} relative")


# ---- conv3d_f16x2, conv3d_bf16x3, deconv3d_x3: forward ------------------------------------------------------------------------------
FWD = [c for c in T.X2 + T.X3 + T.DX3 if not {"dx", "bwd"} & set(c.tags)]


@pytest.mark.parametrize("case", FWD, ids=[c.id for c in FWD])
def test_forward_many_tiles(case, monkeypatch, capsys):
    """plain output, the fused inference epilogue (on f16x2 with the y_cmax hand-off) and the training forward with fused
    BatchNorm statistics; fp32 input on the quad and the single-voxel staging, and the packed px2 input of f16x2"""
    ops = _mods()
    _route(monkeypatch, ops, case.kernel)
    g = _regime(ops, case)
    stride, transposed = T.op_of(case)
    split = case.kernel in ("x2", "x3")
    xg, wg = _t(case, "x").to(DEV), _t(case, "w").to(DEV)
    y_ref = _y_ref(case)
    top = y_ref.abs().max().item()
    lim_plain = 1e-5 * max(1.0, top) if split else 2e-6 * top
    xin = ops.pack_x2(xg) if "px2" in case.tags else xg
    assert ops._is_packed(xin) == ("px2" in case.tags)
    oshape = tuple(y_ref.shape)
    with torch.no_grad():
        if "epi" in case.tags:
            sc, sh, rp, rq = (_t(case, n).to(DEV) for n in ("scale", "shift", "res_pre", "res_post"))
            assert ops._conv_family(xin, None, case.Cin, case.Cout, 3, stride, transposed, sc, rp, SLOPE) == T.FAMILY[case.kernel]
            ref = _truth(case, "epi", lambda: T.ref_epilogue(y_ref, sc, sh, SLOPE, rp, rq))
            lim = 1e-5 * max(1.0, ref.abs().max().item()) if split else 2e-6 * ref.abs().max().item() + 2e-6 * top
            run = lambda: ops.conv3d_fused_inference(xin, wg, stride, transposed, sc, sh, SLOPE, rp, rq)
            _poison(oshape)
            y = run()
            _gate(capsys, case, g, "epilogue", y, ref, lim)
            again = run()
            _same_bits(case, "epilogue", y, again)
            if case.kernel == "x2":
                _same_bits(case, "y_cmax", _check_cmax(ops, case, g, y), _check_cmax(ops, case, g, again))
        elif "stats" in case.tags:
            assert ops._conv_family(xin, None, case.Cin, case.Cout, 3, stride, transposed) == T.FAMILY[case.kernel]
            run = lambda: ops._Conv3d.apply(xin, None, wg, stride, transposed, True)
            _poison(oshape)
            y, part = run()
            _gate(capsys, case, g, "stats y", y, y_ref, lim_plain)
            _check_stats(capsys, ops, case, g, y, part, y_ref)
            y2, part2 = run()
            _same_bits(case, "y", y, y2)
            _same_bits(case, "statistics partials", part.view(torch.int64), part2.view(torch.int64))
            _same_bits(case, "stats y against the plain launch", y, ops.conv3d(xin, wg, stride, transposed))
        else:
            assert ops._conv_family(xin, None, case.Cin, case.Cout, 3, stride, transposed) == T.FAMILY[case.kernel]
            run = lambda: ops.conv3d(xin, wg, stride, transposed)
            _poison(oshape)
            y = run()
            _gate(capsys, case, g, "forward", y, y_ref, lim_plain)
            _same_bits(case, "forward", y, run())


# ---- backward-data through autograd ---------------------------------------------------------------------------------------------------
BWD = [c for c in T.X2 + T.X3 + T.DX3 if {"dx", "bwd"} & set(c.tags)]


@pytest.mark.parametrize("case", BWD, ids=[c.id for c in BWD])
def test_backward_data_many_tiles(case, monkeypatch, capsys):
    """dx of the stride-1 convolution with Cin = 40 (the split kernel over dy with a partial second block of output channels)
    and dx of the stride-2 convolution (deconv3d_x3 over the coarse dy), as ops._Conv3d.backward launches them"""
    ops = _mods()
    _route(monkeypatch, ops, "x2" if case.kernel == "dx3" else case.kernel)
    g = _regime(ops, case)
    stride, _ = T.op_of(case)
    x, w, gy = _t(case, "x"), _t(case, "w"), _t(case, "gy")
    wg, gyg = w.to(DEV), gy.to(DEV)
    N, A, B, dims = T.launch_of(case)
    assert tuple(gy.shape) == (N, A) + tuple(dims)
    # the launch _Conv3d.backward makes: the kernel over dy, transposed for the stride-2 convolution
    assert ops._conv_family(gyg, None, A, B, 3, stride, stride == 2) == T.FAMILY[case.kernel]
    ref = _truth(case, "dx", lambda: T.ref_backward_data(x.shape, w, gy, stride, False))
    lim = 1e-5 * max(1.0, ref.abs().max().item()) if stride == 1 else 2e-6 * ref.abs().max().item()

    def run():
        xg = x.to(DEV).requires_grad_()
        y = ops.conv3d(xg, wg, stride, False)
        _poison(x.shape)
        (gx,) = torch.autograd.grad(y, [xg], gyg)
        return gx
    gx = run()
    _gate(capsys, case, g, "dx", gx, ref, lim)
    _same_bits(case, "dx", gx, run())


# ---- conv3d_s2_f16x2 ------------------------------------------------------------------------------------------------------------------
def _chan(t):
    return t.abs().amax((0, 2, 3, 4)).view(1, -1, 1, 1, 1)


@pytest.mark.parametrize("case", T.S2X2, ids=[c.id for c in T.S2X2])
def test_conv3d_s2_f16x2_many_tiles(case, monkeypatch, capsys):
    """plain and with the inference epilogue (folded BatchNorm, leaky ReLU, res_post, y_cmax slots), per output channel at the
    gate of test_conv3d_s2_f16x2_matches_fp64, the fp32 MFMA kernel on the same data as the yardstick"""
    ops = _mods()
    _route(monkeypatch, ops, "s2x2")
    g = _regime(ops, case)
    xg, wg = _t(case, "x").to(DEV), _t(case, "w").to(DEV)
    y_ref = _y_ref(case)
    scale = _chan(y_ref).clamp_min(1e-30)
    with torch.no_grad():
        if "epi" in case.tags:
            sc, sh, rq = (_t(case, n).to(DEV) for n in ("scale", "shift", "res_post"))
            assert ops._conv_family(xg, None, case.Cin, case.Cout, 3, 2, False, sc, None, SLOPE) == "s2x2"
            ref = _truth(case, "epi", lambda: T.ref_epilogue(y_ref, sc, sh, SLOPE, None, rq))
            run = lambda: ops.conv3d_fused_inference(xg, wg, 2, False, sc, sh, SLOPE, None, rq)
            _poison(y_ref.shape)
            y = run()
            _gate(capsys, case, g, "epilogue", y, ref, 3e-6 * (_chan(ref) + scale))
            again = run()
            _same_bits(case, "epilogue", y, again)
            _same_bits(case, "y_cmax", _check_cmax(ops, case, g, y), _check_cmax(ops, case, g, again))
        else:
            assert ops._conv_family(xg, None, case.Cin, case.Cout, 3, 2, False) == "s2x2"
            monkeypatch.setattr(ops, "CONV_S2_X2", False)
            assert ops._conv_family(xg, None, case.Cin, case.Cout, 3, 2, False) == "mfma"
            y32 = ops.conv3d(xg, wg, 2, False)
            err32 = ((y32.cpu().double() - y_ref).abs() / scale).max().item()
            monkeypatch.setattr(ops, "CONV_S2_X2", True)
            run = lambda: ops.conv3d(xg, wg, 2, False)
            _poison(y_ref.shape)
            y = run()
            _gate(capsys, case, g, "forward", y, y_ref, min(3e-6, 2 * err32 + 2e-7) * scale)
            _same_bits(case, "forward", y, run())


# ---- reduced precision ----------------------------------------------------------------------------------------------------------------
def _counted(monkeypatch, lib, name):
    """counts the calls of a C entry point"""
    calls = []
    real = getattr(lib, name)

    def wrapped(*a):
        calls.append(name)
        return real(*a)
    monkeypatch.setattr(lib, name, wrapped)
    return calls


@pytest.mark.parametrize("case", T.LP, ids=[c.id for c in T.LP])
def test_reduced_precision_many_tiles(case, monkeypatch, capsys):
    """conv3d_lp, conv3d_s2_lp and deconv3d_lp in bf16 and fp16 against the fp64 evaluation of the rounded operands, with
    the folded BatchNorm, leaky ReLU and res_post epilogue each of them has in the network"""
    ops = _mods()
    lib = ops._L()
    g = _regime(ops, case)
    lp = LPT[case.lp]
    x, w = _t(case, "x"), _t(case, "w")
    sc, sh = _t(case, "scale"), _t(case, "shift")
    y_ref = _y_ref(case)
    entry = {"lp": "dca_conv3d_lp_forward", "s2lp": "dca_conv3d_s2_lp_forward", "dlp": "dca_deconv3d_lp_forward"}[case.kernel]
    calls = _counted(monkeypatch, lib, entry)
    other = _counted(monkeypatch, lib, "dca_conv3d_forward_mixed")
    with torch.no_grad():
        if case.kernel == "s2lp":        # 2-byte x -> fp32 y, no residuals
            ref = _truth(case, "epi", lambda: T.ref_epilogue(y_ref, sc, sh, SLOPE))
            lim = 2e-5 * max(1.0, ref.abs().max().item())
            xg = x.to(lp).to(DEV)
            run = lambda: ops.conv3d_s2_lp(xg, w.to(DEV), sc.to(DEV), sh.to(DEV), SLOPE)
            odt = torch.float32
        else:
            rq = _t(case, "res_post").to(lp)
            ref = _truth(case, "epi", lambda: T.ref_epilogue(y_ref, sc, sh, SLOPE, None, rq))
            lim = 2e-5 * max(1.0, ref.abs().max().item()) + ULP[case.lp] * ref.abs()
            odt = lp
            if case.kernel == "lp":      # 2-byte x -> 2-byte y
                xg = x.to(lp).to(DEV)
                run = lambda: ops.conv3d_lp(xg, w.to(DEV), lp, sc.to(DEV), sh.to(DEV), SLOPE, None, rq.to(DEV), lp)
            else:                        # fp32 x (rounded on the fly) -> 2-byte y
                xg = x.to(DEV)
                run = lambda: ops.deconv3d_lp(xg, w.to(DEV), lp, sc.to(DEV), sh.to(DEV), SLOPE, None, rq.to(DEV))
        _poison(ref.shape, odt)
        y = run()
        assert calls == [entry] and not other, (case.id, calls, other)
        assert y.dtype == odt
        _gate(capsys, case, g, case.lp, y, ref, lim)
        assert torch.equal(y, run()), f"{case.id}: not bitwise reproducible"
