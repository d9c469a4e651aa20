"""The streaming 1x1x1 convolution kernels against fp64 beyond one group per wave.

`conv1_x3_kernel` (conv1_x3.hip, fp32 grade on the bf16x3 split), `conv1_mfma_kernel` (conv3d_mfma.hip, fp32 MFMA) and
`conv1_lp_kernel` (conv1_lp.hip, bf16 / fp16) serve the q / k / v / out projections, `cva.fuse` over two inputs,
`cost_agg.redir` and the 27-tap GEMM of the logit heads.  They share one walk: a wave owns groups of 128 voxels of one sample,
`min(ceil(T / 4), 2048)` workgroups of four waves are launched, and wave u loops over the groups u, u + 4 * grid, ...  The
op-level parity tests reach them with at most 30 groups, one trip per wave; what is delicate -- the sample / voxel decode of
a later group, the buffer descriptors rebuilt per group, the statistics shift taken on a wave's first group and reused, the
register or LDS sums that run across groups, the one `fs_flush` per workgroup -- runs only from the second trip on (six
trips per wave at the bench shape).  Every row of tests/_c1_stream_cases.py sits on regimes of that walk (`mixed`, `deep`,
`samples`, `shift`, `idle`) and does five things here: (1) asserts the regimes again from its N and S and requires the
library's size query to give the restated grid on THIS device (the cap is a constant: no row depends on the CU count, none
skips); (2) asserts the route (a spy on `ops._conv_family`, the launches counted at the C ABI, `part.numel() > 0`); (3) runs
through `ops` into memory that held NaN; (4) compares with fp64 at the gate of the existing parity test of the SAME kernel,
per group, so a failure names the worst group, its wave and the trip of that wave's loop; (5) launches again and requires
the same bits (y, dx, statistics partials).  tests/test_c1_stream_cases_cpu.py checks the table, the arithmetic and the
references without a GPU.

Gates (the project's existing ones, unchanged).  conv1_x3 / conv1_mfma forward, fused epilogue and dx: max-abs <= 1e-5
max(1, max|ref|) (`test_conv1x1_two_inputs`, `test_fused_inference_epilogue_unaligned_width`).  Statistics: mean within 2e-6
max|mean| + 1e-6, variance and 1 / std within 2e-6 relative, counts exact (`test_conv3d_stats_fused`) -- against the mean
and biased variance of the fp64 output, not of the kernel's own.  conv1_lp: |err| <= 2e-5 max(1, max|ref|) + ulp |ref|
elementwise against the fp64 evaluation of the rounded operands (`test_conv1x1_lp`).

Not covered: samples above the 31-bit per-sample offset limit (the launchers refuse them); `Cin` layouts
`dca_conv3d_forward` rejects for k = 1 (40 channels, for example); the weight gradient of the 1x1x1 convolutions, which
tests/test_gpu_wgrad_fp64.py rows `g1` / `head` gate in the many-tile regime.

MEASURED on one MI355X (256 CUs); every test prints its row (max-abs error, that error over the gate at the worst element,
relative L2) and its wall time.  Max-abs / gate: conv1_x3 forward and statistics forward 0.016 .. 0.033 (max-abs 7.0e-7 ..
2.0e-6, relative L2 6.9e-8 .. 1.1e-7), inference epilogue 0.014 .. 0.022 (5.0e-8 .. 6.5e-8), dx / dx2 0.018 .. 0.022 (6.9e-8
.. 7.1e-8); conv1_mfma VEC form 0.022 .. 0.031 (6.3e-8 .. 1.0e-7), scalar form 0.022 .. 0.043 (6.6e-8 .. 1.4e-7); conv1_lp with
fp32 output 0.004 .. 0.005 (2.9e-8 .. 4.4e-8); its 2-byte outputs 0.983 .. 0.987 in bf16 (relative L2 1.7e-3) and 0.927 .. 0.944
in fp16 (2.1e-4), where the gate's `ulp |ref|` term is the rounding of the result itself.  Statistics: mean within 9.6e-9 ..
4.6e-8 (max|mean| 1.7e-3 .. 9.3e-2), variance within 4.0e-9 .. 2.6e-7 and 1 / std within 6.8e-8 .. 1.7e-7 relative.  No row is
near a gate that carries no `ulp |ref|` term.  32 tests in 28 s; the slowest row is x3-M-64to64-epi at 1.6 s.  The table per
kernel and path is in DESIGN.md, section 2.

That the gates bite (libraries built from a scratch copy, never committed).  (a) The group loop of all three kernels made
to stop after a wave's first group: the 31 `mixed` and `deep` rows fail (the dropped groups read NaN, or what the memory held
before), the `idle` row -- one group per wave -- passes, and so does every existing parity test of these kernels (`test_conv3d`,
`test_conv1x1_two_inputs`, `test_conv1x1_both_sides_of_the_voxel_count_predicate`,
`test_fused_inference_epilogue_unaligned_width`, `test_conv1x1_lp`, `test_conv3d_stats_fused`,
`test_stat_part_is_the_queried_size`).  (b) The STATS sums of conv1_x3 made to take the wave's first group only, counts left
right: the five statistics rows on M and D fail (mean off by 6e-3 .. 2e-2, variance by 1 % .. 2 %); x3-I-32-stats cannot see
it (no wave of that launch has a second group) and `test_conv3d_stats_fused` passes.  (c) `co_off` ignored in the epilogue's
residual reads: x3-M-64to64-epi fails (every group, 9.7 max-abs); the other nine conv1_x3 forward rows without statistics,
`test_conv1x1_*` and `test_fused_inference_epilogue_unaligned_width` pass.

One defect, found by mutation (a) and not by a row: the shift K of a statistics slot was written to LDS by lane 0 of a wave
half and read back by the whole half with nothing between the two that orders them for the compiler.  The shipped code
object wrote first; built with a group loop of one trip the compiler read first, every lane but lane 0 centred on 0 while
the partial said K, and `test_conv3d_stats_fused` failed at all four 1x1x1 shapes (mean off by about |K|).  conv1_x3.hip now
puts a wavefront-scope release / acquire fence pair around a wave barrier behind the write (no instruction; the statistics
forms also stop spilling: 256 -> 198, 250 -> 186, 256 -> 202 registers, 24 / 0 / 36 -> 0 bytes of scratch).  The
measurements above are the same before and after, and the train step takes 90.21 against 90.21 ms (means of three
alternating runs).  conv3d_bf16x3.hip and deconv3d_x3.hip hand K over in the same way and are not changed here.
"""
import time

import pytest
import torch

import _c1_stream_cases as T
from oracle.seeded import seeded_tensor

pytestmark = pytest.mark.gpu

DEV = "cuda"
LPT = {"bf16": torch.bfloat16, "fp16": torch.float16}
ULP = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11}
SLOPE = 0.1
_TRUTH = {}      # (data key, name) -> tensor on the host; the entries of ONE data key at a time (the rows are sorted by key)
_ROWS = []       # the rows printed so far


def _mods():
    import dcanet_amd  # noqa: F401
    from dcanet_amd import ops
    return ops


def _by_key(rows):
    return sorted(rows, key=lambda c: tuple(map(str, T.data_key(c))))


def _truth(case, name, build):
    key = T.data_key(case)
    if any(k[0] != key for k in _TRUTH):
        _TRUTH.clear()
    if (key, name) not in _TRUTH:
        _TRUTH[(key, name)] = build()
    return _TRUTH[(key, name)]


def _t(case, name):
    return _truth(case, "in." + name, lambda: T.tensor(case, name, seeded_tensor))


def _regime(ops, case):
    """the walk of the row; the regimes it names hold, and the library's size query gives the restated grid on this device"""
    N, S, _ = T.shape_of(case)
    g = T.geometry(N, S)
    for r in case.regimes:
        assert T.REGIMES[r](g) is True, f"{case.id} is not in its regime: {r} (S {S}, G {g.G}, T {g.T}, grid {g.grid})"
    got = ops._L().dca_conv1_x3_stats_chunks(N, S)
    ncu = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    assert got == g.grid, f"{case.id}: the size query gives {got} workgroups on {ncu} CUs, the restated grid rule {g.grid}"
    return g


def _spy_family(monkeypatch, ops):
    """records what ops._conv_family answers for every 1x1x1 convolution"""
    seen = []
    real = ops._conv_family

    def spy(x, x2, A, B, ksize, *a, **kw):
        fam = real(x, x2, A, B, ksize, *a, **kw)
        if ksize == 1:
            seen.append(fam)
        return fam
    monkeypatch.setattr(ops, "_conv_family", spy)
    return seen


def _counted(monkeypatch, lib, name):
    """counts the calls of a C entry point"""
    calls = []
    real = getattr(lib, name)

    def wrapped(*a):
        calls.append(name)
        return real(*a)
    monkeypatch.setattr(lib, name, wrapped)
    return calls


def _poison(shape, dtype=torch.float32):
    """fills a block of the output's size with NaN and frees it, so that the caching allocator hands the launch under test
    memory in which a group that is never written stays NaN"""
    t = torch.full(tuple(shape), float("nan"), device=DEV, dtype=dtype)
    del t


_HEAD = (f"\n{'row':22s} {'grid':>4s} {'groups':>6s} {'trips':>5s}  {'what':8s} {'max err':>9s} {'/ gate':>6s}  {'rel L2':>9s} "
         f"{'max|ref|':>9s}")


def _gate(capsys, case, g, what, got, ref, lim):
    """prints the row, then requires |got - ref| <= lim (a number or a tensor of ref's shape) everywhere, naming the worst
    group.  `got` is on the host"""
    gotd = got.double()
    assert gotd.shape == ref.shape, (case.id, what, gotd.shape, ref.shape)
    finite = bool(torch.isfinite(gotd).all())
    err = (gotd - ref).abs_()
    del gotd
    el2 = (err.norm() / ref.norm().clamp_min(1e-300)).item()
    emax = err.max().item()
    ratio = err.div_(lim)
    worst = ratio.max().item()
    lens = [len(w) for w in g.waves]
    with capsys.disabled():
        if not _ROWS:
            ncu = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
            print(f"\n{torch.cuda.get_device_name()}: {ncu} CUs" + _HEAD)
        print(f"{case.id:22s} {g.grid:4d} {g.T:6d} {min(lens):2d}..{max(lens):<2d} {what:8s} {emax:9.2e} {worst:6.3f}  "
              f"{el2:9.2e} {ref.abs().max().item():9.2e}")
    _ROWS.append(case.id)
    assert finite and worst <= 1.0, f"{case.id} {what}: max err {emax:.3e}; {T.worst_group(ratio, g.N, g.S)}"


def _bits(t):
    return t.view({4: torch.int32, 2: torch.int16, 8: torch.int64}[t.element_size()])


def _same_bits(case, what, a, b):
    assert torch.equal(_bits(a), _bits(b.cpu())), f"{case.id} {what}: not bitwise reproducible"


def _dev(t):
    return None if t is None else t.to(DEV)


def _operands(case):
    """x, x2 (or None), w of the row on the host; for the reduced-precision rows x and x2 in the 2-byte type"""
    x, w = _t(case, "x"), _t(case, "w")
    x2 = _t(case, "x2") if case.C2 else None
    if case.lp:
        x = _truth(case, "lp.x", lambda: x.to(LPT[case.lp]))
        x2 = None if x2 is None else _truth(case, "lp.x2", lambda: x2.to(LPT[case.lp]))
    return x, x2, w


def _y_ref(case):
    """fp64 output of the row's operator on its (for the reduced-precision rows: rounded) operands"""
    def build():
        x, x2, w = _operands(case)
        return T.ref_forward(x, x2, w.to(LPT[case.lp]) if case.lp else w)
    return _truth(case, "y", build)


def _epilogue(case, odt=torch.float32):
    """(scale, shift, res_pre, res_post) on the host and the fp64 result of the epilogue"""
    sc, sh = _t(case, "scale"), _t(case, "shift")
    rp = _truth(case, f"rp.{odt}", lambda: _t(case, "res_pre").to(odt))
    rq = _truth(case, f"rq.{odt}", lambda: _t(case, "res_post").to(odt))
    ref = _truth(case, f"epi.{odt}", lambda: T.ref_epilogue(_y_ref(case), sc, sh, SLOPE, rp, rq))
    return sc, sh, rp, rq, ref


def _timed(capsys, case, t0):
    with capsys.disabled():
        print(f"{'':40s} {case.id}: {time.perf_counter() - t0:.1f} s")


def _check_stats(capsys, ops, case, g, y, part, y_ref):
    """the partials {K, n, s, q} per (channel, workgroup): exact counts per workgroup, mean and biased variance of the fp64
    output at the gate of test_conv3d_stats_fused, and the finalize kernel"""
    C = y.shape[1]
    assert part.numel() == C * g.grid * 4, (case.id, part.numel(), C, g.grid)
    p = part.cpu().view(C, g.grid, 4)
    assert bool(torch.isfinite(p).all()), f"{case.id}: a statistics partial was not written"
    want_n = torch.tensor([float(sum(T.group_voxels(x, g.S) for w in g.waves[4 * b:4 * b + 4] for x in w)) for b in range(g.grid)],
                          dtype=torch.float64)
    bad = (p[..., 1] != want_n.view(1, -1)).any(0).nonzero().flatten().tolist()
    assert not bad, (f"{case.id}: workgroups {bad[:8]} count {p[0, bad[0], 1].item():.0f} voxels, their groups "
                     f"{g.waves[4 * bad[0]:4 * bad[0] + 4]} hold {want_n[bad[0]].item():.0f}")
    if "idle" in case.regimes:
        assert T.REGIMES["idle"](g)
    cnt, mean, var = T.fold_partials(part, C)
    mean_ref, var_ref = T.ref_stats(y_ref)
    assert bool((cnt == float(y_ref.numel() // C)).all())
    e_mean = (mean - mean_ref).abs().max().item()
    e_var = ((var - var_ref).abs() / var_ref).max().item()
    bn = torch.nn.BatchNorm3d(C).to(DEV)
    stats = ops.bn_stats_vector(y, bn.weight, bn.bias, bn.running_mean, bn.running_var, True, 0.1, 1e-5, part)
    inv_ref = 1.0 / torch.sqrt(var_ref + 1e-5)
    e_fmean = (stats[:C].double().cpu() - mean_ref).abs().max().item()
    e_inv = ((stats[C:2 * C].double().cpu() - inv_ref).abs() / inv_ref).max().item()
    with capsys.disabled():
        print(f"{'':40s} statistics: mean {e_mean:.2e} (finalized {e_fmean:.2e}; max|mean| {mean_ref.abs().max().item():.2e}), "
              f"variance {e_var:.2e} and 1 / std {e_inv:.2e} relative")
    lim_mean = 2e-6 * mean_ref.abs().max().item() + 1e-6
    assert e_mean <= lim_mean, f"{case.id}: mean off by {e_mean:.3e} (variance by {e_var:.3e} relative)"
    assert e_var <= 2e-6, f"{case.id}: variance off by {e_var:.3e} relative"
    assert e_fmean <= lim_mean, f"{case.id}: finalized mean off by {e_fmean:.3e}"
    assert e_inv <= 2e-6, f"{case.id}: 1 / std off by {e_inv:.3e} relative"


def _check_head_sentinel(ops, case, xg, wg, y_host):
    """the 27-channel launch at the C ABI on a y inside a sentinel-filled buffer: channels 27..31 of the MFMA block are
    dropped, nothing is written outside y, and the bits are the op's"""
    lib = ops._L()
    N, S, _ = T.shape_of(case)
    wf = torch.empty((lib.dca_conv1_x3_weight_bytes(case.C1) // 2,), device=DEV, dtype=torch.int16)
    ops._chk(lib.dca_conv1_x3_prep_weight(ops._ptr(wg), ops._ptr(wf), case.C1, case.Cout, 0, case.Cout, 0, ops._stream()),
             "dca_conv1_x3_prep_weight")
    pad, n = 4096, y_host.numel()
    big = torch.full((n + 2 * pad,), 777.0, device=DEV)
    yv = big[pad:pad + n]
    ops._chk(lib.dca_conv1_x3_forward(ops._ptr(xg), None, ops._ptr(wf), ops._ptr(yv), None, None, None, None, 1.0, N, case.C1,
                                      0, case.Cout, case.Cout, 0, S, ops._stream()), "dca_conv1_x3_forward")
    assert bool((big[:pad] == 777.0).all()) and bool((big[pad + n:] == 777.0).all()), f"{case.id}: wrote outside y"
    assert torch.equal(_bits(yv.cpu().view(y_host.shape)), _bits(y_host)), f"{case.id}: the C-ABI launch differs from the op"


# ---- conv1_x3 and conv1_mfma: forward -------------------------------------------------------------------------------------------------
FWD = _by_key([c for c in T.X3 + T.MFMA if "dx" not in c.tags])


@pytest.mark.parametrize("case", FWD, ids=[c.id for c in FWD])
def test_forward_many_groups(case, monkeypatch, capsys):
    """plain output, the fused inference epilogue and the training forward with fused BatchNorm statistics; one input of 32
    or 64 channels and two of 32; 32, 27 and 64 (two slices) output channels"""
    t0 = time.perf_counter()
    ops = _mods()
    lib = ops._L()
    # conv1_mfma's VEC rows switch the bf16x3 family off; its scalar rows leave conv1_x3 under the default flags (S % 4)
    monkeypatch.setattr(ops, "CONV_X3", "vec" not in case.tags)
    g = _regime(ops, case)
    family = "c1x3" if case.kernel == "x3" else "mfma"
    entry = "dca_conv1_x3_forward_stats" if "stats" in case.tags else ("dca_conv1_x3_forward" if case.kernel == "x3" else
                                                                       "dca_conv3d_forward")
    seen, calls = _spy_family(monkeypatch, ops), _counted(monkeypatch, lib, entry)
    launches = 2 if "slices" in case.tags else 1
    x, x2, w = _operands(case)
    xg, x2g, wg = _dev(x), _dev(x2), _dev(w)
    y_ref = _y_ref(case)
    oshape = tuple(y_ref.shape)
    part = None
    with torch.no_grad():
        if "epi" in case.tags:
            sc, sh, rp, rq, ref = _epilogue(case)
            scg, shg, rpg, rqg = _dev(sc), _dev(sh), _dev(rp), _dev(rq)
            run = lambda: ops.conv3d_fused_inference(xg, wg, 1, False, scg, shg, SLOPE, rpg, rqg, x2g)
            what = "epilogue"
        elif "stats" in case.tags:
            run, ref, what = (lambda: ops._Conv3d.apply(xg, x2g, wg, 1, False, True)), y_ref, "stats y"
        else:
            run, ref, what = (lambda: ops.conv3d(xg, wg, 1, False, x2=x2g)), y_ref, "forward"
        lim = 1e-5 * max(1.0, ref.abs().max().item())
        _poison(oshape)
        y = run()
        assert seen == [family] and calls == [entry] * launches, (case.id, seen, calls)
        if "stats" in case.tags:
            y, part = y
            assert part.numel() > 0, f"{case.id}: no statistics partials"
        y_host = y.cpu()
        _gate(capsys, case, g, what, y_host, ref, lim)
        if part is not None:
            _check_stats(capsys, ops, case, g, y, part, y_ref)
        del y
        again = run()
        if part is not None:
            _same_bits(case, "statistics partials", part.cpu(), again[1])
            again = again[0]
        _same_bits(case, what, y_host, again)
        del again
        if part is not None:
            _same_bits(case, "stats y against the plain launch", y_host, ops.conv3d(xg, wg, 1, False, x2=x2g))
        if "head" in case.tags:
            _check_head_sentinel(ops, case, xg, wg, y_host)
    _timed(capsys, case, t0)


# ---- conv1_x3: backward-data through autograd -----------------------------------------------------------------------------------------
BWD = _by_key([c for c in T.X3 if "dx" in c.tags])


@pytest.mark.parametrize("case", BWD, ids=[c.id for c in BWD])
def test_backward_data_many_groups(case, monkeypatch, capsys):
    """dx (and dx2) of ops.conv3d as ops._Conv3d.backward launches them: the kernel over dy with the transposed weight, 32
    input channels, 32 or 64 (two slices) output channels"""
    t0 = time.perf_counter()
    ops = _mods()
    lib = ops._L()
    monkeypatch.setattr(ops, "CONV_X3", True)
    g = _regime(ops, case)
    seen, calls = _spy_family(monkeypatch, ops), _counted(monkeypatch, lib, "dca_conv1_x3_forward")
    x, x2, w = _operands(case)
    wg, gyg = _dev(w), _dev(_t(case, "gy"))
    refs = [_truth(case, "dx", lambda: T.ref_backward_data(w, _t(case, "gy"), 0, case.C1))]
    if case.C2:
        refs.append(_truth(case, "dx2", lambda: T.ref_backward_data(w, _t(case, "gy"), case.C1, case.C1 + case.C2)))

    def run():
        leaves = [_dev(x).requires_grad_()] + ([_dev(x2).requires_grad_()] if case.C2 else [])
        y = ops.conv3d(leaves[0], wg, 1, False, x2=leaves[1] if case.C2 else None)
        del seen[:], calls[:]
        for r in refs:
            _poison(r.shape)
        got = torch.autograd.grad(y, leaves, gyg)
        # one _conv_sliced per input; 64 input channels come as two launches with co_off 0 and 32
        assert seen == ["c1x3"] * len(leaves), (case.id, seen)
        assert len(calls) == len(leaves) * (2 if "slices" in case.tags else 1), (case.id, calls)
        return [t.cpu() for t in got]
    got = run()
    for nm, a, r in zip(("dx", "dx2"), got, refs):
        _gate(capsys, case, g, nm, a, r, 1e-5 * max(1.0, r.abs().max().item()))
    for nm, a, b in zip(("dx", "dx2"), got, run()):
        _same_bits(case, nm, a, b)
    _timed(capsys, case, t0)


# ---- conv1_lp -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", _by_key(T.LP), ids=[c.id for c in _by_key(T.LP)])
def test_reduced_precision_many_groups(case, monkeypatch, capsys):
    """conv1_lp in bf16 and fp16 against the fp64 evaluation of the rounded operands: 2-byte output with the folded
    BatchNorm, leaky ReLU and both residuals, two inputs, and the 27-channel fp32 output of the head's tap GEMM"""
    t0 = time.perf_counter()
    ops = _mods()
    lib = ops._L()
    g = _regime(ops, case)
    lp = LPT[case.lp]
    odt = torch.float32 if "out32" in case.tags else lp
    calls = _counted(monkeypatch, lib, "dca_conv1_lp_forward")
    other, other3 = _counted(monkeypatch, lib, "dca_conv3d_forward"), _counted(monkeypatch, lib, "dca_conv1_x3_forward")
    x, x2, w = _operands(case)
    assert x.dtype == lp
    xg, x2g, wg = _dev(x), _dev(x2), _dev(w)
    with torch.no_grad():
        if "epi" in case.tags:
            sc, sh, rp, rq, ref = _epilogue(case, odt)
            scg, shg, rpg, rqg = _dev(sc), _dev(sh), _dev(rp), _dev(rq)
            run = lambda: ops.conv1x1_lp(xg, wg, lp, x2g, scg, shg, SLOPE, rpg, rqg, odt)
        else:
            ref = _y_ref(case)
            run = lambda: ops.conv1x1_lp(xg, wg, lp, x2g, out_dtype=odt)
        lim = floor = 2e-5 * max(1.0, ref.abs().max().item())
        if odt != torch.float32:     # the rounding of the 2-byte result itself
            lim = ref.abs() * ULP[case.lp] + floor
        _poison(ref.shape, odt)
        y = run()
        assert calls == ["dca_conv1_lp_forward"] and not other and not other3, (case.id, calls, other, other3)
        assert y.dtype == odt
        y_host = y.cpu()
        del y
        _gate(capsys, case, g, case.lp, y_host, ref, lim)
        _same_bits(case, case.lp, y_host, run())
    _timed(capsys, case, t0)
