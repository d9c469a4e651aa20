"""fp64 gates of the cost-volume kernels on every launch branch: gwc_fwd_kernel, gwc_bwd_kernel, gwc_bwd_blocked_kernel and
the concat kernels of csrc/volume.hip, gwc_fused_kernel and concat_fused_kernel of csrc/volume_fused.hip.
tests/test_gpu_parity.py::test_gwc_volume reaches the blocked backward kernel -- the one the batch-4 training step runs -- at
two shapes, both CPG 8 and both with one image row per workgroup, and no test reached its `<2>` / `<4>` instantiations, the row
walk (prefetch behind the second barrier, the barrier that keeps the next row's gv stores off the partial sums), the
`iq += rows` loop of the fused builder beyond its first trip or any grid-stride loop beyond its first sweep.  Here every row
of tests/_volume_cases.py sits on one branch of a launcher (the arithmetic is checked without a GPU in
tests/test_volume_cases_cpu.py) and is reached through the public op of ops.py, forward and all gradients.

Route.  Before anything is compared the library is asked which backward kernel serves the shape (`dca_gwc_volume_bwd_rows`:
grid.x of the blocked kernel, 0 = plain) and the answer has to equal the restated predicate's; the fused rows also have to be
on `_CostVolume`.  A row that drifts off its regime fails.

Gate.  Truth: `O.build_gwc_volume` / `O.build_concat_volume` in float64, differentiated by autograd.  Yardstick: the same
functions in float32 on the CPU.  Metric: max |a - ref| / max(1, max |ref|) per output and per gradient.  A kernel passes at
max(4 x yardstick, 2^-22) AND at the fixed tolerance of its sibling parity test (2e-6 gwc forward, 1e-5 gwc gradients, 1e-6
concat gradients); the concat volume is compared bit for bit and the half-plane x < d has to be exactly 0.  The 2-byte
volumes are gated element by element at the fp32 bound plus half an ulp of the storage type.  The gradient seed carries a
factor CPG so that no reference gradient has a maximum below 1 (`seed_scale`).

Blocked rows: the error is taken per image row y and a failure names the worst row, its workgroup y % gx and its trip y // gx.
Each is run once more through the C ABI into NaN-filled gradients inside a sentinel-filled buffer: every element written,
bitwise what the op returned, nothing outside.  Each family's largest row is run twice and compared bit for bit.

Measured on one MI355X: MEASURED below, per case the worst (yardstick, error) of the forward outputs and of the gradients,
as printed by the tests before they assert.

That the gates bite, with libraries built from a scratch copy of the sources (mutations that compute wrong values in bounds;
this file and its siblings on one MI355X, 38 tests here):
  * gwc_bwd_blocked_kernel without `fetch(y + gridDim.x)` (later trips reuse the first row's registers): 5 failed -- the five
    multi-trip rows of test_gwc_blocked, each naming a row with y // gx >= 1 (errors 0.9 .. 1.3), e.g. "worst image row
    y = 34: workgroup y % gx = 2, trip y // gx = 1, gx = 32"; the five one-trip blocked rows, everything else here and all six
    shapes of test_gpu_parity.py::test_gwc_volume passed (39 passed).
  * gwc_fused_kernel with its `iq` loop ended after the first trip: 5 failed -- the four rows of test_cost_volume_fused here
    (the first disparity of the second trip is reported: "x < d must be exactly 0 (d = 16)", d = 4 at W 688 where one thread
    row walks both quads) and the bitwise repeat of the largest; every cost-volume case of tests/test_gpu_fused_nodes.py
    passed (52 passed).
  * concat_bwd_kernel with its grid-stride `for` turned into one `if`: 2 failed -- test_concat[concat-1x12x300x296x4]
    (d L 0.85, d R 1.19) and its bitwise repeat; the other concat rows, test_gpu_parity.py::test_concat_volume and the
    cost-volume cases of tests/test_gpu_fused_nodes.py passed (57 passed).
  * `D >= 6 * cpg` relaxed to `D >= 4 * cpg` in gwc_bwd_blocked_rows: the route assertion of the D = 44 boundary row failed
    before any launch ("dca_gwc_volume_bwd_rows says 2, the case table 0"), 13 other plain / boundary rows passed; without a
    GPU tests/test_volume_cases_cpu.py::test_library_query_equals_the_restated_predicate failed (1 of 101)."""
import pytest
import torch

import _volume_cases as V

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 4096            # floats of sentinel either side of a C-ABI output (a multiple of four: the output stays 16-byte aligned)
SENTINEL = -1024.0

# case id: (forward yardstick, forward error, gradient yardstick, gradient error); the gate applied is per output
MEASURED = {
    "gwc-2x320x40x40x16x48": (1.2e-07, 1.2e-07, 1.4e-07, 9.7e-08),
    "gwc-1x320x40x35x240x48": (1.6e-07, 1.3e-07, 3.7e-07, 1.4e-07),
    "gwc-1x2560x1280x3x8x12": (5.2e-08, 5.3e-08, 8.6e-08, 7.9e-08),
    "gwc-1x16x4x2x256x24": (7.3e-08, 7.3e-08, 1.8e-07, 1.3e-07),
    "gwc-1x8x4x2x256x12": (9.1e-08, 4.5e-08, 1.1e-07, 9.1e-08),
    "gwc-1x16x2x3x8x48": (7.6e-08, 6.3e-08, 9.1e-08, 8.0e-08),
    "gwc-1x8x1x2x236x52": (1.3e-07, 1.2e-07, 3.2e-07, 1.2e-07),
    "gwc-1x8x1x2x216x56": (9.6e-08, 8.5e-08, 2.3e-07, 1.3e-07),
    "gwc-2x256x64x12x32x24": (8.1e-08, 7.8e-08, 1.9e-07, 1.1e-07),
    "gwc-1x128x64x23x64x16": (6.6e-08, 6.6e-08, 1.7e-07, 1.0e-07),
    "gwc-1x8x1x2x240x52": (8.7e-08, 8.7e-08, 2.2e-07, 2.3e-07),
    "gwc-1x8x1x2x192x64": (9.4e-08, 1.1e-07, 2.5e-07, 2.6e-07),
    "gwc-1x8x1x2x16x44": (8.6e-08, 9.7e-08, 1.0e-07, 8.0e-08),
    "gwc-1x4x2x2x260x12": (5.1e-08, 3.9e-08, 1.2e-07, 1.6e-07),
    "gwc-1x32x2x2x16x96": (9.1e-08, 1.0e-07, 1.3e-07, 1.8e-07),
    "gwc-1x4x4x2x16x8": (2.2e-08, 2.2e-08, 7.2e-08, 7.9e-08),
    "gwc-1x8x1x2x16x50": (5.7e-08, 9.3e-08, 7.3e-08, 1.5e-07),
    "gwc-1x8x2x3x17x6": (6.9e-08, 6.7e-08, 1.5e-07, 8.2e-08),
    "gwc-2x32x4x5x18x6": (1.0e-07, 8.8e-08, 7.9e-08, 9.3e-08),
    "gwc-1x4x2x2x19x5": (4.3e-08, 4.1e-08, 6.1e-08, 6.6e-08),
    "gwc-1x16x1x2x40x12": (9.3e-08, 1.5e-07, 1.1e-07, 9.0e-08),
    "gwc-1x4x2x2x6x9": (3.4e-08, 2.7e-08, 4.9e-08, 4.0e-08),
    "gwc-1x16x1x2x208x48": (1.4e-07, 1.6e-07, 2.5e-07, 2.5e-07),
    "gwc-1x16x1x2x516x5": (1.1e-07, 9.5e-08, 1.3e-07, 1.2e-07),
    "concat-2x3x5x18x6": (0.0e+00, 0.0e+00, 8.9e-08, 7.1e-08),
    "concat-1x2x130x509x4": (0.0e+00, 0.0e+00, 7.9e-08, 7.7e-08),
    "concat-1x12x300x296x4": (0.0e+00, 0.0e+00, 7.5e-08, 9.3e-08),
    "fused-seg64+128+128-Cc0-dtypefp32-1x320x40x2x240x48": (1.3e-07, 1.2e-07, 2.7e-07, 1.2e-07),
    "fused-seg64+128+128-Cc0-dtypebf16-1x320x40x2x240x50": (1.1e-07, 3.9e-09, 0.0e+00, 0.0e+00),
    "fused-seg64+128+128-Cc0-dtypefp16-1x320x40x2x240x50": (1.3e-07, 2.2e-08, 0.0e+00, 0.0e+00),
    "fused-seg1-Cc12-dtypefp32-1x1x1x64x688x8": (3.8e-08, 3.8e-08, 1.0e-07, 1.2e-07),
}


def _ops():
    from dcanet_amd import ops
    return ops


def _flags(monkeypatch, ops):
    """the shipped configuration whatever the environment says: f16x2 convolutions, packed operands, producer-side maxima
    (the fused builder emits its per-row maxima only then)"""
    for flag in ("CONV_X3", "CONV_X2", "PACK", "AMAX_EMIT"):
        monkeypatch.setattr(ops, flag, True)


def run(case):
    return V.evaluate(case, torch.float32, DEV, V.public_op(_ops()))


def assert_route(case, out=None):
    """the library's own answer for the backward launch of this shape, against the restated predicate"""
    ops = _ops()
    if case.family != "concat":
        B, C, G, H, W, D = case.shape
        got = ops._L().dca_gwc_volume_bwd_rows(B, C, H, W, D, G)
        assert got == case.rows, f"{case.id}: dca_gwc_volume_bwd_rows says {got}, the case table {case.rows} ({case.branch})"
    if out is not None and V.has_grads(case):
        want = {"gwc": "_GwcVolumeBackward", "concat": "_ConcatVolumeBackward", "fused": "_CostVolumeBackward"}[case.family]
        assert type(out.grad_fn).__name__ == want, f"{case.id}: on {type(out.grad_fn).__name__}, expected {want}"


def zero_half_plane(case, vol):
    """x < d is exactly 0 in every channel, concat part included"""
    D, W = vol.shape[2], vol.shape[4]
    for d in range(1, D):
        assert not bool(vol[:, :, d, :, :min(d, W)].any()), f"{case.id}: x < d must be exactly 0 (d = {d})"


def check(case):
    assert_route(case)
    ref, yard, sib = V.truth(case), V.yardstick(case), V.sibling(case)
    got, out = run(case)
    torch.cuda.synchronize()
    assert_route(case, out)
    print(f"{case.id}: {case.branch}")
    zero_half_plane(case, out.detach())
    failures, worst = [], {"fwd": (0.0, 0.0), "grad": (0.0, 0.0)}
    gx = case.rows
    for name, want in ref.items():
        assert got[name].dtype == torch.float32 and got[name].shape == want.shape, name
        assert torch.isfinite(got[name]).all(), name
        y, e = yard[name], V.error(got[name], want)
        tol = min(V.gate(y), sib[name]) if sib[name] > 0 else 0.0
        print(f"  {name}: |ref|max {want.abs().max().item():.3e}  yardstick {y:.2e}  error {e:.2e}  gate {tol:.2e}")
        kind = "grad" if name.startswith("d ") else "fwd"
        if e >= worst[kind][1]:
            worst[kind] = (y, e)
        if sib[name] == 0:
            if not torch.equal(got[name].cpu().double(), want):
                failures.append(f"{name}: not bit for bit ({e:.3e})")
            continue
        where = ""
        if gx and name in ("d L", "d R"):
            rows = V.row_errors(got[name], want)
            yw = int(rows.argmax())
            where = f" (worst image row y = {yw}: workgroup y % gx = {yw % gx}, trip y // gx = {yw // gx}, gx = {gx})"
            print(f"  {name}: worst row y = {yw} (workgroup {yw % gx}, trip {yw // gx}) {rows[yw].item():.2e}")
        if e > V.gate(y):
            failures.append(f"{name}: {e:.3e} > max(4 x {y:.3e}, 2^-22){where}")
        if e > sib[name]:
            failures.append(f"{name}: {e:.3e} > the sibling's {sib[name]:.0e}{where}")
    print(f'  MEASURED "{case.id}": ({worst["fwd"][0]:.1e}, {worst["fwd"][1]:.1e}, {worst["grad"][0]:.1e}, '
          f'{worst["grad"][1]:.1e}),')
    assert not failures, f"{case.id} ({case.branch}): " + "; ".join(failures)
    return got, out


def ids(cases):
    return [c.id for c in cases]


def guarded(n, fill):
    """n floats of `fill` between two guard bands of SENTINEL: (whole buffer, the view to hand to the C ABI)"""
    big = torch.full((n + 2 * GUARD,), SENTINEL, device=DEV, dtype=torch.float32)
    view = big[GUARD:GUARD + n]
    view.fill_(fill)
    assert view.data_ptr() % 16 == 0
    return big, view


def guards_intact(big, n):
    return bool((big[:GUARD] == SENTINEL).all()) and bool((big[GUARD + n:] == SENTINEL).all())


@pytest.mark.parametrize("case", V.GWC_BLOCKED, ids=ids(V.GWC_BLOCKED))
def test_gwc_blocked(case):
    """gwc_bwd_blocked_kernel<2 | 4 | 8> (and gwc_fwd_kernel in front of it): fp64 gate per image row, then the C entry into
    NaN-filled gradients between guard bands"""
    assert case.rows > 0
    got, _ = check(case)
    ops = _ops()
    B, C, G, H, W, D = case.shape
    t, seed = V.inputs(case)
    L, R, gv = t["L"][0].to(DEV), t["R"][0].to(DEV), seed.to(DEV)
    n = L.numel()
    (bigL, gL), (bigR, gR) = guarded(n, float("nan")), guarded(n, float("nan"))
    assert all(x.data_ptr() % 16 == 0 for x in (L, R, gv)), "the blocked kernel needs 16-byte aligned operands"
    ops._chk(ops._L().dca_gwc_volume_bwd(ops._ptr(gv), ops._ptr(L), ops._ptr(R), ops._ptr(gL), ops._ptr(gR), B, C, H, W, D, G,
                                         ops._stream()), "dca_gwc_volume_bwd")
    torch.cuda.synchronize()
    for name, big, g in (("d L", bigL, gL), ("d R", bigR, gR)):
        unwritten = int(torch.isnan(g).sum())
        assert unwritten == 0, f"{case.id} {name}: {unwritten} of {n} elements were not written"
        assert guards_intact(big, n), f"{case.id} {name}: wrote outside the gradient"
        assert torch.equal(g.view(B, C, H, W), got[name]), f"{case.id} {name}: the C entry differs from the op"


PLAIN = V.GWC_BOUNDARY + V.GWC_PLAIN


@pytest.mark.parametrize("case", PLAIN, ids=ids(PLAIN))
def test_gwc_plain_and_boundary(case):
    """gwc_fwd_kernel<1 .. 16> and gwc_bwd_kernel, vec and not, among them the shapes one step outside the blocked predicate"""
    assert case.rows == 0
    check(case)


@pytest.mark.parametrize("case", V.CONCAT, ids=ids(V.CONCAT))
def test_concat(case):
    check(case)


@pytest.mark.parametrize("case", V.FUSED, ids=ids(V.FUSED))
def test_cost_volume_fused(case, monkeypatch):
    """ops.cost_volume on the fused builder: the `iq` loop past its first trip (fp32 with the emitted per-row maxima; the
    TAIL instantiation into a 2-byte volume) and concat_fused_kernel past its first sweep"""
    ops = _ops()
    _flags(monkeypatch, ops)
    B, C, G, H, W, D = case.shape
    if V.has_grads(case):
        _, out = check(case)
        if case.p["Cc"] == 0:
            tag = ops._tag_ok(out, "_dca_cmax")
            assert tag is not None, f"{case.id}: no valid _dca_cmax on the volume"
            slots, nslots, _ = tag
            assert nslots == B * H, (nslots, B * H)
            s = slots.view(torch.float32).view(G, ops.CSLOTS)[:, :nslots]
            want = out.detach().abs().amax((2, 4)).permute(1, 0, 2).reshape(G, B * H)      # [g][b * H + y]
            bad = (s != want).nonzero().tolist()
            assert not bad, f"{case.id}: emitted row maxima differ from max |volume| at (g, b * H + y) = {bad[:6]}"
        return
    lp, half_ulp = V.LP[case.p["dtype"]]
    assert_route(case)
    ref, yard = V.truth(case), V.yardstick(case)
    got, out = run(case)
    torch.cuda.synchronize()
    print(f"{case.id}: {case.branch}")
    assert out.dtype == lp and out.shape == (B, G, D, H, W)      # a 2-byte volume has the fused builder only (ops.cost_volume)
    zero_half_plane(case, out)
    want, v = ref["fwd"], out.detach().cpu().double()
    assert torch.isfinite(v).all()
    tol = min(V.gate(yard["fwd"]), V.SIBLING["fwd"])
    excess = (v - want).abs() - half_ulp * want.abs()
    e = max(0.0, excess.max().item()) / max(1.0, want.abs().max().item())
    print(f"  fwd: yardstick {yard['fwd']:.2e}  error beyond half an ulp of {case.p['dtype']} {e:.2e}  gate {tol:.2e}")
    print(f'  MEASURED "{case.id}": ({yard["fwd"]:.1e}, {e:.1e}, 0.0e+00, 0.0e+00),')
    if e > tol:
        d = int(excess.amax((0, 1, 3, 4)).argmax())
        pytest.fail(f"{case.id} ({case.branch}): fwd {e:.3e} > {tol:.3e} beyond the store's rounding, worst disparity {d} "
                    f"(quad {d // 4})")


def _offset_view(t):
    """a contiguous copy of t that starts at element 1 of a larger buffer: 4 bytes off 16-byte alignment"""
    buf = torch.empty(t.numel() + 8, device=DEV, dtype=t.dtype)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def test_abi_misaligned_backward_is_the_aligned_one():
    """dca_gwc_volume_bwd with gvol / L / R (and the gradients) 4 bytes off alignment at a W % 4 == 0 shape on the plain
    kernel: its non-vec staging loops, same arithmetic order, so bit for bit the aligned (vec) run; fp64 gate on top"""
    case = V.ABI_MISALIGNED["bwd"]
    ops = _ops()
    assert_route(case)
    B, C, G, H, W, D = case.shape
    t, seed = V.inputs(case)
    L, R, gv = t["L"][0].to(DEV), t["R"][0].to(DEV), seed.to(DEV)
    n = L.numel()
    res = []
    for off in (False, True):
        a = [_offset_view(x) if off else x for x in (gv, L, R)]
        assert all(x.data_ptr() % 16 == (4 if off else 0) for x in a)
        bigL, bigR = (torch.full((n + 2 * GUARD + 1,), SENTINEL, device=DEV) for _ in range(2))
        s = GUARD + 1 if off else GUARD
        gL, gR = bigL[s:s + n], bigR[s:s + n]
        gL.fill_(float("nan")); gR.fill_(float("nan"))
        assert gL.data_ptr() % 16 == (4 if off else 0)
        ops._chk(ops._L().dca_gwc_volume_bwd(*[ops._ptr(x) for x in a], ops._ptr(gL), ops._ptr(gR), B, C, H, W, D, G,
                                             ops._stream()), "dca_gwc_volume_bwd")
        torch.cuda.synchronize()
        for big in (bigL, bigR):
            assert bool((big[:s] == SENTINEL).all()) and bool((big[s + n:] == SENTINEL).all()), "wrote outside the gradient"
        assert not bool(torch.isnan(gL).any()) and not bool(torch.isnan(gR).any())
        res.append((gL.view(B, C, H, W).clone(), gR.view(B, C, H, W).clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]), "misaligned run differs from the aligned one"
    ref, yard = V.truth(case), V.yardstick(case)
    for name, g in zip(("d L", "d R"), res[1]):
        e = V.error(g, ref[name])
        print(f"  {name}: yardstick {yard[name]:.2e}  error {e:.2e}")
        assert e <= min(V.gate(yard[name]), V.SIBLING[name]), (name, e, yard[name])


def test_abi_misaligned_forward_is_the_aligned_one():
    """dca_gwc_volume_fwd into a volume 4 bytes off alignment at W % 4 == 0: the per-element stores of the non-vec branch"""
    case = V.ABI_MISALIGNED["fwd"]
    ops = _ops()
    B, C, G, H, W, D = case.shape
    t, _ = V.inputs(case)
    L, R = t["L"][0].to(DEV), t["R"][0].to(DEV)
    n = B * G * D * H * W
    res = []
    for off in (False, True):
        big = torch.full((n + 2 * GUARD + 1,), SENTINEL, device=DEV)
        s = GUARD + 1 if off else GUARD
        vol = big[s:s + n]
        vol.fill_(float("nan"))
        assert vol.data_ptr() % 16 == (4 if off else 0)
        ops._chk(ops._L().dca_gwc_volume_fwd(ops._ptr(L), ops._ptr(R), ops._ptr(vol), B, C, H, W, D, G, ops._stream()),
                 "dca_gwc_volume_fwd")
        torch.cuda.synchronize()
        assert bool((big[:s] == SENTINEL).all()) and bool((big[s + n:] == SENTINEL).all()), "wrote outside the volume"
        assert not bool(torch.isnan(vol).any()), "an element of the volume was not written"
        res.append(vol.view(B, G, D, H, W).clone())
    assert torch.equal(res[0], res[1]), "misaligned run differs from the aligned one"
    zero_half_plane(case, res[1])
    ref, yard = V.truth(case), V.yardstick(case)
    e = V.error(res[1], ref["fwd"])
    print(f"  fwd: yardstick {yard['fwd']:.2e}  error {e:.2e}")
    assert e <= min(V.gate(yard["fwd"]), V.SIBLING["fwd"]), (e, yard["fwd"])


def test_refused_shape_raises_before_any_launch():
    """CPG 16 at W 1284 needs 164352 B of LDS: the entry returns hipErrorInvalidValue, the op raises, nothing is launched"""
    case = V.REFUSED
    ops = _ops()
    B, C, G, H, W, D = case.shape
    assert ops._L().dca_gwc_volume_bwd_rows(B, C, H, W, D, G) < 0
    x = torch.zeros(B, C, H, W, device=DEV)
    with pytest.raises(RuntimeError, match="dca_gwc_volume_fwd failed with hipError_t 1$"):
        ops.gwc_volume(x, x, D, G)
    g = torch.zeros(B, C, H, W, device=DEV)
    rc = ops._L().dca_gwc_volume_bwd(ops._ptr(x), ops._ptr(x), ops._ptr(x), ops._ptr(g), ops._ptr(g), B, C, H, W, D, G,
                                     ops._stream())
    assert rc == 1
    torch.cuda.synchronize()


LARGEST = [max(cases, key=V.volume_numel) for cases in (V.GWC_BLOCKED, PLAIN, V.CONCAT, V.FUSED)]


@pytest.mark.parametrize("case", LARGEST, ids=ids(LARGEST))
def test_two_calls_are_bit_identical(case, monkeypatch):
    """each family at its largest row (the 35-row walk of the blocked kernel among them): no atomics, fixed summation order"""
    _flags(monkeypatch, _ops())
    (a, _), (b, _) = run(case), run(case)
    print(f"{case.id}: {case.branch}")
    assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)
