"""The weight-gradient kernels against fp64 in the many-tile regime.

csrc/conv3d_wgrad.hip (`wgrad3_kernel<1,32>`, `<1,16>`, `<2,32>`, `wgrad1_kernel<false>` / `<true>`, `wgrad_reduce_kernel`),
conv3d_wgrad_bf16x3.hip, conv3d_wgrad_f16x2.hip (four `<XP, YP>` instantiations) and conv3d_wgrad_s2_f16x2.hip are persistent
kernels: a workgroup walks its share of the tiles, fetches the next tile while it multiplies the current one and writes one
slab; `wgrad_reduce_kernel` adds the slabs.  The first parity tests (tests/test_gpu_parity.py) reach them with at most two
tiles per workgroup and a handful of slabs.  Here every row of tests/_wgrad_cases.py sits on one regime of that control flow
-- several tiles per workgroup with an uneven split between the XCDs, the `nx = 1` walk, the second LDS image set of the
both-packed f16x2 kernel, the pipelined and the plain staging of each generic template, every combination of the two loops
of the reduction -- and does four things: (1) reads `nblk` back from the kernel's own size query and asserts the regime it
names, before anything is compared; (2) runs the kernel through `ops._wgrad` (the autograd node for the logit heads and the
transposed convolution); (3) compares with `torch.nn.grad.conv3d_weight` in fp64; (4) runs it again and requires the same
bits (the reduction order is fixed).  tests/test_wgrad_cases_cpu.py checks the table and the reference without a GPU.

Gates (the project's existing yardsticks, not the code under test).  Split kernels: relative L2 <= 1e-6 (2e-6 with a packed
px2 operand) and max-abs error <= 1.5 x the fp32 MFMA kernel's on the same inputs + 1e-7 x max|ref| (`test_wgrad_bf16x3`,
the px2 round-trip test).  Generic fp32 kernel, also as `wgrad1_kernel<true>`: relative L2 <= 1e-5 and max-abs <= 2e-5 x
max(1, max|ref|) (`test_conv3d`).

Not covered: the `small_offsets == 0` branch of the generic kernels needs an operand above 2 GiB.

MEASURED on one MI355X (256 CUs); every row at the fixed gates above, none needed another yardstick.  Every test prints its
row of this table.  `MFMA` = max-abs error of the generic fp32 kernel on the same inputs (the split kernels' yardstick).

row                          nblk tiles     rel L2      gate    max-abs      gate   MFMA max  max|ref|
x2-uneven-ff                   28    96   1.95e-07  1.00e-06   4.56e-03  1.46e-02   8.41e-03  1.95e+04
x2-uneven-pf                   28    96   1.95e-07  2.00e-06   4.56e-03  1.46e-02   8.41e-03  1.95e+04
x2-uneven-fp                   28    96   1.95e-07  2.00e-06   4.56e-03  1.46e-02   8.41e-03  1.95e+04
x2-uneven-pp                   28    96   1.95e-07  2.00e-06   4.56e-03  1.46e-02   8.41e-03  1.95e+04
x2-nx1-ff                       7    12   1.42e-07  1.00e-06   2.70e-05  1.12e-04   6.36e-05  1.60e+02
x2-nx1-pf                       7    12   1.42e-07  2.00e-06   2.70e-05  1.12e-04   6.36e-05  1.60e+02
x2-nx1-fp                       7    12   1.42e-07  2.00e-06   2.70e-05  1.12e-04   6.36e-05  1.60e+02
x2-nx1-pp                       7    12   1.42e-07  2.00e-06   2.70e-05  1.12e-04   6.36e-05  1.60e+02
x2-partial-ff                  64    75   1.63e-07  1.00e-06   6.16e-05  1.57e-04   8.60e-05  2.80e+02
x2-partial-fp                  64    75   1.63e-07  2.00e-06   6.16e-05  1.57e-04   8.60e-05  2.80e+02
x2-w42-pp                      28    96   1.95e-07  2.00e-06   8.66e-05  2.43e-04   1.36e-04  3.92e+02
x3-uneven                      28    96   2.30e-07  1.00e-06   4.82e-03  1.46e-02   8.41e-03  1.95e+04
x3-nx1                          7    12   1.49e-07  1.00e-06   3.13e-05  1.12e-04   6.36e-05  1.60e+02
x3-partial                     64    75   1.67e-07  1.00e-06   6.57e-05  1.57e-04   8.60e-05  2.80e+02
reduce-x2-1                     1     1   1.12e-07  1.00e-06   7.35e-06  3.60e-05   2.06e-05  5.19e+01
reduce-x3-1                     1     1   1.02e-07  1.00e-06   8.47e-06  3.60e-05   2.06e-05  5.19e+01
reduce-x2-12                   12    12   1.41e-07  1.00e-06   2.12e-05  1.03e-04   5.71e-05  1.69e+02
reduce-x3-12                   12    12   1.45e-07  1.00e-06   2.38e-05  1.03e-04   5.71e-05  1.69e+02
reduce-x2-75                   75    75   1.66e-07  1.00e-06   6.76e-05  1.96e-04   1.07e-04  3.59e+02
reduce-x3-75                   75    75   1.70e-07  1.00e-06   7.63e-05  1.96e-04   1.07e-04  3.59e+02
reduce-x2-120                 120   120   1.79e-07  1.00e-06   9.24e-05  2.73e-04   1.49e-04  4.90e+02
reduce-x3-120                 120   120   1.84e-07  1.00e-06   9.40e-05  2.73e-04   1.49e-04  4.90e+02
reduce-x2-150                 150   150   1.87e-07  1.00e-06   1.13e-04  3.03e-04   1.65e-04  5.55e+02
reduce-x3-150                 150   150   1.93e-07  1.00e-06   1.02e-04  3.03e-04   1.65e-04  5.55e+02
reduce-x2-288                 256   288   2.22e-07  1.00e-06   1.47e-04  3.92e-04   2.12e-04  7.36e+02
reduce-x3-288                 256   288   2.37e-07  1.00e-06   1.72e-04  3.92e-04   2.12e-04  7.36e+02
s2x2-blkoff                    28   120   1.95e-07  1.00e-06   3.91e-03  1.07e-02   5.85e-03  1.88e+04
s2x2-blkoff-scaled             28   120   1.94e-07  1.00e-06   7.38e-11  2.15e-10   1.23e-10  3.05e-04
s2x2-odd                      256   270   1.86e-07  1.00e-06   7.92e-05  1.45e-04   7.17e-05  3.75e+02
s2x2-odd-scaled               256   270   1.89e-07  1.00e-06   7.11e-11  1.42e-10   6.96e-11  3.75e-04
g32-pipelined                  28    96   4.34e-07  1.00e-05   1.78e-02  6.03e-01          -  3.02e+04
g32-plain                      28    96   4.30e-07  1.00e-05   3.13e-04  1.17e-02          -  5.87e+02
g16-pipelined                  28    96   4.38e-07  1.00e-05   3.17e-04  1.15e-02          -  5.75e+02
g16-plain                      28    96   4.28e-07  1.00e-05   2.71e-04  1.07e-02          -  5.35e+02
gs2-vec                        28   100   2.62e-07  1.00e-05   8.44e-05  5.27e-03          -  2.64e+02
gs2-vecx                       28   100   1.69e-07  1.00e-05   4.85e-05  4.07e-03          -  2.04e+02
gs2-scalar                     28   100   2.66e-07  1.00e-05   8.52e-05  5.53e-03          -  2.76e+02
g32-misaligned-x               28    96   4.35e-07  1.00e-05   2.78e-04  1.13e-02          -  5.63e+02
gs2-misaligned-dy              28   100   2.62e-07  1.00e-05   8.44e-05  5.27e-03          -  2.64e+02
g1-vec                         56   144   2.67e-07  1.00e-05   1.04e-02  7.26e-01          -  3.63e+04
g1-scalar                      56   150   2.64e-07  1.00e-05   2.02e-04  1.50e-02          -  7.48e+02
reduce-g1-170x3               170   192   1.94e-07  1.00e-05   1.84e-04  1.58e-02          -  7.92e+02
head-c64                      256   600   2.48e-07  1.00e-05   2.51e-02  1.41e+00          -  7.06e+04
head-c32-small                  8     8   1.52e-07  1.00e-05   2.61e-05  2.48e-03          -  1.24e+02
head-c32-small-expand           8     8   1.52e-07  1.00e-05   2.61e-05  2.48e-03          -  1.24e+02
strided-c1-second-input       128   288   2.42e-07  1.00e-05   2.09e-04  2.05e-02          -  1.03e+03
strided-transposed            256   360   1.95e-07  1.00e-06   1.24e-04  2.42e-04   1.30e-04  4.66e+02

A plain fp32 evaluation of the same sums on the CPU (`torch.nn.grad.conv3d_weight` in fp32) is at 3e-7 .. 1.2e-6 relative L2
on these rows, so the kernels' tile-then-slab summation order is ahead of it; one lost tile is 1/ntiles >= 1.6e-3 relative.

That the gates bite (libraries built from a scratch copy, never committed).  `t_end` of the two stride-1 split kernels made
to drop the last tile of its XCD chunk when the workgroup that owns it has two or more tiles: all 14 x2 / x3 rows and the
12-, 75-, 150- and 288-tile reduction rows fail (relative L2 0.17 .. 0.41), every other row passes, and `test_wgrad_bf16x3`
passes at three of its four shapes -- at (1, 64, 33, (3, 9, 36)) its 18 tiles on 18 workgroups fall into XCD chunks of 2 or
3 tiles shared by 3 or 2 workgroups, so a few workgroups there do get two tiles (and a few none).  The same edit limited
to workgroups with three or more tiles: the six `uneven` / `w42` rows fail and the whole of `test_wgrad_bf16x3` passes.
"""
import pytest
import torch
import torch.nn.functional as F

import _wgrad_cases as W
from oracle.seeded import seeded_tensor

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = 0x7FA5A5A5     # a NaN as fp32: nothing a kernel writes
_TRUTH = {}               # data key -> {"ref": fp64 dW, "e32": (max-abs, rel L2) of the fp32 MFMA kernel on the same inputs}
_ROWS = []                # the rows printed so far


def _mods():
    import dcanet_amd  # noqa: F401
    from dcanet_amd import ops
    return ops


_HEAD = (f"\n{'row':28s} {'nblk':>4s} {'tiles':>5s}  {'rel L2':>9s} {'gate':>9s}  {'max-abs':>9s} {'gate':>9s}  "
         f"{'MFMA max':>9s} {'max|ref|':>9s}")


def _print_row(capsys, r):
    """one line of the MEASURED table, past the capture (the header in front of the first)"""
    mfma = f"{r[7]:9.2e}" if r[7] is not None else f"{'-':>9s}"
    with capsys.disabled():
        if not _ROWS:
            print(_HEAD)
        print("{:28s} {:4d} {:5d}  {:9.2e} {:9.2e}  {:9.2e} {:9.2e}  {} {:9.2e}".format(*r[:7], mfma, r[8]))
    _ROWS.append(r)


def _route(monkeypatch, ops, family):
    """the flags that send a weight gradient to `family`'s kernel, and the name _wgrad_family must then give"""
    split = family in ("x2", "x3", "s2x2")
    monkeypatch.setattr(ops, "CONV_X3", split)
    monkeypatch.setattr(ops, "CONV_X2", family in ("x2", "s2x2"))
    monkeypatch.setattr(ops, "WGRAD_S2_X2", True)
    return family if split else "mfma"


def _ksize(case):
    return 3 if case.family == "head" else W.FAMILIES[case.family][1]


def _stride(case):
    return W.FAMILIES[case.family][2]


def _assert_regime(ops, case):
    """nblk from the size query of the kernel that will run; every regime of the row must hold for it"""
    lib = ops._L()
    fam, dims = case.family, case.dims
    K = 27 if W.FAMILIES[fam][1] == 3 else 1
    if fam in ("x2", "x3"):
        nws = getattr(lib, f"dca_conv3d_wgrad_{fam}_workspace")(case.N, case.Cx, case.Cy, *dims)
    elif fam == "s2x2":
        nws = lib.dca_conv3d_wgrad_s2_x2_workspace(case.N, case.Cx, case.Cy, *dims)
    else:
        nws = lib.dca_conv3d_wgrad_workspace(case.N, case.Cx, case.Cy, *W.out_dims(case), W.FAMILIES[fam][1], _stride(case))
    ncu = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    ntiles, nCT, share, want = W.geometry(case, ncu)
    assert nws > 0 and nws % (nCT * K * 1024) == 0, (case.id, nws)
    nblk = nws // (nCT * K * 1024)
    assert nblk == want, f"{case.id}: the size query gives {nblk} workgroups, the restated grid rule {want} ({ncu} CUs)"
    for r in case.regimes:
        assert W.REGIMES[r](case, ntiles, nCT, nblk) is True, \
            f"{case.id} is not in its regime on this device: {r} (ntiles {ntiles}, nCT {nCT}, nblk {nblk}, {ncu} CUs)"
    return ntiles, nblk


def _misaligned(t):
    """a copy of t on the device that starts one float into a larger buffer: 4 bytes past a 16-byte boundary"""
    buf = torch.empty(t.numel() + 4, device=DEV, dtype=torch.float32)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert buf.data_ptr() % 16 == 0 and v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _errors(got, ref):
    e = got.detach().cpu().double().reshape(ref.shape) - ref
    return e.abs().max().item(), (e.norm() / ref.norm().clamp_min(1e-300)).item()


def _truth(case, x, dy):
    key = W.data_key(case)
    if key not in _TRUTH:
        _TRUTH[key] = {"ref": W.reference(x, dy, _ksize(case), _stride(case))}
    return _TRUTH[key]


def _mfma_error(monkeypatch, ops, case, entry, xg, dyg):
    """(max-abs, rel L2) of the generic fp32 MFMA kernel on the same fp32 inputs: the split kernels' yardstick"""
    if "e32" not in entry:
        assert _route(monkeypatch, ops, "g3s1") == ops._wgrad_family(xg, dyg, case.Cx, case.Cy, 3, _stride(case))
        gw = torch.empty(case.Cy, case.Cx, 27, device=DEV)
        ops._wgrad(xg, dyg, gw, 0, case.Cx, case.Cy, 3, _stride(case), case.Cx * 27, 27)
        entry["e32"] = _errors(gw, entry["ref"])
    return entry["e32"]


def _gate(capsys, case, ntiles, nblk, got, entry, e32, split):
    """prints the row, then asserts the family's gate"""
    ref = entry["ref"]
    emax, el2 = _errors(got, ref)
    top = ref.abs().max().item()
    if split:
        g_l2 = 2e-6 if "p" in case.pack else 1e-6
        g_max = 1.5 * e32[0] + 1e-7 * top
    else:
        g_l2, g_max = 1e-5, 2e-5 * max(1.0, top)
    _print_row(capsys, (case.id, nblk, ntiles, el2, g_l2, emax, g_max, e32[0] if e32 else None, top))
    assert torch.isfinite(got).all()
    assert el2 <= g_l2, f"{case.id}: rel L2 {el2:.3e} > {g_l2:.1e}"
    assert emax <= g_max, f"{case.id}: max-abs {emax:.3e} > {g_max:.3e} (fp32 MFMA kernel {e32})"


def _run_wgrad(ops, case, xg, dyg):
    K = _ksize(case) ** 3
    gw = torch.full((case.Cy * case.Cx * K,), SENTINEL, device=DEV, dtype=torch.int32).view(torch.float32)
    ops._wgrad(xg, dyg, gw, 0, case.Cx, case.Cy, _ksize(case), _stride(case), case.Cx * K, K)
    return gw


# ---- the split kernels ---------------------------------------------------------------------------------------------------------
SPLIT = W.X2 + W.X3 + [c for c in W.REDUCE if c.family in ("x2", "x3")] + W.S2X2


@pytest.mark.parametrize("case", SPLIT, ids=[c.id for c in SPLIT])
def test_split_kernels_many_tiles(case, monkeypatch, capsys):
    """conv3d_wgrad_f16x2.hip (fp32 and packed px2 operands), conv3d_wgrad_bf16x3.hip, conv3d_wgrad_s2_f16x2.hip, and through
    their 32 -> 32 rows every loop combination of wgrad_reduce_kernel"""
    ops = _mods()
    x, dy = W.inputs(case, seeded_tensor)
    entry = _truth(case, x, dy)
    xg, dyg = x.to(DEV), dy.to(DEV)
    e32 = _mfma_error(monkeypatch, ops, case, entry, xg, dyg)
    want = _route(monkeypatch, ops, case.family)
    ntiles, nblk = _assert_regime(ops, case)
    xo = ops.pack_x2(xg) if case.pack[0] == "p" else xg
    yo = ops.pack_x2(dyg) if case.pack[1] == "p" else dyg
    assert ops._is_packed(xo) == (case.pack[0] == "p") and ops._is_packed(yo) == (case.pack[1] == "p")
    assert ops._wgrad_family(xo, yo, case.Cx, case.Cy, 3, _stride(case)) == want
    got = _run_wgrad(ops, case, xo, yo)
    _gate(capsys, case, ntiles, nblk, got, entry, e32, split=True)
    assert torch.equal(got, _run_wgrad(ops, case, xo, yo)), "not bitwise reproducible"


# ---- the generic fp32 kernels --------------------------------------------------------------------------------------------------
GEN = W.GENERIC + [c for c in W.REDUCE if c.family == "g1"]


@pytest.mark.parametrize("case", GEN, ids=[c.id for c in GEN])
def test_generic_kernels_many_tiles(case, monkeypatch, capsys):
    """wgrad3_kernel<1,32>, <1,16>, <2,32> and wgrad1_kernel<false> on their pipelined and plain paths, tile += gridDim.x"""
    ops = _mods()
    x, dy = W.inputs(case, seeded_tensor)
    entry = _truth(case, x, dy)
    xg = _misaligned(x) if case.misalign == "x" else x.to(DEV)
    dyg = _misaligned(dy) if case.misalign == "dy" else dy.to(DEV)
    want = _route(monkeypatch, ops, case.family)
    ntiles, nblk = _assert_regime(ops, case)
    assert ops._wgrad_family(xg, dyg, case.Cx, case.Cy, _ksize(case), _stride(case)) == want
    got = _run_wgrad(ops, case, xg, dyg)
    _gate(capsys, case, ntiles, nblk, got, entry, None, split=False)
    assert torch.equal(got, _run_wgrad(ops, case, xg, dyg)), "not bitwise reproducible"


def test_misaligned_operand_reaches_the_generic_kernel_with_the_split_kernels_on(monkeypatch):
    """the route `ops` itself takes for an operand that is not 16-byte aligned: with the split kernels switched ON the
    weight gradient goes to the generic kernel's plain path, and gives the bits the row above gave"""
    ops = _mods()
    case = next(c for c in W.GENERIC if c.id == "g32-misaligned-x")
    x, dy = W.inputs(case, seeded_tensor)
    xg, dyg = _misaligned(x), dy.to(DEV)
    _route(monkeypatch, ops, "x2")
    assert ops._wgrad_family(xg, dyg, case.Cx, case.Cy, 3, 1) == "mfma"
    on = _run_wgrad(ops, case, xg, dyg)
    _route(monkeypatch, ops, "g3s1")
    assert torch.equal(on, _run_wgrad(ops, case, xg, dyg))
    emax, el2 = _errors(on, _truth(case, x, dy)["ref"])
    assert el2 <= 1e-5, el2


# ---- the logit heads -------------------------------------------------------------------------------------------------------------
def _head_grad(ops, lib, monkeypatch, xg, wg, gyg, fused):
    """weight gradient of ops._Conv3dC1 with the calls of the two routes counted"""
    calls = {"fused": 0, "expand": 0}
    real_f, real_e = lib.dca_conv3d_c1_wgrad, lib.dca_conv3d_c1_expand

    def count(name, fn):
        def wrapped(*a):
            calls[name] += 1
            return fn(*a)
        return wrapped
    monkeypatch.setattr(ops, "C1_WGRAD_FUSED", fused)
    monkeypatch.setattr(lib, "dca_conv3d_c1_wgrad", count("fused", real_f))
    monkeypatch.setattr(lib, "dca_conv3d_c1_expand", count("expand", real_e))
    y = ops._Conv3dC1.apply(xg, wg)
    (gw,) = torch.autograd.grad(y, [wg], gyg)
    monkeypatch.setattr(lib, "dca_conv3d_c1_wgrad", real_f)
    monkeypatch.setattr(lib, "dca_conv3d_c1_expand", real_e)
    assert calls == ({"fused": 1, "expand": 0} if fused else {"fused": 0, "expand": 1}), calls
    return gw


@pytest.mark.parametrize("case", W.HEAD, ids=[c.id for c in W.HEAD])
def test_head_wgrad_many_tiles(case, monkeypatch, capsys):
    """wgrad1_kernel<true> through ops._Conv3dC1 (nn.Conv3d(C, 1, 3, padding=1)): the tap-shifted views of dy are built inside
    the kernel.  The small row also runs the expand + generic route on the same data; both are compared with fp64"""
    ops = _mods()
    lib = ops._L()
    _route(monkeypatch, ops, "x2")
    x, gy = W.inputs(case, seeded_tensor)
    entry = _truth(case, x, gy)                        # (1, C, 27)
    xg, gyg = x.to(DEV), gy.to(DEV)
    wg = (seeded_tensor("wgc.head.w", (1, case.Cx, 3, 3, 3)) * 0.05).to(DEV).requires_grad_()
    ntiles, nblk = _assert_regime(ops, case)
    got = _head_grad(ops, lib, monkeypatch, xg, wg, gyg, True)
    assert got.shape == (1, case.Cx, 3, 3, 3)
    _gate(capsys, case, ntiles, nblk, got, entry, None, split=False)
    assert torch.equal(got, _head_grad(ops, lib, monkeypatch, xg, wg, gyg, True)), "not bitwise reproducible"
    if not case.regimes:
        other = _head_grad(ops, lib, monkeypatch, xg, wg, gyg, False)
        _gate(capsys, case._replace(id=case.id + "-expand"), ntiles, nblk, other, entry, None, split=False)
        emax, el2 = _errors(got, other.detach().cpu().double().reshape(entry["ref"].shape))
        assert el2 <= 1e-5, ("fused against expand", el2)


# ---- the strided destination ---------------------------------------------------------------------------------------------------
def test_strided_destination_second_input_of_a_1x1x1_convolution(monkeypatch, capsys):
    """the layout _Conv3d.backward uses for the 1x1x1 `fuse` convolution of two inputs: dw[cy * Cin + C1 + cx]; only the second
    input's columns are written, the first input's keep the sentinel"""
    ops = _mods()
    case, C1 = W.STRIDED_C1, W.STRIDED_C1_FIRST
    Cin = C1 + case.Cx
    x2, dy = W.inputs(case, seeded_tensor)
    entry = _truth(case, x2, dy)
    want = _route(monkeypatch, ops, case.family)
    ntiles, nblk = _assert_regime(ops, case)
    x2g, dyg = x2.to(DEV), dy.to(DEV)
    assert ops._wgrad_family(x2g, dyg, case.Cx, case.Cy, 1, 1) == want

    def run():
        gw = torch.full((case.Cy * Cin,), SENTINEL, device=DEV, dtype=torch.int32).view(torch.float32)
        ops._wgrad(x2g, dyg, gw, C1, case.Cx, case.Cy, 1, 1, Cin, 1)
        return gw
    got = run()
    expect = torch.zeros(case.Cy * Cin, dtype=torch.float64)
    mask = W.scatter(entry["ref"], expect, Cin, 1, C1)
    words = got.cpu().view(torch.int32)
    assert int(mask.sum()) == case.Cy * case.Cx and bool((words[~mask] == SENTINEL).all()), "wrote outside its columns"
    assert bool((words.view(case.Cy, Cin)[:, :C1] == SENTINEL).all()) and bool((words[mask] != SENTINEL).all())
    entry_flat = {"ref": expect[mask]}
    _gate(capsys, case, ntiles, nblk, got.cpu()[mask], entry_flat, None, split=False)
    assert torch.equal(got.view(torch.int32), run().view(torch.int32)), "not bitwise reproducible"


def test_strided_destination_transposed_convolution(monkeypatch, capsys):
    """the transposed convolution's exchanged roles, _wgrad(dy, x, gw, 0, Cout, Cin, 3, 2, Cout * K, K), against the weight
    gradient autograd gives for F.conv_transpose3d in fp64: called directly into a sentinel-guarded destination at an offset,
    and through the autograd node, which must give the same bits"""
    ops = _mods()
    case = W.STRIDED_T                       # x = the FINE gradient of the output (Cout channels), dy = the coarse input (Cin)
    Cout, Cin, N = case.Cx, case.Cy, case.N
    cdims = W.out_dims(case)
    xc = seeded_tensor("wgc.t.x", (N, Cin) + cdims)
    gy = seeded_tensor("wgc.t.g", (N, Cout) + case.dims)
    w = seeded_tensor("wgc.t.w", (Cin, Cout, 3, 3, 3)) * 0.03
    wd = w.double().requires_grad_()
    (ref,) = torch.autograd.grad(F.conv_transpose3d(xc.double(), wd, None, 2, 1, 1), [wd], gy.double())
    entry = {"ref": ref.reshape(Cin, Cout, 27)}
    xg, gyg = xc.to(DEV), gy.to(DEV)
    e32 = _mfma_error(monkeypatch, ops, case, entry, gyg, xg)
    want = _route(monkeypatch, ops, "s2x2")
    ntiles, nblk = _assert_regime(ops, case)
    assert ops._wgrad_family(gyg, xg, Cout, Cin, 3, 2) == want
    pad = 5
    buf = torch.full((Cin * Cout * 27 + 2 * pad,), SENTINEL, device=DEV, dtype=torch.int32)
    ops._wgrad(gyg, xg, buf.view(torch.float32), pad, Cout, Cin, 3, 2, Cout * 27, 27)
    assert bool((buf[:pad] == SENTINEL).all()) and bool((buf[-pad:] == SENTINEL).all()), "wrote outside the destination"
    direct = buf[pad:-pad].view(torch.float32)
    _gate(capsys, case, ntiles, nblk, direct, entry, e32, split=True)
    wg = w.to(DEV).requires_grad_()
    (gw,) = torch.autograd.grad(ops.conv3d(xg, wg, 2, True), [wg], gyg)
    assert gw.shape == w.shape and torch.equal(gw.reshape(-1), direct), "the autograd node and the direct call differ"
