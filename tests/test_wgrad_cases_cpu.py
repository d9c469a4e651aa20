"""What tests/test_gpu_wgrad_fp64.py relies on, checked without a GPU: the reference helper of tests/_wgrad_cases.py equals
the weight gradient autograd gives in fp64, the scatter helper writes exactly the strided layout, every row of the table is
in the regime it names on a 256-CU device by the tile arithmetic, and every regime the gate exists for has a row -- so a
later edit of the table cannot silently lose a branch."""
import pytest
import torch
import torch.nn.functional as F

import _wgrad_cases as W

IDS = [c.id for c in W.EVERY]


@pytest.mark.parametrize("ksize,stride", [(3, 1), (3, 2), (1, 1)])
@pytest.mark.parametrize("N,Cx,Cy,dims", [(2, 3, 5, (4, 5, 6)), (1, 4, 2, (3, 7, 5))])
def test_reference_is_autograd_conv3d(ksize, stride, N, Cx, Cy, dims):
    g = torch.Generator().manual_seed(11)
    x = torch.randn((N, Cx) + dims, generator=g)
    w = torch.randn((Cy, Cx, ksize, ksize, ksize), generator=g, dtype=torch.float64, requires_grad=True)
    y = F.conv3d(x.double(), w, None, stride, ksize // 2)
    dy = torch.randn(y.shape, generator=g)
    (gw,) = torch.autograd.grad((y * dy.double()).sum(), [w])
    ref = W.reference(x, dy, ksize, stride)
    assert ref.dtype == torch.float64 and ref.shape == (Cy, Cx, ksize ** 3)
    assert torch.allclose(ref, gw.reshape(Cy, Cx, -1), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("N,Cin,Cout,cdims", [(2, 3, 5, (2, 3, 4)), (1, 4, 2, (3, 2, 5))])
def test_reference_is_autograd_conv_transpose3d(N, Cin, Cout, cdims):
    """the transposed convolution's weight gradient is the stride-2 one with the tensors' roles exchanged: the fine gradient
    of the output as x, the coarse input as dy, and dW[cin][cout][k] as the result"""
    g = torch.Generator().manual_seed(12)
    x = torch.randn((N, Cin) + cdims, generator=g)
    w = torch.randn((Cin, Cout, 3, 3, 3), generator=g, dtype=torch.float64, requires_grad=True)
    y = F.conv_transpose3d(x.double(), w, None, 2, 1, 1)
    dy = torch.randn(y.shape, generator=g)
    (gw,) = torch.autograd.grad((y * dy.double()).sum(), [w])
    ref = W.reference(dy, x, 3, 2)
    assert ref.shape == (Cin, Cout, 27)
    assert torch.allclose(ref, gw.reshape(Cin, Cout, 27), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("Cy,Cx,K,s_cy,s_cx,offset,size", [
    (3, 4, 1, 9, 1, 5, 27),          # second input of a two-input 1x1x1 convolution: Cin = 9, C1 = 5
    (2, 3, 27, 81, 27, 0, 162),      # contiguous [Cy][Cx][27]
    (3, 2, 27, 27, 81, 7, 250),      # exchanged roles with an offset
])
def test_scatter_leaves_every_other_element_alone(Cy, Cx, K, s_cy, s_cx, offset, size):
    ref = torch.arange(1, Cy * Cx * K + 1, dtype=torch.float64).view(Cy, Cx, K)
    dest = torch.full((size,), -7.0, dtype=torch.float64)
    mask = W.scatter(ref, dest, s_cy, s_cx, offset)
    assert int(mask.sum()) == ref.numel() and (dest[~mask] == -7.0).all()
    for cy in range(Cy):
        for cx in range(Cx):
            for k in range(K):
                assert dest[offset + cy * s_cy + cx * s_cx + k] == ref[cy, cx, k]


def library_walk(tiles, grid, wg):
    """(status, [begin, end, step]) of dca_tile_walk: csrc/dca_tiles.h, the function the kernels call, run on the host"""
    import ctypes
    from dcanet_amd import _lib
    out = (ctypes.c_int * 3)(-1, -1, -1)
    return _lib.load().dca_tile_walk(tiles, grid, wg, ctypes.addressof(out)), list(out)


@pytest.mark.parametrize("ntiles,nblk", [(96, 28), (12, 7), (75, 64), (270, 256), (120, 28), (288, 256), (9, 9), (1, 1)])
def test_walks_visit_every_tile_once(ntiles, nblk):
    for walk in (W.split_walk, W.generic_walk):
        seen = sorted(t for w in walk(ntiles, nblk) for t in w)
        assert seen == list(range(ntiles)), walk.__name__
    # the arithmetic the kernels run, not only its restatement
    got = []
    for wg in range(nblk):
        st, (begin, end, step) = library_walk(ntiles, nblk, wg)
        assert st == 0 and step >= 1, (wg, st, step)
        got.append(list(range(begin, end, step)))
    assert got == W.split_walk(ntiles, nblk)
    assert sorted(t for w in got for t in w) == list(range(ntiles))


@pytest.mark.parametrize("grid", [256, 7])
def test_library_walk_does_not_overflow_at_the_largest_tile_count(grid):
    """tiles = 0x7ffffffe, the largest count a launcher accepts: T * xcd and T * (xcd + 1) need 64-bit products"""
    T = 0x7ffffffe
    nx = 8 if grid >= 8 else 1
    for wg in (0, 7, grid - 1):
        if wg >= grid:     # wg 7 of a grid of 7 does not exist
            assert library_walk(T, grid, wg)[0] == 1
            continue
        xcd = wg % nx
        want = [T * xcd // nx + wg // nx, T * (xcd + 1) // nx, (grid - xcd + nx - 1) // nx]
        assert library_walk(T, grid, wg) == (0, want), wg


@pytest.mark.parametrize("tiles,grid,wg", [
    (-1, 8, 0),                                  # tiles < 0
    (0x7fffffff, 8, 0), (1 << 40, 8, 0),         # tiles >= 0x7fffffff: tile indices are ints in the kernels
    (10, 0, 0), (10, -3, 0),                     # grid <= 0
    (10, 8, -1), (10, 8, 8), (10, 1, 1),         # wg outside [0, grid)
])
def test_library_walk_refuses_invalid_arguments(tiles, grid, wg):
    st, out = library_walk(tiles, grid, wg)
    assert st == 1 and out == [-1, -1, -1], "hipErrorInvalidValue, nothing written"
    assert library_walk(10, 8, 7)[0] == 0 and library_walk(0, 1, 0) == (0, [0, 0, 1])


@pytest.mark.parametrize("case", W.EVERY, ids=IDS)
def test_row_is_in_its_regime_on_256_cus(case):
    ntiles, nCT, share, nblk = W.geometry(case, 256)
    assert 1 <= nblk <= ntiles
    for r in case.regimes:
        assert W.REGIMES[r](case, ntiles, nCT, nblk) is True, f"{case.id} is not in its regime: {r} " \
                                                              f"(ntiles {ntiles}, nCT {nCT}, nblk {nblk})"


def test_rows_have_the_geometry_they_were_derived_with():
    """the figures the rows were derived with"""
    by = {c.id: W.geometry(c, 256) for c in W.ALL}
    assert by["x2-uneven-pp"] == (96, 9, 9, 28) and by["x3-nx1"] == (12, 36, 36, 7)
    assert by["s2x2-blkoff"] == (120, 15, 9, 28)
    assert by["g1-vec"] == (144, 9, 9, 56) and by["head-c64"] == (600, 2, 2, 256)
    assert [by[f"reduce-x3-{t}"][3] for t in (1, 12, 75, 120, 150, 288)] == [1, 12, 75, 120, 150, 256]
    assert by["reduce-g1-170x3"][3] == 170
    cnt = {len(w) for w in W.split_walk(96, 28)}
    assert cnt == {3, 4}, "chunks of 12 tiles over 4 or 3 workgroups"


def test_every_regime_has_a_row():
    assert set(W.REQUIRED) == set(W.FAMILIES)
    for fam, regimes in W.REQUIRED.items():
        have = {r for c in W.ALL if c.family == fam for r in c.regimes}
        assert set(regimes) <= have, (fam, sorted(set(regimes) - have))
    assert all(r in W.REGIMES for c in W.ALL for r in c.regimes)
    assert {c.pack for c in W.X2 if c.id.startswith("x2-uneven")} == {"ff", "pf", "fp", "pp"}
    assert sum(c.pow2 for c in W.ALL if c.family == "x2") >= 1 and all(
        any(c.pow2 for c in W.ALL if c.family == f) for f in ("x3", "s2x2", "g3s1", "g1", "head"))
    assert len(IDS) == len(set(IDS))


def test_reduce_iters_restates_the_two_loops():
    assert W.reduce_iters(112) == [(0, 7)] * 16
    assert W.reduce_iters(128) == [(1, 0)] * 16 and W.reduce_iters(256) == [(2, 0)] * 16
    assert W.reduce_iters(120) == [(1, 0)] * 8 + [(0, 7)] * 8
    assert W.reduce_iters(150)[0] == (1, 2) and W.reduce_iters(150)[15] == (1, 1)


def test_inputs_are_small():
    from oracle.seeded import seeded_tensor
    for c in W.ALL:
        Cy = 1 if c.family == "head" else c.Cy
        od = W.out_dims(c)
        n = c.N * (c.Cx * c.dims[0] * c.dims[1] * c.dims[2] + Cy * od[0] * od[1] * od[2])
        assert n * 4 <= 96 << 20, (c.id, n)
    x, dy = W.inputs(W.HEAD[1], seeded_tensor)
    assert x.shape == (2, 32, 5, 9, 20) and dy.shape == (2, 1, 5, 9, 20)
