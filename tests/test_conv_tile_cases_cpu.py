"""What tests/test_gpu_conv_tiles_fp64.py relies on, checked without a GPU: every row of tests/_conv_tile_cases.py is in the
regime it names on a 256-CU device by the restated tile arithmetic, every (kernel, variant) has the regimes it needs, the
restated walk is the library's `dca_tile_walk` and a partition of the tiles, the restated tile counts are the ones the
eligibility predicates of ops.py count, and the fp64 references agree with independent formulations -- so a later edit of
the table cannot silently lose a branch, and a wrong reference cannot pass a wrong kernel."""
import pytest
import torch
import torch.nn.functional as F

import _conv_tile_cases as T
from _wgrad_cases import split_walk

IDS = [c.id for c in T.ALL]


def library_walk(tiles, grid, wg):
    """(status, [begin, end, step]) of dca_tile_walk: csrc/dca_tiles.h, the function the kernels call, run on the host"""
    import ctypes
    from dcanet_amd import _lib
    out = (ctypes.c_int * 3)(-1, -1, -1)
    return _lib.load().dca_tile_walk(tiles, grid, wg, ctypes.addressof(out)), list(out)


@pytest.mark.parametrize("case", T.ALL, ids=IDS)
def test_row_is_in_its_regime_on_256_cus(case):
    g = T.geometry(case, 256)
    assert 1 <= g.grid <= g.tiles and case.regimes
    for r in case.regimes:
        assert T.REGIMES[r](g) is True, f"{case.id} is not in its regime: {r} (tiles {g.tiles}, share {g.share}, grid {g.grid})"


def test_every_variant_has_its_regimes():
    assert len(IDS) == len(set(IDS))
    assert {c.kernel for c in T.ALL} == set(T.KERNELS)
    for (kernel, tag, *_), regimes in T.REQUIRED.items():
        lps = ("bf16", "fp16") if kernel in ("lp", "s2lp", "dlp") else (None,)
        for lp in lps:
            have = {r for c in T.ALL if c.kernel == kernel and c.lp == lp and (tag is None or tag in c.tags) for r in c.regimes}
            assert set(regimes) <= have, (kernel, tag, lp, sorted(set(regimes) - have))
    # every variant tag in the table is one REQUIRED knows
    for c in T.ALL:
        for tag in c.tags:
            assert (c.kernel, tag) in T.REQUIRED or c.lp is not None, (c.id, tag)
    # what the model's 32-channel layers launch: one grid row
    for kernel, regimes in T.SHARE1.items():
        have = {r for c in T.ALL if c.kernel == kernel and T.geometry(c).share == 1 for r in c.regimes}
        assert set(regimes) <= have, (kernel, have)
    # conv3d_lp: streaming-weights mode and the unaligned staging, in both types
    for lp in ("bf16", "fp16"):
        rows = [c for c in T.ALL if c.kernel == "lp" and c.lp == lp]
        assert any(c.Cin >= 128 for c in rows) and any(c.dims[2] % 4 for c in rows)


def test_variant_tags_say_what_the_shapes_are():
    for c in T.ALL:
        N, A, B, dims = T.launch_of(c)
        if "quad" in c.tags or "px2" in c.tags:
            assert dims[2] % 4 == 0, c.id
        if "single" in c.tags:
            assert dims[2] % 4 != 0, c.id
        if "px2" in c.tags:
            assert c.kernel == "x2" and A % 8 == 0, c.id
        if "stream" in c.tags:
            assert A >= 64 and chunks(A, c.kernel) >= (4 if c.kernel == "x3" else 8), c.id
        if "dx" in c.tags:      # a partial second block of 32 output channels in dx
            assert c.Cin == 40 and B == 40 and T.geometry(c).share == 2, c.id
        if "bwd" in c.tags:     # the transposed kernel takes it: <= 32 output channels, <= 64 in, coarse W % 4 == 0, even fine dims
            assert B <= 32 and A <= 64 and dims[2] % 4 == 0 and all(d % 2 == 0 for d in c.dims), c.id
        if c.kernel in ("dx3", "dlp"):
            assert B <= 32 and A <= 64, c.id
        if c.kernel == "dx3":
            assert dims[2] % 4 == 0, c.id
        if c.kernel in ("s2x2", "s2lp"):
            assert dims[2] % 4 == 0 and B <= (256 if c.kernel == "s2x2" else 64) and A > 4, c.id
    assert any(c.kernel == "s2x2" and c.Cin % 8 for c in T.S2X2) and any((c.Cin, c.Cout) == (32, 64) for c in T.S2X2)
    assert {(c.Cin, c.Cout) for c in T.DX3 if "bwd" not in c.tags} == {(64, 32), (40, 27)}


def chunks(A, kernel):
    """channel chunks of a launch: 8 channels per chunk in conv3d_f16x2.hip, 16 in conv3d_bf16x3.hip and conv3d_lp.hip"""
    return (A + 7) // 8 if kernel == "x2" else (A + 15) // 16


def test_rows_have_the_geometry_they_were_derived_with():
    by = {c.id: T.geometry(c, 256) for c in T.ALL}
    g = by["x2-m1q-plain"]
    assert (g.tiles, g.share, g.grid, g.nT) == (264, 1, 256, (2, 2, 2)) and sorted(set(map(len, g.walk))) == [1, 2]
    g = by["x3-d3s-stats"]
    assert (g.tiles, g.share, g.grid, g.nT) == (276, 3, 85, (2, 2, 3)) and sorted(set(map(len, g.walk))) == [3, 4]
    assert {(w[1] - w[0]) for w in g.walk} == {10, 11}, "XCDs with 11 and with 10 workgroups"
    g = by["x2-idle-stats"]
    assert (g.tiles, g.grid) == (9, 9) and g.walk[0] == [0] and g.walk[8] == [], "XCD 0: two workgroups, one tile"
    g = by["x2-dx-d"]
    assert (g.tiles, g.share, g.grid) == (384, 2, 128)
    g = by["s2x2-r-epi"]
    assert (g.tiles, g.share, g.grid, g.nT, g.tile) == (276, 3, 85, (2, 2, 3), (2, 4, 32))
    g = by["dx3-d-bwd"]
    assert (g.tiles, g.grid, g.nT, g.tile, g.out_tile) == (768, 256, (2, 2, 2), (2, 8, 16), (4, 16, 32))
    g = by["s2lp-m-fp16"]
    assert (g.tiles, g.grid, g.nT) == (264, 256, (2, 2, 2))


def test_grid_rule():
    assert T.persistent_grid("x3", 1000, 1, 256) == 256 and T.persistent_grid("x3", 1000, 3, 256) == 85
    assert T.persistent_grid("x3", 40, 1, 256) == 40 and T.persistent_grid("x3", 1000, 300, 256) == 1
    assert T.persistent_grid("x3", 5000, 1, 2048) == 2048 and T.persistent_grid("x2", 5000, 1, 2048) == 1024


@pytest.mark.parametrize("case", T.ALL, ids=IDS)
def test_walk_is_the_librarys_and_visits_every_tile_once(case):
    g = T.geometry(case, 256)
    got = []
    for wg in range(g.grid):
        st, (begin, end, step) = library_walk(g.tiles, g.grid, wg)
        assert st == 0 and step >= 1, (wg, st, step)
        got.append(list(range(begin, end, step)))
    assert got == g.walk == split_walk(g.tiles, g.grid)
    assert sorted(t for w in got for t in w) == list(range(g.tiles))
    for t in (0, g.tiles // 2, g.tiles - 1):
        wg, pos, cnt = T.tile_owner(g, t)
        assert g.walk[wg][pos] == t and cnt == len(g.walk[wg])


def test_decode_is_w_fastest():
    nT = (2, 3, 4)
    seen = [T.decode(t, 2, nT) for t in range(2 * 24)]
    assert seen[0] == (0, 0, 0, 0) and seen[1] == (0, 0, 0, 1) and seen[4] == (0, 0, 1, 0) and seen[12] == (0, 1, 0, 0)
    assert seen[24] == (1, 0, 0, 0) and len(set(seen)) == 48


def test_tile_max_follows_the_tile_index():
    g = T.geometry_of("dx3", 2, 8, 8, (3, 9, 20), 256)         # coarse tiles 2 x 8 x 16 -> fine 4 x 16 x 32
    assert g.nT == (2, 2, 2) and g.out_tile == (4, 16, 32)
    v = torch.zeros(2, 3, 6, 18, 40)
    for t in range(g.tiles):
        n, td, th, tw = T.decode(t, g.N, g.nT)
        v[n, t % 3, td * 4, th * 16, tw * 32] = t + 1.0        # the tile's first voxel
    per = T.tile_max(v, g)
    assert per.tolist() == [t + 1.0 for t in range(g.tiles)]
    v[1, 0, 5, 17, 39] = float("nan")                          # the last voxel of the last (partial) tile
    assert T.tile_max(v, g)[-1] == float("inf")
    assert "worst tile 15 = (n 1, d0 4, h0 16, w0 32)" in T.worst_tile(v, g)


# ---- the restated tile counts are the ones ops.py counts ----------------------------------------------------------------------------
def _shape_only(N, dims):
    return torch.empty((N, 1) + tuple(dims)).expand(N, 1, *dims)


@pytest.mark.parametrize("case", [c for c in T.ALL if c.kernel in ("x2", "x3", "s2x2") and "bwd" not in c.tags],
                         ids=lambda c: c.id)
def test_tile_count_is_the_one_the_eligibility_predicate_counts(case, monkeypatch):
    """_x3_eligible and _s2x2_eligible compare `tiles * channel blocks` with _X3_MIN_WORKGROUPS: eligible at exactly the
    restated count, not at one more"""
    from dcanet_amd import ops
    N, A, B, dims = T.launch_of(case)
    g = T.geometry(case)
    x = _shape_only(N, dims)
    monkeypatch.setattr(ops, "CONV_X3", True)
    monkeypatch.setattr(ops, "CONV_X2", True)
    monkeypatch.setattr(ops, "CONV_S2_X2", True)
    for floor, want in ((g.tiles * g.share, True), (g.tiles * g.share + 1, False)):
        monkeypatch.setattr(ops, "_X3_MIN_WORKGROUPS", floor)
        if case.kernel == "s2x2":
            assert ops._s2x2_eligible(x, None, 3, 2, False, A, B, None, None, 1.0) is want, (case.id, floor)
        else:
            assert ops._x3_eligible(x, None, 3, 1, False, A, B) is want, (case.id, floor)


def test_slice_width_matches_the_channel_blocks():
    """the generic launcher's slices (ops._slice_width) against the split kernels' channel blocks: 32 wide at stride 1 and for
    the transposed kernels, 64 wide at stride 2"""
    from dcanet_amd import ops
    assert ops._slice_width(3, 2, True, 32) == 32 and ops._slice_width(3, 2, False, 64) == 64
    assert ops._slice_width(3, 1, False, 32) == 32
    assert T.tiles_s1(1, 32, 96, (4, 8, 16))[2] == 3 and T.tiles_s2x2(1, 32, 160, (4, 8, 64))[2] == 3
    assert T.tiles_coarse_in(1, 64, 32, (2, 8, 16))[2] == 1 and T.tiles_s2lp(1, 16, 64, (4, 16, 32))[2] == 1


# ---- the references against independent formulations --------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [1, 2])
def test_backward_data_is_conv3d_input(stride):
    g = torch.Generator().manual_seed(21)
    N, Cin, Cout, dims = 2, 3, 5, (4, 6, 8)
    w = torch.randn((Cout, Cin, 3, 3, 3), generator=g)
    odims = tuple((d + stride - 1) // stride for d in dims)
    gy = torch.randn((N, Cout) + odims, generator=g)
    got = T.ref_backward_data((N, Cin) + dims, w, gy, stride, False)
    want = torch.nn.grad.conv3d_input((N, Cin) + dims, w.double(), gy.double(), stride=stride, padding=1)
    assert got.dtype == torch.float64 and torch.allclose(got, want, rtol=1e-12, atol=1e-12)


def test_transposed_forward_is_backward_data_of_the_stride_2_convolution():
    g = torch.Generator().manual_seed(22)
    N, Cin, Cout, cdims = 2, 5, 3, (2, 3, 4)
    x = torch.randn((N, Cin) + cdims, generator=g)
    w = torch.randn((Cin, Cout, 3, 3, 3), generator=g)        # ConvTranspose3d layout = Conv3d(Cout -> Cin) layout
    y = T.ref_forward(x, w, 2, True)
    fine = tuple(2 * d for d in cdims)
    assert y.shape == (N, Cout) + fine
    want = T.ref_backward_data((N, Cout) + fine, w, x, 2, False)
    assert torch.allclose(y, want, rtol=1e-12, atol=1e-12)
    # and the transposed operator's own backward-data is the stride-2 convolution
    gy = torch.randn(y.shape, generator=g)
    dx = T.ref_backward_data(x.shape, w, gy, 2, True)
    assert torch.allclose(dx, F.conv3d(gy.double(), w.double(), None, 2, 1), rtol=1e-12, atol=1e-12)


def test_statistics_are_var_mean_and_the_fold_of_partials():
    g = torch.Generator().manual_seed(23)
    y = torch.randn(3, 4, 5, 6, 7, generator=g) * 2.0 + 5.0
    mean, var = T.ref_stats(y)
    v2, m2 = torch.var_mean(y.double().transpose(0, 1).reshape(4, -1), dim=1, unbiased=False)
    assert torch.allclose(mean, m2, rtol=1e-13, atol=0) and torch.allclose(var, v2, rtol=1e-12, atol=0)
    assert torch.equal(T.ref_cmax(y), y.double().abs().transpose(0, 1).reshape(4, -1).amax(1))
    # partials {K, n, s, q} of three "workgroups": two with data, each centred on a value of its own; one without tiles
    flat = y.double().transpose(0, 1).reshape(4, -1)
    parts = torch.zeros(4, 3, 4, dtype=torch.float64)
    for j, sl in enumerate((slice(0, 200), slice(200, None))):
        chunk = flat[:, sl]
        K = chunk[:, 0]
        d = chunk - K[:, None]
        parts[:, j] = torch.stack([K, torch.full((4,), float(chunk.shape[1]), dtype=torch.float64), d.sum(1), (d * d).sum(1)], 1)
    cnt, m3, v3 = T.fold_partials(parts.reshape(-1), 4)
    assert torch.equal(cnt, torch.full((4,), float(flat.shape[1]), dtype=torch.float64))
    assert torch.allclose(m3, m2, rtol=1e-13, atol=0) and torch.allclose(v3, v2, rtol=1e-11, atol=0)


def test_epilogue_reference():
    g = torch.Generator().manual_seed(24)
    y, rp, rq = (torch.randn(2, 3, 2, 3, 4, generator=g) for _ in range(3))
    sc, sh = torch.rand(3, generator=g) + 0.5, torch.randn(3, generator=g)
    got = T.ref_epilogue(y, sc, sh, 0.1, rp, rq)
    want = F.leaky_relu(y.double() * sc.double().view(1, 3, 1, 1, 1) + sh.double().view(1, 3, 1, 1, 1) + rp.double(), 0.1) + rq.double()
    assert torch.allclose(got, want, rtol=1e-14, atol=0)
    assert torch.equal(T.ref_epilogue(y), y.double())


def test_inputs_are_small_and_shared():
    from oracle.seeded import seeded_tensor
    for c in T.ALL:
        od = T.out_dims(c)
        n = c.N * (c.Cin * c.dims[0] * c.dims[1] * c.dims[2] + c.Cout * od[0] * od[1] * od[2])
        assert n * 4 <= 128 << 20, (c.id, n)
    by = {c.id: c for c in T.ALL}
    assert T.data_key(by["x2-m1q-plain"]) == T.data_key(by["x3-m1q-stats"]) == T.data_key(by["x2-m1q-px2"])
    assert T.data_key(by["dx3-m-bwd"]) != T.data_key(by["dx3-m-plain"])
    c = by["x2-idle-epi"]
    assert T.tensor(c, "x", seeded_tensor).shape == (1, 32, 9, 17, 12) and T.tensor(c, "w", seeded_tensor).shape == (32, 32, 3, 3, 3)
    assert T.tensor(by["dx3-idle-stats"], "res_post", seeded_tensor).shape == (1, 32, 10, 34, 32)
    assert T.tensor(by["dx3-idle-stats"], "w", seeded_tensor).shape == (64, 32, 3, 3, 3)
