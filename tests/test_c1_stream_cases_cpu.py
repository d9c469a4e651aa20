"""What tests/test_gpu_c1_stream_fp64.py relies on, checked without a GPU: every row of tests/_c1_stream_cases.py is in the
regimes it names by the restated group walk, every (kernel, variant) and every template instantiation has the regimes it
needs, the restated grid is the library's own size query, the shapes sit on the side of `_c1x3_eligible` the rows claim,
the chunked fp64 references agree with independent formulations, and no row needs more device memory than the stated cap
-- so a later edit of the table cannot silently lose a branch, and a wrong reference cannot pass a wrong kernel."""
import pytest
import torch
import torch.nn.functional as F

import _c1_stream_cases as T

IDS = [c.id for c in T.ALL]
_GEO = {}


def geo(case):
    N, S, _ = T.shape_of(case)
    if (N, S) not in _GEO:
        _GEO[(N, S)] = T.geometry(N, S)
    return _GEO[(N, S)]


@pytest.mark.parametrize("case", T.ALL, ids=IDS)
def test_row_is_in_its_regimes(case):
    g = geo(case)
    assert case.regimes
    for r in case.regimes:
        assert T.REGIMES[r](g) is True, f"{case.id} is not in its regime: {r} (S {g.S}, G {g.G}, T {g.T}, grid {g.grid})"


def test_every_variant_and_instantiation_has_its_regimes():
    assert len(IDS) == len(set(IDS))
    assert {c.kernel for c in T.ALL} == set(T.INSTANCES)
    for (kernel, tag), regimes in T.REQUIRED.items():
        for lp in (("bf16", "fp16") if kernel == "lp" else (None,)):
            have = {r for c in T.ALL if c.kernel == kernel and c.lp == lp and (tag is None or tag in c.tags) for r in c.regimes}
            assert set(regimes) <= have, (kernel, tag, lp, sorted(set(regimes) - have))
    for c in T.ALL:
        assert c.inst in T.INSTANCES[c.kernel], c.id
        for tag in c.tags:
            assert (c.kernel, tag) in T.REQUIRED, (c.id, tag)
    # every instantiation the launchers can make runs past a wave's first group
    for kernel, insts in T.INSTANCES.items():
        for inst in insts:
            assert any(c.kernel == kernel and c.inst == inst and "mixed" in c.regimes for c in T.ALL), (kernel, inst)


def test_shapes_have_the_walk_they_were_derived_with():
    m = T.geometry(*T.shape_of(T.X3[0])[:2])
    assert (m.S, m.G, m.T, m.grid) == (324, 3, 9216, 2048)
    lens = [len(w) for w in m.waves]
    assert lens.count(2) == 1024 and lens.count(1) == 7168 and len(lens) == 8192
    assert m.waves[0] == [0, 8192] and T.decode(0, 324) == (0, 0, 32) and T.decode(8192, 324) == (2730, 256, 17)
    assert T.group_voxels(8192, 324) == 68 and T.decode(1, 324) == (0, 128, 32)
    mu = T.geometry(3072, T.voxels("Mu"))
    assert (mu.S, mu.G, mu.T, mu.grid) == (325, 3, 9216, 2048) and T.decode(2, 325) == (0, 256, 18) and T.group_voxels(2, 325) == 69
    d = T.geometry(T.SHAPES["D"].N, T.voxels("D"))
    assert (d.S, d.G, d.T, d.grid) == (68, 1, 3 * 8192 + 256, 2048)
    lens = [len(w) for w in d.waves]
    assert lens.count(4) == 256 and lens.count(3) == 8192 - 256 and T.decode(9000, 68) == (9000, 0, 17)
    i = T.geometry(1, T.voxels("I"))
    assert (i.S, i.G, i.T, i.grid) == (576, 5, 5, 2) and [len(w) for w in i.waves] == [1, 1, 1, 1, 1, 0, 0, 0]
    # below the thresholds the regimes are not reached: mixed needs T >= 9216, deep T >= 24576
    assert not T.REGIMES["mixed"](T.geometry(3071, 324)) and not T.REGIMES["deep"](T.geometry(24575, 68))
    assert T.REGIMES["mixed"](T.geometry(3072, 324)) and T.REGIMES["deep"](T.geometry(24576, 68))
    # G = 2 divides 4 * grid: no wave ever changes its position in the sample
    assert not T.REGIMES["shift"](T.geometry(6000, 256)) and T.REGIMES["samples"](T.geometry(6000, 256))


def test_walk_visits_every_group_once():
    for N, S in {T.shape_of(c)[:2] for c in T.ALL}:
        g = T.geometry(N, S)
        assert sorted(x for w in g.waves for x in w) == list(range(g.T))
        assert len(g.waves) == 4 * g.grid and g.grid <= T.GRID_CAP
        assert sum(T.group_voxels(x, S) for x in range(g.T)) == N * S


def test_restated_grid_is_the_librarys_size_query():
    """dca_conv1_x3_stats_chunks is `c1x_blocks`, the grid of the conv1_x3 launches; a host function, no device asked"""
    from dcanet_amd import _lib
    lib = _lib.load()
    shapes = {T.shape_of(c)[:2] for c in T.ALL} | {(1, 4), (1, 512), (1, 513), (3, 349184), (3, 349568), (4, 48 * 136 * 240)}
    for N, S in shapes:
        assert lib.dca_conv1_x3_stats_chunks(N, S) == T.grid(N, S), (N, S)
    assert T.grid(4, 48 * 136 * 240) == 2048 and T.groups(4, 48 * 136 * 240)[1] == 48960       # the bench shape: six per wave


def _shape_only(N, C, dims):
    return torch.empty((1, 1, 1, 1, 1)).expand(N, C, *dims)


@pytest.mark.parametrize("case", T.ALL, ids=IDS)
def test_shapes_are_on_the_side_of_the_eligibility_predicate_the_row_claims(case, monkeypatch):
    from dcanet_amd import ops
    monkeypatch.setattr(ops, "CONV_X3", True)
    N, S, dims = T.shape_of(case)
    x = _shape_only(N, case.C1, dims)
    x2 = _shape_only(N, case.C2, dims) if case.C2 else None
    y = _shape_only(N, case.Cout, dims)
    got = ops._c1x3_eligible(x, x2, 1, case.C1 + case.C2, case.C1, y)
    assert got is T.x3_eligible(case), case.id
    if case.kernel == "x3":
        assert got is True
        if "dx" in case.tags:       # the backward-data launches: dy (32 channels) in, C1 / C2 channels out
            assert ops._c1x3_eligible(y, None, 1, case.Cout, case.Cout, x) is True and case.Cout == 32
    if case.kernel == "mfma":
        assert got is ("vec" in case.tags) and ("vec" in case.tags) != ("scalar" in case.tags)
        assert (S % 4 == 0) is ("vec" in case.tags)
        monkeypatch.setattr(ops, "CONV_X3", False)
        assert ops._c1x3_eligible(x, x2, 1, case.C1 + case.C2, case.C1, y) is False
    if case.kernel == "lp":
        assert S % 4 == 0 and case.Cout <= 32 and (case.C1 + 15) // 16 + (case.C2 + 15) // 16 <= 8
    assert (case.C2 > 0) is ("two" in case.tags) and (case.Cout == 27) is ("head" in case.tags)


@pytest.mark.parametrize("case", T.ALL, ids=IDS)
def test_row_stays_under_the_device_memory_cap(case):
    assert T.DEVICE_BYTES_CAP == 1 << 30
    assert T.device_bytes(case) <= T.DEVICE_BYTES_CAP, (case.id, T.device_bytes(case))
    N, S, _ = T.shape_of(case)
    assert 64 * S * 4 < 0x7ffffff0, "inside the 31-bit per-sample offset limit of the launchers"


# ---- the references against independent formulations --------------------------------------------------------------------------------
def test_chunked_reference_is_the_unchunked_one_and_conv3d():
    g = torch.Generator().manual_seed(31)
    N, C1, C2, Cout, dims = 7, 5, 3, 6, (2, 3, 5)
    x, x2 = torch.randn((N, C1) + dims, generator=g), torch.randn((N, C2) + dims, generator=g)
    w = torch.randn((Cout, C1 + C2, 1, 1, 1), generator=g)
    whole = T.ref_forward(x, x2, w, chunk=N)
    assert whole.dtype == torch.float64 and whole.shape == (N, Cout) + dims
    for chunk in (1, 2, 3, 100):
        assert torch.equal(T.ref_forward(x, x2, w, chunk=chunk), whole), chunk
    want = F.conv3d(torch.cat([x, x2], 1).double(), w.double())
    assert torch.allclose(whole, want, rtol=1e-13, atol=1e-13)
    one = T.ref_forward(x, None, w[:, :C1], chunk=2)
    assert torch.allclose(one, F.conv3d(x.double(), w[:, :C1].double()), rtol=1e-13, atol=1e-13)
    # 2-byte operands are taken at their rounded values
    xb, wb = x.to(torch.bfloat16), w.to(torch.bfloat16)
    assert torch.equal(T.ref_forward(xb, None, wb[:, :C1], chunk=3), T.ref_forward(xb.float(), None, wb[:, :C1].float(), chunk=N))


def test_backward_data_reference_is_autograd_of_conv3d():
    g = torch.Generator().manual_seed(32)
    N, C1, C2, Cout, dims = 5, 4, 3, 6, (2, 3, 4)
    w = torch.randn((Cout, C1 + C2, 1, 1, 1), generator=g)
    gy = torch.randn((N, Cout) + dims, generator=g)
    xd = torch.zeros((N, C1 + C2) + dims, dtype=torch.float64, requires_grad=True)
    (gx,) = torch.autograd.grad(F.conv3d(xd, w.double()), [xd], gy.double())
    assert torch.allclose(T.ref_backward_data(w, gy, 0, C1, chunk=2), gx[:, :C1], rtol=1e-13, atol=1e-13)
    assert torch.allclose(T.ref_backward_data(w, gy, C1, C1 + C2, chunk=2), gx[:, C1:], rtol=1e-13, atol=1e-13)


def test_statistics_and_epilogue_are_the_shared_references():
    import _conv_tile_cases as C
    assert T.fold_partials is C.fold_partials and T.ref_epilogue is C.ref_epilogue and T.ref_stats is C.ref_stats


def test_group_max_and_worst_group_follow_the_group_index():
    N, S = 3, 324
    v = torch.zeros(N, 2, 3, 4, 27)
    flat = v.view(N, 2, S)
    for g in range(9):
        n, v0, _ = T.decode(g, S)
        flat[n, g % 2, v0 + (g % 5)] = g + 1.0
    assert T.group_max(v, N, S).tolist() == [g + 1.0 for g in range(9)]
    flat[2, 1, 323] = float("nan")           # the last voxel of the ragged group of the last sample
    assert T.group_max(v, N, S)[-1] == float("inf")
    text = T.worst_group(v, N, S)
    assert "worst group 8 = (n 2, voxels 256..323, 17 lanes)" in text and "wave 8 = workgroup 2 wave 0, trip 1 of its 1" in text
    # a group of a wave's second trip
    M = T.SHAPES["M"].N
    e = torch.zeros(M, 1, 3, 4, 27)
    e.view(M, 1, S)[2730, 0, 300] = 2.0
    text = T.worst_group(e, M, S)
    assert "worst group 8192 = (n 2730, voxels 256..323, 17 lanes)" in text, text
    assert "wave 0 = workgroup 0 wave 0, trip 2 of its 2; 1 of 9216 groups over the gate" in text, text


def test_inputs_are_shared_between_rows_of_one_key():
    from oracle.seeded import seeded_tensor
    by = {c.id: c for c in T.ALL}
    assert T.data_key(by["x3-M-32-plain"]) == T.data_key(by["x3-M-32-stats"]) == T.data_key(by["mfma-M-32-epi"])
    assert T.data_key(by["x3-M-32-plain"]) != T.data_key(by["lp-M-32-epi-bf16"])
    c = by["x3-I-32-stats"]
    assert T.tensor(c, "x", seeded_tensor).shape == (1, 32, 2, 4, 72) and T.tensor(c, "w", seeded_tensor).shape == (32, 32, 1, 1, 1)
    c = by["x3-M-27-plain"]
    assert T.tensor(c, "w", seeded_tensor).shape == (27, 32, 1, 1, 1) and T.tensor(c, "scale", seeded_tensor).shape == (27,)
