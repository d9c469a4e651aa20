"""The table, the chunk arithmetic, the plants and the reference of tests/test_gpu_bn_chunks_fp64.py, checked without a GPU:
a row that is not in the regimes it names, a plant that is not where it claims to be or is not its channel's extreme, or data
on which PyTorch's own fp32 BatchNorm misses the gates would make the GPU test prove nothing."""
import math

import pytest
import torch

import _bn_cases as B
from oracle.seeded import seeded_tensor

IDS = [c.id for c in B.CASES]


def test_chunking_mirror_on_known_values():
    """`chunking` by hand: want = min(256, ceil(2048 / C)), len = ceil(S / want) up to a multiple of 1024, nchunk =
    ceil(S / len)"""
    assert B.chunking(288, 32) == (1, 1024) and B.chunking(1024, 8) == (1, 1024) and B.chunking(1025, 8) == (2, 1024)
    assert B.chunking(4320, 32) == (5, 1024)                    # want 64 -> 68 -> 1024
    assert B.chunking(69120, 32) == (34, 2048)                  # want 64 -> 1080 -> 2048; 33 full chunks + 1536
    assert B.chunking(69120, 4) == (68, 1024)                   # want 256 -> 270 -> 1024; 67 full chunks + 512
    assert B.chunking(261392, 8) == (256, 1024)                 # want 256 -> 1022 -> 1024; 255 full chunks + 272
    assert B.chunking(262144, 8) == (256, 1024) and B.chunking(262145, 8) == (129, 2048)     # the cap: never above 256
    assert B.pack_chunks(32, 69120) == B.chunking(69120, 4) and B.plain_chunks(32, 69120) == B.chunking(69120, 32)
    for C in (1, 4, 8, 12, 32, 64, 2048, 4096):
        for S in (1, 1023, 1024, 1025, 65536, 65537, 261392, 10 ** 7):
            n, length = B.chunking(S, C)
            assert 1 <= n <= B.BN_MAX_CHUNKS and length % 1024 == 0 and (n - 1) * length < S <= n * length


@pytest.mark.parametrize("cid", IDS)
def test_rows_are_in_their_regimes(cid):
    case = B.BY_ID[cid]
    g = B.geometry(case)
    assert g.S == case.S and g.plain == case.plain, (cid, g)
    assert (case.pack is None) == (not g.packable) and (case.pack is None or g.pack == case.pack), (cid, g)
    assert g.plain_len % g.pack_len == 0 or g.pack_len % g.plain_len == 0     # a coarse chunk is a union of fine ones
    for r in case.regimes:
        assert B.REGIMES[r](g) is True, f"{cid} is not in its regime: {r} ({g})"
    assert g.N * g.C * g.S <= 2.25e6      # "add no larger row": over64-pack is 2.21 M floats


def test_table_covers_every_regime():
    named = {r for c in B.CASES for r in c.regimes}
    assert named == set(B.REGIMES), set(B.REGIMES) - named
    # the first size at which the two counts differ at C = 32 lies past 1024 * 64 voxels
    assert B.plain_chunks(32, 65536)[0] == B.pack_chunks(32, 65536)[0] == 64
    assert B.plain_chunks(32, 65537)[0] == 33 and B.pack_chunks(32, 65537)[0] == 65


@pytest.mark.parametrize("cid", IDS)
def test_plants_lie_in_the_chunks_they_claim(cid):
    case = B.BY_ID[cid]
    g = B.geometry(case)
    seen = set()
    for q in B.QUANTITIES:
        ps = B.plants(case, q)
        assert [p.c for p in ps] == list(range(case.C))
        kinds = {p.kind for p in ps}
        assert kinds == set(B.KINDS), (cid, q, kinds)
        for p in ps:
            assert 0 <= p.voxel < g.S and 0 <= p.n < g.N
            assert (p.voxel // g.plain_len, p.voxel // g.pack_len) == (p.plain_chunk, p.pack_chunk)
            assert (p.plain_chunk, p.pack_chunk) == B.claimed_chunks(case, p.kind), (cid, q, p)
            if p.kind == "last":      # the clipped chunk of BOTH chunkings
                assert p.voxel >= (g.plain - 1) * g.plain_len and p.voxel >= (g.pack - 1) * g.pack_len
            if p.kind == "high":
                most = max(g.plain, g.pack)
                assert 0 < p.plain_chunk < g.plain - 1 and 0 < p.pack_chunk < g.pack - 1
                assert max(p.plain_chunk, p.pack_chunk) >= 64 if most > 65 else True, (cid, q, p)
            assert (p.n, p.c, p.voxel) not in seen
            seen.add((p.n, p.c, p.voxel))
    for c in range(case.C):     # one channel's four plants sit at more than one position
        assert len({B.plants(case, q)[c].kind for q in B.QUANTITIES}) == 3


def _strict_max(t, ps, what):
    """the plant of every channel is the strict maximum of |t| over the channel"""
    N, C = t.shape[0], t.shape[1]
    a = t.detach().abs().double().reshape(N, C, -1)
    for p in ps:
        top = a[p.n, p.c, p.voxel].item()
        rest = a[:, p.c].clone()
        rest[p.n, p.voxel] = -1.0
        assert top > rest.max().item(), (what, p, top, rest.max().item())


@pytest.mark.parametrize("cid", IDS)
def test_plants_are_the_strict_channel_maxima(cid):
    case = B.BY_ID[cid]
    d = B.data(case, seeded_tensor)
    v = (1, case.C, 1, 1, 1)
    yd = d["y"].double()
    _strict_max(yd - yd.mean((0, 2, 3, 4)).view(v), B.plants(case, "y"), "|y - mean| (training)")
    _strict_max(yd - d["rm"].double().view(v), B.plants(case, "y"), "|y - running mean| (eval)")
    _strict_max(d["dz"], B.plants(case, "dz"), "|dz|")
    _strict_max(d["rp_big"], B.plants(case, "rp"), "|res_pre|")
    _strict_max(d["rq_big"], B.plants(case, "rq"), "|res_post|")
    # max |g|, g = dz (u > 0 ? 1 : slope): the dz plant sits where u > 0 in every configuration that has a gradient mask
    for training, pre, rp in ((True, False, "rp"), (True, True, "rp"), (True, True, "rp_big"), (False, True, "rp_eval")):
        u = B.preactivation(case, seeded_tensor, training, pre, rp)
        for slope in (0.0, 0.1):
            _strict_max(d["dz"].double() * torch.where(u > 0, 1.0, slope), B.plants(case, "dz"),
                        f"|g| {training} {pre} {rp} {slope}")
    # a planted residual is >= 2^8 times the bound |gamma| sqrt(N S) + |beta| of bn_bound_exp: a reader that misses its slot
    # scales the operand 2^8 too far up, past the f16 range
    bound = B.residual_bound(case, d["gamma"], d["beta"])
    for name, q in (("rp_big", "rp"), ("rq_big", "rq")):
        for p in B.plants(case, q):
            assert abs(d[name][p.n, p.c].view(-1)[p.voxel].item()) >= 2.0 ** 8 * bound[p.c].item()
    # the parameters are in the ranges the issue sets
    assert bool(((d["gamma"] >= 0.5) & (d["gamma"] <= 1.5)).all()) and d["beta"].abs().max() < 1.0


@pytest.mark.parametrize("cid", IDS)
def test_no_preactivation_near_the_kink(cid):
    """the sign of u = BN(y) + res_pre decides the gradient mask; |u| >= MARGIN / 2 everywhere (fp32 rounding of u is ~1e-6),
    in every configuration the GPU test runs"""
    case = B.BY_ID[cid]
    for training, pre, rp in ((True, False, "rp"), (True, True, "rp"), (True, True, "rp_big"), (False, True, "rp_eval")):
        u = B.preactivation(case, seeded_tensor, training, pre, rp)
        assert u.abs().min().item() >= B.MARGIN / 2, (cid, training, pre, rp, u.abs().min().item())


RUNS = [(True,) + c for c in B.COMBOS] + [(False,) + B.EVAL_COMBO]


@pytest.mark.parametrize("cid", IDS)
def test_pytorch_fp32_meets_the_gates(cid, capsys):
    """PyTorch's own fp32 CPU BatchNorm, forward and backward, on the row's data against the fp64 reference: inside every
    gate of test_bn_act.  A row on which fp32 arithmetic itself misses a gate would be a wrong row."""
    case = B.BY_ID[cid]
    worst = {}
    for training, slope, pre, post in RUNS:
        rp = "rp" if training else "rp_eval"
        ref = B.reference(case, seeded_tensor, training, slope, pre, post, torch.float64, rp=rp)
        f32 = B.reference(case, seeded_tensor, training, slope, pre, post, torch.float32, rp=rp)
        assert set(ref) == set(f32)
        for name in ref:
            r = B.gate_ratio(f32[name], ref[name], B.GATES[name])
            worst[name] = max(worst.get(name, 0.0), r)
            assert r <= 1.0, (f"{cid} training={training} slope={slope} pre={pre} post={post} {name}: fp32 / gate = {r:.3f}; "
                              + (B.worst_chunk(f32[name], ref[name], B.geometry(case).plain_len) if ref[name].dim() == 5 else ""))
    with capsys.disabled():
        print(f"\n{cid:16s} PyTorch fp32 / gate: " + "  ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))


def test_expected_exps_agree_with_the_mirror():
    b = torch.tensor([1.0, 1.00001, 1.5, 1.99999, 2.0, 3e5, 7e-4, 0.0], dtype=torch.float64)
    exps, sure = B.expected_exps(b)
    assert sure.tolist() == [False, False, True, False, False, True, True, False]
    for x, e, ok in zip(b.tolist(), exps.tolist(), sure.tolist()):
        if ok:
            assert e == B.x2_scale_exp(torch.tensor(x, dtype=torch.float32).item())
            assert e == B.x2_scale_exp(torch.tensor(x * (1 + 5e-5), dtype=torch.float32).item()) == B.x2_scale_exp(x * (1 - 5e-5))


@pytest.mark.parametrize("cid", [c.id for c in B.CASES if c.pack is not None])
def test_exponent_bounds_depend_on_the_planted_slots(cid):
    """the exponent checks of the GPU test bite: a reader that misses the slot of a plant derives another exponent.
    z: a planted residual is 2^8 times the rest of the bound, so the exponent moves by 8 or 9.  dy, with dz_corr: the bound
    without the y plants of one kind gives another exponent in at least a quarter of that kind's channels."""
    case = B.BY_ID[cid]
    for rp, rq in (("rp_big", None), (None, "rq_big"), ("rp_big", "rq_big")):
        full, sure = B.expected_exps(B.z_bound(case, seeded_tensor, rp, rq))
        none, _ = B.expected_exps(B.z_bound(case, seeded_tensor))
        assert bool(((none - full) >= 8).all()), (cid, rp, rq, (none - full).tolist())
        assert int(sure.sum()) >= case.C * 3 // 4
    full, sure = B.expected_exps(B.dy_bound(case, seeded_tensor, 1.0, "dz_corr"))
    assert int(sure.sum()) >= case.C * 3 // 4
    for kind in ("last", "high"):
        miss, _ = B.expected_exps(B.dy_bound(case, seeded_tensor, 1.0, "dz_corr", without_plant_of={kind}))
        chans = [p.c for p in B.plants(case, "y") if p.kind == kind]
        moved = [c for c in chans if sure[c] and miss[c] != full[c]]
        assert len(moved) * 4 >= len(chans) and moved, (cid, kind, moved, chans)
        others = [c for c in range(case.C) if c not in chans]
        assert all(miss[c] == full[c] for c in others)
    # the bound holds: no |dy| of the fp64 reference is above it
    ref = B.reference(case, seeded_tensor, True, 1.0, False, False, dz="dz_corr")
    assert bool((ref["dy"].abs().amax((0, 2, 3, 4)) <= B.dy_bound(case, seeded_tensor, 1.0, "dz_corr")).all())


def test_worst_chunk_names_the_chunk():
    ref = torch.zeros(2, 3, 1, 1, 2500)
    got = ref.clone()
    got[1, 2, 0, 0, 2100] = 1.0
    msg = B.worst_chunk(got, ref, 1024)
    assert "worst chunk 2 of 3" in msg and "[2048, 2500)" in msg and "clipped" in msg and "sample 1, channel 2" in msg
    got[1, 2, 0, 0, 2100] = float("nan")
    assert "inf" in B.worst_chunk(got, ref, 1024)
    assert B.gate_ratio(got, ref, 1.0) == float("inf")


def test_x2_scale_exp_mirror():
    """141 - biased exponent = 15 - frexp exponent: v * 2^e lands in [2^14, 2^15)"""
    for k in range(-126, 128):
        for v in (2.0 ** k, math.nextafter(2.0 ** k, 0.0), math.nextafter(2.0 ** k, math.inf), 1.5 * 2.0 ** k):
            v = torch.tensor(v, dtype=torch.float32).item()       # the fp32 number the kernel sees
            if not math.isfinite(v):
                continue
            want = max(-100, min(126, 15 - math.frexp(v)[1]))
            assert B.x2_scale_exp(v) == want, (v, k)
            if -100 < want < 126:
                assert 2.0 ** 14 <= v * 2.0 ** want < 2.0 ** 15
    assert B.x2_scale_exp(0.0) == 0
    assert B.x2_scale_exp(2.0 ** -127) == 0 and B.x2_scale_exp(2.0 ** -149) == 0          # denormals: a zero exponent field
    assert B.x2_scale_exp(2.0 ** -126) == 126 and B.x2_scale_exp(2.0 ** -112) == 126       # upper clamp: 15 + 126 = 141 > 126
    assert B.x2_scale_exp(2.0 ** -111) == 125 and B.x2_scale_exp(2.0 ** -110) == 124
    assert B.x2_scale_exp(2.0 ** 114) == -100 and B.x2_scale_exp(2.0 ** 113) == -99        # lower clamp: 15 - 115 = -100
    assert B.x2_scale_exp(3.4e38) == -100 and B.x2_scale_exp(float("inf")) == -100
