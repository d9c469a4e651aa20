"""What tests/test_gpu_volume_fp64.py relies on, checked without a GPU: every row of tests/_volume_cases.py is on the launch
branch it names, every regime the gate promises has a row, the library's `dca_gwc_volume_bwd_rows` (host arithmetic: it runs
without a device) answers what the restated predicate answers, no input exceeds 64 MiB, and the float64 and float32 oracles
agree to fp32 grade with no gradient so small that the relative gate would become an absolute one."""
import math

import pytest
import torch

import _volume_cases as V

ROWS = V.ALL + list(V.ABI_MISALIGNED.values()) + [V.REFUSED]
IDS = [c.id for c in ROWS]
NUMERIC = V.ALL
NUM_IDS = [c.id for c in NUMERIC]


@pytest.mark.parametrize("case", ROWS, ids=IDS)
def test_branch_arithmetic_holds(case):
    assert case.arith() is True, f"{case.id} is not on its branch: {case.branch}"


def test_every_regime_has_a_row():
    have = {r for c in ROWS for r in c.regimes}
    assert not set(V.REQUIRED_REGIMES) - have, sorted(set(V.REQUIRED_REGIMES) - have)
    assert {c.cpg for c in V.GWC} == set(V.CPGS)
    assert {c.cpg for c in V.GWC_BLOCKED} == {2, 4, 8}, "an instantiation of gwc_bwd_blocked_kernel has no row"
    for cpg in (2, 4, 8):
        multi = [c for c in V.GWC_BLOCKED if c.cpg == cpg and max(V.trips(c.shape[3], c.rows)) > 1]
        assert multi, f"no multi-trip row for gwc_bwd_blocked_kernel<{cpg}>"
    assert all(c.rows > 0 for c in V.GWC_BLOCKED) and all(c.rows == 0 for c in V.GWC_BOUNDARY + V.GWC_PLAIN)
    assert {s % 4 for s in (c.shape[4] for c in V.GWC_PLAIN)} == {0, 1, 2, 3}


def test_launcher_constants():
    """the boundary pairs really straddle their limits, and the stride rows exceed their caps by less than one more sweep"""
    assert V.VOL_EW_CAP == 1048576 and V.FUSED_EW_CAP == 2097152 and V.BLOCKED_LDS_MAX == 81920 and V.LDS_REFUSE == 163840
    assert V.blocked_lds(8, 240, 48) == 74752 and V.blocked_lds(8, 236, 52) == 79424 and V.blocked_lds(8, 216, 56) == 79488
    assert V.blocked_lds(8, 192, 64) == 83200 and 52 * 60 == 3120 and 52 * 59 == 3068
    assert V.plain_bwd_lds(16, 208, 48) == 66560 and V.fwd_lds(16, 516) == 66048 and V.fwd_lds(16, 1284) == 164352
    assert V.fused_iq_trips(240, 48) == [3, 3, 3, 3] and V.fused_iq_trips(12, 8) == [1, 1]
    assert V.trips(40, 16) == [3] * 8 + [2] * 8 and sum(V.trips(35, 32)) == 35


def test_restated_predicate_on_the_parity_shapes():
    """the six shapes of test_gpu_parity.py::test_gwc_volume: plain, plain, plain, blocked gx 7, blocked gx 2, plain"""
    assert [V.bwd_rows(*s) for s in V.PARITY_SHAPES] == V.PARITY_ROUTES == [0, 0, 0, 7, 2, 0]


def test_library_query_equals_the_restated_predicate():
    """dca_gwc_volume_bwd_rows on every gwc / fused row, the parity shapes, one step either side of each limit, and what the
    entry refuses"""
    from dcanet_amd import _lib
    lib = _lib.load()
    shapes = [c.shape for c in ROWS if c.family != "concat"] + V.PARITY_SHAPES
    for B, C, G, H, W, D in list(shapes):
        shapes += [(B, C, G, H, W + 4, D), (B, C, G, H, max(4, W - 4), D), (B, C, G, H, W, D + 4), (B, C, G, H, W, max(4, D - 4)),
                   (B, C, G, H + 1, W, D), (2 * B, C, G, H, W, D)]
    shapes += [(1, 24, 8, 2, 16, 24), (1, 8, 0, 2, 16, 48), (1, 9, 2, 2, 16, 48), (0, 8, 1, 2, 16, 48), (1, 8, 1, 65536, 16, 48),
               (1, 8, 1, 2, 16, 0), (1, 8, 1, 4096, 256, 48), (1, 8, 1, 65535, 256, 48)]
    seen = set()
    for B, C, G, H, W, D in shapes:
        want = V.bwd_rows(B, C, G, H, W, D) if G > 0 else -1
        got = lib.dca_gwc_volume_bwd_rows(B, C, H, W, D, G)
        assert (got < 0) == (want < 0) and (want < 0 or got == want), ((B, C, G, H, W, D), got, want)
        seen.add(-1 if want < 0 else (1 if want else 0))
    assert seen == {-1, 0, 1}
    assert V.bwd_rows(1, 8, 1, 65535, 256, 48) == 0      # 48 * 65535 * 256 * 4 bytes: the 31-bit offset term alone


@pytest.mark.parametrize("case", NUMERIC, ids=NUM_IDS)
def test_input_size(case):
    assert max(V.input_sizes(case)) <= V.MAX_INPUT_BYTES


@pytest.mark.parametrize("case", NUMERIC, ids=NUM_IDS)
def test_references_agree_to_fp32_grade(case):
    y = V.yardstick(case)
    ref = V.truth(case)
    want = {"fwd"} | ({"d L", "d R"} if V.has_grads(case) else set()) | ({"concat", "d cl", "d cr"} if case.p.get("Cc") else set())
    assert set(y) == want and set(y) <= set(V.sibling(case)), sorted(y)
    assert all(math.isfinite(v) and 0.0 <= v <= 1e-6 for v in y.values()), y
    exact = [k for k in y if V.sibling(case)[k] == 0.0]
    assert all(y[k] == 0.0 for k in exact), "the concat volume is a copy: float32 and float64 must agree exactly"
    assert all(torch.isfinite(t).all() for t in ref.values())
    # the metric divides by max(1, max |ref|): a gradient whose largest element is below 1 would be gated absolutely, at a
    # bound that an unwritten element can pass (hence `seed_scale`)
    grads = {k: t.abs().max().item() for k, t in ref.items() if k.startswith("d ")}
    assert all(v >= 1.0 for v in grads.values()), grads
    assert ref["fwd"].abs().max() > 0


def test_gate_form():
    assert V.gate(0.0) == 2.0 ** -22 and V.gate(1e-6) == 4e-6 and V.FACTOR == 4.0 and V.MAX_INPUT_BYTES == 64 << 20
