"""What tests/test_gpu_heads_dca_fp64.py relies on, checked without a GPU: every row of tests/_heads_cases.py is on the launch
branch it names, the context cases have the same k* in float32 and float64 and a float64 top-2 probability gap of at least
1e-4 away from their constructed ties, every yardstick is finite and no case needs more than 64 MiB of input."""
import math

import pytest
import torch
import torch.nn.functional as F

import _heads_cases as H

IDS = [c.id for c in H.ALL]
CTX_IDS = [c.id for c in H.CONTEXT]


def test_tables_cover_every_family():
    assert set(H.FAMILIES) == set(H.SIBLING) and all(H.FAMILIES[f] for f in H.FAMILIES)
    assert {c.p["mode"] for c in H.SOFTARGMIN} == {0, 1, 2}
    assert {c.p["scale"] for c in H.UP_SOFTARGMIN} == {2, 3, 4, 8}
    assert {c.p["build"] for c in H.CONTEXT} == {"margin", "tie", "absent"}


@pytest.mark.parametrize("case", H.ALL, ids=IDS)
def test_branch_arithmetic_holds(case):
    assert case.arith() is True, f"{case.id} is not on its branch: {case.branch}"


def test_launcher_constants():
    """the pairs really straddle their thresholds and the stride cases exceed their caps by less than one more sweep"""
    assert H.VOL_EW_CAP == 1048576 and H.EW_CAP == 2097152
    sa = [c for c in H.SOFTARGMIN if "grid-stride" in c.branch]
    assert len(sa) == 3 and all(c.shape[0] * c.shape[2] * c.shape[3] == 1049600 for c in sa)
    nc_d = sorted(c.shape[1] * c.shape[2] for c in H.TRILINEAR if c.p["scale"] == 2)[:2]
    assert nc_d == [H.GRID_YZ, H.GRID_YZ + 1]
    assert sorted(c.shape[1] * ((c.shape[2] + 1) // 2) for c in H.AVGPOOL) == [H.GRID_YZ, H.GRID_YZ + 1]
    assert sorted({c.shape[1] for c in H.FOCAL}) == [H.FL_NT_SWITCH, H.FL_NT_SWITCH + 1, H.FL_KMAX]
    assert {(c.shape[2] + 7) // 8 for c in H.ATTENTION} == {3, 5, 7}


@pytest.mark.parametrize("case", H.ALL, ids=IDS)
def test_input_size(case):
    assert H.input_bytes(case) <= H.MAX_INPUT_BYTES


@pytest.mark.parametrize("case", H.ALL, ids=IDS)
def test_yardstick_is_finite(case):
    y = H.yardstick(case)
    assert set(y) == set(H.SIBLING[case.family][1]), (sorted(y), sorted(H.SIBLING[case.family][1]))
    assert all(math.isfinite(v) and v >= 0.0 for v in y.values()), y
    ref, _ = H.truth(case)
    assert all(torch.isfinite(t).all() for t in ref.values())
    if not (case.family in ("softargmin", "up_softargmin") and case.shape[1] == 1):   # one plane: the gradient is exactly 0
        assert all(t.abs().max() > 0 for t in ref.values()), "a reference that is identically zero checks nothing"
    # the metric divides by max(1, max |ref|): a gradient whose largest element is far below 1 would be gated absolutely, at
    # a bound that garbage in an unwritten element can pass (hence `seed_scale`)
    assert all(t.abs().max() == 0 or t.abs().max() >= 0.1 for t in ref.values()), {k: t.abs().max().item() for k, t in ref.items()}


@pytest.mark.parametrize("case", H.CONTEXT, ids=CTX_IDS)
def test_context_kstar_and_probability_gap(case):
    """k* of the float32 and of the float64 oracle are identical, equal to the lowest index among the maxima, and the
    float64 top-2 gap is at least MIN_GAP wherever no tie was constructed; on a tie pixel the two maxima are exactly equal in
    both precisions, the lower index wins, and the third probability is MIN_GAP away"""
    (t, other), n = H.inputs(case), case.shape[2]
    preds, tie = t["preds"], other["tie"]
    H.yardstick(case)                  # asserts that the float32 oracle's k* equals the float64 oracle's
    _, e64 = H.truth(case)
    for dtype in (torch.float32, torch.float64):
        p = F.softmax(preds.to(dtype), 1)
        assert torch.equal(H.lowest_argmax(p), e64["kstar"])
        top = p.topk(min(3, n), dim=1).values
        gap = top[:, 0] - top[:, 1]
        assert (gap[tie] == 0).all()
        if dtype == torch.float64:
            assert gap[~tie].min().item() >= H.MIN_GAP, gap[~tie].min().item()
            if tie.any():
                assert (top[:, 0] - top[:, 2])[tie].min().item() >= H.MIN_GAP
    build = case.p["build"]
    assert tie.any() == (build == "tie")
    if build == "tie":
        assert 0.4 < tie.float().mean().item() < 0.6
        # the tied partner sits above k* except where the winner was the last plane and its copy went below it
        eq = (preds == preds.amax(1, keepdim=True)).sum(1)
        assert (eq[tie] == 2).all() and (eq[~tie] == 1).all()
        second = torch.where(preds == preds.amax(1, keepdim=True), torch.arange(n).view(1, n, 1, 1), -1).amax(1)
        assert (second[tie] > e64["kstar"][tie]).all()
    if build == "absent":
        k = e64["kstar"]
        assert (k[0] == H.ABSENT_CLASS).sum() == 0 and (k[1] == H.ABSENT_CLASS).sum() > 0
    if case.mag >= 40:
        assert F.softmax(preds.double(), 1).amax(1).median().item() > 0.999, "not saturated"


def test_margin_bound_is_independent_of_the_map_size():
    """the margin bounds the gap by (1 - exp(-MARGIN)) / n whatever HW: the two-megapixel case has no smaller gap than that"""
    for case in H.CONTEXT:
        if case.p["build"] == "tie":
            continue
        p = F.softmax(H.inputs(case)[0]["preds"].double(), 1).topk(2, dim=1).values
        assert (p[:, 0] - p[:, 1]).min().item() >= (1 - math.exp(-H.MARGIN)) / case.shape[2] * 0.999


def test_gate_form():
    assert H.gate(0.0) == 2.0 ** -22 and H.gate(1e-6) == 4e-6 and H.FACTOR == 4.0
