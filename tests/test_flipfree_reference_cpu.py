"""CPU-only condition behind tests/test_gpu_flipfree_gradients.py: every committed (shape, variant, seed) is flip-free.

For each case the fp64 and fp32 oracles are traced through one train-mode step (tests/_flipfree_reference.py): at every
activation site min |u64| >= 8 x max |u32 - u64|, at every arg-max site the top-two gap >= 8 x 2 max |p32 - p64|, and the
`reference_stability` conditions of tests/test_gpu_unaligned.py hold.  The reference alone must also meet the skip cap of the
gradient gate: at most 5 % of the gradient tensors with a norm below 1e-6.  A seed that fails is replaced
(tools/flipfree_seed_search.py prints the next one), never the condition."""
import pytest
import torch
import torch.nn.functional as F

import _flipfree_reference as R
from test_gpu_flipfree_gradients import ALIGNED, SEEDS


@pytest.mark.parametrize("case", list(SEEDS), ids=lambda c: f"{c[0]}-{c[1]}")
def test_committed_seeds_are_flip_free(case):
    sid, variant = case
    shape, concat, suffix = R.SHAPES[sid], variant == "gc", SEEDS[case]
    bad = R.flip_free_violations(shape, concat, suffix)
    assert not bad, bad
    r = R.oracle_train(shape, concat, suffix, torch.float64)
    B, h, w, D = shape
    assert r["heads"]["pred4_q"].shape == (B, 1, h, w) and r["heads"]["pred_dca3"].shape == (B, 1, 4 * h, 4 * w)
    assert all(torch.isfinite(g).all() for g in r["grads"]) and len(r["grads"]) == len(r["names"]) >= 150
    tiny = [n for n, g in zip(r["names"], r["grads"]) if g.norm().item() < 1e-6]
    assert len(tiny) <= 0.05 * len(r["grads"]), tiny
    assert R.activation_inputs(shape, concat, suffix) <= 1.2e5
    assert h % 2 == 0 and w % 2 == 0 and (w % 8 == 0) == (sid in ALIGNED) and (sid in ALIGNED or w % 4 == 2)


def test_the_required_shape_classes_are_present():
    shapes = {R.SHAPES[sid] for sid, _ in SEEDS}
    assert any(s[0] == 1 and s[2] % 8 == 0 for s in shapes) and any(s[0] == 2 and s[2] % 8 == 0 for s in shapes)
    assert any(s[2] % 4 == 2 for s in shapes)
    assert all((sid, v) in SEEDS for sid in R.SHAPES for v in ("g", "gc"))


def test_the_tracer_sees_every_activation_and_leaves_the_oracle_alone():
    """40 activation sites per train-mode hot_path, the traced step bit-identical to the untraced one, and
    torch.nn.functional restored afterwards"""
    from oracle import dcanet_oracle as O
    shape, suffix = R.SHAPES["b1w8"], "s0"
    relu, lrelu = F.relu, F.leaky_relu
    t = R.traced_forward(shape, False, suffix, torch.float32)
    assert F.relu is relu and F.leaky_relu is lrelu
    assert len(t["act"]) == R.SITES and sum(u.numel() for u in t["act"]) == 59392
    sd = O.clone_sd(O.seeded_state_dict(O.hot_path_shapes(False)))
    fL, fR = R.features(shape, False, suffix)
    with torch.no_grad():
        plain = O.hot_path(sd, fL, fR, shape[3], True)
    for got, ref in zip(t["probs"], R._probs(plain)):
        assert torch.equal(got, ref)
    m = R.margins(R.traced_forward(shape, False, suffix, torch.float64), t)
    assert all(lo >= 0 and err > 0 and rms > 0 for lo, err, rms, _ in m["act"]) and len(m["argmax"]) == 3


def test_a_near_zero_activation_input_is_reported():
    """the margin rule itself: a site whose smallest |u64| is within M x the fp32 error is a violation"""
    u64 = torch.tensor([1.0, -2.0, 3e-6], dtype=torch.float64)
    sites = lambda v, dt: [v.to(dt)] + [torch.ones(3, dtype=dt)] * (R.SITES - 1)
    p = torch.tensor([[[[0.7]], [[0.2]], [[0.1]]]], dtype=torch.float64)
    t64 = dict(act=sites(u64, torch.float64), probs=[p] * 3)
    t32 = dict(act=sites(u64 + 1e-6, torch.float32), probs=[(p + 1e-7).float()] * 3)
    a, k = R.achieved_margin(R.margins(t64, t32))
    assert 2.5 < a < 3.5 and a < R.M and k > R.M
