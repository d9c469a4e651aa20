"""tests/_lp_reference.py without a GPU: the restatement's wiring against the oracle, forced mode against free-running
mode, the teeth of the stage gates, and the arg-max margin of the seeds the GPU stage tests run on.

Seed tags (tests/_lp_reference.py SEED_TAG): A-g "a0", B-g "b0", B-gc "b0" -- features
seeded_tensor("lpst.<tag>.fL" / ".fR"); weights and BatchNorm buffers are the oracle's key-seeded state dict.  All three
pass the margin check below for lp in (None, bf16, fp16)."""
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle import dcanet_oracle as O
from _lp_reference import CASES, LP_STORED, MUTATIONS, STAGES, case_inputs, gate, hot_path_lp, kstar, miss, q

LPS = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]


@functools.lru_cache(maxsize=None)
def free(cid, lp):
    sd, fL, fR, cL, cR, maxdisp = case_inputs(cid)
    with torch.no_grad():
        return hot_path_lp(sd, fL, fR, maxdisp, lp, cL, cR)


@functools.lru_cache(maxsize=None)
def mutated(cid, lp):
    """every mutation at once, forced from the unmutated free-running outputs: under forcing each stage reads the same
    inputs as the unmutated one, so the mutations do not interact"""
    sd, fL, fR, cL, cR, maxdisp = case_inputs(cid)
    with torch.no_grad():
        return hot_path_lp(sd, fL, fR, maxdisp, lp, cL, cR, forced=free(cid, lp), mutate=tuple(MUTATIONS))


@pytest.mark.parametrize("cid", list(CASES))
def test_restatement_without_rounding_is_the_oracle_hot_path(cid):
    sd, fL, fR, cL, cR, maxdisp = case_inputs(cid)
    dbl = lambda t: None if t is None else t.double()
    with torch.no_grad():
        ref = O.hot_path(O.clone_sd(sd, torch.float64), fL.double(), fR.double(), maxdisp, False, 40, dbl(cL), dbl(cR))
    got = free(cid, None)
    pairs = [("pred4_q", "pred4_q"), ("cost0", "cost0")]
    pairs += [(f"prob_volume{i}", f"cva{i}.prob") for i in (1, 2, 3)] + [(f"out{i}", f"cva{i}.out") for i in (1, 2, 3)]
    for okey, stage in pairs:
        r, g = ref[okey], got[stage]
        assert r.shape == g.shape and g.dtype == torch.float64, (okey, r.shape, g.shape)
        err = (g - r).abs().max().item()
        assert err <= 1e-10 * max(1.0, r.abs().max().item()), f"{stage} vs oracle {okey}: {err:.3e}"
    assert ref["pred4_q"].std() > 0.1, "degenerate case: flat disparity map"


@pytest.mark.parametrize("lp", LPS, ids=IDS)
@pytest.mark.parametrize("cid", list(CASES))
def test_forced_from_own_outputs_equals_free_running(cid, lp):
    sd, fL, fR, cL, cR, maxdisp = case_inputs(cid)
    ref = free(cid, lp)
    with torch.no_grad():
        got = hot_path_lp(sd, fL, fR, maxdisp, lp, cL, cR, forced=ref)
    assert tuple(got) == STAGES
    for s in STAGES:
        assert torch.equal(got[s], ref[s]), s
    # forced from the stored form (what a GPU run hands over: the 2-byte stages rounded) gives the same again
    stored = {s: q(v, lp) if s in LP_STORED else v for s, v in ref.items()}
    with torch.no_grad():
        got = hot_path_lp(sd, fL, fR, maxdisp, lp, cL, cR, forced=stored)
    for s in STAGES:
        assert torch.equal(got[s], ref[s]), s
    # and the rounding is not a no-op: the path differs from the unrounded one
    assert not torch.equal(ref["pred4_q"], free(cid, None)["pred4_q"])


@pytest.mark.parametrize("lp", LPS, ids=IDS)
@pytest.mark.parametrize("name", list(MUTATIONS))
@pytest.mark.parametrize("cid", list(CASES))
def test_gates_have_teeth(cid, name, lp):
    """each wiring mistake, on the same forced inputs, misses the stage's gate by at least a factor of 10"""
    ref, mut = free(cid, lp), mutated(cid, lp)
    stage = MUTATIONS[name]
    worst, _ = miss(stage, mut[stage], ref[stage], lp)
    assert worst >= 10.0, f"{name}: {stage} misses its gate by {worst:.2f}x only"


@pytest.mark.parametrize("lp", LPS, ids=IDS)
@pytest.mark.parametrize("cid", list(CASES))
def test_forcing_keeps_a_mistake_local(cid, lp):
    """why one forced run can carry all mutations: a stage of a kind that no mutation touches is bitwise unchanged"""
    ref, mut = free(cid, lp), mutated(cid, lp)
    kinds = {s.split(".")[-1] for s in MUTATIONS.values()}
    assert kinds == {"fused", "skip", "out", "c2", "cost0", "pooled", "aug"}
    for s in STAGES:
        if s.split(".")[-1] not in kinds:
            assert torch.equal(mut[s], ref[s]), s


@pytest.mark.parametrize("lp", [None] + LPS, ids=["fp64"] + IDS)
@pytest.mark.parametrize("cid", list(CASES))
def test_argmax_margin_of_the_chosen_seeds(cid, lp):
    """the context injection takes an arg-max over softmax(prob): the top-two gap must exceed 1e-6 at every pixel of all
    three blocks, or an fp32 kernel may legitimately pick the other bin; a seed that fails is replaced"""
    r = free(cid, lp)
    for b in ("cva1", "cva2", "cva3"):
        p = F.softmax(r[f"{b}.prob"].squeeze(1), dim=1)
        top = p.topk(2, dim=1).values
        gap = (top[:, 0] - top[:, 1]).min().item()
        assert gap > 1e-6, f"{cid} {b}: top-two gap {gap:.3e}"
        assert torch.equal(kstar(r[f"{b}.prob"]), p.argmax(1))


def test_gate_is_per_element_for_two_byte_stages_only():
    ref = torch.tensor([0.0, 4.0, -100.0], dtype=torch.float64)
    assert torch.equal(gate("cva1.c2", ref, torch.float16), torch.full_like(ref, 2e-5 * 100))
    assert torch.allclose(gate("cva1.out", ref, torch.bfloat16), 2e-5 * 100 + 2.0 ** -8 * ref.abs(), rtol=0, atol=1e-15)
    assert torch.allclose(gate("cva2.aug", ref, torch.float16), 2e-6 * 100 + 2.0 ** -11 * ref.abs(), rtol=0, atol=1e-15)
    assert torch.equal(gate("cva3.pooled", ref, torch.float16), torch.full_like(ref, 1e-6 * 100))
