"""The reduced-precision inference hot path (ops.reduced_precision(bf16 | fp16)) restated on the CPU in fp64, stage by
stage, where a stage is one stored tensor of that path.  Shared by tests/test_lp_reference_cpu.py (which proves the wiring
against the oracle, and that the gates below notice a wrong wiring) and tests/test_gpu_lowprec_stages.py (which feeds each
stage the GPU's own input tensors: teacher forcing, so only summation order and the final store differ).

Weights, BatchNorm buffers, slopes and residuals are read from the state dict along the reference model's definition
(oracle/dcanet_oracle.py: hot_path, dres0, dres1, cva, multi_aggregation, classif); nothing is imported from the package.
The closed forms without a rounding point of their own (volume builders, context injection with its attention block,
soft-argmin) are the oracle's functions, run in fp64.

Rounding points (q = round to the 2-byte type, then fp64):
  * every 3x3x3 stride-1 conv + BN rounds its input and its weight and stores in the type of its input;
  * the 1x1x1 convolutions `fuse` and `redir`, the stride-2 `conv1` and the `classif3` logit head read 2-byte tensors and
    round their weight; the transposed `conv3` rounds its fp32 input `c2` and its weight;
  * the logit head of cva.classify and the 1x1x1 projections of slc_net are fp32 kernels: nothing is rounded;
  * epilogue: act(conv * scale + shift + res_pre) + res_post with the eval-BatchNorm affine (eps 1e-5), then the store.
"""
from collections import OrderedDict

import torch
import torch.nn.functional as F

from oracle import dcanet_oracle as O

BLOCKS = ("cva1", "cva2", "cva3")
TOP = ("volume", "dres0.a", "dres0", "dres1.a", "cost0")
CVA = ("pooled", "cost_down", "h", "prob", "aug_down", "aug", "fused", "c1", "c2", "skip", "out")
HEAD = ("classif3.h", "logits3", "pred4_q")
STAGES = TOP + tuple(f"{b}.{s}" for b in BLOCKS for s in CVA) + HEAD
# stored in the 2-byte type; every other stage is fp32
LP_STORED = frozenset(("volume", "dres0.a", "dres0", "dres1.a", "cost0", "classif3.h")
                      + tuple(f"{b}.{s}" for b in BLOCKS for s in ("aug", "fused", "skip", "out")))
# deliberate wiring mistakes (tests/test_lp_reference_cpu.py): name -> the first stage that must miss its gate
MUTATIONS = {
    "fuse_swapped": "cva2.fused",            # cat([x, aug]) instead of cat([aug, x])
    "skip_slope0": "cva2.skip",              # ReLU on the redir branch
    "cva1_no_res_post": "cva1.out",          # out1 without `+ cost0`
    "res_pre_after_act": "cva3.out",         # relu(conv3) + skip instead of relu(conv3 + skip)
    "conv2_affine_of_conv1": "cva1.c2",      # conv2 folded with conv1's BatchNorm
    "dres1_slope0": "cost0",                 # ReLU before `+ cost0`
    "pool_divisor_in_range": "cva1.pooled",  # count_include_pad=False
    "align_corners": "cva3.aug",             # align_corners=True
}


# the stage tests' cases: id -> (1/4-res feature shape, maxdisp, concat volume); 1/8-res interior 4 x 8 x 16 (the shape of
# the hot_path goldens) and 5 x 5 x 12 (odd depth and height, partial tiles; gc: dres0 with 64 input channels)
CASES = {"A-g": ((2, 320, 16, 32), 32, False), "B-g": ((1, 320, 10, 24), 40, False), "B-gc": ((1, 332, 10, 24), 40, True)}
# the record of the chosen seed suffixes: tensors are seeded_tensor(f"lpst.{SEED_TAG[id]}.<name>", shape); a seed at which
# the arg-max margin of tests/test_lp_reference_cpu.py fails is replaced here
SEED_TAG = {"A-g": "a0", "B-g": "b0", "B-gc": "b0"}


def case_inputs(cid):
    """(state dict, fL, fR, cL, cR, maxdisp) of a case; the state dict is the oracle's key-seeded one"""
    from oracle.seeded import seeded_tensor
    shape, maxdisp, concat = CASES[cid]
    sd = O.seeded_state_dict(O.hot_path_shapes(concat))
    fL, fR = (seeded_tensor(f"lpst.{SEED_TAG[cid]}.{n}", shape) for n in ("fL", "fR"))
    if concat:
        return sd, fL[:, :320].contiguous(), fR[:, :320].contiguous(), fL[:, 320:].contiguous(), fR[:, 320:].contiguous(), maxdisp
    return sd, fL, fR, None, None, maxdisp


def ulp(lp):
    """largest relative error of rounding to nearest: half a unit in the last place"""
    return 0.0 if lp is None else 2.0 ** -8 if lp == torch.bfloat16 else 2.0 ** -11


def q(t, lp):
    return t.double() if lp is None else t.to(lp).double()


def kstar(prob):
    """arg-max map of the context injection (oracle.context_inject: softmax over the bins, then argmax)"""
    p = prob.double()
    return F.softmax(p.squeeze(1) if p.dim() == 5 else p, dim=1).argmax(1)


def gate(stage, ref, lp):
    """per-element bound on |gpu - ref| for a stage; scale = max(1, |ref|max).  Sources: module docstring of
    tests/test_gpu_lowprec_stages.py."""
    scale = max(1.0, ref.abs().max().item())
    kind = stage.split(".")[-1]
    if kind == "pooled":
        lim = 1e-6 * scale
    elif kind in ("aug", "volume"):
        lim = 2e-6 * scale
    elif kind == "pred4_q":
        lim = 2e-6 * scale
    else:                                   # convolution stages, and aug_down (fp32)
        lim = 2e-5 * scale
    lim = torch.full_like(ref, lim)
    return lim + ulp(lp) * ref.abs() if stage in LP_STORED else lim


def miss(stage, got, ref, lp):
    """(worst err / gate, flat index of that element)"""
    r = (got.double() - ref).abs() / gate(stage, ref, lp)
    i = int(r.argmax())
    return r.flatten()[i].item(), i


def _affine(sd, bn):
    sc = sd[bn + ".weight"] / torch.sqrt(sd[bn + ".running_var"] + 1e-5)
    return sc.view(1, -1, 1, 1, 1), (sd[bn + ".bias"] - sd[bn + ".running_mean"] * sc.view(-1)).view(1, -1, 1, 1, 1)


def _epilogue(sd, y, bn, slope, res_pre=None, res_post=None, pre_after_act=False):
    sc, sh = _affine(sd, bn)
    y = y * sc + sh
    if res_pre is not None and not pre_after_act:
        y = y + res_pre
    y = torch.where(y > 0, y, y * slope)
    if res_pre is not None and pre_after_act:
        y = y + res_pre
    return y if res_post is None else y + res_post


def hot_path_lp(sd, fL, fR, maxdisp, lp, cL=None, cR=None, forced=None, mutate=()):
    """From the 1/4-res features to `pred4_q`: OrderedDict stage name (STAGES) -> fp64 tensor BEFORE the store, so that a
    2-byte stage (LP_STORED) is gated like the kernel tests gate theirs -- against the unrounded value, with half a unit in
    the last place of slack -- and rounded only when a later stage reads it.  lp=None: no rounding anywhere (the oracle's
    hot path in eval mode).  forced=None: every stage reads this function's own earlier outputs; forced = {stage: tensor}:
    every stage reads its inputs from there.  `mutate`: names of MUTATIONS to apply."""
    sd = {k: v.double() for k, v in sd.items() if v.is_floating_point()}
    unknown = set(mutate) - set(MUTATIONS)
    assert not unknown, unknown
    out = OrderedDict()

    def src(name):
        """a stage as the path stores it: the 2-byte stages rounded (the identity on a tensor that has that type)"""
        v = out[name] if forced is None else forced[name].detach().cpu().double()
        return q(v, lp) if name in LP_STORED else v

    def put(name, v):
        out[name] = v

    def conv3(x, p, slope, res_post=None, bn=None):
        """3x3x3 stride-1 convbn_3d at prefix p (keys p.0.weight, p.1.*): input and weight rounded"""
        y = F.conv3d(q(x, lp), q(sd[p + ".0.weight"], lp), None, 1, 1)
        return _epilogue(sd, y, p + ".1" if bn is None else bn, slope, None, res_post)

    d = maxdisp // 4
    vol = O.build_gwc_volume(fL.double(), fR.double(), d, 40)
    if cL is not None:
        vol = torch.cat((vol, O.build_concat_volume(cL.double(), cR.double(), d)), 1)
    put("volume", vol)
    put("dres0.a", conv3(src("volume"), "dres0.0", 0.0))
    put("dres0", conv3(src("dres0.a"), "dres0.2", 0.0))
    put("dres1.a", conv3(src("dres0"), "dres1.0", 0.0))
    put("cost0", conv3(src("dres1.a"), "dres1.2", 0.0 if "dres1_slope0" in mutate else 1.0, res_post=src("dres0")))

    x_name = "cost0"
    for b in BLOCKS:
        x = src(x_name)
        pool = F.avg_pool3d(x, (3, 3, 3), stride=2, padding=1, count_include_pad="pool_divisor_in_range" not in mutate)
        put(f"{b}.pooled", pool)
        put(f"{b}.cost_down", conv3(src(f"{b}.pooled"), f"{b}.downsample.1", 0.0))
        put(f"{b}.h", conv3(src(f"{b}.cost_down"), f"{b}.classify.0", 0.0))
        put(f"{b}.prob", F.conv3d(src(f"{b}.h"), sd[f"{b}.classify.2.weight"], None, 1, 1))
        put(f"{b}.aug_down", O.semantic_level_context(sd, f"{b}.slc_net", src(f"{b}.cost_down"),
                                                      src(f"{b}.prob").squeeze(1), False))
        put(f"{b}.aug", F.interpolate(src(f"{b}.aug_down"), scale_factor=(2, 2, 2), mode="trilinear",
                                      align_corners=True if "align_corners" in mutate else None))
        pair = [x, src(f"{b}.aug")] if "fuse_swapped" in mutate else [src(f"{b}.aug"), x]
        y = F.conv3d(torch.cat(pair, 1), q(sd[f"{b}.fuse.0.0.weight"], lp))
        put(f"{b}.fused", _epilogue(sd, y, f"{b}.fuse.0.1", 1.0))
        a = f"{b}.cost_agg"
        fused = src(f"{b}.fused")
        y = F.conv3d(fused, q(sd[a + ".conv1.0.0.weight"], lp), None, 2, 1)
        put(f"{b}.c1", _epilogue(sd, y, a + ".conv1.0.1", 0.0))
        put(f"{b}.c2", conv3(src(f"{b}.c1"), a + ".conv2.0", 0.0,
                             bn=a + ".conv1.0.1" if "conv2_affine_of_conv1" in mutate else None))
        y = F.conv3d(fused, q(sd[a + ".redir.0.weight"], lp))
        put(f"{b}.skip", _epilogue(sd, y, a + ".redir.1", 0.0 if "skip_slope0" in mutate else 1.0))
        y = F.conv_transpose3d(q(src(f"{b}.c2"), lp), q(sd[a + ".conv3.0.weight"], lp), None, 2, 1, 1)
        res_post = src("cost0") if b == "cva1" and "cva1_no_res_post" not in mutate else None    # cost0 + augmented_cost
        put(f"{b}.out", _epilogue(sd, y, a + ".conv3.1", 0.0, src(f"{b}.skip"), res_post, "res_pre_after_act" in mutate))
        x_name = f"{b}.out"

    put("classif3.h", conv3(src("cva3.out"), "classif3.0", 0.0))
    put("logits3", F.conv3d(src("classif3.h"), q(sd["classif3.2.weight"], lp), None, 1, 1))
    put("pred4_q", O.disparity_regression(F.softmax(src("logits3").squeeze(1), dim=1), d))
    assert tuple(out) == STAGES
    return out
