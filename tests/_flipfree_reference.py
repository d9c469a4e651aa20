"""Flip-free train-step references: the margin tracer behind tests/test_gpu_flipfree_gradients.py, its CPU condition
(tests/test_flipfree_reference_cpu.py) and the seed search (tools/flipfree_seed_search.py).  CPU only.

A train step of `GwcNet.hot_path` is discontinuous in the sign of every (leaky-)ReLU input (40 activation sites) and in the
arg-max of the three context injections.  On an input whose fp64 reference keeps every such decision far from its
boundary -- far measured in units of the fp32 oracle's own error at the same site -- the step is locally smooth, two
fp32-grade implementations take the same branch everywhere, and every gradient tensor can be held to the fp32-grade
yardstick of tests/test_gpu_unaligned.py (`check_yardstick`).

The oracle is traced from outside: `torch.nn.functional.relu` / `leaky_relu` are wrapped while `oracle.dcanet_oracle.hot_path`
runs (the oracle calls them through the module attribute), so what the oracle computes does not change.

A case = (shape (B, H4, W4, maxdisp), concat, seed suffix); every tensor is `seeded_tensor(f"ff.<suffix>.<name>", shape)`.
It is FLIP-FREE when
  * at every activation site   min |u64|  >=  M x max |u32 - u64|          (u = the activation's input, whole site)
  * at every arg-max site      smallest top-two gap of the softmaxed predictions in fp64  >=  M x 2 max |p32 - p64|
  * the `reference_stability` conditions of tests/test_gpu_unaligned.py hold: fp32 oracle within a quarter of each forward
    gate of the fp64 oracle, identical arg-max maps k*, train step and eval forward.
M = 8: the margin is measured against the fp32 oracle's error; the f16x2 kernels are granted a factor 4 ("two bits") over fp32
arithmetic by the project's yardstick, and that is doubled because the site maximum of one implementation's error bounds
another's only roughly.  A seed that misses M is replaced, or the shape shrunk -- never M."""
import functools

import torch
import torch.nn.functional as F

from oracle import dcanet_oracle as O
from oracle.seeded import seeded_tensor
from test_gpu_unaligned import HEADS, EVAL_OUT, head_tol, split, _kstar

M = 8.0
SHAPES = {            # id: (B, H4, W4, maxdisp); each under ~1.2e5 activation inputs -- above that no seed reaches M
    "b1w8": (1, 4, 8, 16),        # B = 1, aligned: eighth-res 2 x 2 x 4, width still a multiple of 4        59 392 inputs
    "b2w8": (2, 4, 8, 16),        # B = 2, aligned: batch statistics and BatchNorm-backward sums cross samples 118 784
    "b1w10": (1, 4, 10, 16),      # W4 % 4 == 2: the fallback side of every width predicate (eighth-res width 5) 74 240
    "b1w16": (1, 4, 16, 16),      # two quads per row at eighth res                                          118 784
}
SITES = 40           # activation calls of one train-mode hot_path (dres0 2, dres1 1, 3 x cva 11, 4 x classif 1)


class ActivationTrace:
    """records the input of every F.relu / F.leaky_relu call made while active (in call order)"""

    def __enter__(self):
        self.inputs = []
        self._saved = (F.relu, F.leaky_relu)

        def wrap(fn):
            def traced(x, *a, **k):
                self.inputs.append(x.detach())
                return fn(x, *a, **k)
            return traced
        F.relu, F.leaky_relu = wrap(F.relu), wrap(F.leaky_relu)
        return self

    def __exit__(self, *exc):
        F.relu, F.leaky_relu = self._saved
        return False


def tag_of(suffix):
    return f"ff.{suffix}"


def features(shape, concat, suffix):
    B, h, w, _ = shape
    C = 320 + (12 if concat else 0)
    return seeded_tensor(f"{tag_of(suffix)}.fL", (B, C, h, w)), seeded_tensor(f"{tag_of(suffix)}.fR", (B, C, h, w))


def seeded_loss(r, suffix, dtype=torch.float32):
    """the seven-head seeded loss of test_gpu_unaligned.seeded_loss under this module's seed tags"""
    loss = 0
    for i, k in enumerate(HEADS):
        g = seeded_tensor(f"{tag_of(suffix)}.g{i}", r[k].shape).to(dtype)
        loss = loss + (r[k] * g.to(r[k].device)).sum()
    return loss


@functools.lru_cache(maxsize=None)
def _weights(concat, dtype):
    return O.clone_sd(O.seeded_state_dict(O.hot_path_shapes(concat)), dtype)


def _hot(sd, a, b, shape, concat, training):
    args = split(a, b, concat)
    return O.hot_path(sd, args[0], args[1], shape[3], training, 40, *(args[2:] if concat else (None, None)))


def _probs(r):
    """the softmaxed predictions the three context injections take their arg-max of"""
    return [F.softmax(r[f"prob_volume{i}"].detach().squeeze(1), dim=1) for i in (1, 2, 3)]


def traced_forward(shape, concat, suffix, dtype):
    """train-mode forward only (no gradients): activation inputs and arg-max predictions; what the seed search runs first"""
    sd = O.clone_sd(_weights(concat, dtype))
    fL, fR = features(shape, concat, suffix)
    with torch.no_grad(), ActivationTrace() as tr:
        r = _hot(sd, fL.to(dtype), fR.to(dtype), shape, concat, True)
    return dict(act=tr.inputs, probs=_probs(r))


@functools.lru_cache(maxsize=None)
def oracle_train(shape, concat, suffix, dtype):
    """one train-mode step of the CPU oracle in `dtype`: heads, gradients of both feature maps and of every parameter
    tensor, running statistics after the step, k* maps, and the trace (activation inputs, arg-max predictions)"""
    sd = O.clone_sd(_weights(concat, dtype))
    names = [k for k, v in sd.items() if v.is_floating_point() and "running" not in k]
    for k in names:
        sd[k].requires_grad_()
    fL, fR = features(shape, concat, suffix)
    a, b = fL.to(dtype).requires_grad_(), fR.to(dtype).requires_grad_()
    with ActivationTrace() as tr:
        r = _hot(sd, a, b, shape, concat, True)
    grads = torch.autograd.grad(seeded_loss(r, suffix, dtype), [a, b] + [sd[k] for k in names])
    return dict(heads={k: r[k].detach() for k in HEADS}, names=["fL", "fR"] + names, grads=[g.detach() for g in grads],
                stats={k: v.detach() for k, v in sd.items() if "running" in k}, kstar=_kstar(r), act=tr.inputs,
                probs=_probs(r))


@functools.lru_cache(maxsize=None)
def oracle_eval(shape, concat, suffix, dtype):
    sd = O.clone_sd(_weights(concat, dtype))
    fL, fR = features(shape, concat, suffix)
    with torch.no_grad():
        r = _hot(sd, fL.to(dtype), fR.to(dtype), shape, concat, False)
    return dict(out={k: r[k] for k in EVAL_OUT}, kstar=_kstar(r))


def reference_stability(shape, concat, suffix):
    """test_gpu_unaligned.reference_stability for a case of this module: the list of violations"""
    bad, what = [], f"{shape} {'gc' if concat else 'g'} {suffix}"
    for mode, fn, field in (("train", oracle_train, "heads"), ("eval", oracle_eval, "out")):
        r64, r32 = fn(shape, concat, suffix, torch.float64), fn(shape, concat, suffix, torch.float32)
        for k, ref in r64[field].items():
            err = (r32[field][k].double() - ref).abs().max().item()
            tol = head_tol(k, ref) / 4
            if not err <= tol:
                bad.append(f"{what} {mode} {k}: |o32 - o64| = {err:.3e} > {tol:.1e}")
        for i, (k64, k32) in enumerate(zip(r64["kstar"], r32["kstar"])):
            if not torch.equal(k64, k32):
                bad.append(f"{what} {mode} k* of cva{i + 1}: {(k64 != k32).sum().item()} pixels differ")
    return bad


def margins(t64, t32):
    """per decision site of one traced train-mode step, fp64 trace against fp32 trace:
    act:    [(min |u64|, max |u32 - u64|, rms u64, elements)]        one row per activation site
    argmax: [(smallest top-two gap of p64, max |p32 - p64|)]         one row per context injection"""
    assert len(t64["act"]) == len(t32["act"]) == SITES, (len(t64["act"]), len(t32["act"]))
    act = []
    for u64, u32 in zip(t64["act"], t32["act"]):
        assert u64.dtype == torch.float64 and u32.dtype == torch.float32 and u64.shape == u32.shape
        act.append((u64.abs().min().item(), (u32.double() - u64).abs().max().item(), u64.square().mean().sqrt().item(),
                    u64.numel()))
    argmax = []
    for p64, p32 in zip(t64["probs"], t32["probs"]):
        top = p64.topk(2, dim=1).values
        argmax.append(((top[:, 0] - top[:, 1]).min().item(), (p32.double() - p64).abs().max().item()))
    return dict(act=act, argmax=argmax)


def achieved_margin(m):
    """(smallest min |u64| / max |u32 - u64| over the activation sites, smallest gap / (2 max |p32 - p64|) over the arg-max
    sites): the case is flip-free in the sense of the first two conditions when both are >= M"""
    ratio = lambda a, b: a / b if b > 0 else float("inf")
    return min(ratio(lo, err) for lo, err, _, _ in m["act"]), min(ratio(gap, 2 * err) for gap, err in m["argmax"])


def flip_free_violations(shape, concat, suffix):
    """every violated condition of the module docstring for this case (empty list: the case is flip-free)"""
    r64, r32 = (oracle_train(shape, concat, suffix, d) for d in (torch.float64, torch.float32))
    m = margins(r64, r32)
    what = f"{shape} {'gc' if concat else 'g'} {suffix}"
    bad = [f"{what} activation site {i}: min |u64| = {lo:.3e} < {M:g} x max |u32 - u64| = {M * err:.3e}"
           for i, (lo, err, _, _) in enumerate(m["act"]) if not lo >= M * err]
    bad += [f"{what} arg-max of cva{i + 1}: top-two gap {gap:.3e} < {M:g} x 2 max |p32 - p64| = {2 * M * err:.3e}"
            for i, (gap, err) in enumerate(m["argmax"]) if not gap >= M * 2 * err]
    return bad + reference_stability(shape, concat, suffix)


def activation_inputs(shape, concat, suffix):
    return sum(n for _, _, _, n in margins(*(oracle_train(shape, concat, suffix, d)
                                             for d in (torch.float64, torch.float32)))["act"])
