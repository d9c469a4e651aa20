"""What the self-supervised loss costs on one MI355X, forward + backward, two disparity maps:

  (F) `ops.selfsup_loss` (csrc/selfsup.hip: three launches)
  (T) the same loss written in torch operations on the device (tests/_selfsup_reference.py, float32: gather,
      avg_pool2d, element-wise passes, autograd)

at 4 x 544 x 960 and 4 x 256 x 512.  Wall time around `--iters` iterations, device-synchronised at both ends, after a
warm-up; the two arms alternate for `--reps` repetitions; medians and min..max in us per iteration.  The minimum traffic is
computed from the shapes: per map the forward and the backward together must read I and R (3 planes each), d and valid,
and write the gradient: 8 planes read, 1 written, 4 bytes per element.  bytes/s = that over the median time of (F).

With `--step`: the whole model at 4 x 3 x 256 x 512, D = 192, seeded weights -- `TrainStep` (supervised: focal loss +
smooth L1) against `SelfSupStep(mask=None)` and `SelfSupStep(mask="lr")`, alternating, ms per step.

    python tools/bench_selfsup.py [--iters 50] [--reps 7] [--step]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_selfsup.py --only f --reps 1 --iters N
        (launches per iteration = the difference of the dispatch counts of two such runs over the difference of N)
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = ((4, 544, 960), (4, 256, 512))
LEVELS, WEIGHTS = 2, (1.8, 2.1)


def inputs(shape, seed=0):
    """seeded device tensors: two images, LEVELS disparity maps in [0, W/4) and a float mask that keeps four pixels in five"""
    B, H, W = shape
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *s: torch.rand(*s, device="cuda", generator=g)
    left, right = 2 * r(B, 3, H, W) - 1, 2 * r(B, 3, H, W) - 1
    disps = [(W / 4) * r(B, H, W) for _ in range(LEVELS)]
    valid = (r(B, H, W) < 0.8).float()
    return left, right, disps, valid


def min_bytes(shape):
    B, H, W = shape
    return LEVELS * 9 * B * H * W * 4


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / iters


def loss_arms(shape):
    import _selfsup_reference as S
    from dcanet_amd import ops
    left, right, disps, valid = inputs(shape)
    disps = [d.requires_grad_() for d in disps]

    def fused():
        loss, _ = ops.selfsup_loss(left, right, disps, WEIGHTS, valid)
        return torch.autograd.grad(loss, disps)

    def composed():
        loss, _ = S.selfsup_reference(left, right, disps, WEIGHTS, valid, dtype=torch.float32)
        return torch.autograd.grad(loss, disps)

    return {"F": fused, "T": composed}


def step_arms():
    import dcanet_amd  # noqa: F401
    from dcanet_amd.models.gwcnet_dca_g import GwcNet
    from dcanet_amd.training import SelfSupStep, TrainStep
    from oracle import dcanet_oracle as O
    B, H, W = SHAPES[1]
    left, right, disps, _ = inputs(SHAPES[1])
    gt = disps[0].clamp(1.0, 191.0)
    arms = {}
    for name in ("S", "U", "L"):
        net = GwcNet(192, use_concat_volume=False)
        net.load_state_dict(O.seeded_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}), strict=True)
        net = net.cuda().train()
        opt = torch.optim.SGD(net.parameters(), lr=1e-6)
        if name == "S":
            ts = TrainStep(net, opt)
            arms[name] = lambda ts=ts: ts.step(left, right, gt)
        else:
            ss = SelfSupStep(net, opt, mask="lr" if name == "L" else None)
            arms[name] = lambda ss=ss: ss.step(left, right)
    return arms


def run(arms, warmup, reps, iters, only=None):
    if only:
        arms = {only: arms[only]}
    for fn in arms.values():
        for _ in range(warmup):
            fn()
    t = {k: [] for k in arms}
    for _ in range(reps):
        for k, fn in arms.items():
            t[k].append(timed(fn, iters))
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=["f", "t"], default=None, help="one arm alone (for a kernel trace)")
    ap.add_argument("--shape", type=int, default=None, help="index into SHAPES (default: both)")
    ap.add_argument("--step", action="store_true", help="also the whole-model steps")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    result = {}
    for shape in SHAPES if a.shape is None else (SHAPES[a.shape],):
        t = run(loss_arms(shape), a.warmup, a.reps, a.iters, a.only.upper() if a.only else None)
        name = "x".join(map(str, shape))
        for k, v in t.items():
            print(f"{name} ({k}) {statistics.median(v):.1f} us median ({min(v):.1f}..{max(v):.1f}) over {a.reps} x {a.iters}")
        if "F" in t:
            f = statistics.median(t["F"])
            print(f"{name} minimum traffic {min_bytes(shape) / 1e6:.1f} MB -> (F) moves {min_bytes(shape) / f / 1e6:.3f} TB/s of it")
        if "F" in t and "T" in t:
            print(f"{name} (T) / (F) = {statistics.median(t['T']) / statistics.median(t['F']):.2f}")
        result[name] = t
    if a.step:
        t = run(step_arms(), 3, max(3, a.reps // 2), 5)
        for k, label in (("S", "TrainStep"), ("U", "SelfSupStep(mask=None)"), ("L", 'SelfSupStep(mask="lr")')):
            print(f"step ({k}) {label}: {statistics.median(t[k]) / 1e3:.2f} ms median ({min(t[k]) / 1e3:.2f}..{max(t[k]) / 1e3:.2f})")
        result["step"] = t
    print("RESULT " + json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
