"""What the left-right check costs per frame on one MI355X: KITTI-size uint8 pairs (375x1242 in the
384x1248 frame), D = 192, seeded GwcNet-G, fp16, hot path replayed from a hipGraph, device I/O:

  (P) `KittiInference(model, dtype=fp16, device_io=True)(l, r)`       -> disp
  (L) `KittiInferenceLR(model, dtype=fp16, device_io=True)(l, r)`     -> (disp_filled, valid)

Wall time around each loop of `--frames` frames, device-synchronised at both ends, after a warm-up; the two arms
alternate for `--reps` repetitions; median and min..max in ms per frame.  (L) is two full passes of the network (the
frames, then the mirrored, swapped frames) plus two small launches, so about twice (P) is expected.  After the timing the
share of valid pixels is printed (seeded weights: the number says nothing about accuracy).

    python tools/bench_lr.py [--frames 20] [--reps 7]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_lr.py --only l --reps 1
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--tau", type=float, default=1.0)
    ap.add_argument("--only", choices=["p", "l"], default=None, help="one arm alone (for a kernel trace)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    import dcanet_amd  # noqa: F401
    from bench_frame_io import pairs, timed
    from dcanet_amd.inference import KittiInference, KittiInferenceLR
    from dcanet_amd.models.gwcnet_dca_g import GwcNet
    from oracle import dcanet_oracle as O
    net = GwcNet(192, use_concat_volume=False)
    net.load_state_dict(O.seeded_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}), strict=True)
    net = net.cuda().eval()
    data = pairs(4)
    P = KittiInference(net, graph=True, dtype=torch.float16, device_io=True)
    L = KittiInferenceLR(net, graph=True, dtype=torch.float16, device_io=True, tau=a.tau)
    arms = {"P": lambda ps: [P(l, r) for l, r in ps], "L": lambda ps: [L(l, r) for l, r in ps]}
    if a.only:
        arms = {a.only.upper(): arms[a.only.upper()]}
    for run in arms.values():
        run([data[i % len(data)] for i in range(a.warmup)])
    t = {k: [] for k in arms}
    for _ in range(a.reps):
        for k, run in arms.items():
            t[k].append(timed(run, data, a.frames))
    for k, v in t.items():
        print(f"({k}) {statistics.median(v):.3f} ms/frame median ({min(v):.3f}..{max(v):.3f}) over {a.reps} x {a.frames} frames")
    if "P" in t and "L" in t:
        p, l = statistics.median(t["P"]), statistics.median(t["L"])
        print(f"(L) / (P) = {l / p:.3f}; (L) - 2 (P) = {(l - 2 * p) * 1e3:.0f} us/frame; spread of (P) "
              f"{(max(t['P']) - min(t['P'])) * 1e3:.0f} us")
    print("RESULT " + json.dumps(t))
    if not a.only:
        _, valid = L(*data[0])
        print(f"valid: {100 * valid.mean():.2f} % of the pixels", flush=True)


if __name__ == "__main__":
    main()
