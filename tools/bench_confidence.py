"""What the confidence map costs per frame on one MI355X: KITTI-size uint8 pairs (375x1242 in the
384x1248 frame), D = 192, seeded GwcNet-G, fp16, hot path replayed from a hipGraph, device I/O:

  (P) `KittiInference(model, dtype=fp16, device_io=True)(l, r)`                 -> disp
  (C) `KittiInferenceWithConfidence(model, dtype=fp16, device_io=True)(l, r)`   -> (disp, conf)

Wall time around each loop of `--frames` frames, device-synchronised at both ends, after a warm-up; the two arms
alternate for `--reps` repetitions; median and min..max in ms per frame.  After the timing the disparities of the two
arms are compared bit for bit (with deterministic MIOpen convolutions in the 2D networks, which are slow: not timed).

    python tools/bench_confidence.py [--frames 20] [--reps 7]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_confidence.py --only c --reps 1
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--only", choices=["p", "c"], default=None, help="one arm alone (for a kernel trace)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    import dcanet_amd  # noqa: F401
    from bench_frame_io import pairs, timed
    from dcanet_amd.inference import KittiInference, KittiInferenceWithConfidence
    from dcanet_amd.models.gwcnet_dca_g import GwcNet
    from oracle import dcanet_oracle as O
    net = GwcNet(192, use_concat_volume=False)
    net.load_state_dict(O.seeded_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}), strict=True)
    net = net.cuda().eval()
    data = pairs(4)
    P = KittiInference(net, graph=True, dtype=torch.float16, device_io=True)
    C = KittiInferenceWithConfidence(net, graph=True, dtype=torch.float16, device_io=True)
    arms = {"P": lambda ps: [P(l, r) for l, r in ps], "C": lambda ps: [C(l, r) for l, r in ps]}
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
    if "P" in t and "C" in t:
        d = statistics.median(t["C"]) - statistics.median(t["P"])
        print(f"(C) - (P) = {d * 1e3:.0f} us/frame = {100 * d / statistics.median(t['P']):.2f} % of the frame; spread of (P) "
              f"{(max(t['P']) - min(t['P'])) * 1e3:.0f} us")
    print("RESULT " + json.dumps(t))
    if not a.only:
        torch.backends.cudnn.deterministic = True   # the 2D networks' MIOpen convolutions, for the bitwise comparison
        dp, (dc, conf) = P(*data[0]), C(*data[0])
        print(f"disparity bitwise equal: {dp.tobytes() == dc.tobytes()}; confidence in [{conf.min():.4f}, {conf.max():.4f}], "
              f"mean {conf.mean():.4f}", flush=True)


if __name__ == "__main__":
    main()
