"""Whole-frame inference time on one MI355X: KITTI-size uint8 pairs (375x1242 -> 384x1248 frame), D = 192, seeded GwcNet-G,
hot path replayed from a hipGraph, fp32 and fp16:

  (A) `KittiInference(model)(l, r)`: numpy normalisation and padding, pageable fp32 upload, blocking read-back, host crop;
  (B) `KittiInference(model, device_io=True)(l, r)`: uint8 upload, the frame_io kernels, pinned read-back, per call;
  (C) `KittiInference(model, device_io=True).stream(pairs, depth=2)`: (B) with the copies of neighbouring frames overlapped.

Wall time around each loop of `--frames` frames, device-synchronised at both ends, after a warm-up; the arms alternate for
`--reps` repetitions; median and min..max in ms per frame.  Also the host-side split of (A): normalise, pad, upload.

    python tools/bench_frame_io.py [--frames 20] [--reps 5] [--out FILE.md]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_frame_io.py --only-b --configs fp32 --reps 1
    python tools/bench_frame_io.py --kernel-trace DIR/.../..._kernel_trace.csv          # per-frame device time table
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAME_KERNELS = ("frame_hist_kernel", "frame_lut_kernel", "frame_apply_kernel", "disp_export_kernel")


def pairs(n, h=375, w=1242, seed=0):
    """smooth synthetic scenes with sensor-like noise (what a histogram of a camera image looks like: a few crowded bins)"""
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w]
    out = []
    for i in range(n):
        base = np.stack([120 + 90 * np.sin(x / (37.0 + i) + c) * np.cos(y / 23.0 - c) for c in range(3)], -1)
        left = np.clip(base + rs.normal(0, 6, base.shape), 0, 255).astype(np.uint8)
        right = np.clip(np.roll(base, -7, 1) + rs.normal(0, 6, base.shape), 0, 255).astype(np.uint8)
        out.append((left, right))
    return out


def timed(run, data, frames_n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run([data[i % len(data)] for i in range(frames_n)])
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / frames_n


def host_split(data, reps=5):
    """ms per pair of the three host terms of (A), best and mean of `reps`"""
    from dcanet_amd.inference import normalize_pair, pad_or_crop
    res = {}
    left, right = data[0]
    norm = normalize_pair(left, right)
    fl, fr, _, _ = pad_or_crop(norm)

    def upload():
        a, b = fl.cuda(), fr.cuda()
        torch.cuda.synchronize()
        return a, b

    for name, fn in (("normalize_pair", lambda: normalize_pair(left, right)), ("pad_or_crop", lambda: pad_or_crop(norm)),
                     ("upload of the two fp32 frames (pageable)", upload)):
        fn()
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        res[name] = (min(ts), statistics.mean(ts))
    return res


def kernel_table(path, skip):
    """per-frame device time of the frame_io kernels from a rocprofv3 kernel trace of an --only-b run, over the frames after
    the first `skip` ones; a frame ends with its disp_export_kernel"""
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    ends = [i for i, r in enumerate(rows) if "disp_export_kernel" in r["Kernel_Name"]]
    assert len(ends) > skip, "fewer frames in the trace than --skip-frames"
    win, nframes = rows[ends[skip - 1] + 1:ends[-1] + 1], len(ends) - skip
    dur = lambda r: int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
    total = sum(dur(r) for r in win)
    lines = [f"| kernel ({nframes} frames) | calls / frame | us / frame |", "|---|---|---|"]
    mine, calls = 0.0, 0
    for name in FRAME_KERNELS:
        hit = [r for r in win if name in r["Kernel_Name"]]
        ns = sum(dur(r) for r in hit)
        mine, calls = mine + ns, calls + len(hit)
        lines.append(f"| {name} | {len(hit) / nframes:.2f} | {ns / nframes / 1e3:.1f} |")
    lines.append(f"| frame_io kernels together | | {mine / nframes / 1e3:.1f} |")
    lines.append(f"| every other kernel (2D networks, hot path, up-sampler) | {(len(win) - calls) / nframes:.0f} | "
                 f"{(total - mine) / nframes / 1e3:.1f} |")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--configs", default="fp32,fp16")
    ap.add_argument("--only-b", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-trace", default=None, help="a rocprofv3 *_kernel_trace.csv of an --only-b run: print the table")
    ap.add_argument("--skip-frames", type=int, default=4)
    a = ap.parse_args()
    if a.kernel_trace:
        print(kernel_table(a.kernel_trace, a.skip_frames))
        return
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    import dcanet_amd  # noqa: F401
    from dcanet_amd.inference import KittiInference
    from dcanet_amd.models.gwcnet_dca_g import GwcNet
    from oracle import dcanet_oracle as O
    net = GwcNet(192, use_concat_volume=False)
    net.load_state_dict(O.seeded_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}), strict=True)
    net = net.cuda().eval()
    data = pairs(4)
    out = []
    if not a.only_b:
        out += ["Host terms of (A), ms per pair (best / mean of 5):", "", "| step | best | mean |", "|---|---|---|"]
        for name, (best, mean) in host_split(data).items():
            out.append(f"| {name} | {best:.2f} | {mean:.2f} |")
        out.append("")
        print("\n".join(out), flush=True)
    head = ["| precision | (A) host I/O, ms/frame median (min..max) | (B) device I/O per call | (C) stream(depth=2) | A / B | B / C |",
            "|---|---|---|---|---|---|"]
    lines, results = [], {}
    for cfg in a.configs.split(","):
        dtype = torch.float16 if cfg == "fp16" else None
        A = KittiInference(net, graph=True, dtype=dtype)
        B = KittiInference(net, graph=True, dtype=dtype, device_io=True)
        arms = {"B": lambda ps: [B(l, r) for l, r in ps]}
        if not a.only_b:
            arms = {"A": lambda ps: [A(l, r) for l, r in ps], **arms, "C": lambda ps: list(B.stream(ps, depth=2))}
        for run in arms.values():
            run([data[i % len(data)] for i in range(a.warmup)])
        if not a.only_b:        # the outputs of (A) and (B) on one pair, next to (A) against itself
            da, da2, db = A(*data[0]), A(*data[0]), B(*data[0])
            print(f"  check {cfg}: max |B - A| = {np.abs(da - db).max():.3e}, max |A - A again| = {np.abs(da - da2).max():.3e}",
                  flush=True)
        t = {k: [] for k in arms}
        for _ in range(a.reps):
            for k, run in arms.items():
                t[k].append(timed(run, data, a.frames))
        results[cfg] = t
        fmt = lambda v: f"{statistics.median(v):.2f} ({min(v):.2f}..{max(v):.2f})" if v else "-"
        med = lambda k: statistics.median(t[k])
        lines.append(f"| {cfg} | {fmt(t.get('A'))} | {fmt(t['B'])} | {fmt(t.get('C'))} | "
                     + (f"{med('A') / med('B'):.2f} | {med('B') / med('C'):.2f} |" if "A" in t else "- | - |"))
        print(lines[-1], flush=True)
        if "A" in t:
            print(f"  {cfg}: slowest (B) {max(t['B']):.2f} ms < fastest (A) {min(t['A']):.2f} ms: {max(t['B']) < min(t['A'])}; "
                  f"median (C) <= median (B): {med('C') <= med('B')}", flush=True)
    out += head + lines
    table = "\n".join(out)
    print(table)
    print("RESULT " + json.dumps(results))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
