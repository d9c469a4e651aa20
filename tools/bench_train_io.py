"""Whole training-step time on one MI355X with the input side included: 375x1242 uint8 pairs with a uint16 disparity (the
KITTI size), crop 256x512, D = 192, seeded GwcNet-G, Adam; batch 4 and batch 12:

  (A) the host path -- `TrainInput(device_io=False)` in this process (no worker pool), `.cuda()` of the fp32 crops -- plus
      the reference-shaped loop: boolean-indexed EPE, `loss.item()` and `epe.item()` every step (main_dca.py:122-141);
  (B) `TrainInput(device_io=True)` + `TrainStep`: uint8 upload through pinned memory, the train_io kernels, no
      synchronisation before the end of the loop.

Wall time around each loop of `--steps` steps, device-synchronised at both ends, after a warm-up; the arms alternate for
`--reps` repetitions; median and min..max in ms per step.  Also the host milliseconds per sample of (A)'s input side.
The reference hides part of (A)'s input side behind DataLoader workers; this measurement does not.

    python tools/bench_train_io.py [--batches 4,12] [--steps 4] [--reps 5] [--out FILE.md]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_train_io.py --only-b --batches 4 --reps 1
    python tools/bench_train_io.py --kernel-trace DIR/.../..._kernel_trace.csv          # per-sample device time table
"""
import argparse
import csv
import json
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TRAIN_KERNELS = ("train_luma_sum_kernel", "train_tables_kernel", "train_patch_sum_kernel", "train_patch_final_kernel",
                 "train_crop_norm_kernel", "train_disp_crop_kernel")
CROP, MAXDISP = (256, 512), 192


def samples(n, h=375, w=1242, seed=0):
    """smooth synthetic scenes with sensor-like noise, a sparse KITTI-like uint16 disparity, and the loader's draws"""
    from dcanet_amd.training import draw_kitti
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w]
    out = []
    for i in range(n):
        base = np.stack([120 + 90 * np.sin(x / (37.0 + i) + c) * np.cos(y / 23.0 - c) for c in range(3)], -1)
        left = np.clip(base + rs.normal(0, 6, base.shape), 0, 255).astype(np.uint8)
        right = np.clip(np.roll(base, -7, 1) + rs.normal(0, 6, base.shape), 0, 255).astype(np.uint8)
        disp = (rs.rand(h, w) * 150 * 256).astype(np.uint16)
        disp[rs.rand(h, w) < 0.7] = 0
        out.append((left, right, disp, draw_kitti(w, h, CROP, np.random.RandomState(seed + i), random.Random(seed + i))))
    return out


def kernel_table(path):
    """device time of the train_io kernels per sample, from a rocprofv3 kernel trace of an --only-b run; a sample ends with
    its train_disp_crop_kernel"""
    rows = list(csv.DictReader(open(path)))
    n = sum("train_disp_crop_kernel" in r["Kernel_Name"] for r in rows)
    assert n, "no train_io kernels in the trace"
    dur = lambda r: int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
    lines, total = [f"| kernel ({n} samples) | calls / sample | us / sample |", "|---|---|---|"], 0.0
    for name in TRAIN_KERNELS:
        hit = [r for r in rows if name in r["Kernel_Name"]]
        ns = sum(dur(r) for r in hit)
        total += ns
        lines.append(f"| {name} | {len(hit) / n:.2f} | {ns / n / 1e3:.1f} |")
    lines.append(f"| train_io kernels together | | {total / n / 1e3:.1f} |")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="4,12")
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only-b", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-trace", default=None, help="a rocprofv3 *_kernel_trace.csv of an --only-b run: print the table")
    a = ap.parse_args()
    if a.kernel_trace:
        print(kernel_table(a.kernel_trace))
        return
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    import dcanet_amd  # noqa: F401
    from dcanet_amd.models.gwcnet_dca_g import GwcNet
    from dcanet_amd.models.loss import focal_loss, model_loss
    from dcanet_amd.training import TrainInput, TrainStep
    from oracle import dcanet_oracle as O
    data = samples(12)
    out, lines, results = [], [], {}
    for B in (int(b) for b in a.batches.split(",")):
        net = GwcNet(MAXDISP, use_concat_volume=False)
        net.load_state_dict(O.seeded_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}), strict=True)
        net = net.cuda().train()
        opt = torch.optim.Adam(net.parameters(), lr=1e-3, betas=(0.9, 0.999))
        host_in = TrainInput(B, CROP, MAXDISP, "kitti")
        dev_in = TrainInput(B, CROP, MAXDISP, "kitti", device_io=True, depth=2)
        ts = TrainStep(net, opt, MAXDISP)
        host_ms = []

        def fill(ti, k):
            for b in range(B):
                ti.load(b, *data[(k * B + b) % len(data)])
            return ti.batch()

        def arm_a(steps):
            for k in range(steps):
                t0 = time.perf_counter()
                imgL, imgR, disp_true, _ = fill(host_in, k)
                host_ms.append((time.perf_counter() - t0) * 1e3 / B)
                net.train()
                imgL, imgR, disp_true = imgL.cuda(), imgR.cuda(), disp_true.cuda().unsqueeze(1)
                mask = ((disp_true < MAXDISP) & (disp_true > 0)).byte().bool()
                mask.detach_()
                opt.zero_grad()
                cls_outputs, disp_outputs = net(imgL, imgR)
                loss = focal_loss(cls_outputs, disp_true, MAXDISP, 5.0, False) + model_loss(disp_outputs, disp_true, mask)
                epe = torch.mean(torch.abs(disp_outputs[-1][mask] - disp_true[mask]))
                loss.backward()
                opt.step()
                loss.item(), epe.item()

        def arm_b(steps):
            for k in range(steps):
                ts.step(*fill(dev_in, k))

        arms = {"B": arm_b} if a.only_b else {"A": arm_a, "B": arm_b}
        for run in arms.values():
            run(a.warmup)
        host_ms.clear()
        t = {k: [] for k in arms}
        for _ in range(a.reps):
            for k, run in arms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(a.steps)
                torch.cuda.synchronize()
                t[k].append((time.perf_counter() - t0) * 1e3 / a.steps)
        results[B] = t
        fmt = lambda v: f"{statistics.median(v):.1f} ({min(v):.1f}..{max(v):.1f})" if v else "-"
        host = f"{statistics.median(host_ms):.2f} ({min(host_ms):.2f}..{max(host_ms):.2f})" if host_ms else "-"
        ahead = "-" if "A" not in t else ("yes" if max(t["B"]) < min(t["A"]) else "no")
        lines.append(f"| {B} | {fmt(t.get('A'))} | {fmt(t['B'])} | {host} | {ahead} |")
        print(lines[-1], flush=True)
        del net, opt, ts, host_in, dev_in
        torch.cuda.empty_cache()
    out += ["| batch | (A) host input + reference loop, ms/step median (min..max) | (B) TrainInput(device_io) + TrainStep | "
            "(A)'s input side on the host, ms/sample | slowest (B) < fastest (A) |", "|---|---|---|---|---|"] + lines
    table = "\n".join(out)
    print(table)
    print("RESULT " + json.dumps(results))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
