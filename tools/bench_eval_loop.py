"""Evaluation-loop throughput on one MI355X: N frames at 540x960, D = 192, batch 1 of

  (A) the forward plus the reference-style metric tail written with torch / numpy on the package's pre-existing surface
      (boolean indexing, `.item()`, `.cpu().numpy()`, `np.bincount`: main_dca.py:176-232 as a user has to write it
      without the evaluation ops; `forward` hands out only `prob_volume2`, so that one volume is scored three times and
      both sides do the same amount of work);
  (B) `dcanet_amd.evaluation.EvalStep.step` (three HIP launches behind the forward, no host synchronisation per frame);

for fp32 / fp16, hot path eager / replayed from a hipGraph.  Wall time around the whole loop, device-synchronised at
both ends, after a warm-up; (A) and (B) alternate for `--reps` repetitions; median and min..max are reported.

    python tools/bench_eval_loop.py [--frames 20] [--reps 5] [--out profiles/eval_step.md]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_eval_loop.py --only-b --configs fp32-eager --reps 1
    python tools/bench_eval_loop.py --kernel-trace DIR/.../..._kernel_trace.csv        # per-frame device time table
"""
import argparse
import contextlib
import csv
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

METRIC_KERNELS = ("disp_metrics_partial_kernel", "disp_metrics_final_kernel", "region_confusion_kernel",
                  "eval_accumulate_kernel")


class TorchTail:
    """(A): what a user of the package had to write before the evaluation ops existed"""

    def __init__(self, net, maxdisp, graph, dtype):
        from dcanet_amd.graph import GraphedHotPath
        self.net, self.maxdisp, self.graph, self.dtype, self.graphed = net, maxdisp, graph, dtype, None
        self.GraphedHotPath = GraphedHotPath
        self.totals = np.zeros(10)
        self.n = 0

    @torch.no_grad()
    def step(self, imgL, imgR, disp_true):
        from dcanet_amd import ops
        from dcanet_amd.evaluation import SegmentationMetric, pad16
        net = self.net
        mask = (disp_true > 0) & (disp_true < self.maxdisp)
        left, right, top_pad, _ = pad16(imgL, imgR)
        fl, fr = net.feature_extraction(left), net.feature_extraction(right)
        guidance = net.guidance(left)["g"]
        args = [fl["gwc_segments"], fr["gwc_segments"]]
        with ops.reduced_precision(self.dtype) if self.dtype is not None else contextlib.nullcontext():
            if self.graph:
                if self.graphed is None:
                    self.graphed = self.GraphedHotPath(net, *args)
                r = self.graphed(*args)
            else:
                r = net.hot_path(*args)
        pred = net.prop(guidance, r["pred4_q"]).squeeze(1)[:, top_pad:, :]
        volume = r["prob_volume2"].squeeze(1)
        self.n += 1
        if len(disp_true[mask]) == 0:
            return
        loss = F.smooth_l1_loss(pred[mask], disp_true[mask])
        epe = (pred - disp_true).abs().view(-1)[mask.view(-1)]
        vals = [loss.item(), epe.mean().item(), (epe > 1).float().mean().item(), (epe > 3).float().mean().item()]
        H, W = disp_true.shape[1:]
        label = F.adaptive_avg_pool2d(disp_true / 8, (H // 8, W // 8)).floor().cpu().numpy().astype("int64")
        off = volume.shape[2] - H // 8
        metric, mpa, miou = SegmentationMetric(volume.shape[1]), [], []
        for _ in range(3):
            metric.addBatch(volume.argmax(1)[:, off:, :W // 8].cpu().numpy(), label)
            mpa.append(metric.meanPixelAccuracy())
            miou.append(metric.meanIntersectionOverUnion())
        self.totals += np.asarray(vals + mpa + miou)


def frames(n, seed=0):
    from make_eval_golden import synthetic_batch
    g = torch.Generator().manual_seed(seed)
    out = []
    for i in range(n):
        gt = torch.from_numpy(synthetic_batch(seed + i, 1, 540, 960)[0]).cuda()
        out.append((torch.randn(1, 3, 540, 960, generator=g).cuda(), torch.randn(1, 3, 540, 960, generator=g).cuda(), gt))
    return out


def timed(step, data, frames_n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(frames_n):
        step(*data[i % len(data)])
    torch.cuda.synchronize()
    return frames_n / (time.perf_counter() - t0)


def kernel_table(path, skip):
    """per-frame device time from a rocprofv3 kernel trace, over the frames AFTER the first `skip` ones (their launches hold
    MIOpen's solver search and code-object loading): a frame ends with its eval_accumulate_kernel"""
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    ends = [i for i, r in enumerate(rows) if "eval_accumulate_kernel" in r["Kernel_Name"]]
    assert len(ends) > skip, "fewer frames in the trace than --skip-frames"
    win, nframes = rows[ends[skip - 1] + 1:ends[-1] + 1], len(ends) - skip
    dur = lambda r: int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
    total = sum(dur(r) for r in win)
    lines = [f"| kernel ({nframes} frames) | calls / frame | us / frame |", "|---|---|---|"]
    metric, calls = 0.0, 0
    for name in METRIC_KERNELS:
        hit = [r for r in win if name in r["Kernel_Name"]]
        ns = sum(dur(r) for r in hit)
        metric, calls = metric + ns, calls + len(hit)
        lines.append(f"| {name} | {len(hit) / nframes:.2f} | {ns / nframes / 1e3:.1f} |")
    lines.append(f"| metric kernels together | | {metric / nframes / 1e3:.1f} |")
    lines.append(f"| every other kernel (forward: 2D networks, hot path, up-sampler) | {(len(win) - calls) / nframes:.0f} | {(total - metric) / nframes / 1e3:.1f} |")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--configs", default="fp32-eager,fp32-graph,fp16-eager,fp16-graph")
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
    from dcanet_amd.evaluation import EvalStep
    from dcanet_amd.models.gwcnet_dca_g import GwcNet
    from oracle import dcanet_oracle as O
    net = GwcNet(192, use_concat_volume=False)        # seeded weights and BatchNorm statistics: finite in fp16 too
    net.load_state_dict(O.seeded_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}), strict=True)
    net = net.cuda().eval()
    data = frames(4)
    lines = ["| configuration | (A) torch/numpy tail, frames/s median (min..max) | (B) EvalStep, frames/s median (min..max) | B / A |",
             "|---|---|---|---|"]
    results = {}
    for cfg in a.configs.split(","):
        dtype = torch.float16 if cfg.startswith("fp16") else None
        graph = cfg.endswith("graph")
        A, B = TorchTail(net, 192, graph, dtype), EvalStep(net, 192, graph=graph, dtype=dtype)
        for _ in range(a.warmup):
            for d in data:
                if not a.only_b:
                    A.step(*d)
                B.step(*d)
        B.reset()
        fa, fb = [], []
        for _ in range(a.reps):
            if not a.only_b:
                fa.append(timed(A.step, data, a.frames))
            fb.append(timed(B.step, data, a.frames))
        res = B.result()
        results[cfg] = {"A": fa, "B": fb, "frames_B": res["batches"]}
        fmt = lambda v: f"{statistics.median(v):.1f} ({min(v):.1f}..{max(v):.1f})" if v else "-"
        ratio = f"{statistics.median(fb) / statistics.median(fa):.2f}" if fa else "-"
        lines.append(f"| {cfg} | {fmt(fa)} | {fmt(fb)} | {ratio} |")
        print(lines[-1], flush=True)
        if fa:      # both sides scored the same frames: the values agree (A scores prob_volume2 three times, B the three heads)
            print(f"  check: epe A {A.totals[1] / max(A.n, 1):.6f}  B {res['epe']:.6f}", flush=True)
    table = "\n".join(lines)
    print(table)
    print("RESULT " + json.dumps(results))
    if a.out:
        with open(a.out, "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
