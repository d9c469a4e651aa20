"""What the picture stage costs on one MI355X.

  (O) the launches alone at the KITTI frame (375x1242 inside 384x1248), all buffers passed in: `ops.disp_error_image` (uint8
      out; and float32 + uint8), `ops.disp_range`, `ops.disp_colorize` (KITTI map, device range).  Device events around
      `--iters` back-to-back calls, after a warm-up, `--reps` windows; us per call, median (min..max).  Twice: issued from
      Python (the wrapper's host time bounds the rate) and replayed from a hipGraph that holds the `--iters` calls.
  (H) the host path they replace, for one frame: device -> host copies of the two float32 maps (prediction, ground truth) with
      their synchronisation, then the numpy restatement of the error map (`dcanet_amd.utils.disp_error_image_func` on CPU
      tensors, the reference's ten-pass loop); the same for the colour map (one map, `disp_to_color`).  Wall clock, ms.
  (P) / (C) frames, with `--frames N` > 0: `KittiInference` against `KittiInferenceColor` on KITTI-size uint8 pairs, D = 192,
      seeded GwcNet-G, fp16, hot path from a hipGraph, device I/O, per-call use: wall time around N frames, synchronised at
      both ends, the two arms alternating; ms per frame, median (min..max).

    python tools/bench_visualize.py [--iters 200] [--reps 7] [--frames 20]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

H, W, HC, WC = 375, 1242, 384, 1248


def fmt(v, unit):
    return f"{statistics.median(v):.3f} {unit} median ({min(v):.3f}..{max(v):.3f})"


def scene():
    g = torch.Generator().manual_seed(0)
    gt = torch.rand((1, H, W), generator=g) * 180 + 2
    gt[torch.rand((1, H, W), generator=g) < 0.3] = 0.0                         # KITTI ground truth is sparse
    pred = torch.zeros((1, HC, WC))
    pred[:, HC - H:, :W] = (gt + torch.randn((1, H, W), generator=g) * 2).clamp_min(0.1)
    return pred, gt


def operators(a):
    from dcanet_amd import ops
    pred, gt = (t.cuda() for t in scene())
    window = (HC - H, H, W)
    out_u8 = torch.empty((1, H, W, 3), device="cuda", dtype=torch.uint8)
    out_f32 = torch.empty((1, 3, H, W), device="cuda")
    rgb = torch.empty((H, W, 3), device="cuda", dtype=torch.uint8)
    rng = ops.disp_range(pred, window)
    arms = {
        "error_image_u8": lambda: ops.disp_error_image(pred, gt, f32=False, u8=True, out_u8=out_u8),
        "error_image_f32_u8": lambda: ops.disp_error_image(pred, gt, u8=True, out_f32=out_f32, out_u8=out_u8),
        "range": lambda: ops.disp_range(pred, window),
        "colorize_kitti": lambda: ops.disp_colorize(pred, *window, range=rng, out=rgb),
        "colorize_gray_fixed": lambda: ops.disp_colorize(pred, *window, max_disp=192.0, cmap="gray", out=rgb),
    }
    for run in arms.values():
        for _ in range(a.warmup):
            run()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    for k, run in list(arms.items()):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            for _ in range(a.iters):
                run()
        graph.replay()
        arms[k + "_graph"] = graph
    res = {k: [] for k in arms}
    for _ in range(a.reps):
        for k, run in arms.items():
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            start.record()
            if k.endswith("_graph"):
                run.replay()
            else:
                for _ in range(a.iters):
                    run()
            stop.record()
            stop.synchronize()
            res[k].append(start.elapsed_time(stop) * 1e3 / a.iters)
    for k, v in res.items():
        print(f"(O) {k}: {fmt(v, 'us per call')} over {a.reps} x {a.iters} calls, {H}x{W} in {HC}x{WC}")
    return res


def host_path(a):
    from dcanet_amd.utils import disp_error_image_func, disp_to_color
    pred, gt = (t.cuda() for t in scene())
    res = {"copy_two_maps_ms": [], "error_image_numpy_ms": [], "copy_one_map_ms": [], "disp_to_color_numpy_ms": []}
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        p, g = pred[:, HC - H:, :W].cpu(), gt.cpu()                            # .cpu() synchronises
        t1 = time.perf_counter()
        disp_error_image_func.forward(None, p, g)
        t2 = time.perf_counter()
        p = pred[0, HC - H:, :W].cpu()
        t3 = time.perf_counter()
        disp_to_color(p, 192.0)
        t4 = time.perf_counter()
        for k, v in zip(res, (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
            res[k].append(v * 1e3)
    for k, v in res.items():
        print(f"(H) {k}: {fmt(v, 'ms')} over {a.reps} frames")
    return res


def frames(a):
    from bench_frame_io import pairs, timed
    from dcanet_amd.inference import KittiInference, KittiInferenceColor
    from dcanet_amd.models.gwcnet_dca_g import GwcNet
    from oracle import dcanet_oracle as O
    net = GwcNet(192, use_concat_volume=False)
    net.load_state_dict(O.seeded_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}), strict=True)
    net = net.cuda().eval()
    data = pairs(4)
    P = KittiInference(net, graph=True, dtype=torch.float16, device_io=True)
    C = KittiInferenceColor(net, graph=True, dtype=torch.float16)
    A = KittiInferenceColor(net, graph=True, dtype=torch.float16, max_disp="auto")
    arms = {"P": lambda ps: [P(l, r) for l, r in ps], "C": lambda ps: [C(l, r) for l, r in ps],
            "C_auto": lambda ps: [A(l, r) for l, r in ps]}
    for run in arms.values():
        run([data[i % len(data)] for i in range(6)])
    t = {k: [] for k in arms}
    for _ in range(a.reps):
        for k, run in arms.items():
            t[k].append(timed(run, data, a.frames))
    for k, v in t.items():
        print(f"({k}) {fmt(v, 'ms/frame')} over {a.reps} x {a.frames} frames")
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--frames", type=int, default=0, help="> 0: also time whole frames of KittiInference / KittiInferenceColor")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    import dcanet_amd  # noqa: F401
    res = {"operators_us": operators(a), "host_ms": host_path(a)}
    if a.frames > 0:
        res["frames_ms"] = frames(a)
    print("RESULT " + json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
