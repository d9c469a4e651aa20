"""What the stixel stage costs on one MI355X.

  (O) the operator at the KITTI frame: the 375 x 1242 window of the 384 x 1248 frame, width 5 (248 columns of 375 cells),
      max_disp 192, on the synthetic road of tools/bench_ground.py (a plane at 1.65 m, three cars, 0.3 px noise, sky without a
      measurement) under the record `ops.ground_plane` fits to it; device-event time around `--iters` calls with every buffer
      passed in (nothing allocated), eager launches and hipGraph replays alternating for `--reps` repetitions; median
      (min..max) in us, for `ops.stixels` with all outputs and with the list alone (count, stixels, energy through the
      workspace).  The results are compared with the numpy restatement before anything is timed.
  (F) frames, with `--frames N` > 0: `KittiInferenceStixels` against `KittiInferenceGround` on the same KITTI-size uint8 pairs
      in one process, seeded GwcNet-G, D = 192, hipGraph hot path, fp32; wall time around N frames, device-synchronised, arms
      alternating; median (min..max) in ms per frame.

    python tools/bench_stixel.py [--iters 200] [--reps 7] [--frames 20]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_stixel.py --iters 20 --reps 1
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
from bench_ground import H, HBM_BYTES_PER_US, HC, NB, W, WC, event_time, fmt, scene  # noqa: E402

WIDTH = 5


def operators(a, calib):
    from dcanet_amd import ground as G, ops, stixel as S
    frame = scene(calib)
    window = (HC - H, H, W)
    static = torch.from_numpy(frame).cuda()
    plane = ops.ground_plane(static, NB, calib, window=window)["plane"]
    CS = W // WIDTH
    kinds = S._STIXEL_KINDS
    shapes = {"cells": (H, CS, 2), "seg_class": (H, CS), "seg_disp": (H, CS), "count": (CS,), "stixels": (CS, S.STIXEL_MAX_SEGMENTS, 4),
              "energy": (CS,)}
    out = {k: torch.empty(shapes[k], device="cuda", dtype=kinds[k]) for k in kinds}
    ws = ops.stixel_workspace(H, W, "cuda", WIDTH, 1)
    listed = ("count", "stixels", "energy")
    calls = {"stixels (all)": lambda: ops.stixels(static, plane, NB, width=WIDTH, window=window, out=out),
             "stixels (list)": lambda: ops.stixels(static, plane, NB, width=WIDTH, window=window, outputs=listed,
                                                   out={k: out[k] for k in listed}, workspace=ws)}
    # the window read once, the cells written and read once (4 B each), then what is asked for
    n, cells = H * W, H * CS
    traffic = {"stixels (all)": 4 * n + 2 * 4 * cells + 5 * cells + CS * (12 + 16 * S.STIXEL_MAX_SEGMENTS),
               "stixels (list)": 4 * n + 2 * 4 * cells + CS * (12 + 16 * S.STIXEL_MAX_SEGMENTS)}
    for run in calls.values():
        run()
    torch.cuda.synchronize()
    rec = plane.cpu().numpy()
    ref = S.stixels_host(frame, rec, NB, width=WIDTH, window=window)
    for k, v in ref.items():
        assert out[k].cpu().numpy().tobytes() == v.tobytes(), k
    assert ws.cpu().numpy().tobytes() == ref["cells"].tobytes()
    m = S.stixels_metric(ref["stixels"], ref["count"], rec, calib, WIDTH)
    near = m["Z"] < 40.0
    note = (f"plane status {int(rec[5])}; {CS} columns x {H} cells; segments per column {ref['count'].min()}..{ref['count'].max()} "
            f"(mean {ref['count'].mean():.2f}), {int((ref['stixels'][..., 2] == 1).sum())} object stixels, {int(near.sum())} nearer than "
            f"40 m with Z {m['Z'][near].min():.1f}..{m['Z'][near].max():.1f} m; cells by class "
            f"{np.bincount(ref['seg_class'].ravel(), minlength=3)[:3].tolist()}; dependent steps of the dynamic programme per column: {H}")
    res = {}
    for op, run in calls.items():
        for _ in range(a.warmup):
            run()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=torch.cuda.Stream()):
            run()
        for _ in range(a.warmup):
            graph.replay()
        t = {"eager": [], "graph": []}
        for _ in range(a.reps):
            for k, f in (("eager", run), ("graph", graph.replay)):
                t[k].append(event_time(f, a.iters))
        res[op] = t
        for k, v in t.items():
            print(f"(O) {op:14s} {k:5s}: {fmt(v, 'us')} over {a.reps} x {a.iters} calls; compulsory traffic "
                  f"{traffic[op] / 1e6:.2f} MB = {traffic[op] / HBM_BYTES_PER_US:.2f} us at 8 TB/s", flush=True)
    print("(O) " + note, flush=True)
    return res


def frames(a, calib):
    from bench_frame_io import pairs, timed
    from dcanet_amd.inference import KittiInferenceGround, KittiInferenceStixels
    from dcanet_amd.models.gwcnet_dca_g import GwcNet
    from oracle import dcanet_oracle as O
    net = GwcNet(NB, use_concat_volume=False)
    net.load_state_dict(O.seeded_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}), strict=True)
    net = net.cuda().eval()
    data = pairs(4)
    kw = dict(graph=True, device_io=True)
    nets = {"KittiInferenceGround": KittiInferenceGround(net, calib, **kw), "KittiInferenceStixels": KittiInferenceStixels(net, calib, **kw)}
    arms = {k: (lambda ps, f=f: [f(l, r) for l, r in ps]) for k, f in nets.items()}
    for run in arms.values():
        run([data[i % len(data)] for i in range(a.warmup_frames)])
    t = {k: [] for k in arms}
    for _ in range(a.reps):
        for k, run in arms.items():
            t[k].append(timed(run, data, a.frames))
    for k, v in t.items():
        print(f"(F) fp32 {k}: {fmt(v, 'ms/frame')} = {1e3 / statistics.median(v):.1f} frames/s over {a.reps} x {a.frames} frames",
              flush=True)
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--frames", type=int, default=0, help="> 0: also time whole frames of KittiInferenceStixels and KittiInferenceGround")
    ap.add_argument("--warmup-frames", type=int, default=6)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    import dcanet_amd  # noqa: F401
    from dcanet_amd.geometry import StereoCalib
    calib = StereoCalib(721.5377, 0.5327, 609.5593, 172.854)
    res = {"operators_us": operators(a, calib)}
    if a.frames > 0:
        res["frames_ms"] = frames(a, calib)
    print("RESULT " + json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
