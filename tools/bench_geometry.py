"""What the geometry stage costs on one MI355X.

  (O) the two operators alone: `ops.disp_to_depth` (fp32 out) + `ops.point_cloud` (with colours) on a 384x1248 frame in
      which EVERY pixel is kept (the most records the emit kernel can write), all buffers passed in.  Device events around
      `--iters` back-to-back pairs, after a warm-up, `--reps` windows; us per pair, median (min..max).  Twice: launched
      eagerly (four launches per pair from Python) and replayed from a hipGraph that holds one pair.
  (P) / (G) frames, with `--frames N` > 0: `KittiInference` against `KittiInference3D` (no mask) on KITTI-size uint8 pairs
      (375x1242 in the 384x1248 frame), D = 192, seeded GwcNet-G, fp16, hot path from a hipGraph, device I/O, per-call use:
      wall time around N frames, synchronised at both ends, the two arms alternating; ms per frame, median (min..max).

    python tools/bench_geometry.py [--iters 200] [--reps 7] [--frames 20]
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


def fmt(v, unit):
    return f"{statistics.median(v):.3f} {unit} median ({min(v):.3f}..{max(v):.3f})"


def operators(a):
    from dcanet_amd import ops
    from dcanet_amd.geometry import StereoCalib
    Hc, Wc = 384, 1248
    calib = StereoCalib(721.5377, 0.5327, 609.5593, 172.854)
    g = torch.Generator().manual_seed(0)
    pred = (torch.rand((Hc, Wc), generator=g) * 180 + 5).cuda()              # 5..185 px: 2..77 m, every pixel kept
    rgb = torch.randint(0, 256, (Hc, Wc, 3), generator=g, dtype=torch.uint8).cuda()
    depth = torch.empty((Hc, Wc), device="cuda")
    vert = torch.empty((Hc * Wc, 4), device="cuda")
    ws = ops.point_cloud_workspace(Hc, Wc, "cuda")

    def pair():
        ops.disp_to_depth(pred, calib, out_f32=depth)
        ops.point_cloud(pred, calib, rgb, out=vert, workspace=ws)

    for _ in range(a.warmup):
        pair()
    torch.cuda.synchronize()
    assert ws[1].tolist() == [Hc * Wc, Hc * Wc], ws[1].tolist()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        pair()
    for _ in range(a.warmup):
        graph.replay()
    res = {"eager": [], "graph": []}
    arms = {"eager": pair, "graph": graph.replay}
    for _ in range(a.reps):
        for k, run in arms.items():
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            start.record()
            for _ in range(a.iters):
                run()
            stop.record()
            stop.synchronize()
            res[k].append(start.elapsed_time(stop) * 1e3 / a.iters)
    for k, v in res.items():
        print(f"(O) {k}: {fmt(v, 'us per depth + point cloud')} over {a.reps} x {a.iters} pairs, {Hc}x{Wc}, all pixels kept")
    return res


def frames(a):
    from bench_frame_io import pairs, timed
    from dcanet_amd.geometry import StereoCalib
    from dcanet_amd.inference import KittiInference, KittiInference3D
    from dcanet_amd.models.gwcnet_dca_g import GwcNet
    from oracle import dcanet_oracle as O
    net = GwcNet(192, use_concat_volume=False)
    net.load_state_dict(O.seeded_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}), strict=True)
    net = net.cuda().eval()
    data = pairs(4)
    calib = StereoCalib(721.5377, 0.5327, 609.5593, 172.854)
    P = KittiInference(net, graph=True, dtype=torch.float16, device_io=True)
    G = KittiInference3D(net, calib, graph=True, dtype=torch.float16, device_io=True)
    arms = {"P": lambda ps: [P(l, r) for l, r in ps], "G": lambda ps: [G(l, r) for l, r in ps]}
    for run in arms.values():
        run([data[i % len(data)] for i in range(6)])
    t = {k: [] for k in arms}
    for _ in range(a.reps):
        for k, run in arms.items():
            t[k].append(timed(run, data, a.frames))
    for k, v in t.items():
        print(f"({k}) {fmt(v, 'ms/frame')} over {a.reps} x {a.frames} frames")
    out = G(*data[0])
    print(f"(G) {len(out.vertices)} points of {out.disp.size} pixels in the first frame")
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--frames", type=int, default=0, help="> 0: also time whole frames of KittiInference / KittiInference3D")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    import dcanet_amd  # noqa: F401
    res = {"operators_us": operators(a)}
    if a.frames > 0:
        res["frames_ms"] = frames(a)
    print("RESULT " + json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
