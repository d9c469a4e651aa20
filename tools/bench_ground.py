"""What the ground stage costs on one MI355X.

  (O) operators at the KITTI frame: the 375 x 1242 window of the 384 x 1248 frame, max_disp 192, refine 2, on a synthetic road
      scene (a plane from `ground.plane_from_pose` at 1.65 m, cars as walls, 0.3 px noise, sky without a measurement);
      device-event time around `--iters` calls with every buffer passed in (nothing allocated), eager launches and hipGraph
      replays alternating for `--reps` repetitions; median (min..max) in us, for `ops.ground_plane` (six launches) and
      `ops.ground_segment` (two).  The results are compared with the numpy restatement before anything is timed.
  (F) frames, with `--frames N` > 0: `KittiInferenceGround` against `KittiInference3D` on the same KITTI-size uint8 pairs in
      one process, seeded GwcNet-G, D = 192, hipGraph hot path, fp32; wall time around N frames, device-synchronised, arms
      alternating; median (min..max) in ms per frame.

    python tools/bench_ground.py [--iters 200] [--reps 7] [--frames 20]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_ground.py --iters 20 --reps 1
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
HC, WC, H, W, NB = 384, 1248, 375, 1242, 192
HBM_BYTES_PER_US = 8.0e6          # 8 TB/s, the MI355X's peak


def fmt(v, unit):
    return f"{statistics.median(v):.3f} {unit} median ({min(v):.3f}..{max(v):.3f})"


def scene(calib):
    """the (HC,WC) frame: a road seen from 1.65 m with 1 degree of pitch and half a degree of roll, three cars, noise"""
    from dcanet_amd import ground as G
    rec = G.plane_from_pose(1.65, 1.0, 0.5, calib, H, W)
    p = G.plane_disp(rec, H, W).astype(np.float64)
    d = np.where(p >= 0.25, p, 0.0)
    for r0, r1, c0, c1 in ((200, 290, 500, 640), (190, 240, 900, 980), (230, 360, 60, 330)):
        d[r0:r1, c0:c1] = p[r1 - 1, (c0 + c1) // 2]
    rng = np.random.default_rng(1)
    d = np.where(d > 0, d + rng.normal(0.0, 0.3, d.shape), d)
    frame = np.zeros((HC, WC), np.float32)
    frame[HC - H:, :W] = d
    return frame


def event_time(run, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(iters):
        run()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / iters


def operators(a, calib):
    from dcanet_amd import ground as G, ops
    frame = scene(calib)
    window = (HC - H, H, W)
    static = torch.from_numpy(frame).cuda()
    ws = ops.ground_workspace(H, W, NB, "cuda")
    NX, NZ = G.segment_scalars("bench", ValueError, NB, G.GROUND_MIN_DISP, 1.0, 0.15, 3.0, 3, G.GROUND_GRID)[-1][3:]
    out_p = {"plane": torch.empty(G.PLANE_LEN, device="cuda", dtype=torch.float64),
             "vdisp": torch.empty((H, NB), device="cuda", dtype=torch.int32)}
    out_s = {"label": torch.empty((H, W), device="cuda", dtype=torch.uint8), "height": torch.empty((H, W), device="cuda"),
             "free_row": torch.empty(W, device="cuda", dtype=torch.int32), "free_disp": torch.empty(W, device="cuda"),
             "bev": torch.empty((2, NZ, NX), device="cuda", dtype=torch.int32)}
    calls = {"ground_plane": lambda: ops.ground_plane(static, NB, calib, window=window, workspace=ws, out=out_p),
             "ground_segment": lambda: ops.ground_segment(static, out_p["plane"], calib, NB, window=window, out=out_s)}
    n = H * W
    # one read of the disparity per launch that reads it (v-disparity, two rounds of sums over the lower half; the two
    # launches of the segmentation), plus what is written: 1 B + 4 B per pixel and the grid
    traffic = {"ground_plane": 4 * n + 2 * 4 * (n // 2) + 4 * H * NB, "ground_segment": 2 * 4 * n + 5 * n + 2 * 4 * 2 * NZ * NX}
    for run in calls.values():
        run()
    torch.cuda.synchronize()
    ref = G.ground_plane_host(frame, NB, calib, window=window)
    assert out_p["plane"].cpu().numpy().tobytes() == ref["plane"].tobytes() and np.array_equal(out_p["vdisp"].cpu().numpy(), ref["vdisp"])
    seg = G.ground_segment_host(frame, ref["plane"], calib, NB, window=window)
    for k, v in seg.items():
        assert out_s[k].cpu().numpy().tobytes() == v.tobytes(), k
    pose = G.plane_pose(ref["plane"], calib)
    note = (f"status {int(ref['plane'][5])}, {int(ref['plane'][3])} inliers, rms {ref['plane'][4]:.3f} px, height {pose['height']:.3f} m, "
            f"pitch {pose['pitch']:.3f}, roll {pose['roll']:.3f} deg; labels {np.bincount(seg['label'].ravel(), minlength=5).tolist()}")
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
    from dcanet_amd.inference import KittiInference3D, KittiInferenceGround
    from dcanet_amd.models.gwcnet_dca_g import GwcNet
    from oracle import dcanet_oracle as O
    net = GwcNet(NB, use_concat_volume=False)
    net.load_state_dict(O.seeded_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}), strict=True)
    net = net.cuda().eval()
    data = pairs(4)
    kw = dict(graph=True, device_io=True)
    nets = {"KittiInference3D": KittiInference3D(net, calib, **kw), "KittiInferenceGround": KittiInferenceGround(net, calib, **kw)}
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
    ap.add_argument("--frames", type=int, default=0, help="> 0: also time whole frames of KittiInferenceGround and KittiInference3D")
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
