"""What temporal stereo costs on one MI355X.

  (O) operators at the KITTI image, 375 x 1242, 1 m forward: a synthetic state (a road seen from 1.65 m, a box on it, a backdrop
      at 40 m, 0.3 px noise, variances and ages per pixel) and a noisy measurement in the 384 x 1248 frame; device-event time
      around `--iters` eager calls with every buffer passed in (nothing allocated), `--reps` repetitions; median (min..max) in
      us, for `ops.disp_reproject` (three launches) and `ops.temporal_fuse` (one).  The results are compared with the numpy
      restatement before anything is timed.  No hipGraph arm: the matrix goes by value, the operators are launched eagerly.
  (F) frames, with `--frames N` > 0: `KittiInferenceTemporal` without and with `guide=` against `KittiInferenceWithConfidence`
      on the same KITTI-size uint8 pairs in one process, seeded GwcNet-G, D = 192, hipGraph hot path, fp32; 1 m forward per
      frame; wall time around N frames, device-synchronised, arms alternating; median (min..max) in ms per frame.

    python tools/bench_temporal.py [--iters 200] [--reps 7] [--frames 20]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_temporal.py --iters 20 --reps 1
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
    """the state of the frame before, (H,W): the road's disparity grows linearly below the horizon, the backdrop is constant
    above it, a box of one disparity stands on the road; and a measurement of the same scene in the (HC,WC) frame"""
    rng = np.random.default_rng(1)
    v = np.arange(H, dtype=np.float64)[:, None] + np.zeros((1, W))
    road = calib.baseline * (v - calib.cy) / 1.65
    d = np.maximum(road, calib.f * calib.baseline / 40.0)
    d[150:260, 520:700] = np.maximum(d[150:260, 520:700], road[259, 600])
    noisy = lambda: (d + rng.normal(0.0, 0.3, d.shape)).astype(np.float32)       # noqa: E731
    state = {"disp": noisy(), "var": rng.uniform(0.05, 0.5, d.shape).astype(np.float32),
             "age": rng.integers(0, 8, d.shape).astype(np.uint8)}
    frame = np.zeros((HC, WC), np.float32)
    frame[HC - H:, :W] = noisy()
    return state, frame


def event_time(run, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(iters):
        run()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / iters


def forward(metres):
    T = np.eye(4)
    T[2, 3] = metres
    return T


def operators(a, calib):
    from dcanet_amd import ops, temporal as T
    from dcanet_amd.geometry import relative_pose
    state, frame = scene(calib)
    G = T.reproject_matrix(calib, relative_pose(np.eye(4), forward(1.0)))
    window = (HC - H, H, W)
    dstate = {k: torch.from_numpy(v).cuda() for k, v in state.items()}
    meas = torch.from_numpy(frame).cuda()
    ws = ops.temporal_workspace(H, W, "cuda")
    out_p = {"pred": torch.empty((H, W), device="cuda"), "var": torch.empty((H, W), device="cuda"),
             "age": torch.empty((H, W), device="cuda", dtype=torch.uint8), "hints": torch.empty((H, W), device="cuda"),
             "count": torch.empty(2, device="cuda", dtype=torch.int64)}
    out_f = {"disp": torch.empty((H, W), device="cuda"), "var": torch.empty((H, W), device="cuda"),
             "age": torch.empty((H, W), device="cuda", dtype=torch.uint8)}
    calls = {"disp_reproject": lambda: ops.disp_reproject(dstate, G, calib, max_disp=NB, workspace=ws, out=out_p),
             "temporal_fuse": lambda: ops.temporal_fuse(out_p, meas, 0.09, window=window, out=out_f)}
    n = H * W
    # reproject: 8 B cleared, 4 B read and 8 B of atomic per source, 8 B read per target, 9 B gathered, 13 B written = ~50 B a pixel;
    # fuse: 9 B of prediction and 4 B of measurement read, 9 B written
    traffic = {"disp_reproject": 50 * n, "temporal_fuse": 22 * n}
    for run in calls.values():
        run()
    torch.cuda.synchronize()
    ref = T.disp_reproject_host(state, G, calib, max_disp=NB)
    for k in T.REPROJECT_OUTPUTS:
        assert out_p[k].cpu().numpy().tobytes() == ref[k].tobytes(), k
    fused = T.temporal_fuse_host(ref, frame, 0.09, window=window)
    for k, v in fused.items():
        assert out_f[k].cpu().numpy().tobytes() == v.tobytes(), k
    note = (f"{int(ref['count'][1])} of {n} sources kept, {int(ref['count'][0])} targets visible; fused: "
            f"{int((fused['age'] > 0).sum())} pixels carry on, {int(((fused['age'] == 0) & (fused['disp'] > 0)).sum())} start again")
    res = {}
    for op, run in calls.items():
        for _ in range(a.warmup):
            run()
        t = [event_time(run, a.iters) for _ in range(a.reps)]
        res[op] = t
        print(f"(O) {op:14s} eager: {fmt(t, 'us')} over {a.reps} x {a.iters} calls; traffic {traffic[op] / 1e6:.2f} MB = "
              f"{traffic[op] / HBM_BYTES_PER_US:.2f} us at 8 TB/s", flush=True)
    print("(O) " + note, flush=True)
    return res


def frames(a, calib):
    from bench_frame_io import pairs, timed
    from dcanet_amd.inference import KittiInferenceTemporal, KittiInferenceWithConfidence
    from dcanet_amd.models.gwcnet_dca_g import GwcNet
    from oracle import dcanet_oracle as O
    net = GwcNet(NB, use_concat_volume=False)
    net.load_state_dict(O.seeded_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}), strict=True)
    net = net.cuda().eval()
    data = pairs(4)
    kw = dict(graph=True, device_io=True)
    conf = KittiInferenceWithConfidence(net, **kw)
    plain, guided = KittiInferenceTemporal(net, calib, **kw), KittiInferenceTemporal(net, calib, guide=(10.0, 1.0), **kw)

    def sequence(f):
        return lambda ps: [f(l, r, forward(1.0 * i)) for i, (l, r) in enumerate(ps)]
    arms = {"KittiInferenceWithConfidence": lambda ps: [conf(l, r) for l, r in ps], "KittiInferenceTemporal": sequence(plain),
            "KittiInferenceTemporal guide=(10, 1)": sequence(guided)}
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
    ap.add_argument("--frames", type=int, default=0, help="> 0: also time whole frames of KittiInferenceTemporal")
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
