"""What stereo visual odometry costs on one MI355X.

  (O) operators at the KITTI image, 375 x 1242: a synthetic previous frame (a road seen from 1.65 m, a box on it, a backdrop at
      40 m, 0.3 px of disparity noise) with a smooth texture, and the current image as that texture shifted by the flow of
      0.5 m forward; device-event time around `--iters` eager calls with every buffer passed in (nothing allocated), `--reps`
      repetitions; median (min..max) in us, for `ops.grey_pyramid`, `ops.disp_pyramid`, `ops.ego_motion` (1 + 2 levels iters
      launches; per launch = the call over that number) and `ops.pose_chain`.  The results are compared with the numpy
      restatement before anything is timed.  Whether the call is launch-bound is read off two further arms: the same call
      with iters = 1 (the cost of a dependent iteration is the slope) and at one level.
  (F) frames, with `--frames N` > 0: `KittiInferenceOdometry` against `KittiInferenceTemporal` (given poses) on the same
      KITTI-size uint8 pairs in one process, seeded GwcNet-G, D = 192, hipGraph hot path, fp32; wall time around N frames,
      device-synchronised, arms alternating; median (min..max) in ms per frame.
  (T) with `--train K` > 0: K steps of the unchanged training step through bench.py, its result line repeated.

    python tools/bench_odometry.py [--iters 50] [--reps 7] [--frames 20] [--train 10]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_odometry.py --iters 5 --reps 1
  (the kernel trace is a run of its own: per-launch device time of od_sums_kernel, od_solve_kernel, ... from its stats file)
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_temporal import H, NB, W, event_time, fmt, forward, scene  # noqa: E402


def images(calib, state):
    """the previous and the current left image (H,W,3) uint8: a smooth texture, and the same texture read where 0.5 m forward
    moves every pixel from (inverse warp by the flow of the state's disparity, nearest pixel: enough for a timing)"""
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))

    def tex(x, y):
        return 128 + 40 * np.sin(x / 9.0) * np.cos(y / 7.0) + 35 * np.sin((x + 2 * y) / 23.0) + 25 * np.cos((x - y) / 41.0)
    z = 1.0 - 0.5 * (state["disp"].astype(np.float64) / (calib.f * calib.baseline))          # Z_cur / Z_prev
    prev = np.clip(np.rint(tex(u, v)), 0, 255).astype(np.uint8)
    cur = np.clip(np.rint(tex((u - calib.cx) * z + calib.cx, (v - calib.cy) * z + calib.cy)), 0, 255).astype(np.uint8)
    return np.repeat(prev[..., None], 3, -1), np.repeat(cur[..., None], 3, -1)


def operators(a, calib):
    from dcanet_amd import odometry as OD, ops
    state, _ = scene(calib)
    prev_rgb, cur_rgb = images(calib, state)
    levels, iters = OD.ODOMETRY_LEVELS, OD.ODOMETRY_ITERS
    n = OD.pyramid_len(H, W, levels)
    dprev, dcur, ddisp = (torch.from_numpy(x).cuda() for x in (prev_rgb, cur_rgb, state["disp"]))
    pyr = [torch.empty(n, device="cuda", dtype=torch.uint8) for _ in range(2)]
    dpyr = torch.empty(n, device="cuda")
    out = {"rec": torch.empty(OD.REC_LEN, device="cuda", dtype=torch.float64), "g": torch.empty(24, device="cuda")}
    ws = torch.empty(OD.SUMS, device="cuda", dtype=torch.int64)
    world, odo = torch.zeros(12, device="cuda", dtype=torch.float64), torch.empty(OD.FRAME_LEN, device="cuda", dtype=torch.float64)
    one = OD.pyramid_len(H, W, 1)

    def ego(lv, it):
        m = OD.pyramid_len(H, W, lv)
        return lambda: ops.ego_motion(pyr[0][:m], pyr[1][:m], dpyr[:m], (H, W), calib, lv, it, max_disp=NB, out=out, workspace=ws)
    calls = {"grey_pyramid": (lambda: ops.grey_pyramid(dcur, levels, out=pyr[1]), levels),
             "disp_pyramid": (lambda: ops.disp_pyramid(ddisp, levels, out=dpyr), levels),
             f"ego_motion {levels}x{iters}": (ego(levels, iters), 1 + 2 * levels * iters),
             f"ego_motion {levels}x1": (ego(levels, 1), 1 + 2 * levels),
             f"ego_motion 1x{iters}": (ego(1, iters), 1 + 2 * iters),
             "ego_motion 1x1": (ego(1, 1), 3),
             "pose_chain": (lambda: ops.pose_chain(out["rec"], world, out=odo), 1)}
    ops.grey_pyramid(dprev, levels, out=pyr[0])
    for k in ("grey_pyramid", "disp_pyramid", f"ego_motion {levels}x{iters}"):
        calls[k][0]()
    torch.cuda.synchronize()
    hp, hc, hd = OD.grey_pyramid_host(prev_rgb, levels), OD.grey_pyramid_host(cur_rgb, levels), OD.disp_pyramid_host(state["disp"], levels)
    assert pyr[0].cpu().numpy().tobytes() == hp.tobytes() and pyr[1].cpu().numpy().tobytes() == hc.tobytes()
    assert dpyr.cpu().numpy().tobytes() == hd.tobytes()
    ref = OD.ego_motion_host(hp, hc, hd, (H, W), calib, levels, iters, max_disp=NB)
    assert out["rec"].cpu().numpy().tobytes() == ref["rec"].tobytes(), "the record differs from the restatement"
    t = ref["rec"][[3, 7, 11]]
    note = (f"status {ref['rec'][OD.REC_STATUS]:.0f}, {ref['rec'][OD.REC_COUNT]:.0f} of {H * W} pixels in the last iteration, residual "
            f"{ref['rec'][OD.REC_RESIDUAL]:.2f}, t = ({t[0]:.3f}, {t[1]:.3f}, {t[2]:.3f}) m for 0.5 m forward; level 0 alone: {one} pixels")
    res = {}
    for op, (run, launches) in calls.items():
        for _ in range(a.warmup):
            run()
        v = [event_time(run, a.iters) for _ in range(a.reps)]
        res[op] = v
        print(f"(O) {op:18s} eager: {fmt(v, 'us')} over {a.reps} x {a.iters} calls; {launches} launches = "
              f"{statistics.median(v) / launches:.2f} us per launch", flush=True)
    print("(O) " + note, flush=True)
    return res


def frames(a, calib):
    from bench_frame_io import pairs, timed
    from dcanet_amd.inference import KittiInferenceOdometry, KittiInferenceTemporal
    from dcanet_amd.models.gwcnet_dca_g import GwcNet
    from oracle import dcanet_oracle as O
    net = GwcNet(NB, use_concat_volume=False)
    net.load_state_dict(O.seeded_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}), strict=True)
    net = net.cuda().eval()
    data = pairs(4)
    kw = dict(graph=True, device_io=True)
    temporal, odometry = KittiInferenceTemporal(net, calib, **kw), KittiInferenceOdometry(net, calib, **kw)
    arms = {"KittiInferenceTemporal (given poses)": lambda ps: [temporal(l, r, forward(1.0 * i)) for i, (l, r) in enumerate(ps)],
            "KittiInferenceOdometry": lambda ps: [odometry(l, r) for l, r in ps]}
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


def train(a):
    """the unchanged training step: bench.py in a fresh process (this one has the GPU open; it is not replaced)"""
    run = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(a.train), "--warmup", "3"],
                         capture_output=True, text=True, cwd=ROOT, timeout=900)
    line = next((ln for ln in reversed(run.stdout.splitlines()) if ln.startswith("{")), run.stdout[-300:] + run.stderr[-300:])
    print("(T) " + line, flush=True)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames", type=int, default=0, help="> 0: also time whole frames of KittiInferenceOdometry")
    ap.add_argument("--warmup-frames", type=int, default=6)
    ap.add_argument("--train", type=int, default=0, help="> 0: also run that many steps of the training benchmark")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    import dcanet_amd  # noqa: F401
    from dcanet_amd.geometry import StereoCalib
    calib = StereoCalib(721.5377, 0.5327, 609.5593, 172.854)
    res = {"operators_us": operators(a, calib)}
    if a.frames > 0:
        res["frames_ms"] = frames(a, calib)
    if a.train > 0:
        res["train"] = train(a)
    print("RESULT " + json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
