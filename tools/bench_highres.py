"""What the high-resolution path costs on one MI355X.

  (O) operators at Middlebury-F size, scale 2 (2000 x 2964 <-> 1000 x 1482), device-event time around `--iters` calls with
      every buffer passed in (nothing allocated), `--reps` repetitions; median (min..max) in us:
        `ops.area_downscale_pair`, `ops.area_downscale_disp`, `ops.guided_upsample` (r = 1, 2, 3; both outputs; C = 3)
      each next to its compulsory traffic -- the bytes that have to cross HBM once whatever the algorithm -- and the share
      of the 8 TB/s peak that traffic over the measured time amounts to; and, for scale, torch's
      `F.interpolate(mode="bilinear")` of the same map to the same size.  The results are compared with the numpy
      restatements before anything is timed (`--no-check` skips the upsampler's, which takes numpy half a minute).
  (F) frames, with `--frames N` > 0: `HighResInference(scale=2)` on such pairs in a 1008 x 1488 frame, seeded GwcNet-G,
      D = 192, hipGraph hot path, fp32; wall time around N frames, device-synchronised; ms per frame.

    python tools/bench_highres.py [--iters 100] [--reps 7] [--frames 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
H, W, S = 2000, 2964, 2
HBM_BYTES_PER_US = 8.0e6          # 8 TB/s, the MI355X's peak


def fmt(v, unit):
    return f"{statistics.median(v):.2f} {unit} median ({min(v):.2f}..{max(v):.2f})"


def event_time(run, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(iters):
        run()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / iters


def scene(seed=1):
    """a full-resolution pair of smooth colour patches with noise, a ground truth with infinities, and the disparity a network
    might return at 1/S: two surfaces, 2 % of it invalid"""
    rng = np.random.default_rng(seed)
    h, w = -(-H // S), -(-W // S)
    patches = rng.integers(0, 256, (H // 40 + 1, W // 40 + 1, 3), dtype=np.uint8)
    base = np.repeat(np.repeat(patches, 40, 0), 40, 1)[:H, :W].astype(np.int16)
    left = np.clip(base + rng.integers(-6, 7, base.shape, dtype=np.int16), 0, 255).astype(np.uint8)
    right = np.clip(base + rng.integers(-6, 7, base.shape, dtype=np.int16), 0, 255).astype(np.uint8)
    gt = rng.uniform(1, 800, (H, W)).astype(np.float32)
    gt[rng.random((H, W)) < 0.01] = np.inf
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    lo = (40 + np.float32(0.05) * x + np.where(x > w // 2 + np.float32(0.2) * y, np.float32(90), 0)).astype(np.float32)
    lo[rng.random((h, w)) < 0.02] = 0
    return left, right, gt, lo


def operators(a):
    from dcanet_amd import highres, ops
    h, w = highres.small_hw(H, W, S)
    left, right, gt, lo = scene()
    L, R, G, LO = (torch.from_numpy(t).cuda() for t in (left, right, gt, lo))
    small = torch.empty((2, h, w, 3), device="cuda", dtype=torch.uint8)
    small_gt = torch.empty((h, w), device="cuda")
    out = {"disp": torch.empty((H, W), device="cuda"), "valid": torch.empty((H, W), device="cuda")}
    ops.area_downscale_pair(L, R, S, out=small)
    tables = {r: highres.jbu_tables(S, r) for r in (1, 2, 3)}
    tdev = {r: highres.device_tables(t, "cuda") for r, t in tables.items()}
    calls = {"area_downscale_pair": (lambda: ops.area_downscale_pair(L, R, S, out=small), 2 * 3 * (H * W + h * w)),
             "area_downscale_disp": (lambda: ops.area_downscale_disp(G, S, out=small_gt), 4 * (H * W + h * w))}
    for r in (1, 2, 3):
        calls[f"guided_upsample r={r}"] = (lambda r=r: ops.guided_upsample(LO, small[0], L, S, tdev[r], out=out),
                                           3 * H * W + 7 * h * w + 8 * H * W)
    calls["F.interpolate bilinear"] = (lambda: torch.nn.functional.interpolate(LO[None, None], size=(H, W), mode="bilinear",
                                                                               align_corners=False), 4 * h * w + 4 * H * W)
    # the results first
    torch.cuda.synchronize()
    want_small = highres.area_downscale_pair_host(left, right, S)
    assert small.cpu().numpy().tobytes() == want_small.tobytes()
    ops.area_downscale_disp(G, S, out=small_gt)
    assert small_gt.cpu().numpy().tobytes() == highres.area_downscale_disp_host(gt, S).tobytes()
    if a.check:
        t0 = time.perf_counter()
        ref = highres.guided_upsample_host(lo, want_small[0], left, S, tables[2])
        ops.guided_upsample(LO, small[0], L, S, tdev[2], out=out)
        assert all(out[k].cpu().numpy().tobytes() == ref[k].tobytes() for k in out)
        print(f"(O) guided_upsample r=2 equals the numpy restatement bit for bit at {H}x{W} (numpy: "
              f"{time.perf_counter() - t0:.1f} s); valid {int(ref['valid'].sum())} of {H * W}", flush=True)
    res = {}
    for name, (run, traffic) in calls.items():
        for _ in range(a.warmup):
            run()
        t = [event_time(run, a.iters) for _ in range(a.reps)]
        res[name] = t
        floor = traffic / HBM_BYTES_PER_US
        print(f"(O) {name:24s}: {fmt(t, 'us')} over {a.reps} x {a.iters} calls; compulsory traffic {traffic / 1e6:.1f} MB = "
              f"{floor:.1f} us at 8 TB/s: {100 * floor / statistics.median(t):.1f} % of the peak", flush=True)
    return res


def frames(a):
    from dcanet_amd.inference import HighResInference
    from dcanet_amd.models.gwcnet_dca_g import GwcNet
    from oracle import dcanet_oracle as O
    net = GwcNet(192, use_concat_volume=False)
    net.load_state_dict(O.seeded_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}), strict=True)
    net = net.cuda().eval()
    pairs = [scene(seed)[:2] for seed in (2, 3)]
    infer = HighResInference(net, scale=S, crop_height=1008, crop_width=1488)
    for i in range(a.warmup_frames):
        infer(*pairs[i % 2])
    t = []
    for _ in range(a.reps_frames):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(a.frames):
            disp, valid = infer(*pairs[i % 2])
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3 / a.frames)
    print(f"(F) HighResInference(scale={S}) {H}x{W} -> frame 1008x1488 -> {disp.shape[0]}x{disp.shape[1]}, fp32, D=192: "
          f"{fmt(t, 'ms/frame')} over {a.reps_frames} x {a.frames} frames; valid {int(valid.sum())} of {valid.size}", flush=True)
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--frames", type=int, default=0, help="> 0: also time whole frames of HighResInference")
    ap.add_argument("--reps-frames", type=int, default=3)
    ap.add_argument("--warmup-frames", type=int, default=2)
    ap.add_argument("--no-check", dest="check", action="store_false", help="skip the restatement of the upsampler at full size")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    import dcanet_amd  # noqa: F401
    res = {"operators_us": operators(a)}
    if a.frames > 0:
        res["frames_ms"] = frames(a)
    print("RESULT " + json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
