"""Cost of projecting a LiDAR scan on the device, one MI355X: a synthetic scan of 120 000 points (64
beams, one turn, the scene of tests/_lidar_reference.py) into the 375 x 1242 rectified image of a KITTI-like calibration.

  (1) `geometry.lidar_disparity_host`, the numpy restatement: wall time per scan, `--reps` repetitions.
  (2) `ops.lidar_disparity` alone, scan, outputs and z-buffer on the device: device events around `--launches` back-to-back
      calls (three launches each) after a warm-up; us per scan, median (min..max) of `--reps` repetitions.  The result is
      compared with (1) bit for bit first.
  (3) `geometry.LidarProjector(...).stream(scans)`: wall time per scan around `--frames` scans from host memory, device-
      synchronised at both ends.

Per-kernel device times: run this file under `rocprofv3 --kernel-trace --stats -- python tools/bench_lidar.py --kernel-only`.

    python tools/bench_lidar.py [--launches 200] [--frames 50] [--reps 7] [--kernel-only] [--out FILE.md]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

OUTPUTS = ("disp", "depth", "disp_u16", "count")
FILTERS = dict(occl=(2, 4, 0.1), min_depth=1.0, max_depth=100.0, min_disp=0.0, max_disp=192.0)


def fmt(v):
    return f"{statistics.median(v):.2f} ({min(v):.2f}..{max(v):.2f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    import dcanet_amd  # noqa: F401
    from _lidar_reference import KITTI_HW, calib_for, scan_points
    from dcanet_amd import ops
    from dcanet_amd.geometry import LidarProjector, lidar_disparity_host
    calib = calib_for(KITTI_HW)
    scans = [scan_points(calib, seed=s) for s in range(4)]
    out, results = [], {}

    # (1) the restatement on the host
    host = []
    for i in range(a.reps if not a.kernel_only else 1):
        t0 = time.perf_counter()
        want = lidar_disparity_host(scans[0], calib, outputs=OUTPUTS, **FILTERS)
        host.append((time.perf_counter() - t0) * 1e3)
    out.append(f"(1) lidar_disparity_host, {len(scans[0])} points -> {KITTI_HW}, all four outputs: {fmt(host)} ms per scan; "
               f"{int(want['count'][1])} points kept, {int(want['count'][0])} pixels written")
    results["host_ms"] = host

    # (2) the three launches alone
    pts = torch.from_numpy(scans[0]).cuda()
    H, W = calib.hw
    bufs = {"disp": torch.empty((H, W), device="cuda"), "depth": torch.empty((H, W), device="cuda"),
            "disp_u16": torch.empty((H, W), device="cuda", dtype=torch.uint16),
            "count": torch.empty(2, device="cuda", dtype=torch.int64)}
    zbuf = torch.empty(H * W, device="cuda", dtype=torch.int32)
    for _ in range(20):
        got = ops.lidar_disparity(pts, calib, outputs=OUTPUTS, out=bufs, workspace=zbuf, **FILTERS)
    for k in OUTPUTS:
        assert got[k].cpu().numpy().tobytes() == want[k].tobytes(), k
    us, us_disp = [], []
    arms = ((OUTPUTS, us),) if a.kernel_only else ((OUTPUTS, us), (("disp",), us_disp))     # a trace holds one variant
    for outputs, into in arms * a.reps:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.launches):
            ops.lidar_disparity(pts, calib, outputs=outputs, out=bufs, workspace=zbuf, **FILTERS)
        e1.record()
        torch.cuda.synchronize()
        into.append(e0.elapsed_time(e1) * 1e3 / a.launches)
    out.append(f"(2) ops.lidar_disparity, the same scan on the device, equal to (1) bit for bit, {a.launches} back-to-back calls "
               f"x {a.reps}, issued from Python: {fmt(us)} us per scan with all four outputs"
               + (f", {fmt(us_disp)} us with `disp` alone (no counters)" if us_disp else ""))
    results["device_us"], results["device_disp_only_us"] = us, us_disp

    # (3) scans from host memory through the staging ring
    if not a.kernel_only:
        proj = LidarProjector(calib, "cuda", capacity=len(scans[0]), depth=2, outputs=OUTPUTS, **FILTERS)
        for _ in proj.stream(scans):
            pass
        ms = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in proj.stream(scans[i % len(scans)] for i in range(a.frames)):
                pass
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3 / a.frames)
        out.append(f"(3) LidarProjector.stream, {a.frames} scans from host memory x {a.reps}: {fmt(ms)} ms per scan (wall clock, "
                   "copy into pinned memory and upload included)")
        results["stream_ms"] = ms
    print("\n".join(out), flush=True)
    print("RESULT " + json.dumps(results))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
