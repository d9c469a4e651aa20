"""Cost of rectifying on the device, one MI355X, KITTI raw sizes: (512,1392,3) uint8 pairs ->
(375,1242,3), a calibration with KITTI-like intrinsics, distortion and rectifying rotations.

  (1) `ops.rectify_pair` alone: device events around `--launches` back-to-back launches into a preallocated output, after a
      warm-up, and around one replay of a hipGraph holding the same launches (no Python between them); `--reps` repetitions;
      us per launch, median (min..max), next to its compulsory traffic (maps read once, output written once, source read
      once).
  (2) `KittiInference(model, device_io=True[, rectify=maps]).stream(pairs, depth=2)` in the 384x1248 frame, D = 192, seeded
      GwcNet-G, hot path from a hipGraph: wall time around `--frames` frames, device-synchronised at both ends; the arm without
      rectify= gets the host-rectified pairs; the arms alternate for `--reps` repetitions; ms per frame, median (min..max).

    python tools/bench_rectify.py [--launches 200] [--frames 20] [--reps 5] [--out FILE.md]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

SRC, DST = (512, 1392), (375, 1242)


def rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    return np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) \
        @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])


def kitti_like_maps():
    from dcanet_amd.geometry import RectifyMaps
    K = [np.array([[958.3, 0, 697.4], [0, 955.7, 225.9], [0, 0, 1]]), np.array([[902.6, 0, 694.1], [0, 900.2, 244.8], [0, 0, 1]])]
    D = [[-0.3712, 0.2014, 0.0011, -0.0008, -0.0713], [-0.3644, 0.1822, -0.0009, 0.0013, -0.0586]]
    R = [rot(0.004, -0.011, 0.006), rot(-0.007, 0.013, -0.004)]
    P = [np.array([[721.5, 0, 609.6, 44.9], [0, 721.5, 172.9, 0], [0, 0, 1, 0]]),
         np.array([[721.5, 0, 609.6, -339.6], [0, 721.5, 172.9, 0], [0, 0, 1, 0]])]
    return RectifyMaps.from_matrices(K, D, R, P, SRC, DST)


def fmt(v):
    return f"{statistics.median(v):.2f} ({min(v):.2f}..{max(v):.2f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    import dcanet_amd  # noqa: F401
    from bench_frame_io import pairs
    from dcanet_amd import ops
    from dcanet_amd.geometry import rectify_pair_host
    maps = kitti_like_maps()
    raw = pairs(4, *SRC)
    out = []

    # (1) the launch alone
    L, R = (torch.from_numpy(x).cuda() for x in raw[0])
    n = DST[0] * DST[1] * 3
    off = (n + 15) & ~15
    buf = torch.empty(off + n, dtype=torch.uint8, device="cuda")
    dst = (buf[:n].view(*DST, 3), buf[off:off + n].view(*DST, 3))
    for _ in range(20):
        ops.rectify_pair(L, R, maps, out=dst)
    want = rectify_pair_host(*raw[0], maps)
    assert dst[0].cpu().numpy().tobytes() == want[0].tobytes() and dst[1].cpu().numpy().tobytes() == want[1].tobytes()
    us = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.launches):
            ops.rectify_pair(L, R, maps, out=dst)
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / a.launches)
    # the same launches captured into ONE hipGraph (a single branch): the replay leaves the Python wrapper's time out
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(a.launches):
            ops.rectify_pair(L, R, maps, out=dst)
    g.replay()
    gus = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        gus.append(e0.elapsed_time(e1) * 1e3 / a.launches)
    npix = DST[0] * DST[1]
    traffic = {"maps": 2 * 2 * 4 * npix, "output": 2 * 3 * npix, "source": 2 * 3 * SRC[0] * SRC[1]}
    total = sum(traffic.values())
    med = statistics.median(gus)
    out += [f"(1) ops.rectify_pair {SRC} -> {DST}, C = 3, {a.launches} back-to-back launches x {a.reps}: {fmt(us)} us per launch "
            f"from Python, {fmt(gus)} us per launch replayed from one hipGraph",
            f"    compulsory traffic {total / 1e6:.2f} MB ({', '.join(f'{k} {v / 1e6:.2f}' for k, v in traffic.items())}): "
            f"{total / med / 1e6:.3f} TB/s at the median; valid pixels {maps.valid.mean():.4f}"]
    print("\n".join(out), flush=True)
    results = {"rectify_pair_us": us, "rectify_pair_graph_us": gus, "traffic_bytes": total}

    # (2) whole frames
    if not a.kernel_only:
        from dcanet_amd.inference import KittiInference
        from dcanet_amd.models.gwcnet_dca_g import GwcNet
        from oracle import dcanet_oracle as O
        net = GwcNet(192, use_concat_volume=False)
        net.load_state_dict(O.seeded_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}), strict=True)
        net = net.cuda().eval()
        rect = [rectify_pair_host(l, r, maps) for l, r in raw]
        plain, with_rect = KittiInference(net, device_io=True), KittiInference(net, device_io=True, rectify=maps)
        arms = {"stream(depth=2), host-rectified pairs": (plain, rect), "stream(depth=2), rectify=maps, raw pairs": (with_rect, raw)}
        for infer, data in arms.values():
            list(infer.stream([data[i % len(data)] for i in range(a.warmup)], depth=2))
        d0, d1 = plain(*rect[0]), with_rect(*raw[0])
        print(f"    check: max |with rectify= - host-rectified| = {np.abs(d0 - d1).max():.3e}", flush=True)
        t = {k: [] for k in arms}
        for _ in range(a.reps):
            for k, (infer, data) in arms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                list(infer.stream([data[i % len(data)] for i in range(a.frames)], depth=2))
                torch.cuda.synchronize()
                t[k].append((time.perf_counter() - t0) * 1e3 / a.frames)
        lines = ["(2) ms per frame, median (min..max):"] + [f"    {k}: {fmt(v)}" for k, v in t.items()]
        print("\n".join(lines), flush=True)
        out += lines
        results["frames_ms"] = t
    print("RESULT " + json.dumps(results))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
