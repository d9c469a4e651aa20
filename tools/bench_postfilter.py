"""What the disparity post-filter costs on one MI355X.

  (O) operators at the KITTI frame size 384x1248, device-event time around `--iters` calls with every buffer passed in
      (nothing allocated), eager launches and hipGraph replays alternating for `--reps` repetitions; median (min..max) in us:
        `ops.speckle_filter(d, 200, 2.0)` on three inputs -- the scene of the tests at frame size (planes, an object, a
        speckle, 3 % salt), the constant frame (ONE component: the worst case of the count launch, every tile adds to one
        word) and the snake (one component through every tile on every second row: the worst case of the chain depth);
        `ops.median_filter(d, 3 | 5)` on the scene.
      Each next to its compulsory traffic: the bytes that have to cross HBM once whatever the algorithm -- 4 B/pixel in,
      4 B/pixel per output map -- and the time that takes at the peak rate.  The results are compared with the numpy
      restatement before anything is timed.
  (H) with scipy importable: `scipy.sparse.csgraph.connected_components` on the scene's graph on the host, graph
      construction included and excluded, labelled as such: what a user without the kernels would run.
  (F) frames, with `--frames N` > 0: `KittiInference3D(speckle=(200, 2.0))` against the same class with `speckle=None` in
      one process, KITTI-size uint8 pairs, seeded GwcNet-G, D = 192, hipGraph hot path, fp32 and fp16; wall time around N
      frames, device-synchronised, arms alternating; median (min..max) in ms per frame and the overhead per frame.  A
      third arm, `speckle=(0, 2.0)`, runs the same launches and removes nothing: with seeded weights the disparity is noise,
      (200, 2.0) removes most of it, and the frame gets FASTER by the vertices it no longer copies to the host -- the third
      arm is the filter's own cost at an unchanged point count.

    python tools/bench_postfilter.py [--iters 200] [--reps 7] [--frames 20]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_postfilter.py --iters 20 --reps 1 \
        --inputs snake --no-host
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
HC, WC = 384, 1248
HBM_BYTES_PER_US = 8.0e6          # 8 TB/s, the MI355X's peak


def fmt(v, unit):
    return f"{statistics.median(v):.3f} {unit} median ({min(v):.3f}..{max(v):.3f})"


def inputs():
    """the three frames (HC,WC) float32"""
    rng = np.random.default_rng(1)
    y, x = np.mgrid[0:HC, 0:WC].astype(np.float32)
    scene = (20 + np.float32(0.05) * x + np.float32(0.02) * y + np.where(x >= WC // 2, np.float32(7.3), 0)).astype(np.float32)
    scene[HC // 4:HC // 4 + 90, WC // 8:WC // 8 + 200] = 55.5
    scene[HC // 2 + 3:HC // 2 + 6, WC // 2 + 9:WC // 2 + 13] = 3.25
    salt = rng.random((HC, WC)) < 0.03
    scene[salt] += rng.uniform(3, 30, int(salt.sum())).astype(np.float32)
    snake = np.full((HC, WC), 50, np.float32)
    snake[0::2] = 10
    snake[1::4, WC - 1] = 10
    snake[3::4, 0] = 10
    return {"scene": scene, "constant": np.full((HC, WC), 7.5, np.float32), "snake": snake}


def event_time(run, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(iters):
        run()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / iters


def operators(a):
    from dcanet_amd import ops
    from dcanet_amd.postfilter import median_filter_host, speckle_filter_host
    n = HC * WC
    static = torch.empty((HC, WC), device="cuda")
    out = {"disp": torch.empty((HC, WC), device="cuda"), "valid": torch.empty((HC, WC), device="cuda"),
           "size": torch.empty((HC, WC), device="cuda", dtype=torch.int32)}
    med = torch.empty((HC, WC), device="cuda")
    ws = ops.speckle_workspace(HC, WC, "cuda")
    calls = {"speckle": lambda: ops.speckle_filter(static, 200, 2.0, out=out, workspace=ws),
             "median3": lambda: ops.median_filter(static, 3, out=med), "median5": lambda: ops.median_filter(static, 5, out=med)}
    traffic = {"speckle": 16 * n, "median3": 8 * n, "median5": 8 * n}
    frames = {k: v for k, v in inputs().items() if k in a.inputs.split(",")}
    res = {}
    for name, frame in frames.items():
        static.copy_(torch.from_numpy(frame))
        for op in (("speckle",) if name != "scene" else ("speckle", "median3", "median5")):
            run = calls[op]
            for _ in range(a.warmup):
                run()
            torch.cuda.synchronize()
            if op == "speckle":
                ref = speckle_filter_host(frame, 200, 2.0)
                for k in ("size", "valid", "disp"):
                    assert np.array_equal(out[k].cpu().numpy().view(np.int32), ref[k].view(np.int32)), (name, k)
                note = f"largest component {int(ref['size'].max())} of {n} pixels, {int((ref['valid'] == 0).sum())} removed"
            else:
                assert med.cpu().numpy().tobytes() == median_filter_host(frame, int(op[-1])).tobytes(), op
                note = "masked median, no mask"
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=torch.cuda.Stream()):
                run()
            for _ in range(a.warmup):
                graph.replay()
            t = {"eager": [], "graph": []}
            for _ in range(a.reps):
                for k, f in (("eager", run), ("graph", graph.replay)):
                    t[k].append(event_time(f, a.iters))
            res[f"{op} {name}"] = t
            floor = traffic[op] / HBM_BYTES_PER_US
            for k, v in t.items():
                print(f"(O) {op:8s} {name:8s} {k:5s}: {fmt(v, 'us')} over {a.reps} x {a.iters} calls; compulsory traffic "
                      f"{traffic[op] / 1e6:.2f} MB = {floor:.2f} us at 8 TB/s; {note}", flush=True)
    return res


def host(a):
    try:
        from scipy import sparse
        from scipy.sparse import csgraph
    except ImportError:
        print("(H) scipy is not importable here: no host arm")
        return None
    d = inputs()["scene"]
    idx = np.arange(d.size).reshape(d.shape)
    t = {"graph construction + components": [], "components alone": []}
    for _ in range(max(3, a.reps // 2)):
        t0 = time.perf_counter()
        u, v = [], []
        for p, q in ((np.s_[:, :-1], np.s_[:, 1:]), (np.s_[:-1], np.s_[1:])):
            join = np.abs(d[p] - d[q]) <= np.float32(2.0)
            u.append(idx[p][join])
            v.append(idx[q][join])
        u, v = np.concatenate(u), np.concatenate(v)
        g = sparse.coo_matrix((np.ones(len(u), np.int8), (u, v)), shape=(d.size,) * 2).tocsr()
        t1 = time.perf_counter()
        _, comp = csgraph.connected_components(g, directed=False)
        size = np.bincount(comp)[comp]
        t2 = time.perf_counter()
        t["graph construction + components"].append((t2 - t0) * 1e3)
        t["components alone"].append((t2 - t1) * 1e3)
    for k, v in t.items():
        print(f"(H) host, scipy csgraph, scene {HC}x{WC}, {k}: {fmt(v, 'ms')}; largest component {int(size.max())}", flush=True)
    return t


def frames(a):
    from bench_frame_io import pairs, timed
    from dcanet_amd.geometry import StereoCalib
    from dcanet_amd.inference import KittiInference3D
    from dcanet_amd.models.gwcnet_dca_g import GwcNet
    from oracle import dcanet_oracle as O
    net = GwcNet(192, use_concat_volume=False)
    net.load_state_dict(O.seeded_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}), strict=True)
    net = net.cuda().eval()
    data = pairs(4)
    calib = StereoCalib(721.5377, 0.5327, 609.5593, 172.854)
    res = {}
    for label, dtype in (("fp32", None), ("fp16", torch.float16)):
        kw = dict(graph=True, dtype=dtype, device_io=True)
        nets = {"speckle=None": KittiInference3D(net, calib, **kw),
                "speckle=(0, 2.0)": KittiInference3D(net, calib, speckle=(0, 2.0), **kw),
                "speckle=(200, 2.0)": KittiInference3D(net, calib, speckle=(200, 2.0), **kw)}
        arms = {k: (lambda ps, f=f: [f(l, r) for l, r in ps]) for k, f in nets.items()}
        for run in arms.values():
            run([data[i % len(data)] for i in range(a.warmup_frames)])
        t = {k: [] for k in arms}
        for _ in range(a.reps):
            for k, run in arms.items():
                t[k].append(timed(run, data, a.frames))
        points = {k: len(f(*data[0]).vertices) for k, f in nets.items()}
        p = statistics.median(t["speckle=None"])
        for k, v in t.items():
            print(f"(F) {label} {k}: {fmt(v, 'ms/frame')} over {a.reps} x {a.frames} frames; {points[k]} points in the first "
                  f"frame; {(statistics.median(v) - p) * 1e3:+.0f} us/frame ({100 * (statistics.median(v) / p - 1):+.2f} %) against "
                  f"speckle=None", flush=True)
        print(f"(F) {label}: spread of the unfiltered arm {(max(t['speckle=None']) - min(t['speckle=None'])) * 1e3:.0f} us")
        res[label] = t
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--frames", type=int, default=0, help="> 0: also time whole frames of KittiInference3D with and without speckle=")
    ap.add_argument("--warmup-frames", type=int, default=6)
    ap.add_argument("--inputs", default="scene,constant,snake", help="the operator inputs to time (one alone for a kernel trace)")
    ap.add_argument("--no-host", action="store_true", help="skip the scipy arm")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    import dcanet_amd  # noqa: F401
    res = {"operators_us": operators(a), "host_ms": None if a.no_host else host(a)}
    if a.frames > 0:
        res["frames_ms"] = frames(a)
    print("RESULT " + json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
