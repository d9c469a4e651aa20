"""What semi-global matching costs on one MI355X.

  (O) the operators at the KITTI image: 375 x 1242, D = 192, with 4 and with 8 paths, on smooth synthetic pairs with sensor
      noise and a shift of 7 px (tools/bench_frame_io.py); device-event time around `--iters` calls with every buffer passed in
      (nothing allocated), eager launches and hipGraph replays alternating for `--reps` repetitions, each repetition at least
      `--fill` seconds long; median (min..max) in us.  Timed: `ops.sgm_census` alone; `ops.sgm_disparity` with the left view's
      outputs; with all five outputs.  A call is census + paths + winner-take-all launches, so the differences give the launches:
      a diagonal path = (8 paths - 4 paths) / 4, the right view = (all outputs - left outputs); the kernels one by one come
      from the profiler (below).  The 8-path result is compared with the numpy restatement before anything is timed
      (`--no-check` skips that: the restatement takes about 20 s at this size).
  (F) frames, with `--frames N` > 0: `SGMInference` alone, then `KittiInferenceGuided(sgm=)` against `KittiInference` on the same
      KITTI-size uint8 pairs in one process, seeded GwcNet-G, D = 192, hipGraph hot path, fp32; wall time around N frames,
      device-synchronised, arms alternating; median (min..max) in ms per frame.

    python tools/bench_sgm.py [--iters 20] [--reps 5] [--frames 20]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_sgm.py --iters 5 --reps 1 --fill 0 --no-check
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
from bench_frame_io import pairs, timed  # noqa: E402
from bench_ground import HBM_BYTES_PER_US, event_time, fmt  # noqa: E402

H, W, D = 375, 1242, 192


def operators(a):
    from dcanet_amd import ops, sgm as S
    left, right = pairs(1, H, W)[0]
    l8, r8 = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
    ws = ops.sgm_workspace(H, W, D, "cuda")
    out = {k: torch.empty((H, W), device="cuda", dtype=S._SGM_KINDS[k]) for k in S.SGM_OUTPUTS}
    census = torch.empty((2, H, W), device="cuda", dtype=torch.int64)
    left_names = S.SGM_OUTPUTS[:3]

    def disparity(paths, names):
        return lambda: ops.sgm_disparity(l8, r8, D, paths=paths, outputs=names, out={k: out[k] for k in names}, workspace=ws)

    calls = {"census": lambda: ops.sgm_census(l8, r8, out=census)}
    for paths in (4, 8):
        calls[f"{paths} paths, left view"] = disparity(paths, left_names)
        calls[f"{paths} paths, both views"] = disparity(paths, S.SGM_OUTPUTS)
    # compulsory traffic: the images read and the census written; per path the census read and S written (the first path) or read
    # and written (the others); per view S read once
    n, c = H * W, left.shape[2]
    vol = 2 * n * D
    img = 2 * n * c + 16 * n
    traffic = {"census": img}
    for paths in (4, 8):
        agg = img + paths * 16 * n + (2 * paths - 1) * vol
        traffic[f"{paths} paths, left view"] = agg + vol + 12 * n
        traffic[f"{paths} paths, both views"] = agg + 2 * vol + 20 * n
    if not a.no_check:
        calls["8 paths, both views"]()
        torch.cuda.synchronize()
        ref = S.sgm_host(left, right, D, outputs=S.SGM_OUTPUTS)
        for k, v in ref.items():
            assert out[k].cpu().numpy().tobytes() == v.tobytes(), k
        print(f"(O) equals the restatement bit for bit; {ref['valid'].mean():.3f} of the pixels valid, median disparity "
              f"{np.median(ref['disp'][ref['valid'] > 0])}", flush=True)
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
        iters = max(a.iters, int(a.fill * 1e6 / max(event_time(graph.replay, a.iters), 1.0)))      # a repetition fills `fill` seconds
        t = {"eager": [], "graph": []}
        for _ in range(a.reps):
            for k, f in (("eager", run), ("graph", graph.replay)):
                t[k].append(event_time(f, iters))
        res[op] = t
        for k, v in t.items():
            print(f"(O) {op:22s} {k:5s}: {fmt(v, 'us')} over {a.reps} x {iters} calls; compulsory traffic "
                  f"{traffic[op] / 1e6:.1f} MB = {traffic[op] / HBM_BYTES_PER_US:.1f} us at 8 TB/s", flush=True)
    med = lambda op: statistics.median(res[op]["graph"])
    print(f"(O) by difference (graph medians): a diagonal path {(med('8 paths, left view') - med('4 paths, left view')) / 4:.1f} us "
          f"({H} dependent steps per wave, {W} waves); the right view {med('8 paths, both views') - med('8 paths, left view'):.1f} us; "
          f"4 axis paths + left view {med('4 paths, left view') - med('census'):.1f} us", flush=True)
    return res


def frames(a):
    from dcanet_amd.inference import KittiInference, KittiInferenceGuided, SGMInference
    from dcanet_amd.models.gwcnet_dca_g import GwcNet
    from oracle import dcanet_oracle as O
    data = pairs(4, H, W)
    res = {}
    sgm = SGMInference(D)
    alone = lambda ps: [sgm(l, r) for l, r in ps]
    alone([data[i % len(data)] for i in range(a.warmup_frames)])
    res["SGMInference"] = [timed(alone, data, a.frames) for _ in range(a.reps)]
    streamed = lambda ps: list(sgm.stream(iter(ps)))
    streamed(data)
    res["SGMInference.stream"] = [timed(streamed, data, a.frames) for _ in range(a.reps)]
    net = GwcNet(D, use_concat_volume=False)
    net.load_state_dict(O.seeded_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}), strict=True)
    net = net.cuda().eval()
    kw = dict(graph=True, device_io=True)
    nets = {"KittiInference": KittiInference(net, **kw), "KittiInferenceGuided(sgm=)": KittiInferenceGuided(net, sgm=dict(max_disp=D), **kw)}
    arms = {k: (lambda ps, f=f: [f(l, r) for l, r in ps]) for k, f in nets.items()}
    for run in arms.values():
        run([data[i % len(data)] for i in range(a.warmup_frames)])
    t = {k: [] for k in arms}
    for _ in range(a.reps):
        for k, run in arms.items():
            t[k].append(timed(run, data, a.frames))
    res.update(t)
    for k, v in res.items():
        print(f"(F) fp32 {k}: {fmt(v, 'ms/frame')} = {1e3 / statistics.median(v):.1f} frames/s over {a.reps} x {a.frames} frames",
              flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--fill", type=float, default=1.0, help="seconds of device time a repetition fills at least")
    ap.add_argument("--no-check", action="store_true", help="skip the comparison with the numpy restatement")
    ap.add_argument("--frames", type=int, default=0, help="> 0: also time whole frames of SGMInference and KittiInferenceGuided(sgm=)")
    ap.add_argument("--warmup-frames", type=int, default=6)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    import dcanet_amd  # noqa: F401
    res = {"operators_us": operators(a)}
    if a.frames > 0:
        res["frames_ms"] = frames(a)
    print("RESULT " + json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
