"""Guided stereo timings: the guided fused builder against the unguided one at 544x960 / D=192
(quarter resolution 136 x 240, D 48, B 1; fp32 and fp16 volumes; 5 % and 100 % of the cells hinted), the stand-alone
`ops.volume_modulate` on the 251 MB fp32 volume against its traffic floor, and the fp32 eager eval forward at 384x1248 with
and without hints.  Every figure is the median of BLOCKS block means of REPS launches between two device events, the
configurations alternating block by block; the spread printed is min .. max of the block means.

    python tools/bench_guided.py [--out profiles/guided.json] [--only builder]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import dcanet_amd  # noqa: E402,F401
from dcanet_amd import ops  # noqa: E402

BLOCKS, REPS = 15, 20
BN_APPLY_TBS = 5.4          # the project's BatchNorm apply pass, the rate streaming kernels reach here


def blocks(fns, blocks=BLOCKS, reps=REPS):
    """{name: [block mean in us]}: every fn warmed up, then the fns alternate block by block"""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(blocks):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out[k].append(e0.elapsed_time(e1) / reps * 1e3)
    return out


def summary(v):
    return {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}


def hints4(B, H, W, D, share, seed):
    g = torch.Generator().manual_seed(seed)
    h = torch.rand((B, H, W), generator=g) * (D - 1) + 0.25
    h[torch.rand((B, H, W), generator=g) >= share] = 0
    return h.cuda().contiguous()


def builder(res):
    d, h, w = 48, 136, 240
    fl, fr = torch.randn(1, 320, h, w, device="cuda"), torch.randn(1, 320, h, w, device="cuda")
    segs = lambda t: (t[:, :64].contiguous(), t[:, 64:192].contiguous(), t[:, 192:].contiguous())  # noqa: E731
    sl, sr = segs(fl), segs(fr)
    h5, h100 = hints4(1, h, w, d, 0.05, 1), hints4(1, h, w, d, 1.0, 2)
    for dt, name, vol_bytes in ((torch.float32, "fp32", 40 * d * h * w * 4), (torch.float16, "fp16", 40 * d * h * w * 2)):
        t = blocks({"unguided": lambda: ops.cost_volume(sl, sr, d, 40, out_dtype=dt),
                    "guided_5": lambda: ops.cost_volume(sl, sr, d, 40, out_dtype=dt, hints4=h5),
                    "guided_100": lambda: ops.cost_volume(sl, sr, d, 40, out_dtype=dt, hints4=h100)})
        s = {k: summary(v) for k, v in t.items()}
        un = s["unguided"]
        total = vol_bytes + 2 * 320 * h * w * 4                 # the volume's write and both feature maps' read
        bw = total / (un["median_us"] * 1e-6)
        hint_us = 40 * h * w * 4 / bw * 1e6                     # every (y, g) workgroup reads its hint row: G times the map
        budget = un["median_us"] + hint_us + (un["max_us"] - un["min_us"])
        res[f"builder_{name}"] = dict(s, unguided_TBs=round(bw / 1e12, 2), hint_read_us=round(hint_us, 2),
                                      budget_us=round(budget, 2))
        print(f"builder {name}: unguided {un}  {bw / 1e12:.2f} TB/s; budget {budget:.1f} us; guided 5 % {s['guided_5']}; "
              f"100 % {s['guided_100']}", flush=True)


def modulate(res):
    d, h, w = 48, 136, 240
    vol = torch.randn(1, 40, d, h, w, device="cuda")
    out = torch.empty_like(vol)
    h5, h100 = hints4(1, h, w, d, 0.05, 1), hints4(1, h, w, d, 1.0, 2)
    with torch.no_grad():
        t = blocks({"modulate_5": lambda: ops.volume_modulate(vol, h5, out=out),
                    "modulate_100": lambda: ops.volume_modulate(vol, h100, out=out),
                    "inplace_100": lambda: ops.volume_modulate(out, h100, out=out)})
    floor = 2 * vol.numel() * 4 / (BN_APPLY_TBS * 1e12) * 1e6
    s = {k: summary(v) for k, v in t.items()}
    res["modulate"] = dict(s, floor_us=round(floor, 2), ratio_100=round(s["modulate_100"]["median_us"] / floor, 3),
                           ratio_5=round(s["modulate_5"]["median_us"] / floor, 3))
    print(f"volume_modulate 251 MB: {s}; floor at {BN_APPLY_TBS} TB/s {floor:.1f} us", flush=True)


def forward(res):
    from dcanet_amd.models.gwcnet_dca_g import GwcNet
    torch.manual_seed(0)
    model = GwcNet(192, use_concat_volume=False).cuda().eval()
    left, right = torch.randn(1, 3, 384, 1248, device="cuda"), torch.randn(1, 3, 384, 1248, device="cuda")
    g = torch.Generator().manual_seed(3)
    hints = torch.rand((1, 384, 1248), generator=g) * 150 + 1
    hints[torch.rand((1, 384, 1248), generator=g) >= 0.05] = 0      # a Velodyne scan covers about 5 % of the pixels
    hints = hints.cuda()
    with torch.no_grad():
        t = blocks({"forward": lambda: model(left, right), "forward_hints": lambda: model(left, right, hints=hints)},
                   blocks=8, reps=3)
    s = {k: summary(v) for k, v in t.items()}
    res["forward_384x1248_fp32"] = s
    print(f"eval forward 384x1248 fp32 eager: {s}", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, choices=("builder", "modulate", "forward"), help="one part (for a kernel trace)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "timings need the MI355X"
    res = {"device": torch.cuda.get_device_name(0), "blocks": BLOCKS, "reps": REPS}
    for name, part in (("builder", builder), ("modulate", modulate), ("forward", forward)):
        if a.only in (None, name):
            with torch.no_grad():
                part(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))
