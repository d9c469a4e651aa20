"""What the wrappers of frame_ops.py hand to libdca_hip.so for arguments they accept, pinned against a record.

`frame_ops._L` is replaced by the recorder of test_dispatch_cpu.py (tests/_recorder.py): it notes every call as (entry-point
name, per argument: the int / float value, or 1 / 0 for a pointer given / null), forwards only the pure host size queries
(names ending in _tiles, _workspace, _len) to the real library and answers 0 to everything else, so no kernel is launched.
Every public function is called on device tensors of the smallest shapes that reach each of its branches
(tests/_frame_ops_cases.py): the map layouts, with and without a mask, the windows, every `out` / `workspace` passed in and
none, every `outputs=` subset.  tests/golden/frame_ops_trace.json holds per case the recorded sequence and, per returned
tensor, its dtype, its shape and which of the caller's buffers it lives in (-1: a tensor of the wrapper's own).

    python tests/test_gpu_frame_ops_trace.py --record COMMIT      rewrites the file, noting COMMIT as its origin

The file was recorded on the commit before the wrappers moved out of ops.py (there the recorder goes onto `ops._L`; see its
"recorded_on") and is a record of behaviour: re-record it only in a change that means to alter a call, and read the diff."""
import itertools
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import _frame_ops_cases as C  # noqa: E402
from _frame_ops_cases import EDGE, F, H, W, WIN  # noqa: E402
from _recorder import Recorder  # noqa: E402

GOLDEN_FILE = os.path.join(ROOT, "tests", "golden", "frame_ops_trace.json")
HOST_QUERIES = ("_tiles", "_workspace", "_len")


def _new(kind, *shape):
    return lambda c, kw: getattr(c, kind)(*shape)


def _subsets(names, empty=True):
    return [s for n in range(0 if empty else 1, len(names) + 1) for s in itertools.combinations(names, n)]


def _layouts(key, batch=2):
    """the map argument `key` as (8,12), (B,8,12) and (B,1,8,12)"""
    return [("hw", {key: _new("f32", H, W)}), ("bhw", {key: _new("f32", batch, H, W)}), ("b1hw", {key: _new("f32", batch, 1, H, W)})]


def _like(key):
    return lambda c, kw: torch.zeros_like(kw[key])


def cases():
    """(id, function, overrides of its base arguments)"""
    out = []

    def add(op, tag, **ov):
        out.append((f"{op}/{tag}", op, ov))

    add("disp_metrics", "plain")
    add("disp_metrics", "b1hw_mask", pred=_new("f32", 2, 1, H, W), mask=_new("b", 2, H, W))
    add("disp_metrics", "padded", pred=_new("f32", 2, H + 2, W + 2))
    add("region_confusion", "one")
    add("region_confusion", "two", volumes=lambda c, kw: [c.f32(2, 3, 1, 2), c.f32(2, 3, 1, 2)])
    add("region_confusion", "three_b1", volumes=lambda c, kw: [c.f32(2, 1, 3, 2, 3) for _ in range(3)])
    add("eval_state", "3")
    add("eval_accumulate", "plain")
    add("conf_histogram", "plain")
    for tag, shape in (("hw", (H, W)), ("b1hw", (2, 1, H, W))):
        add("mirror_pair", tag, left=_new("f32", *shape), right=_new("f32", *shape))
        add("mirror_pair", tag + "_out", left=_new("f32", *shape), right=_new("f32", *shape), out=_new("f32", 2, *shape))
    for tag, shape in (("bhw", (2, H, W)), ("b1hw", (2, 1, H, W))):
        add("lr_consistency", tag, disp_left=_new("f32", *shape), disp_right_mirrored=_new("f32", *shape), tau=0.5, cols=7)
    for names in _subsets(F.LR_OUTPUTS):
        add("lr_consistency", "outputs_" + "_".join(names), outputs=names)
    add("selfsup_loss", "plain")
    add("selfsup_loss", "valid_f32", valid=_new("f32", 1, 4, 5), alpha=0.5, lam=0.2, c1=1e-3, c2=2e-3)
    add("selfsup_loss", "valid_bool", valid=_new("b", 1, 1, 4, 5), photo_scale=0.0)
    for ch in (3, 4):
        img = dict(left_u8=_new("u8", 6, 10, ch), right_u8=_new("u8", 6, 10, ch))
        add("frame_histogram", f"c{ch}", **img)
        add("frame_apply", f"c{ch}", **img)
        add("frame_apply", f"c{ch}_edge_out", **img, src_y0=0, dst_y0=2, rows=6, cols=10, out=_new("f32", 2, 3, H, W))
        add("rectify_pair", f"c{ch}", **img)
        add("rectify_pair", f"c{ch}_out", **img, out=_new("u8", 2, 5, 7, ch))
        add("rectify_pair", f"c{ch}_out_pair", **img, out=lambda c, kw, ch=ch: (c.u8(5, 7, ch), c.u8(5, 7, ch)))
        add("train_luma_sum", f"c{ch}", **img)
        add("train_patch_colour", f"c{ch}", right_u8=_new("u8", 6, 10, ch))
        add("train_crop_norm", f"c{ch}", **img)
    add("frame_apply", "empty", rows=0, cols=0)
    add("frame_lut", "plain")
    for tag, pred in (("hw", _new("f32", H, W)), ("11hw", _new("f32", 1, 1, H, W))):
        for wtag, (y0, h, w) in (("win", WIN), ("edge", EDGE), ("whole", (0, H, W))):
            add("disp_export", f"{tag}_{wtag}", pred=pred, y0=y0, h=h, w=w)
    add("disp_export", "u16", f32=False, u16=True, scale=128.0)
    add("disp_export", "both", u16=True)
    add("disp_export", "both_out", u16=True, out_f32=_new("f32", 5, 7), out_u16=_new("u16", 5, 7))
    add("train_tables", "plain")
    add("train_patch_colour", "edge", y1=2, x1=3, th=4, tw=7)
    add("train_crop_norm", "edge", y1=2, x1=3, out_left=_new("f32", 3, 4, 7), out_right=_new("f32", 3, 4, 7))
    add("train_crop_norm", "patch", patch=(0, 2, 1, 3), norm=_new("f32", 2, 3, 256), colour=_new("u8", 3))
    add("train_crop_norm", "patch_empty", patch=(1, 1, 2, 2), norm=_new("f32", 2, 3, 256), colour=_new("u8", 3))
    add("train_disp_crop", "f32")
    add("train_disp_crop", "u16_flip", disp=_new("u16", 6, 10), flip_rows=True, scale=1.0 / 256, inf_to_zero=True)
    add("train_disp_crop", "edge", y1=2, x1=3, out_gt=_new("f32", 4, 7), out_mask=_new("b", 4, 7))
    # geometry: one frame, (8,12) or (1,1,8,12)
    for tag, pred in (("hw", _new("f32", H, W)), ("11hw", _new("f32", 1, 1, H, W))):
        for wtag, win in (("whole", None), ("win", WIN), ("edge", EDGE)):
            add("disp_to_depth", f"{tag}_{wtag}", pred=pred, window=win)
            add("disp_to_depth", f"{tag}_{wtag}_mask", pred=pred, window=win, mask=_like("pred"), mask_min=0.25)
            add("point_cloud", f"{tag}_{wtag}", pred=pred, window=win)
            add("point_cloud", f"{tag}_{wtag}_mask", pred=pred, window=win, mask=_like("pred"), mask_min=0.25)
    add("disp_to_depth", "u16", window=WIN, f32=False, u16=True, scale=100.0, min_disp=1.0, max_depth=50.0)
    add("disp_to_depth", "both", window=WIN, u16=True)
    add("disp_to_depth", "both_out", window=WIN, u16=True, out_f32=_new("f32", 5, 7), out_u16=_new("u16", 5, 7))
    add("point_cloud_tiles", "5x7")
    add("point_cloud_workspace", "5x7")
    for ch in (3, 4):
        add("point_cloud", f"rgb{ch}", window=WIN, v0=1, rgb=_new("u8", 6, 10, ch))
    add("point_cloud", "stride_cap", window=WIN, stride=2, cap=5)
    add("point_cloud", "cap0", window=WIN, cap=0)
    add("point_cloud", "out", window=WIN, out=_new("f32", 40, 4))
    add("point_cloud", "out_cap", window=WIN, out=_new("f32", 40, 4), cap=9)
    add("point_cloud", "workspace", window=WIN, workspace=lambda c, kw: (c.i32(2), c.i64(2)))
    add("point_cloud", "out_workspace", window=WIN, out=_new("f32", 35, 4), workspace=lambda c, kw: (c.i32(4), c.i64(2)))
    kinds = {"disp": "f32", "depth": "f32", "disp_u16": "u16", "count": "i64"}
    for names in _subsets(tuple(kinds), empty=False):
        add("lidar_disparity", "outputs_" + "_".join(names), outputs=names)
    add("lidar_disparity", "all_rows", n=None, occl=(0, 0, 0.2), min_depth=2.0, max_depth=90.0, min_disp=1.0, max_disp=100.0)
    add("lidar_disparity", "no_points", points=_new("f32", 0, 4), n=None)
    add("lidar_disparity", "out_workspace", outputs=tuple(kinds), workspace=_new("i32", H * W + 3),
        out=lambda c, kw: {k: getattr(c, v)(*((2,) if k == "count" else (H, W))) for k, v in kinds.items()})
    add("lidar_disparity", "out_some", outputs=("disp", "count"), out=lambda c, kw: {"disp": c.f32(H, W), "depth": c.f32(H, W)})
    add("speckle_workspace", "5x7")
    add("speckle_workspace", "5x7_b2", batch=2)
    for ltag, lay in _layouts("disp"):
        for wtag, win in (("whole", None), ("win", WIN), ("edge", EDGE)):
            add("speckle_filter", f"{ltag}_{wtag}", **lay, window=win)
            add("speckle_filter", f"{ltag}_{wtag}_mask", **lay, window=win, mask=_like("disp"), mask_min=0.25, fill=-1.0)
            add("median_filter", f"{ltag}_{wtag}", **lay, window=win)
            add("median_filter", f"{ltag}_{wtag}_mask5", **lay, window=win, mask=_like("disp"), mask_min=0.25, ksize=5)
            add("disp_range", f"{ltag}_{wtag}", **lay, window=win)
            add("disp_range", f"{ltag}_{wtag}_mask", **lay, window=win, mask=_like("disp"), mask_min=0.25)
    for names in _subsets(F.SPECKLE_OUTPUTS):
        add("speckle_filter", "outputs_" + "_".join(names), outputs=names)
    add("speckle_filter", "out_workspace", disp=_new("f32", 2, H, W), window=WIN, workspace=lambda c, kw: (c.i32(70), c.i32(75)),
        out=lambda c, kw: {"disp": c.f32(2, 5, 7), "valid": c.f32(2, 5, 7), "size": c.i32(2, 5, 7)})
    add("speckle_filter", "out_some", window=WIN, outputs=("size",), out=lambda c, kw: {"size": c.i32(5, 7), "disp": c.f32(5, 7)})
    add("median_filter", "out", disp=_new("f32", 2, 1, H, W), window=WIN, out=_new("f32", 2, 1, 5, 7))
    add("disp_error_image", "plain")
    add("disp_error_image", "b1hw_padded", pred=_new("f32", 2, 1, H + 2, W + 2), abs_thres=2.0, rel_thres=0.1, legend=False)
    add("disp_error_image", "u8", f32=False, u8=True)
    add("disp_error_image", "both", u8=True)
    add("disp_error_image", "both_out", u8=True, out_f32=_new("f32", 2, 3, H, W), out_u8=_new("u8", 2, H, W, 3))
    for tag, disp in (("hw", _new("f32", H, W)), ("11hw", _new("f32", 1, 1, H, W))):
        for wtag, (y0, rows, cols) in (("win", WIN), ("edge", EDGE), ("whole", (0, H, W))):
            add("disp_colorize", f"{tag}_{wtag}", disp=disp, y0=y0, rows=rows, cols=cols)
            add("disp_colorize", f"{tag}_{wtag}_mask", disp=disp, y0=y0, rows=rows, cols=cols, mask=_like("disp"), mask_min=0.25)
    add("disp_colorize", "range12", max_disp=None, range=_new("f32", 1, 2), cmap="gray")
    add("disp_colorize", "range2", max_disp=None, range=_new("f32", 2))
    add("disp_colorize", "out", out=_new("u8", 5, 7, 3))
    return out


def _tensors(v):
    """the tensors of a result or of an argument, named by their place in it"""
    if isinstance(v, torch.Tensor):
        yield "", v
    elif isinstance(v, dict):
        for k in sorted(v):
            for n, t in _tensors(v[k]):
                yield f"[{k}]{n}", t
    elif isinstance(v, (tuple, list)):
        for i, e in enumerate(v):
            for n, t in _tensors(e):
                yield f"[{i}]{n}", t


def _run(op, overrides, setattr_, real):
    """one traced call -> {"calls": the recorded sequence, "returns": per returned tensor [place, dtype, shape, the caller's
    buffer (a place in out* / workspace) whose storage it lives in or ""]}"""
    c = C.Factory("cuda")
    kw = C.arguments(c, op, overrides)
    rec = Recorder(real, forward=lambda name: name.endswith(HOST_QUERIES), sizes=())
    setattr_(F, "_L", lambda: rec)
    res = getattr(F, op)(**kw)
    if op == "selfsup_loss":
        res[0].backward()
        res = (res, [d.grad for d in kw["disps"]])
    given = {k + n: t.untyped_storage().data_ptr() for k, v in kw.items() if k.startswith("out") or k == "workspace"
             for n, t in _tensors(v)}
    returns = [[n, str(t.dtype), list(t.shape), next((k for k, p in given.items() if p == t.untyped_storage().data_ptr()), "")]
               for n, t in _tensors(res)]
    if not isinstance(res, (torch.Tensor, tuple, list, dict)):
        returns = [["", type(res).__name__, res, ""]]
    return {"calls": rec.calls, "returns": returns}


def _trace_all(setattr_):
    real = C._lib.load()
    return {cid: _run(op, ov, setattr_, real) for cid, op, ov in cases()}


@pytest.mark.gpu
def test_frame_ops_trace(monkeypatch):
    assert F.__name__.endswith("frame_ops")
    assert sorted({op for _, op, _ in cases()}) == C.public_functions()
    with open(GOLDEN_FILE) as f:
        golden = json.load(f)["cases"]
    got = json.loads(json.dumps(_trace_all(monkeypatch.setattr)))
    assert sorted(got) == sorted(golden)
    bad = [f"{cid}:\n    recorded {golden[cid]}\n    now      {got[cid]}" for cid in got if got[cid] != golden[cid]]
    assert not bad, f"{len(bad)} of {len(got)} calls changed:\n" + "\n".join(bad)


def record(commit):
    traces = _trace_all(setattr)
    with open(GOLDEN_FILE, "w") as f:
        json.dump({"recorded_on": commit, "cases": traces}, f, sort_keys=True, separators=(",", ":"))
        f.write("\n")
    print(len(traces), "cases,", sum(len(t["calls"]) for t in traces.values()), "calls,", os.path.getsize(GOLDEN_FILE), "bytes")


if __name__ == "__main__":
    if "--record" in sys.argv:
        record(sys.argv[sys.argv.index("--record") + 1])
