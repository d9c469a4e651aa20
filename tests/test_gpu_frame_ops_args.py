"""Every wrapper of frame_ops.py refuses a call with one thing wrong, by name, before it touches the library.

`frame_ops._L` is replaced by an object whose every attribute access fails the row.  A row of TABLE is (function, what is
wrong, overrides of the base arguments of tests/_frame_ops_cases.py, flags); it must raise RuntimeError (ValueError for
`cmap`) with a message that starts with the function's name.  Flags:
  new      the commit before the wrappers moved out of ops.py let the ValueError of the conversion through here (a
           malformed `window` of disp_to_depth, point_cloud and disp_range); every other row was refused there as well
  queries  `point_cloud` sizes its workspace with the host-side query dca_point_cloud_tiles before it can judge the buffers
           it was given: in these rows the stand-in answers that one query (no launch) and fails everything else
No kernel is launched.  The rows with a buffer on a second device need two GPUs and skip on a machine with one."""
import math
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import _frame_ops_cases as C  # noqa: E402
from _frame_ops_cases import F, H, W  # noqa: E402


class LibraryTouched(BaseException):
    pass


class NoLibrary:
    def __init__(self, queries=False):
        self._queries = queries

    def __getattr__(self, name):
        if self._queries and name == "dca_point_cloud_tiles":
            return getattr(C._lib.load(), name)
        raise LibraryTouched(name)


def cpu(key):
    return {key: lambda c, kw: kw[key].cpu()}


def dtype(key):
    return {key: lambda c, kw: kw[key].to(torch.float64 if kw[key].dtype != torch.float64 else torch.float32)}


def strided(key):
    """same shape and dtype, every second element of a buffer twice as wide"""
    return {key: lambda c, kw: c.t(kw[key].dtype, *kw[key].shape[:-1], 2 * kw[key].shape[-1])[..., ::2]}


def shape(key, *s):
    return {key: lambda c, kw: c.t(kw[key].dtype, *s)}


def new(key, kind, *s):
    return {key: lambda c, kw: getattr(c, kind)(*s)}


def grad(key):
    return {key: lambda c, kw: kw[key].requires_grad_()}


def _rows():
    rows = []

    def add(op, what, ov, *flags, expect=RuntimeError):
        rows.append((op, what, ov, expect, flags))

    def tensor(op, key, contiguous=True):
        add(op, f"{key} on the CPU", cpu(key))
        add(op, f"{key} of another dtype", dtype(key))
        if contiguous:
            add(op, f"{key} not contiguous", strided(key))

    tensor("disp_metrics", "pred", False), tensor("disp_metrics", "gt", False)
    add("disp_metrics", "mask on the CPU", {"mask": lambda c, kw: torch.zeros(2, H, W, dtype=torch.bool)})
    add("disp_metrics", "mask of another dtype", new("mask", "f32", 2, H, W))
    add("disp_metrics", "mask of another shape", new("mask", "b", 2, H, W - 1))
    add("disp_metrics", "pred smaller than gt", new("pred", "f32", 2, H - 1, W))
    tensor("region_confusion", "volumes", False), tensor("region_confusion", "gt", False)
    for key in ("state", "rec", "cm"):
        tensor("eval_accumulate", key)
    for key in ("conf", "pred", "gt"):
        tensor("conf_histogram", key, False)
    tensor("conf_histogram", "state")
    add("conf_histogram", "gt of another shape", new("gt", "f32", 2, H, W - 1))
    tensor("mirror_pair", "left"), tensor("mirror_pair", "right")
    add("mirror_pair", "right of another shape", new("right", "f32", H, W - 1))
    add("mirror_pair", "out of the wrong shape", new("out", "f32", 2, H, W - 1))
    add("mirror_pair", "out aliasing the input", {"left": lambda c, kw: c.f32(3, H, W)[2], "out": lambda c, kw: kw["left"]._base[:2]})
    add("mirror_pair", "left requires grad", grad("left"))
    tensor("lr_consistency", "disp_left"), tensor("lr_consistency", "disp_right_mirrored")
    add("lr_consistency", "maps of two shapes", new("disp_right_mirrored", "f32", 2, H, W - 1))
    add("lr_consistency", "unknown output", {"outputs": ("valid", "depth")})
    add("lr_consistency", "disp_left requires grad", grad("disp_left"))
    tensor("selfsup_loss", "left"), tensor("selfsup_loss", "right")
    add("selfsup_loss", "a map on the CPU", {"disps": lambda c, kw: [kw["disps"][0], torch.zeros(1, 4, 5)]})
    add("selfsup_loss", "a map of another dtype", {"disps": lambda c, kw: [kw["disps"][0], c.f64(1, 4, 5)]})
    add("selfsup_loss", "a map not contiguous", {"disps": lambda c, kw: [kw["disps"][0], c.f32(1, 4, 10)[..., ::2]]})
    add("selfsup_loss", "valid on the CPU", {"valid": lambda c, kw: torch.zeros(1, 4, 5)})
    add("selfsup_loss", "valid of another dtype", new("valid", "f64", 1, 4, 5))
    add("selfsup_loss", "valid of another shape", new("valid", "f32", 1, 4, 4))
    add("selfsup_loss", "valid not contiguous", {"valid": lambda c, kw: c.f32(1, 4, 10)[..., ::2]})
    for op in ("frame_histogram", "frame_apply", "rectify_pair", "train_luma_sum", "train_crop_norm"):
        tensor(op, "left_u8"), tensor(op, "right_u8")
        add(op, "images of two shapes", new("right_u8", "u8", 6, 9, 3))
        add(op, "images with two channels", {**new("left_u8", "u8", 6, 10, 2), **new("right_u8", "u8", 6, 10, 2)})
    tensor("frame_lut", "hist")
    add("frame_lut", "hist of the wrong shape", shape("hist", 2, 3, 255))
    tensor("frame_apply", "lut")
    add("frame_apply", "window one row too tall for the source", {"rows": 6})
    add("frame_apply", "window one row too tall for the frame", {"src_y0": 0, "dst_y0": 3, "rows": 6})
    add("frame_apply", "window one column too wide", {"cols": 11})
    add("frame_apply", "negative src_y0", {"src_y0": -1})
    add("frame_apply", "out of the wrong shape", new("out", "f32", 2, 3, H, W + 1))
    add("frame_apply", "out of another dtype", new("out", "f64", 2, 3, H, W))
    tensor("disp_export", "pred")
    add("disp_export", "window one row too tall", {"h": 7})
    add("disp_export", "window one column too wide", {"w": 13})
    add("disp_export", "negative y0", {"y0": -1})
    add("disp_export", "nothing to export", {"f32": False})
    add("disp_export", "out_f32 of the wrong shape", new("out_f32", "f32", 5, 8))
    add("disp_export", "out_u16 of another dtype", {"u16": True, **new("out_u16", "f32", 5, 7)})
    add("rectify_pair", "maps for another source", {"left_u8": lambda c, kw: c.u8(6, 11, 3), "right_u8": lambda c, kw: c.u8(6, 11, 3)})
    add("rectify_pair", "out of the wrong shape", new("out", "u8", 2, 5, 8, 3))
    add("rectify_pair", "out aliasing the input", {"left_u8": lambda c, kw: c.u8(400)[:180].view(6, 10, 3),
                                                   "out": lambda c, kw: (kw["left_u8"]._base[100:205].view(5, 7, 3), c.u8(5, 7, 3))})
    add("rectify_pair", "out[0] aliasing out[1]",
        {"out": lambda c, kw: (lambda b: (b[:105].view(5, 7, 3), b[50:155].view(5, 7, 3)))(c.u8(200))})
    tensor("train_luma_sum", "bg")
    add("train_luma_sum", "bg of the wrong shape", shape("bg", 2, 255))
    for key in ("S", "bg", "norm"):
        tensor("train_tables", key)
    tensor("train_patch_colour", "right_u8"), tensor("train_patch_colour", "U")
    add("train_patch_colour", "window one row too tall", {"th": 6})
    add("train_patch_colour", "window one column too wide", {"tw": 9})
    add("train_patch_colour", "negative y1", {"y1": -1})
    add("train_patch_colour", "negative x1", {"x1": -1})
    for key in ("T", "out_left", "out_right"):
        tensor("train_crop_norm", key)
    add("train_crop_norm", "out_right of the wrong shape", shape("out_right", 3, 3, 5))
    add("train_crop_norm", "window one row too tall", {"y1": 4})
    add("train_crop_norm", "window one column too wide", {"x1": 7})
    add("train_crop_norm", "negative y1", {"y1": -1})
    add("train_crop_norm", "patch leaves the crop", {"patch": (0, 4, 0, 1), **new("norm", "f32", 2, 3, 256), **new("colour", "u8", 3)})
    add("train_crop_norm", "patch without norm", {"patch": (0, 2, 0, 1)})
    add("train_disp_crop", "disp on the CPU", cpu("disp"))
    add("train_disp_crop", "disp of another dtype", dtype("disp"))
    add("train_disp_crop", "disp not contiguous", strided("disp"))
    tensor("train_disp_crop", "out_gt"), tensor("train_disp_crop", "out_mask")
    add("train_disp_crop", "out_mask of the wrong shape", shape("out_mask", 3, 5))
    add("train_disp_crop", "window one row too tall", {"y1": 4})
    add("train_disp_crop", "window one column too wide", {"x1": 7})
    add("train_disp_crop", "negative x1", {"x1": -1})
    # the map-plus-mask family: (function, the map's name, whether a malformed `window` is refused only since the move;
    # None: the window comes as y0, rows, cols)
    for op, key, window_new in (("disp_to_depth", "pred", True), ("point_cloud", "pred", True), ("speckle_filter", "disp", False),
                                ("median_filter", "disp", False), ("disp_range", "disp", True), ("disp_colorize", "disp", None)):
        tensor(op, key)
        mask = {"mask": lambda c, kw, key=key: torch.zeros_like(kw[key])}
        add(op, "mask on the CPU", {"mask": lambda c, kw, key=key: torch.zeros_like(kw[key]).cpu()})
        add(op, "mask of another dtype", {"mask": lambda c, kw, key=key: torch.zeros_like(kw[key], dtype=torch.float64)})
        add(op, "mask of another shape", {"mask": lambda c, kw, key=key: c.f32(*kw[key].shape[:-1], W - 1)})
        add(op, "mask not contiguous", {"mask": lambda c, kw, key=key: c.f32(*kw[key].shape[:-1], 2 * W)[..., ::2]})
        add(op, "NaN mask_min with a mask", {**mask, "mask_min": math.nan})
        add(op, f"{key} requires grad", grad(key))
        add(op, "mask requires grad", {"mask": lambda c, kw, key=key: torch.zeros_like(kw[key]).requires_grad_()})
        add(op, "empty map", new(key, "f32", 0, W))
        if window_new is None:
            add(op, "window one row too tall", {"rows": 7})
            add(op, "window one column too wide", {"cols": 13})
            add(op, "negative y0", {"y0": -1})
            add(op, "empty window", {"rows": 0})
        else:
            add(op, "window one row too tall", {"window": (2, 7, 7)})
            add(op, "window one column too wide", {"window": (2, 5, 13)})
            add(op, "negative y0", {"window": (-1, 5, 7)})
            add(op, "empty window", {"window": (2, 0, 7)})
            add(op, "window 'x'", {"window": "x"}, *(("new",) if window_new else ()))
            add(op, "window of two numbers", {"window": (2, 5)}, *(("new",) if window_new else ()))
    add("disp_to_depth", "two frames", new("pred", "f32", 2, H, W))
    add("disp_to_depth", "nothing to compute", {"f32": False})
    add("disp_to_depth", "out_f32 of the wrong shape", new("out_f32", "f32", H, W + 1))
    add("disp_to_depth", "out_u16 of another dtype", {"u16": True, **new("out_u16", "f32", H, W)})
    add("disp_to_depth", "NaN mask_min without a mask", {"mask_min": math.nan})
    add("point_cloud", "rgb on the CPU", {"window": (2, 5, 7), "rgb": lambda c, kw: torch.zeros(6, 10, 3, dtype=torch.uint8)})
    add("point_cloud", "rgb of another dtype", {"window": (2, 5, 7), **new("rgb", "f32", 6, 10, 3)})
    add("point_cloud", "rgb with two channels", {"window": (2, 5, 7), **new("rgb", "u8", 6, 10, 2)})
    add("point_cloud", "window one row too tall for rgb", {"window": (2, 5, 7), "v0": 2, **new("rgb", "u8", 6, 10, 3)})
    add("point_cloud", "window one column too wide for rgb", {"window": (2, 5, 7), **new("rgb", "u8", 6, 6, 3)})
    add("point_cloud", "out of the wrong shape", new("out", "f32", 40, 3), "queries")
    add("point_cloud", "out of another dtype", new("out", "f64", 40, 4), "queries")
    add("point_cloud", "cap beyond out", {"cap": 41, **new("out", "f32", 40, 4)}, "queries")
    add("point_cloud", "workspace one word short", {"window": (2, 5, 7), "workspace": lambda c, kw: (c.i32(1), c.i64(2))}, "queries")
    add("point_cloud", "workspace count of another dtype", {"workspace": lambda c, kw: (c.i32(2), c.i32(2))}, "queries")
    tensor("lidar_disparity", "points")
    add("lidar_disparity", "points require grad", grad("points"))
    add("lidar_disparity", "n beyond the points", {"n": 6})
    add("lidar_disparity", "unknown output", {"outputs": ("disp", "valid")})
    add("lidar_disparity", "out of the wrong shape", {"out": lambda c, kw: {"disp": c.f32(H, W + 1)}})
    add("lidar_disparity", "out of another dtype", {"out": lambda c, kw: {"disp": c.f64(H, W)}})
    add("lidar_disparity", "out with an unknown key", {"out": lambda c, kw: {"valid": c.f32(H, W)}})
    add("lidar_disparity", "workspace one word short", new("workspace", "i32", H * W - 1))
    add("lidar_disparity", "workspace of another dtype", new("workspace", "f32", H * W))
    add("speckle_filter", "unknown output", {"outputs": ("disp", "depth")})
    add("speckle_filter", "out of the wrong shape", {"out": lambda c, kw: {"disp": c.f32(H, W + 1)}})
    add("speckle_filter", "out of another dtype", {"out": lambda c, kw: {"size": c.f32(H, W)}})
    add("speckle_filter", "out with an unknown key", {"out": lambda c, kw: {"depth": c.f32(H, W)}})
    add("speckle_filter", "workspace one word short", {"workspace": lambda c, kw: (c.i32(H * W), c.i32(H * W - 1))})
    add("speckle_filter", "workspace of another dtype", {"workspace": lambda c, kw: (c.i32(H * W), c.f32(H * W))})
    add("speckle_filter", "workspace twice the same buffer", {"workspace": lambda c, kw: (lambda b: (b, b))(c.i32(H * W))})
    add("speckle_filter", "negative max_size", {"max_size": -1})
    add("median_filter", "ksize 4", {"ksize": 4})
    add("median_filter", "out of the wrong shape", new("out", "f32", H, W + 1))
    add("median_filter", "out aliasing the input", {"out": lambda c, kw: kw["disp"]})
    tensor("disp_error_image", "pred", False), tensor("disp_error_image", "gt", False)
    add("disp_error_image", "pred smaller than gt", new("pred", "f32", 2, H, W - 1))
    add("disp_error_image", "nothing to compute", {"f32": False})
    add("disp_error_image", "out_f32 of the wrong shape", new("out_f32", "f32", 2, 3, H, W + 1))
    add("disp_error_image", "out_u8 of another dtype", {"u8": True, **new("out_u8", "f32", 2, H, W, 3)})
    add("disp_colorize", "two frames", new("disp", "f32", 2, H, W))
    add("disp_colorize", "unknown cmap", {"cmap": "jet"}, expect=ValueError)
    add("disp_colorize", "max_disp and range", new("range", "f32", 2))
    add("disp_colorize", "range on the CPU", {"max_disp": None, "range": lambda c, kw: torch.zeros(2)})
    add("disp_colorize", "range of three", {"max_disp": None, **new("range", "f32", 3)})
    add("disp_colorize", "out of the wrong shape", new("out", "u8", 5, 7, 4))
    add("disp_colorize", "out of another dtype", new("out", "f32", 5, 7, 3))
    return rows


TABLE = _rows()

# a caller's buffer on another device than the input: (function, overrides with the factory of the second device)
OTHER_DEVICE = [
    ("mirror_pair", lambda o: {"out": o.f32(2, H, W)}),
    ("frame_apply", lambda o: {"out": o.f32(2, 3, H, W)}),
    ("disp_export", lambda o: {"out_f32": o.f32(5, 7)}),
    ("disp_export", lambda o: {"u16": True, "out_u16": o.u16(5, 7)}),
    ("rectify_pair", lambda o: {"out": o.u8(2, 5, 7, 3)}),
    ("train_crop_norm", lambda o: {"out_left": o.f32(3, 3, 4)}),
    ("train_crop_norm", lambda o: {"out_right": o.f32(3, 3, 4)}),
    ("train_disp_crop", lambda o: {"out_gt": o.f32(3, 4)}),
    ("train_disp_crop", lambda o: {"out_mask": o.b(3, 4)}),
    ("disp_to_depth", lambda o: {"out_f32": o.f32(H, W)}),
    ("disp_to_depth", lambda o: {"u16": True, "out_u16": o.u16(H, W)}),
    ("point_cloud", lambda o: {"out": o.f32(96, 4)}),
    ("point_cloud", lambda o: {"workspace": (o.i32(2), o.i64(2))}),
    ("lidar_disparity", lambda o: {"out": {"disp": o.f32(H, W)}}),
    ("lidar_disparity", lambda o: {"workspace": o.i32(H * W)}),
    ("speckle_filter", lambda o: {"out": {"valid": o.f32(H, W)}}),
    ("speckle_filter", lambda o: {"workspace": (o.i32(H * W), o.i32(H * W))}),
    ("median_filter", lambda o: {"out": o.f32(H, W)}),
    ("disp_error_image", lambda o: {"out_f32": o.f32(2, 3, H, W)}),
    ("disp_error_image", lambda o: {"u8": True, "out_u8": o.u8(2, H, W, 3)}),
    ("disp_colorize", lambda o: {"out": o.u8(5, 7, 3)}),
]


def outcome(op, overrides, expect, queries, setattr_):
    """"" for a call refused as it should be, else what happened instead"""
    kw = C.arguments(C.Factory("cuda:0"), op, overrides)
    setattr_(F, "_L", lambda: NoLibrary(queries))
    try:
        getattr(F, op)(**kw)
    except expect as e:
        return "" if str(e).startswith(op) else f"refused without the function's name: {e}"
    except LibraryTouched as e:
        return f"reached the library ({e}) before any refusal"
    except Exception as e:
        return f"raised {type(e).__name__}: {e}"
    return "was accepted"


def run_table(setattr_):
    return [(op, what, flags, outcome(op, ov, expect, "queries" in flags, setattr_)) for op, what, ov, expect, flags in TABLE]


@pytest.mark.gpu
def test_one_thing_wrong_is_refused_by_name_before_the_library(monkeypatch):
    assert {op for op, *_ in TABLE} <= set(C.public_functions())
    bad = [f"{op}, {what}: {res}" for op, what, _, res in run_table(monkeypatch.setattr) if res]
    assert not bad, f"{len(bad)} of {len(TABLE)} rows:\n" + "\n".join(bad)


@pytest.mark.gpu
@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="a buffer on a second device needs two GPUs")
def test_a_buffer_on_another_device_is_refused(monkeypatch):
    other = C.Factory("cuda:1")
    bad = [f"{op} {sorted(ov(other))}: {res}" for op, ov in OTHER_DEVICE
           for res in [outcome(op, ov(other), RuntimeError, op == "point_cloud", monkeypatch.setattr)] if res]
    assert not bad, "\n".join(bad)


if __name__ == "__main__":          # every row's outcome, one per line (used once on the commit before the move)
    for op, what, flags, res in run_table(setattr):
        print(f"{op:20s} {what:45s} {' '.join(flags):8s} {res or 'refused'}")
