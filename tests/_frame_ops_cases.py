"""Arguments for the wrappers of frame_ops.py, shared by test_gpu_frame_ops_trace.py and test_gpu_frame_ops_args.py.

`base(c, op)` gives, for the public function `op`, the keyword arguments of one small accepted call; a case is (function,
overrides): the base call with some arguments replaced.  An override is a value, or a callable (c, kw) -> value that builds
a fresh tensor with the factory `c` or refers to the base arguments `kw` (for a buffer that aliases an input).  Shapes: maps 8 x 12,
uint8 images 6 x 10, the windows (2, 5, 7) and (3, 5, 12), which touches the last row and column, points (5,4) with n = 3,
images (1,3,4,5) with two disparity levels for the self-supervised loss."""
import inspect

import numpy as np
import torch

import dcanet_amd  # noqa: F401
from dcanet_amd import _lib, geometry

try:
    from dcanet_amd import frame_ops as F
except ImportError:              # the commit before the move, on which the golden trace was recorded: they were in ops.py
    from dcanet_amd import ops as F

H, W = 8, 12
WIN, EDGE = (2, 5, 7), (3, 5, 12)
CALIB = geometry.StereoCalib(721.5, 0.54, 6.0, 4.0)
LIDAR = geometry.LidarCalib(np.array([[700.0, 0, 6, 0], [0, 700.0, 4, 0], [0, 0, 1, 0]]), CALIB, (H, W))


class Factory:
    """zero tensors on one device"""

    def __init__(self, dev):
        self.dev = torch.device(dev)

    def t(self, dtype, *shape):
        if dtype == torch.uint16:            # as the wrappers make theirs: torch has few kernels for the type
            return torch.empty(shape, dtype=dtype, device=self.dev)
        return torch.zeros(shape, dtype=dtype, device=self.dev)

    def f32(self, *s): return self.t(torch.float32, *s)
    def f64(self, *s): return self.t(torch.float64, *s)
    def u8(self, *s): return self.t(torch.uint8, *s)
    def u16(self, *s): return self.t(torch.uint16, *s)
    def i32(self, *s): return self.t(torch.int32, *s)
    def i64(self, *s): return self.t(torch.int64, *s)
    def b(self, *s): return self.t(torch.bool, *s)

    def maps(self):
        z = np.zeros((2, 5, 7), np.int32)
        return geometry.RectifyMaps.from_fixed(z, z, (6, 10))


def base(c, op):
    img = lambda ch=3: dict(left_u8=c.u8(6, 10, ch), right_u8=c.u8(6, 10, ch))
    return {
        "disp_metrics": lambda: dict(pred=c.f32(2, H, W), gt=c.f32(2, H, W), maxdisp=192),
        "region_confusion": lambda: dict(volumes=c.f32(2, 3, 1, 2), gt=c.f32(2, 8, 16)),
        "eval_state": lambda: dict(num_classes=3, device=c.dev),
        "eval_accumulate": lambda: dict(state=c.f64(_lib.load().dca_eval_state_len(3)), rec=c.f64(2, F.EVAL_REC),
                                        cm=c.i64(1, 3, 3), gt_shape=(2, 8, 16)),
        "conf_histogram": lambda: dict(conf=c.f32(2, H, W), pred=c.f32(2, H, W), gt=c.f32(2, H, W), state=c.i64(4, 3), maxdisp=192),
        "mirror_pair": lambda: dict(left=c.f32(H, W), right=c.f32(H, W)),
        "lr_consistency": lambda: dict(disp_left=c.f32(2, H, W), disp_right_mirrored=c.f32(2, H, W)),
        "selfsup_loss": lambda: dict(left=c.f32(1, 3, 4, 5), right=c.f32(1, 3, 4, 5), weights=(1.0, 0.5),
                                     disps=[c.f32(1, 4, 5).requires_grad_(), c.f32(1, 1, 4, 5).requires_grad_()]),
        "frame_histogram": lambda: img(),
        "frame_lut": lambda: dict(hist=c.i32(2, 3, 256), n_pixels=60),
        "frame_apply": lambda: dict(**img(), lut=c.f32(2, 3, 256), frame_hw=(H, W), src_y0=1, dst_y0=2, rows=5, cols=7),
        "disp_export": lambda: dict(pred=c.f32(H, W), y0=2, h=5, w=7),
        "rectify_pair": lambda: dict(**img(), maps=c.maps()),
        "train_luma_sum": lambda: dict(**img(), bg=c.u8(2, 256)),
        "train_tables": lambda: dict(S=c.i64(2), n_pixels=60, bg=c.u8(2, 256), contrast=(1.1, 0.9), norm=c.f32(2, 3, 256)),
        "train_patch_colour": lambda: dict(right_u8=c.u8(6, 10, 3), U=c.u8(2, 256), y1=1, x1=2, th=3, tw=4),
        "train_crop_norm": lambda: dict(**img(), T=c.f32(2, 3, 256), y1=1, x1=2, out_left=c.f32(3, 3, 4), out_right=c.f32(3, 3, 4)),
        "train_disp_crop": lambda: dict(disp=c.f32(6, 10), y1=1, x1=2, maxdisp=192, out_gt=c.f32(3, 4), out_mask=c.b(3, 4)),
        "disp_to_depth": lambda: dict(pred=c.f32(H, W), calib=CALIB),
        "point_cloud_tiles": lambda: dict(rows=5, cols=7),
        "point_cloud_workspace": lambda: dict(rows=5, cols=7, device=c.dev),
        "point_cloud": lambda: dict(pred=c.f32(H, W), calib=CALIB),
        "lidar_disparity": lambda: dict(points=c.f32(5, 4), calib=LIDAR, n=3),
        "speckle_workspace": lambda: dict(rows=5, cols=7, device=c.dev),
        "speckle_filter": lambda: dict(disp=c.f32(H, W), max_size=3, max_diff=1.0),
        "median_filter": lambda: dict(disp=c.f32(H, W), ksize=3),
        "disp_error_image": lambda: dict(pred=c.f32(2, H, W), gt=c.f32(2, H, W)),
        "disp_range": lambda: dict(disp=c.f32(2, H, W)),
        "disp_colorize": lambda: dict(disp=c.f32(H, W), y0=2, rows=5, cols=7, max_disp=64.0),
    }[op]()


def arguments(c, op, overrides):
    """the keyword arguments of the base call of `op` with `overrides` applied"""
    kw = base(c, op)
    for k, v in overrides.items():
        kw[k] = v(c, kw) if callable(v) else v
    return kw


def public_functions():
    """the names of the public functions that the module defines itself"""
    return sorted(n for n, f in vars(F).items()
                  if inspect.isfunction(f) and not n.startswith("_") and f.__module__ == F.__name__)
