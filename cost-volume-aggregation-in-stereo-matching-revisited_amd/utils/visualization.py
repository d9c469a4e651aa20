"""Mirror of the reference's utils/visualization.py (the KITTI error map) plus the colour-coded disparity map.

`disp_error_image_func` / `disp_error_image`: tensors on the ROCm device go through ONE launch of csrc/visualize.hip
(`ops.disp_error_image`) and the image comes back as a device tensor; CPU tensors go through the numpy restatement below,
which follows the reference line by line (citations are utils/visualization.py of the reference tree) and equals it bit for
bit.  `disp_to_color` is the numpy restatement of `ops.disp_colorize` with a fixed range (include/dca_hip.h has the
definitions)."""
import numpy as np
import torch


def _package():
    from . import _package as find
    return find()


def _tables():
    """the tables of include/dca_hip.h: the ten colour rows, the devkit's edges and corners"""
    c = _package()._lib.CONSTANTS
    rgb = [c[f"DCA_ERRMAP_RGB_{i}"] for i in range(c["DCA_ERRMAP_BINS"])]
    edges = [c[f"DCA_KITTI_EDGE_{k}"] for k in range(8)]
    corners = [[(c["DCA_KITTI_CORNERS"] >> (4 * k + s)) & 1 for s in (2, 1, 0)] for k in range(8)]
    return (np.array([[(v >> 16) & 255, (v >> 8) & 255, v & 255] for v in rgb], dtype=np.float32),
            np.array(edges, dtype=np.float32), np.array(corners, dtype=np.float32))


def gen_error_colormap():
    """visualization.py:11-24: ten rows (lower edge, upper edge, r, g, b), the edges 2^-4 .. 2^4 around 0 and +inf, the
    colours as float32(byte) / 255"""
    rgb = _tables()[0]
    cols = np.zeros((rgb.shape[0], 5), dtype=np.float32)
    cols[1:, 0] = 2.0 ** np.arange(-4, 5)                    # 0.1875 / 3 = 1 / 16, ..., 48 / 3 = 16: exact
    cols[:-1, 1] = cols[1:, 0]
    cols[-1, 1] = np.inf
    cols[:, 2:5] = rgb
    cols[:, 2:5] /= 255.                                     # :23, a float32 division
    return cols


error_colormap = gen_error_colormap()


def _error_image_host(D_est_np, D_gt_np, abs_thres, rel_thres, legend=True):
    """visualization.py:34-55 on numpy arrays -> float32 (B,3,H,W)"""
    D_gt_np, D_est_np = np.asarray(D_gt_np, dtype=np.float32), np.asarray(D_est_np, dtype=np.float32)
    B, H, W = D_gt_np.shape
    mask = D_gt_np > 0                                                        # :36
    with np.errstate(all="ignore"):
        error = np.abs(D_gt_np - D_est_np)                                    # :38
        error[np.logical_not(mask)] = 0                                       # :39
        error[mask] = np.minimum(error[mask] / np.float32(abs_thres),
                                 (error[mask] / D_gt_np[mask]) / np.float32(rel_thres))      # :40
    cols = error_colormap
    error_image = np.zeros([B, H, W, 3], dtype=np.float32)                    # :44
    for i in range(cols.shape[0]):                                            # :45-46
        error_image[np.logical_and(error >= cols[i][0], error < cols[i][1])] = cols[i, 2:]
    error_image[np.logical_not(mask)] = 0.                                    # :49
    if legend:
        for i in range(cols.shape[0]):                                        # :51-53
            distance = 20
            error_image[:, :10, i * distance:(i + 1) * distance, :] = cols[i, 2:]
    return np.ascontiguousarray(error_image.transpose([0, 3, 1, 2]))          # :55


def disp_error_image(D_est, D_gt, abs_thres=3., rel_thres=0.05):
    """The KITTI error map of D_est against D_gt, both (B,H,W): float32 (B,3,H,W) in [0,1] with the colour key in the
    top-left corner, on the device of D_gt.  Device tensors: one HIP launch, no synchronisation (D_est may be the padded
    frame, rows on top and columns on the right: `ops.disp_error_image`); CPU tensors: numpy."""
    if isinstance(D_gt, torch.Tensor) and D_gt.is_cuda:
        return _package().ops.disp_error_image(D_est.detach(), D_gt.detach(), abs_thres, rel_thres)[0]
    est, gt = (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t) for t in (D_est, D_gt))
    if gt.ndim != 3 or est.shape != gt.shape:
        raise ValueError(f"disp_error_image: expected two (B,H,W) maps of one shape, got {est.shape} and {gt.shape}")
    return torch.from_numpy(_error_image_host(est, gt, abs_thres, rel_thres))


class disp_error_image_func:
    """The reference's class of this name (visualization.py:30-58), callable every way the reference's is:
    `disp_error_image_func.forward(None, est, gt)` (its old-style method), `disp_error_image_func()(est, gt)` and
    `disp_error_image_func.apply(est, gt)`.  The result carries no gradient (`backward` returns None, :57-58).
    `dilate_radius` is accepted and ignored, as in the reference (a TODO there, :47-48)."""

    def forward(self, D_est_tensor, D_gt_tensor, abs_thres=3., rel_thres=0.05, dilate_radius=1):
        return disp_error_image(D_est_tensor, D_gt_tensor, abs_thres, rel_thres)

    def backward(self, grad_output):
        return None

    def __call__(self, *args, **kwargs):
        return self.forward(*args, **kwargs)

    @classmethod
    def apply(cls, *args, **kwargs):
        return cls().forward(*args, **kwargs)


def disp_to_color(disp, max_disp, cmap="kitti"):
    """numpy restatement of `ops.disp_colorize(disp, ..., max_disp=max_disp, cmap=cmap)`: disp (...,H,W) -> uint8 (...,H,W,3).
    t = min(d / max(max_disp, 1e-5), 1) in float32; "kitti": the KITTI devkit's disp_to_color (eight corner colours, segment
    widths 114, 185, 114, 174, 114, 185, 114 of 1000); "gray": rint(t * 255) three times.  Pixels that are not finite or not
    > 0 are black."""
    if cmap not in ("kitti", "gray"):
        raise ValueError(f"disp_to_color: cmap is 'gray' or 'kitti', got {cmap!r}")
    if not 0.0 < float(max_disp) < np.inf:
        raise ValueError(f"disp_to_color: max_disp must be positive and finite, got {max_disp}")
    d = disp.detach().cpu().numpy() if isinstance(disp, torch.Tensor) else np.asarray(disp)
    d = d.astype(np.float32)
    f = np.float32
    with np.errstate(all="ignore"):
        ok = np.isfinite(d) & (d > 0)
        t = np.minimum(np.maximum((d - f(0)) / np.maximum(f(max_disp) - f(0), f(1e-5)), f(0)), f(1))
    t = np.where(ok, t, f(0)).astype(np.float32)
    if cmap == "gray":
        rgb = np.repeat(np.rint(t * f(255)).astype(np.uint8)[..., None], 3, axis=-1)
    else:
        _, C, corners = _tables()
        s = t * f(1000)
        ind = (s[..., None] > C[1:7]).sum(-1)
        w = ((s - C[ind]) / (C[ind + 1] - C[ind]))[..., None]
        a, z = corners[ind], corners[ind + 1]
        v = np.where(a == z, a, np.where(z > a, w, f(1) - w)).astype(np.float32)
        rgb = np.rint(v * f(255)).astype(np.uint8)
    rgb[~ok] = 0
    return rgb
