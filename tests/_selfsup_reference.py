"""The self-supervised loss of DESIGN.md section 6h (include/dca_hip.h, dca_selfsup_loss_fwd) restated in plain torch --
gather, avg_pool2d(3, 1) and autograd, usable in float64 and float32, on any device -- and the seeded scenes the tests
run it on.  The restatement is the yardstick of tests/test_gpu_selfsup.py: in float64 it is the truth, in float32 on the
same scene it is the error a straightforward implementation makes.

A scene keeps every pixel away from every kink of the loss (where the gradient jumps and a comparison of gradients
would depend on which side rounding falls): `margins` reports, per scene, the smallest distance of
  frac:   frac(xs) to 0 or 1                      (the interpolation changes its pair of samples)
  border: xs to 0 or W-1                          (in view / clamped)
  l1:     |I_c - Y_c| to 0
  ssim:   (1 - SSIM_c) / 2 to 0 or 1              (the clamp)
  dd:     neighbour disparity differences to 0    (the smoothness term's |.|)
Disparities are drawn as d = k + f with an integer -W//8 <= k <= W//2 and f in [1/8, 7/8], so `frac` and `border` hold
by construction; pixels that offend one of the others are redrawn from the scene's own generator until every margin is
at least MARGIN.  No pixel is excused."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

MARGIN = 1e-3
ALPHA, LAM, C1, C2 = 0.85, 0.1, 1e-4, 9e-4
WEIGHTS = (1.8, 2.1, 0.7)                       # the first L of them
# (B, H, W, L): one interior row; two samples, two levels; crosses the 16 x 64 tile edges both ways; three levels, three tile columns
SHAPES = ((1, 3, 5, 1), (2, 7, 37, 2), (1, 19, 70, 2), (2, 33, 130, 3))
TRAIN_SHAPE = (2, 256, 512, 2)


def warp_row(R, d):
    """R (B,3,H,W), d (B,H,W) -> (Y (B,3,H,W), inview (B,H,W) bool, xs (B,H,W)): the warp along the row"""
    B, C, H, W = R.shape
    x = torch.arange(W, dtype=d.dtype, device=d.device).view(1, 1, W)
    xs = x - d
    xc = xs.clamp(0, W - 1)
    x0 = xc.detach().floor().clamp(max=W - 2)
    t = (xc - x0).unsqueeze(1)
    idx = x0.long().unsqueeze(1).expand(B, C, H, W)
    r0, r1 = R.gather(3, idx), R.gather(3, idx + 1)
    return r0 + t * (r1 - r0), (xs >= 0) & (xs <= W - 1), xs


def ssim_interior(I, Y, c1=C1, c2=C2):
    """(B,3,H-2,W-2): SSIM of the 3x3 windows around the interior pixels, no padding"""
    mu_i, mu_y = F.avg_pool2d(I, 3, 1), F.avg_pool2d(Y, 3, 1)
    var_i = F.avg_pool2d(I * I, 3, 1) - mu_i * mu_i
    var_y = F.avg_pool2d(Y * Y, 3, 1) - mu_y * mu_y
    cov = F.avg_pool2d(I * Y, 3, 1) - mu_i * mu_y
    return ((2 * mu_i * mu_y + c1) * (2 * cov + c2)) / ((mu_i * mu_i + mu_y * mu_y + c1) * (var_i + var_y + c2))


def smoothness(d, I):
    """the reference's util.py:76-86 on d (B,H,W), I (B,3,H,W)"""
    d = d.unsqueeze(1)
    wx = torch.exp(-(I[:, :, :, :-1] - I[:, :, :, 1:]).abs().mean(1, keepdim=True))
    wy = torch.exp(-(I[:, :, :-1, :] - I[:, :, 1:, :]).abs().mean(1, keepdim=True))
    num = ((d[:, :, :, :-1] - d[:, :, :, 1:]).abs() * wx).sum() + ((d[:, :, :-1, :] - d[:, :, 1:, :]).abs() * wy).sum()
    return num / (wx.sum() + wy.sum())


def level_terms(I, R, d, valid=None, alpha=ALPHA, c1=C1, c2=C2):
    """(photo, smooth, sum M) of one level, 0-dim tensors of d's dtype"""
    d = d.reshape(d.shape[0], d.shape[-2], d.shape[-1])
    Y, inview, _ = warp_row(R, d)
    S = ssim_interior(I, Y, c1, c2)
    e = alpha * ((1 - S) / 2).clamp(0, 1).mean(1) + (1 - alpha) * (I - Y).abs().mean(1)[:, 1:-1, 1:-1]
    M = inview[:, 1:-1, 1:-1].to(d.dtype)
    if valid is not None:
        M = M * valid.reshape(d.shape)[:, 1:-1, 1:-1].to(d.dtype)
    sum_m = M.sum()
    return (M * e).sum() / sum_m.clamp(min=1), smoothness(d, I), sum_m


def selfsup_reference(I, R, disps, weights, valid=None, alpha=ALPHA, lam=LAM, c1=C1, c2=C2, dtype=torch.float64):
    """-> (loss, (L,3) per-level photo / smooth / sum M), computed in `dtype` from inputs of any float dtype; the loss
    keeps its graph to `disps` when they are already of `dtype` (or through the cast otherwise)"""
    I, R = I.to(dtype), R.to(dtype)
    total, rows = 0, []
    for d, w in zip(disps, weights):
        photo, smooth, sum_m = level_terms(I, R, d.to(dtype), valid, alpha, c1, c2)
        total = total + w * (photo + lam * smooth)
        rows.append(torch.stack([photo.detach(), smooth.detach(), sum_m.detach()]))
    return total, torch.stack(rows)


def reference_grads(I, R, disps, weights, valid=None, alpha=ALPHA, lam=LAM, c1=C1, c2=C2, dtype=torch.float64):
    """-> (loss, stats, [d loss / d d_l]) with everything evaluated in `dtype`"""
    ds = [d.detach().to(dtype).requires_grad_() for d in disps]
    loss, stats = selfsup_reference(I, R, ds, weights, valid, alpha, lam, c1, c2, dtype)
    grads = torch.autograd.grad(loss, ds)
    return loss.detach(), stats, list(grads)


# ---- scenes ----------------------------------------------------------------------------------------------------------------
def _texture(rs, B, H, W):
    """(B,3,H,W) float32: a few plane waves plus noise, about the range of a normalised image"""
    y, x = np.arange(H, dtype=np.float64)[:, None], np.arange(W, dtype=np.float64)[None, :]
    out = np.zeros((B, 3, H, W))
    for b in range(B):
        for c in range(3):
            for _ in range(4):
                fy, fx, ph, amp = rs.uniform(-0.9, 0.9), rs.uniform(-0.9, 0.9), rs.uniform(0, 2 * np.pi), rs.uniform(0.2, 0.8)
                out[b, c] += amp * np.sin(fy * y + fx * x + ph)
    return (out + 0.3 * rs.standard_normal(out.shape)).astype(np.float32)


def _draw(rs, n, W):
    return (rs.randint(-(W // 8), W // 2 + 1, n) + rs.uniform(0.125, 0.875, n)).astype(np.float32)


def margins(I, R, d, c1=C1, c2=C2):
    """per-pixel distances to the kinks, float64 numpy (B,H,W) each (inf where a kink does not apply to the pixel), for
    float32 numpy inputs I, R (B,3,H,W) and d (B,H,W)"""
    It, Rt, dt = (torch.from_numpy(np.asarray(a)).double() for a in (I, R, d))
    B, H, W = dt.shape
    Y, _, xs = warp_row(Rt, dt)
    fr = xs - xs.floor()
    out = {"frac": torch.minimum(fr, 1 - fr), "border": torch.minimum(xs.abs(), (xs - (W - 1)).abs()),
           "l1": (It - Y).abs().amin(1)}
    h = (1 - ssim_interior(It, Y, c1, c2)) / 2
    ssim = torch.full((B, H, W), float("inf"), dtype=torch.float64)
    ssim[:, 1:-1, 1:-1] = torch.minimum(h.abs(), (h - 1).abs()).amin(1)
    out["ssim"] = ssim
    dd = torch.full((B, H, W), float("inf"), dtype=torch.float64)
    dx, dy = (dt[:, :, :-1] - dt[:, :, 1:]).abs(), (dt[:, :-1, :] - dt[:, 1:, :]).abs()
    dd[:, :, :-1] = torch.minimum(dd[:, :, :-1], dx)
    dd[:, :, 1:] = torch.minimum(dd[:, :, 1:], dx)
    dd[:, :-1, :] = torch.minimum(dd[:, :-1, :], dy)
    dd[:, 1:, :] = torch.minimum(dd[:, 1:, :], dy)
    out["dd"] = dd
    return {k: v.numpy() for k, v in out.items()}


def kept_share(d, valid=None):
    """sum M over the interior pixel count for a numpy disparity map (B,H,W)"""
    B, H, W = d.shape
    xs = np.arange(W, dtype=np.float64)[None, None, :] - d.astype(np.float64)
    m = ((xs >= 0) & (xs <= W - 1)).astype(np.float64)
    if valid is not None:
        m = m * valid
    return float(m[:, 1:-1, 1:-1].sum() / (B * (H - 2) * (W - 2)))


@functools.lru_cache(maxsize=None)
def scene(shape, seed=0):
    """-> dict of numpy arrays: left, right (B,3,H,W) float32; disps: L maps (B,H,W) float32; valid (B,H,W) float32 of
    0 / 1 (four pixels in five kept); margins: {kink: smallest distance over all levels}; kept: per level the share of
    interior pixels kept (without valid, with valid).  Deterministic in (shape, seed); do not modify what it returns."""
    B, H, W, L = shape
    for attempt in range(64):
        rs = np.random.RandomState(1000003 * seed + 7919 * attempt + 31 * (H * W + L) + B)
        left, right = _texture(rs, B, H, W), _texture(rs, B, H, W)
        valid = (rs.uniform(size=(B, H, W)) < 0.8).astype(np.float32)
        disps, least = [], {}
        for _ in range(L):
            d = _draw(rs, B * H * W, W).reshape(B, H, W)
            for _ in range(400):
                m = margins(left, right, d)
                bad = np.zeros((B, H, W), bool)
                for v in m.values():
                    bad |= v < MARGIN
                if not bad.any():
                    break
                d[bad] = _draw(rs, int(bad.sum()), W)
            else:
                raise RuntimeError(f"scene {shape}: the redraws did not clear every kink")
            disps.append(d)
            for k, v in m.items():
                least[k] = min(least.get(k, np.inf), float(v.min()))
        kept = [(kept_share(d), kept_share(d, valid)) for d in disps]
        if all(0.3 <= s <= 0.9 for pair in kept for s in pair):
            return {"left": left, "right": right, "disps": disps, "valid": valid, "margins": least, "kept": kept}
    raise RuntimeError(f"scene {shape}: no attempt kept between 0.3 and 0.9 of the interior pixels")


def to_torch(sc, device="cpu"):
    """(left, right, [disps], valid) of a scene as float32 tensors on `device`"""
    t = lambda a: torch.from_numpy(a).to(device)
    return t(sc["left"]), t(sc["right"]), [t(d) for d in sc["disps"]], t(sc["valid"])
