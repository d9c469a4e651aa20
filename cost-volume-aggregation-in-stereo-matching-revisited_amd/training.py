"""The training step's input side and bookkeeping without per-pixel host arithmetic and without a host round trip per
step: the reference's loaders after the decode (dataloader/datasets.py:221-254 SceneFlow, :270-317 KITTI; the ETH3D
and Middlebury classes repeat the KITTI body; the one used for Middlebury, datasets.py:547-673, halves the pair and the ground
truth first: `downscale=2` here) and its `train()` (main_dca.py:122-141, train_kitti.py:92-120).

The loaders run three full-image PIL enhancer passes per image (brightness, gamma, contrast), crop, paint an occlusion
patch into one right crop in five, apply ToTensor + Normalize and hand two fp32 crops to the upload.  Each enhancer maps a
byte to a byte, so their composition is ONE 256-entry table per image; the only value that depends on the pixels is the
contrast mean, an exact integer sum.  This module restates every step in numpy (`host_sample`: the `device_io=False`
path and the yardstick of the GPU tests) and `TrainInput(device_io=True)` runs the same steps as HIP kernels
(csrc/train_io.hip) on the uint8 pair and the raw disparity as the decoder delivered them.

`SelfSupStep` is a training step WITHOUT ground truth (no counterpart in the reference): the
supervised losses are replaced by `models.loss.PhotometricLoss` on the image pair.

`train()` indexes with the mask for the EPE (a device-to-host stall) and calls `.item()` twice; `TrainStep` keeps
[steps, sum loss, sum epe, sum #mask] in a device fp64 state and synchronises only in `result()`.

Randomness stays on the host: `draw_kitti` / `draw_sceneflow` consume the generators in the reference's order and return
an `AugParams`; everything after that is deterministic given the parameters.  File listing and decoding (PNG / PFM) are
not part of this package."""
from __future__ import annotations

import dataclasses
import random as _pyrandom
from typing import Optional, Tuple

import numpy as np
import torch

from .evaluation import all_reduce_state  # noqa: F401  (same contract: every entry of the state is a sum)
from .inference import imagenet_lut

STEPS, SUM_LOSS, SUM_EPE, PIXELS = 0, 1, 2, 3      # TrainStep.state
SS_STEPS, SS_LOSS, SS_PHOTO, SS_SMOOTH, SS_KEPT = 0, 1, 2, 3, 4      # SelfSupStep.state


# ---- byte tables -------------------------------------------------------------------------------------------------------
def blend_table(c: int, f: float) -> np.ndarray:
    """PIL's `Image.blend(constant image c, image, f)` (Blend.c) as a table over the image's byte value v, which is what
    ImageEnhance's `enhance(f)` computes: in fp32, product then sum, t = c + f * (v - c); for 0 <= f <= 1 the result is t
    truncated, otherwise 0 for t <= 0, 255 for t >= 255 and truncation in between.  Restated operation for operation by
    the `train_tables` kernel."""
    f32 = np.float32(f)
    if not np.isfinite(f32):
        raise ValueError(f"blend factor {f}")
    v = np.arange(256, dtype=np.int64)
    t = np.float32(int(c)) + f32 * (v - int(c)).astype(np.float32)
    assert t.dtype == np.float32
    out = np.trunc(t).astype(np.int64)
    if not 0 <= f32 <= 1:
        out = np.where(t <= 0, 0, np.where(t >= 255, 255, out))
    return out.astype(np.uint8)


def brightness_table(f: float) -> np.ndarray:
    """ImageEnhance.Brightness(img).enhance(f) = torchvision's PIL adjust_brightness (datasets.py:285): blend with black."""
    return blend_table(0, f)


def gamma_table(gamma: float, gain: float = 1.0) -> np.ndarray:
    """torchvision's PIL `adjust_gamma` (transforms/_functional_pil.py; called at datasets.py:286): the image goes through
    `img.point([int((255 + 1 - 1e-3) * gain * pow(v / 255.0, gamma)) for v in range(256)] * 3)`, in Python floats.
    torchvision is no dependency of this package: the formula is restated here, and `TrainInput(gamma_table=...)` takes
    another one.  Entries are clipped to a byte (gain 1 never leaves it)."""
    gamma, gain = float(gamma), float(gain)
    return np.array([min(255, max(0, int((255 + 1 - 1e-3) * gain * pow(v / 255.0, gamma)))) for v in range(256)], np.uint8)


def contrast_table(mean: int, f: float) -> np.ndarray:
    """ImageEnhance.Contrast(img).enhance(f) = adjust_contrast (datasets.py:287): blend with the constant image `mean`."""
    return blend_table(mean, f)


def luma_plane(img: np.ndarray, bg: Optional[np.ndarray] = None) -> np.ndarray:
    """PIL's convert("L") of an (H,W,>=3) uint8 image (Convert.c rgb2l), after the byte table bg when given."""
    p = np.asarray(img)[:, :, :3]
    p = (p if bg is None else np.asarray(bg)[p]).astype(np.int64)
    return ((19595 * p[:, :, 0] + 38470 * p[:, :, 1] + 7471 * p[:, :, 2] + 32768) >> 16).astype(np.uint8)


def luma_sum(img: np.ndarray, bg: Optional[np.ndarray] = None) -> int:
    """Sum of `luma_plane` as a Python int (the `train_luma_sum` kernel)."""
    return int(luma_plane(img, bg).astype(np.int64).sum())


def contrast_mean(S: int, n: int) -> int:
    """ImageEnhance.Contrast: int(ImageStat.Stat(img.convert("L")).mean[0] + 0.5), the mean being sum / count in fp64."""
    return int(float(S) / float(n) + 0.5)


def patch_bytes(crop: np.ndarray) -> np.ndarray:
    """The occlusion patch's colour (datasets.py:306): `np.mean(np.mean(right_img, 0), 0)` assigned into the uint8 crop,
    i.e. per channel the mean truncated; here floor(sum / (th tw)) in integers (the `train_patch_colour` kernel): the
    EXACT mean is followed.  The loader's fp64 mean of column means equals it whenever th is a power of two (the column
    means k / th are exact: the reference's 256 x 512 crop) and whenever the exact mean is no integer.  At other heights
    a crop whose channel sum is a multiple of th tw (about one crop in th tw) can come out just below the integer in the
    loader's arithmetic and truncate to one less (tests/test_train_io_cpu.py)."""
    crop = np.asarray(crop)[:, :, :3]
    return (crop.reshape(-1, 3).astype(np.int64).sum(0) // (crop.shape[0] * crop.shape[1])).astype(np.uint8)


def crop_disparity(disp, y1, x1, th, tw, maxdisp, flip_rows=False, scale=1.0, inf_to_zero=False):
    """Ground-truth crop and mask (the `train_disp_crop` kernel): disp (H,W) float32 or uint16; flip_rows: a bottom-up
    PFM payload (the reference's readPFM flips it); scale: 1, or 1/256 for KITTI PNGs (datasets.py:308, exact in fp32);
    inf_to_zero: the Middlebury loaders (datasets.py:459).  Returns (gt (th,tw) float32, mask (th,tw) bool) with
    mask = gt > 0 & gt < maxdisp (main_dca.py:127)."""
    d = np.asarray(disp)
    if d.ndim != 2 or d.dtype not in (np.float32, np.uint16):
        raise ValueError(f"expected an (H,W) float32 or uint16 disparity, got {d.dtype} {d.shape}")
    if flip_rows:
        d = d[::-1]
    if min(y1, x1) < 0 or y1 + th > d.shape[0] or x1 + tw > d.shape[1]:
        raise ValueError(f"the {th} x {tw} window at ({y1}, {x1}) does not fit the {d.shape[0]} x {d.shape[1]} disparity")
    g = d[y1:y1 + th, x1:x1 + tw].astype(np.float32)              # a copy
    if d.dtype == np.uint16 or np.float32(scale) != 1:
        g = g * np.float32(scale)
    if inf_to_zero:
        g[g == np.inf] = 0
    with np.errstate(invalid="ignore"):
        mask = (g > 0) & (g < np.float32(maxdisp))
    return g, mask


# ---- the draws ---------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class AugParams:
    """What a loader draws for one sample: the crop corner, the photometric factors of (left, right) and the occlusion
    patch as (r0, r1, c0, c1) -- rows r0:r1, columns c0:c1 of the right crop -- or None."""
    x1: int
    y1: int
    brightness: Tuple[float, float] = (1.0, 1.0)
    gamma: Tuple[float, float] = (1.0, 1.0)
    contrast: Tuple[float, float] = (1.0, 1.0)
    patch: Optional[Tuple[int, int, int, int]] = None


def draw_sceneflow(w, h, crop=(256, 512), py_random=_pyrandom) -> AugParams:
    """datasets.py:235-236: `random.randint` for x1, then for y1; the SceneFlow loader has no photometric augmentation."""
    th, tw = crop
    x1 = py_random.randint(0, w - tw)
    y1 = py_random.randint(0, h - th)
    return AugParams(x1, y1)


def draw_kitti(w, h, crop=(256, 512), np_random=np.random, py_random=_pyrandom) -> AugParams:
    """datasets.py:282-306 in the order the generators are consumed: np uniform x3 of size 2 (brightness [0.5,2], gamma
    and contrast [0.8,1.2]), random.randint x2 (x1, y1), np binomial(1, 0.2) and, if it hits, sx, sy, cx, cy -- sx / cx
    count ROWS of the crop although the reference names them x.  The rectangle is clipped to the crop; at the reference's
    256 x 512 it never leaves it."""
    th, tw = crop
    brightness = np_random.uniform(0.5, 2.0, 2)
    gamma = np_random.uniform(0.8, 1.2, 2)
    contrast = np_random.uniform(0.8, 1.2, 2)
    x1 = py_random.randint(0, w - tw)
    y1 = py_random.randint(0, h - th)
    patch = None
    if np_random.binomial(1, 0.2):
        sx = int(np_random.uniform(35, 100))
        sy = int(np_random.uniform(25, 75))
        cx = int(np_random.uniform(sx, th - sx))
        cy = int(np_random.uniform(sy, tw - sy))
        r0, r1, c0, c1 = max(0, cx - sx), min(th, cx + sx), max(0, cy - sy), min(tw, cy + sy)
        patch = (r0, max(r0, r1), c0, max(c0, c1))
    return AugParams(x1, y1, tuple(float(v) for v in brightness), tuple(float(v) for v in gamma),
                     tuple(float(v) for v in contrast), patch)


# ---- the complete host path ----------------------------------------------------------------------------------------------
def downscaled_inputs(left, right, disp, downscale, inf_to_zero=False, flip_rows=False):
    """The decoded sample at 1 / downscale of its size (`highres.area_downscale_pair_host`, `area_downscale_disp_host`): the
    uint8 pair block-averaged, the disparity block-averaged and divided by the factor (a uint16 payload is widened to
    float32 first, which is exact), top-down whatever `flip_rows` says about the source."""
    from .highres import area_downscale_disp_host, area_downscale_pair_host
    small = area_downscale_pair_host(left, right, downscale)
    disp = np.asarray(disp)
    if disp.dtype == np.uint16:
        disp = disp.astype(np.float32)
    return small[0], small[1], area_downscale_disp_host(disp, downscale, inf_to_zero, flip_rows)


def _check_pair(left, right):
    left, right = np.ascontiguousarray(left), np.ascontiguousarray(right)
    if left.dtype != np.uint8 or right.dtype != np.uint8 or left.ndim != 3 or left.shape[2] not in (3, 4) \
            or left.shape != right.shape:
        raise ValueError(f"expected two (H,W,3) or (H,W,4) uint8 images of one shape, got {left.dtype} {left.shape} and "
                         f"{right.dtype} {right.shape}")
    return left, right


def _check_params(p, h, w, th, tw):
    if min(p.x1, p.y1) < 0 or p.y1 + th > h or p.x1 + tw > w:
        raise ValueError(f"the {th} x {tw} crop at ({p.y1}, {p.x1}) does not fit the {h} x {w} image")
    if p.patch is not None:
        r0, r1, c0, c1 = p.patch
        if not (0 <= r0 <= r1 <= th and 0 <= c0 <= c1 <= tw):
            raise ValueError(f"the patch rows {r0}:{r1}, columns {c0}:{c1} leave the {th} x {tw} crop")


def photometric_tables(params: AugParams, gamma_fn=gamma_table) -> np.ndarray:
    """bg (2,256) uint8: gamma o brightness of (left, right) -- the part of the augmentation the parameters alone fix."""
    return np.stack([np.asarray(gamma_fn(params.gamma[i]), np.uint8)[brightness_table(params.brightness[i])]
                     for i in range(2)])


def host_sample(left, right, disp, params: AugParams, crop=(256, 512), maxdisp=192, kind="kitti", norm=None,
                gamma_fn=gamma_table, flip_rows=False, scale=None, inf_to_zero=False, downscale=1):
    """One sample as the reference's loader produces it, from the decoded uint8 pair and the raw disparity:
    kind "kitti" (datasets.py:282-315): brightness, gamma, contrast on the whole image, crop, occlusion patch on the right
    crop, ToTensor + Normalize; kind "sceneflow" (datasets.py:235-245): crop, ToTensor + Normalize.  norm: (2,3,256)
    float32 table of the normalisation (default `inference.imagenet_lut()`); scale: of the disparity (default 1/256 for
    "kitti", 1 for "sceneflow").  downscale = s in 2..4: the pair and the disparity go through the area downscale of
    `highres` first (`downscaled_inputs`), and everything else -- the crop parameters too -- refers to the small images;
    downscale=2 with inf_to_zero=True is the reference's myImageFloder_middlebury_additional (datasets.py:547-673).
    Returns numpy (imgL (3,th,tw) float32, imgR, gt (th,tw) float32, mask (th,tw) bool)."""
    if kind not in ("kitti", "sceneflow"):
        raise ValueError(f"kind {kind!r}")
    left, right = _check_pair(left, right)
    if downscale != 1:
        left, right, disp = downscaled_inputs(left, right, disp, downscale, inf_to_zero, flip_rows)
        flip_rows = False
    h, w = left.shape[:2]
    th, tw = crop
    _check_params(params, h, w, th, tw)
    norm = np.asarray(imagenet_lut() if norm is None else norm, dtype=np.float32)
    y1, x1 = params.y1, params.x1
    crops = []
    for i, img in enumerate((left, right)):
        c = img[y1:y1 + th, x1:x1 + tw, :3]
        if kind == "kitti":
            bg = photometric_tables(params, gamma_fn)[i]
            U = contrast_table(contrast_mean(luma_sum(img, bg), h * w), params.contrast[i])[bg]
            c = U[c]
            if i == 1 and params.patch is not None:
                r0, r1, c0, c1 = params.patch
                c = c.copy()
                c[r0:r1, c0:c1] = patch_bytes(c)
        crops.append(np.stack([norm[i, ch][c[:, :, ch]] for ch in range(3)]))
    if scale is None:
        scale = 1.0 / 256 if kind == "kitti" else 1.0
    gt, mask = crop_disparity(disp, y1, x1, th, tw, maxdisp, flip_rows, scale, inf_to_zero)
    return crops[0], crops[1], gt, mask


# ---- TrainInput ------------------------------------------------------------------------------------------------------------
def _up16(n):
    return (n + 15) & ~15


class _Stage:
    """Buffers and events of one sample in flight (device I/O), after inference._Slot: a pinned and a device byte buffer
    that grow on demand and hold [left | right | disparity | byte tables], each part at a multiple of 16."""

    def __init__(self, device):
        self.device = device
        self.pin = self.dev = None
        self.small = self.small_d = None             # TrainInput(downscale=): the downscaled pair and disparity
        self.uploaded, self.computed = torch.cuda.Event(), torch.cuda.Event()

    def reserve_small(self, nbytes, nfloats):
        """views of nbytes uint8 and nfloats float32 on the device, in buffers that grow on demand (their readers run on the
        one compute stream, in order, so a replaced buffer is freed behind them)"""
        if self.small is None or self.small.numel() < nbytes:
            self.small = torch.empty(nbytes, device=self.device, dtype=torch.uint8)
        if self.small_d is None or self.small_d.numel() < nfloats:
            self.small_d = torch.empty(nfloats, device=self.device, dtype=torch.float32)
        return self.small[:nbytes], self.small_d[:nfloats]

    def reserve(self, nbytes):
        if self.pin is None or self.pin.numel() < nbytes:
            torch.cuda.synchronize(self.device)          # rare: nothing in flight may still use the old buffers
            self.pin = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
            self.dev = torch.empty(nbytes, device=self.device, dtype=torch.uint8)


class TrainInput:
    """`ti = TrainInput(B); for b: ti.load(b, left_u8, right_u8, disp, params); imgL, imgR, gt, mask = ti.batch()`.

    kind "kitti": photometric augmentation, crop, occlusion patch, normalisation; the disparity is the uint16 PNG payload
    (scale 1/256) or float32.  kind "sceneflow": crop and normalisation; the disparity is float32, `flip_rows=True` for a
    PFM payload as stored.  Source sizes may differ from sample to sample.  downscale = s in 2..4: the uploaded pair and
    the raw disparity go through `ops.area_downscale_pair` / `ops.area_downscale_disp` first (two more launches; a uint16
    disparity is widened to float32 before the upload) and the crop refers to the small images, as in `host_sample`;
    downscale=2 with `load(..., inf_to_zero=True)` is the reference's Middlebury training branch.

    device_io=False: `host_sample` into CPU tensors, as a DataLoader hands them over.
    device_io=True: `load` copies the uint8 pair, the raw disparity and 512 bytes of tables into pinned memory, uploads
    them on a copy stream and enqueues the kernels on the current stream -- a quarter of the bytes of two fp32 crops, no
    per-pixel host arithmetic.  The staging buffers form a ring of `depth` batches ordered by events, so loading batch
    i + 1 right after step i was enqueued overlaps its upload with that step.  The OUTPUTS are one set of static device
    tensors (the kernels that fill them run on the compute stream, behind the step that still reads them), so a
    `GraphedTrainStep` reads them in place.  No queue setting is changed."""

    def __init__(self, batch, crop=(256, 512), maxdisp=192, kind="sceneflow", device_io=False, depth=2, device="cuda",
                 norm=None, gamma_table=gamma_table, disp_scale=None, downscale=1):
        if kind not in ("kitti", "sceneflow"):
            raise ValueError(f"kind {kind!r}")
        if downscale != 1:
            from .highres import _scale
            downscale = _scale("TrainInput", downscale, ValueError)
        self.downscale = downscale
        if batch < 1 or depth < 1:
            raise ValueError("batch >= 1 and depth >= 1")
        self.B, self.crop, self.maxdisp, self.kind = int(batch), (int(crop[0]), int(crop[1])), maxdisp, kind
        self.device_io, self.depth = bool(device_io), int(depth)
        self.gamma_fn = gamma_table
        self.scale = (1.0 / 256 if kind == "kitti" else 1.0) if disp_scale is None else float(disp_scale)
        norm = imagenet_lut() if norm is None else torch.as_tensor(norm, dtype=torch.float32)
        if tuple(norm.shape) != (2, 3, 256):
            raise ValueError("norm must be a (2,3,256) table")
        th, tw = self.crop
        dev = torch.device(device) if self.device_io else torch.device("cpu")
        self.device = dev
        self.norm = norm.to(dev).contiguous()
        self.imgL = torch.zeros((self.B, 3, th, tw), device=dev, dtype=torch.float32)
        self.imgR = torch.zeros((self.B, 3, th, tw), device=dev, dtype=torch.float32)
        self.gt = torch.zeros((self.B, th, tw), device=dev, dtype=torch.float32)
        self.mask = torch.zeros((self.B, th, tw), device=dev, dtype=torch.bool)
        self._loaded = [False] * self.B
        self._cur = 0
        self._ring = None
        self._copy = None

    def _stage(self, b):
        if self._ring is None:
            self._ring = [[_Stage(self.device) for _ in range(self.B)] for _ in range(self.depth)]
            self._copy = torch.cuda.Stream(self.device)
            self._copy.wait_stream(torch.cuda.current_stream(self.device))
        return self._ring[self._cur][b]

    def load(self, b, left_u8, right_u8, disp, params: AugParams, flip_rows=False, inf_to_zero=False):
        """fills slot b of the batch that the next `batch()` hands out"""
        if not 0 <= b < self.B:
            raise IndexError(f"slot {b} of a batch of {self.B}")
        if not self.device_io:
            l, r, g, m = host_sample(left_u8, right_u8, disp, params, self.crop, self.maxdisp, self.kind, self.norm.numpy(),
                                     self.gamma_fn, flip_rows, self.scale, inf_to_zero, self.downscale)
            self.imgL[b], self.imgR[b] = torch.from_numpy(l), torch.from_numpy(r)
            self.gt[b], self.mask[b] = torch.from_numpy(g), torch.from_numpy(m)
        else:
            self._load_device(b, left_u8, right_u8, disp, params, flip_rows, inf_to_zero)
        self._loaded[b] = True

    def _load_device(self, b, left, right, disp, p, flip_rows, inf_to_zero):
        from . import ops
        left, right = _check_pair(left, right)
        disp = np.ascontiguousarray(disp)
        h, w, c = left.shape
        th, tw = self.crop
        ds = self.downscale
        hs, ws = -(-h // ds), -(-w // ds)                 # the size the crop parameters refer to
        _check_params(p, hs, ws, th, tw)
        if disp.dtype not in (np.float32, np.uint16) or disp.shape != (h, w):
            raise ValueError(f"expected a ({h},{w}) float32 or uint16 disparity, got {disp.dtype} {disp.shape}")
        if ds > 1 and disp.dtype == np.uint16:
            disp = disp.astype(np.float32)               # (exact; the downscale kernel takes float32)
        n, nd = h * w * c, disp.nbytes
        off_r = _up16(n)
        off_d = _up16(off_r + n)
        off_t = _up16(off_d + nd)
        total = off_t + 512
        s = self._stage(b)
        s.reserve(total)
        s.uploaded.synchronize()                         # the previous copy out of the pinned buffer
        pin = s.pin.numpy()
        pin[:n] = left.reshape(-1)
        pin[off_r:off_r + n] = right.reshape(-1)
        pin[off_d:off_d + nd] = disp.reshape(-1).view(np.uint8)
        if self.kind == "kitti":
            pin[off_t:total] = photometric_tables(p, self.gamma_fn).reshape(-1)
        compute, copy = torch.cuda.current_stream(self.device), self._copy
        with torch.cuda.stream(copy):
            copy.wait_event(s.computed)                  # the previous sample of this stage has been read
            s.dev[:total].copy_(s.pin[:total], non_blocking=True)      # one copy per sample
            s.uploaded.record(copy)
        compute.wait_event(s.uploaded)
        L, R = s.dev[:n].view(h, w, c), s.dev[off_r:off_r + n].view(h, w, c)
        D = s.dev[off_d:off_d + nd].view(torch.uint16 if disp.dtype == np.uint16 else torch.float32).view(h, w)
        if ds > 1:       # two more launches; from here on the sample is the small one, top-down
            small, small_d = s.reserve_small(2 * hs * ws * c, hs * ws)
            L, R = ops.area_downscale_pair(L, R, ds, out=small.view(2, hs, ws, c))
            D = ops.area_downscale_disp(D, ds, inf_to_zero, flip_rows, out=small_d.view(hs, ws))
            h, w, flip_rows = hs, ws, False
        if self.kind == "kitti":
            bg = s.dev[off_t:total].view(2, 256)
            U, T = ops.train_tables(ops.train_luma_sum(L, R, bg), h * w, bg, p.contrast, self.norm)
            patch = p.patch if p.patch is not None and p.patch[1] > p.patch[0] and p.patch[3] > p.patch[2] else None
            colour = ops.train_patch_colour(R, U, p.y1, p.x1, th, tw) if patch is not None else None
            ops.train_crop_norm(L, R, T, p.y1, p.x1, self.imgL[b], self.imgR[b], patch, self.norm, colour)
        else:
            ops.train_crop_norm(L, R, self.norm, p.y1, p.x1, self.imgL[b], self.imgR[b])
        ops.train_disp_crop(D, p.y1, p.x1, self.maxdisp, self.gt[b], self.mask[b], flip_rows, self.scale, inf_to_zero)
        s.computed.record(compute)

    def batch(self):
        """(imgL (B,3,th,tw), imgR, gt (B,th,tw) float32, mask (B,th,tw) bool): the static tensors, valid until the next
        `load` is enqueued behind their readers on the same stream; moves on to the next staging batch of the ring"""
        if not all(self._loaded):
            raise RuntimeError(f"slots {[i for i, ok in enumerate(self._loaded) if not ok]} of the batch were not loaded")
        self._loaded = [False] * self.B
        self._cur = (self._cur + 1) % self.depth
        return self.imgL, self.imgR, self.gt, self.mask


# ---- TrainStep -------------------------------------------------------------------------------------------------------------
class TrainStep:
    """`ts = TrainStep(model, optimizer); for batch: ts.step(imgL, imgR, gt, mask); print(ts.result())` -- `train()` of
    main_dca.py:122-141 (train_kitti.py:92-120 differs only in the loss weights it spells out) without its two `.item()`
    calls and without indexing by the mask.

    `step` enqueues mask, zero_grad, forward, focal_loss + model_loss, backward, the optimizer step and adds
    [1, loss, epe, #mask] to `state` (device, float64), all without a host synchronisation; `result()` is the one
    synchronisation.  epe = sum_b sum|pred - gt| / sum_b #mask over the batch's masked pixels, from `ops.disp_metrics`
    (e in fp32, summed in fp64 in a fixed order).  An EMPTY mask gives epe = loss = NaN for that step, as `torch.mean` of
    an empty selection does in the reference, and the sums stay NaN from then on.

    gt: (B,H,W) or (B,1,H,W) float32; mask: bool of gt's shape or None (gt > 0 & gt < maxdisp).  Across ranks call
    `all_reduce_state(ts.state)` before `result()`.

    With `dcanet_amd.graph.GraphedTrainStep`: `ts.bind(imgL, imgR, gt, mask)` once with static tensors (those of
    `TrainInput.batch()`), then `GraphedTrainStep(ts.local_step, ts.optimizer_step, ...)` with an optimizer built with
    capturable=True.  Its warm-up runs REAL steps on the bound batch, and they are added to `state` like any other.
    Without `restore=` they stay: parameters, optimizer moments and the state all hold warm-up + replays, which equals
    that many eager steps on the same batch (tests/test_gpu_train_io.py checks exactly this: 3 warm-ups + 2 replays
    against 5 eager steps).  With `restore=` the parameters are put back, so the warm-up steps did not happen as far as
    the run is concerned: then `ts.state` must be among the restored tensors too, or the run's sums start with the
    warm-up steps' losses.  Restore both or neither.  The callables contain no host synchronisation of their own.  The
    test replays them for a model that starts at the 1/4-resolution features (the part dcanet_amd.graph captures
    elsewhere); with the 2D networks inside, whether MIOpen's convolutions capture is the caller's to check."""

    def __init__(self, model, optimizer, maxdisp=192, focal_coefficient=5.0, sparse=False):
        self.model, self.optimizer = model, optimizer
        self.maxdisp, self.focal_coefficient, self.sparse = maxdisp, focal_coefficient, sparse
        dev = next(model.parameters()).device
        self.state = torch.zeros(4, device=dev, dtype=torch.float64)
        self._one = torch.ones((), device=dev, dtype=torch.float64)
        self._bound = None
        self.last = None      # (loss, epe) of the last step: 0-dim device tensors

    def reset(self):
        self.state.zero_()

    def bind(self, imgL, imgR, gt, mask=None):
        gt4 = gt if gt.dim() == 4 else gt.unsqueeze(1)
        if gt4.dim() != 4 or gt4.shape[1] != 1 or gt4.dtype != torch.float32:
            raise ValueError(f"expected a (B,H,W) or (B,1,H,W) float32 ground truth, got {gt.dtype} {tuple(gt.shape)}")
        if mask is not None:
            if mask.dtype != torch.bool or mask.numel() != gt4.numel():
                raise ValueError("expected a bool mask of the ground truth's shape")
            mask = mask.view(gt4.shape)
        self._bound = (imgL, imgR, gt4, mask)

    def local_step(self):
        """zero_grad, forward, losses, backward, metrics into the state; returns the detached loss"""
        from . import ops
        from .models.loss import focal_loss, model_loss
        imgL, imgR, gt4, mask = self._bound
        self.model.train()
        m = ((gt4 < self.maxdisp) & (gt4 > 0)) if mask is None else mask
        self.optimizer.zero_grad()
        cls_outputs, disp_outputs = self.model(imgL, imgR)
        loss = focal_loss(cls_outputs, gt4, self.maxdisp, self.focal_coefficient, self.sparse) + \
            model_loss(disp_outputs, gt4, m)
        loss.backward()
        with torch.no_grad():
            rec = ops.disp_metrics(disp_outputs[-1].detach(), gt4[:, 0], self.maxdisp, m[:, 0])
            n = rec[:, 0].sum()
            epe = rec[:, 2].sum() / n                    # 0 / 0 = NaN for an empty mask
            loss_d = loss.detach()
            self.state += torch.stack([self._one, loss_d.double(), epe, n])
        self.last = (loss_d, epe)
        return loss_d

    def optimizer_step(self):
        self.optimizer.step()

    def step(self, imgL, imgR, gt, mask=None):
        self.bind(imgL, imgR, gt, mask)
        loss = self.local_step()
        self.optimizer_step()
        return loss

    def result(self):
        """one device -> host copy: {"steps", "loss", "epe"} (means over the steps) and "pixels" (masked pixels seen)"""
        s = self.state.cpu().numpy()
        steps = s[STEPS]
        return {"steps": int(steps), "loss": float(s[SUM_LOSS] / steps) if steps else 0.0,
                "epe": float(s[SUM_EPE] / steps) if steps else 0.0,
                "pixels": int(s[PIXELS]) if np.isfinite(s[PIXELS]) else 0}


# ---- SelfSupStep -----------------------------------------------------------------------------------------------------------
class SelfSupStep:
    """`ss = SelfSupStep(model, optimizer); for batch: ss.step(imgL, imgR); print(ss.result())` -- a training step that
    needs no ground truth, in the shape of `TrainStep`: `bind`, `local_step`, `optimizer_step`, `step`, `result`.

    `step` enqueues (the mask pass,) zero_grad, the training forward, `loss(disp_outputs, imgL, imgR, valid)`, backward and
    the optimizer step, and adds [1, loss, sum_l w_l photo_l / sum_l w_l, sum_l w_l smooth_l / sum_l w_l, share of interior
    pixels kept (sum M over the interior pixel count, mean over the levels)] to `state` (device, float64), all without a
    host synchronisation; `result()` is the one synchronisation.

    Only `disp_outputs` (`[pred_dca3, pred4]`) are supervised: the five class-volume heads of the training forward
    (`cls_outputs`) take no part in this loss, so the parameters that only they depend on get NO gradient in such a step
    (their `.grad` stays None after `zero_grad`, and the optimizer leaves them alone).  To train them as well, add the
    supervised loss on the pairs that have a label: `loss_a + loss_b`.

    mask=None: every in-view interior pixel counts.  mask="lr": `valid` is `model.predict_lr(imgL, imgR, tau)["valid"]`,
    taken BEFORE the training forward with the weights as they are: two more forward passes in eval mode under no_grad,
    which leave the BatchNorm running statistics alone; the model is put back into train mode afterwards.  Across ranks
    every rank divides by its own sum M (the note at `models.loss.PhotometricLoss`); `all_reduce_state(ss.state)` before
    `result()` as with `TrainStep`."""

    def __init__(self, model, optimizer, loss=None, mask=None, tau=1.0):
        if mask not in (None, "lr"):
            raise ValueError(f"mask {mask!r}: None or 'lr'")
        if loss is None:
            from .models.loss import PhotometricLoss
            loss = PhotometricLoss()
        self.model, self.optimizer, self.loss, self.mask, self.tau = model, optimizer, loss, mask, float(tau)
        dev = next(model.parameters()).device
        self.state = torch.zeros(5, device=dev, dtype=torch.float64)
        self._one = torch.ones((), device=dev, dtype=torch.float64)
        self._w = torch.tensor(loss.weights, device=dev, dtype=torch.float64)
        self._w /= self._w.sum()
        self._bound = None
        self.last = None      # (loss, per-level (photo, smooth, sum M)) of the last step: device tensors

    def reset(self):
        self.state.zero_()

    def bind(self, imgL, imgR):
        if imgL.dim() != 4 or imgL.shape[1] != 3 or imgL.shape != imgR.shape or imgL.dtype != torch.float32:
            raise ValueError(f"expected two (B,3,H,W) float32 images, got {tuple(imgL.shape)} and {tuple(imgR.shape)}")
        self._bound = (imgL, imgR)

    def local_step(self):
        """(mask pass,) zero_grad, forward, loss, backward, sums into the state; returns the detached loss"""
        imgL, imgR = self._bound
        valid = None
        if self.mask == "lr":
            valid = self.model.predict_lr(imgL, imgR, self.tau)["valid"]
        self.model.train()
        self.optimizer.zero_grad()
        _cls_outputs, disp_outputs = self.model(imgL, imgR)
        loss = self.loss(disp_outputs, imgL, imgR, valid)
        loss.backward()
        with torch.no_grad():
            stats = self.loss.last.double()               # (L,3): photo, smooth, sum M
            interior = float(imgL.shape[0] * (imgL.shape[2] - 2) * (imgL.shape[3] - 2))
            loss_d = loss.detach()
            self.state += torch.stack([self._one, loss_d.double(), (self._w * stats[:, 0]).sum(),
                                       (self._w * stats[:, 1]).sum(), stats[:, 2].mean() / interior])
        self.last = (loss_d, self.loss.last)
        return loss_d

    def optimizer_step(self):
        self.optimizer.step()

    def step(self, imgL, imgR):
        self.bind(imgL, imgR)
        loss = self.local_step()
        self.optimizer_step()
        return loss

    def result(self):
        """one device -> host copy: {"steps", "loss", "photo", "smooth", "kept"}, means over the steps"""
        s = self.state.cpu().numpy()
        n = s[SS_STEPS]
        mean = (lambda i: float(s[i] / n)) if n else (lambda i: 0.0)
        return {"steps": int(n), "loss": mean(SS_LOSS), "photo": mean(SS_PHOTO), "smooth": mean(SS_SMOOTH),
                "kept": mean(SS_KEPT)}
