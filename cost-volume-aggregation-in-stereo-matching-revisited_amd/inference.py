"""KITTI-style single-pair inference around the hipGraph-captured hot path (BASELINE config 5):
the host side of the reference's my_img.py:47-110 -- per-image per-channel mean/std normalisation (:59-68), top/right
zero padding to a fixed 384x1248 frame (:71-87), `model(left, right)` in eval mode (:95-101), crop back (:105-108)
and the uint16 x256 PNG (:110) -- with the 3D part replayed as ONE hipGraph (dcanet_amd.graph.GraphedHotPath).

The reference's script calls `.squeeze()` on the model's return value although eval `forward` returns a tuple
(gwcnet_dca_g.py:282); the disparity is element 0.

`KittiInference(..., device_io=True)` moves the arithmetic around the model call to the GPU (csrc/frame_io.hip): the
uint8 pair is uploaded as it is, normalised through a histogram-built table, placed in the frame, and the cropped
float32 / uint16 disparity is read back -- two copies are all that is left on the host.

`KittiInferenceWithConfidence` returns a confidence map next to every disparity map: the probability mass of the final
disparity distribution within `radius` bins of its peak, up-sampled with the disparity in one launch (DESIGN.md section
6e; nothing in the reference computes it).

`KittiInferenceLR` returns the left-right-checked, filled disparity and its validity mask: a second pass on the mirrored,
swapped frames gives the right view's disparity, one launch cross-checks and fills (nothing in the
reference computes it).

`KittiInference3D` adds the geometry stage behind any of the three: metric depth and a coloured point cloud from a
StereoCalib, filtered by the confidence or the left-right validity.

`KittiInferenceColor` hands out the colour-coded disparity map (the KITTI devkit's colours, or grey) next to the disparity,
coloured on the device in one launch behind any of the three (csrc/visualize.hip).

`SGMInference` takes no model: semi-global matching on a census cost (csrc/sgm.hip) turns the uploaded
uint8 pair into `(disp, valid)`, optionally through its own left-right check and the post-filter;
`KittiInferenceGuided(model, sgm=...)` uses that map as the hints of the guided network, so guided stereo needs no LiDAR.

Every class takes `rectify=` a geometry.RectifyMaps: the pair is then a RAW camera pair, rectified on the device in one
launch (csrc/rectify.hip) in front of the unchanged chain.

Two layers.  `FramePipeline` is the device I/O of a frame without any network: slots, upload, the head of
the compute stage (waits, `rectify=`), read-back, result, `stream`; a subclass fills one hook, `_fill`, which turns the uint8 pair
in device memory into the frame's record.  `KittiInference` fills it with the network and its fixed frame, `SGMInference` with
semi-global matching.  The stages behind the network (filters, geometry, ground, stixels, colour) share one preamble,
`_StageMixin._stage_maps`."""
from __future__ import annotations

import collections
import math

import numpy as np
import torch

from .geometry import depth_png, rectify_pair_host  # noqa: F401  (depth_png: the depth exporter, next to disparity_png)
from .geometry import LidarCalib, LidarProjector
from .graph import GraphedHotPath


def normalize_pair(left_rgb: np.ndarray, right_rgb: np.ndarray) -> np.ndarray:
    """my_img.py:47-69 `load_data` after the file read: (H,W,3) uint8 x2 -> (6,H,W) float32, every colour plane
    shifted / scaled by its own mean and (population) standard deviation."""
    left_rgb, right_rgb = np.asarray(left_rgb), np.asarray(right_rgb)
    assert left_rgb.ndim == 3 and left_rgb.shape[2] >= 3 and left_rgb.shape[:2] == right_rgb.shape[:2]
    out = np.zeros((6,) + left_rgb.shape[:2], "float32")
    for i, img in enumerate((left_rgb, right_rgb)):
        for c in range(3):
            plane = img[:, :, c]
            out[3 * i + c] = (plane - np.mean(plane[:])) / np.std(plane[:])
    return out


def pad_or_crop(temp_data: np.ndarray, crop_height: int = 384, crop_width: int = 1248):
    """my_img.py:71-87 `my_transform`: images no larger than the frame go to its BOTTOM-LEFT corner (zero rows on top,
    zero columns on the right); larger ones are cropped (vertically centred, from column 0 -- the reference computes a
    horizontal offset and does not use it).  Returns (left (1,3,Hc,Wc), right, h, w)."""
    _, h, w = temp_data.shape
    if h <= crop_height and w <= crop_width:
        frame = np.zeros((6, crop_height, crop_width), "float32")
        frame[:, crop_height - h:crop_height, 0:w] = temp_data
    else:
        start_y = int((h - crop_height) / 2)
        frame = temp_data[:, start_y:start_y + crop_height, 0:crop_width]
    left = torch.from_numpy(np.ascontiguousarray(frame[None, 0:3])).float()
    right = torch.from_numpy(np.ascontiguousarray(frame[None, 3:6])).float()
    return left, right, h, w


def crop_back(disp: np.ndarray, h: int, w: int, crop_height: int = 384, crop_width: int = 1248) -> np.ndarray:
    """my_img.py:105-108"""
    if h <= crop_height and w <= crop_width:
        return disp[crop_height - h:crop_height, 0:w]
    return disp


def disparity_png(path: str, disp: np.ndarray) -> None:
    """my_img.py:110: `imsave(savename, (disp * 256).astype('uint16'))` (KITTI's 16-bit disparity format)."""
    from PIL import Image
    Image.fromarray((disp * 256).astype("uint16")).save(path, format="PNG")


def lut_from_histogram(hist: np.ndarray, n: int):
    """numpy restatement of the `frame_lut` kernel, operation for operation: hist (..., 256) counts of the byte values of a
    plane of n pixels -> (lut (..., 256) float32, stats (..., 2) float64 = mean, population std), with
    lut[v] = float32((v - mean) / std) -- the value `normalize_pair` gives a pixel of value v.  The mean is exact (integer
    sum, one division); the variance is summed over v = 0..255 in that order (np.cumsum is sequential)."""
    hist = np.asarray(hist)
    assert hist.shape[-1] == 256 and n > 0
    h = hist.astype(np.int64)
    v = np.arange(256, dtype=np.int64)
    mean = (h * v).sum(-1).astype(np.float64) / np.float64(n)
    d = v.astype(np.float64) - mean[..., None]
    var = np.cumsum(h.astype(np.float64) * (d * d), axis=-1)[..., -1] / np.float64(n)
    std = np.sqrt(var)
    with np.errstate(divide="ignore", invalid="ignore"):      # a constant plane: NaN, as on the host path
        lut = (d / std[..., None]).astype(np.float32)
    return lut, np.stack([mean, std], -1)


def placement(h: int, w: int, crop_height: int = 384, crop_width: int = 1248):
    """`pad_or_crop` as a window: (src_y0, dst_y0, rows, cols) -- rows x cols pixels from source row src_y0, column 0,
    land at frame row dst_y0, column 0; the rest of the frame is zero.  An image larger than the frame in one direction
    and smaller in the other gives a mis-shaped frame on the host path and is refused here."""
    if h <= 0 or w <= 0:
        raise ValueError(f"empty image {h} x {w}")
    if h <= crop_height and w <= crop_width:
        return 0, crop_height - h, h, w
    if h >= crop_height and w >= crop_width:
        return int((h - crop_height) / 2), 0, crop_height, crop_width
    raise ValueError(f"a {h} x {w} image neither fits into the {crop_height} x {crop_width} frame nor covers it")


def imagenet_lut() -> torch.Tensor:
    """The fixed table of the training loaders (dataloader/data_io.py:11-12, 27-35: ToTensor, then Normalize with the
    ImageNet statistics) in the (2,3,256) form `ops.frame_apply` takes: the same float32 torch operations applied to the
    256 byte values, repeated for both images."""
    mean = torch.tensor([0.485, 0.456, 0.406], dtype=torch.float32).view(3, 1)
    std = torch.tensor([0.229, 0.224, 0.225], dtype=torch.float32).view(3, 1)
    v = torch.arange(256, dtype=torch.uint8).view(1, 256).expand(3, 256)
    lut = v.float().div(255).sub(mean).div(std)
    return torch.stack([lut, lut]).contiguous()


class _Frame(collections.namedtuple("_Frame", "h w c src_y0 dst_y0 rows cols off")):
    """The frame in a slot: the h x w x c uint8 images as they were uploaded, the right one `off` bytes behind the left; and the
    placement of the image (the rectified one, with rectify=) in the network's frame as `placement` gives it -- rows x cols
    pixels from source row src_y0 land at frame row dst_y0.  Without a network's frame the window is the image itself."""
    __slots__ = ()

    @property
    def window(self):
        """(y0, rows, cols): where the image lies in the frame's maps"""
        return self.dst_y0, self.rows, self.cols

    @property
    def placement(self):
        return self.src_y0, self.dst_y0, self.rows, self.cols


class _Slot:
    """Buffers and events of one frame in flight (device I/O): pinned + device uint8 inputs that grow on demand, and ONE device +
    ONE pinned byte buffer for what the frame hands out, sized once for the class's worst case.  The record of the frame in
    the slot is a list of fields (name, dtype, shape) laid back to back from byte 0 (`set_fields`), so one copy of `out_bytes`
    brings all of it to the host.  Whatever else a stage keeps per slot lives in `scratch`."""

    def __init__(self, device, out_capacity):
        self.device = device
        self.in_pin = self.in_dev = None
        self.out_dev = torch.empty(out_capacity, device=device, dtype=torch.uint8)
        self.out_pin = torch.empty(out_capacity, dtype=torch.uint8).pin_memory()
        self.dev, self.pin, self.out_bytes = {}, {}, 0
        self.uploaded, self.computed, self.done = (torch.cuda.Event() for _ in range(3))
        self.frame = None            # the _Frame in the slot
        self.item = None             # what the frame carries beside the pair, as the class's `_upload` left it (hints, a matrix)
        self.out_hw = None           # the size of the maps the frame hands out (the window's; HighResInference: the image's)
        self.copy = None             # the stream the record went out on
        self.rect = {}               # channels -> the rectified pair (rectify=), allocated once for the maps' dst_hw
        self.left = None             # the left image the frame in the slot was built from, as it lies in device memory
        self._scratch = {}

    def reserve_input(self, nbytes):
        """room for two images of nbytes each, the second at the next multiple of 16 (vector loads); returns its offset"""
        off = (nbytes + 15) & ~15
        if self.in_pin is None or self.in_pin.numel() < off + nbytes:
            torch.cuda.synchronize(self.device)          # rare: nothing in flight may still use the old buffers
            self.in_pin = torch.empty(off + nbytes, dtype=torch.uint8).pin_memory()
            self.in_dev = torch.empty(off + nbytes, device=self.device, dtype=torch.uint8)
        return off

    def reserve_output(self, nbytes, drop=()):
        """room for a record of nbytes, after the slot's previous frame has been handed out (rare: SGMInference's largest image
        grew); `drop`: the scratch keys whose buffers were sized with the record, to be built again"""
        if self.out_dev.numel() >= nbytes:
            return
        self.done.synchronize()                      # the read-back out of the old buffers
        self.out_dev = torch.empty(nbytes, device=self.device, dtype=torch.uint8)
        self.out_pin = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
        for key in drop:
            self._scratch.pop(key, None)

    def rectified(self, hd, wd, c):
        """the two (hd,wd,c) uint8 images `ops.rectify_pair` writes, the second at a multiple of 16 bytes (vector stores)"""
        if c not in self.rect:
            n = hd * wd * c
            off = (n + 15) & ~15
            buf = torch.empty(off + n, device=self.device, dtype=torch.uint8)
            self.rect[c] = (buf[:n].view(hd, wd, c), buf[off:off + n].view(hd, wd, c))
        return self.rect[c]

    def scratch(self, key, build):
        """a stage's own per-slot buffers, built by `build()` when first asked for"""
        if key not in self._scratch:
            self._scratch[key] = build()
        return self._scratch[key]

    def set_fields(self, fields):
        """lays out the record of the frame in the slot: `dev` and `pin` become {name: view} of its fields in the device and in
        the pinned output buffer, `out_bytes` the bytes in use"""
        self.dev, self.pin, off = {}, {}, 0
        for name, dtype, shape in fields:
            end = off + _nbytes([(name, dtype, shape)])
            self.dev[name] = self.out_dev[off:end].view(dtype).view(shape)
            self.pin[name] = self.out_pin[off:end].view(dtype).view(shape)
            off = end
        self.out_bytes = off


def _nbytes(fields):
    return sum(math.prod(shape) * dtype.itemsize for _, dtype, shape in fields)


def _disp_valid(rows, cols):
    """the record of the classes that hand out a float32 disparity and its float32 1.0 / 0.0 validity"""
    return [("disp", torch.float32, (rows, cols)), ("valid", torch.float32, (rows, cols))]


def _maps2d(maps):
    """the frame's disparity and its mask (None: none), contiguous, as 2-D views"""
    pred = maps[0].contiguous()
    pred = pred.view(pred.shape[-2:])
    mask = maps[1] if len(maps) > 1 else None
    return pred, None if mask is None else mask.contiguous().view_as(pred)


def _check_tau(tau) -> float:
    tau = float(tau)
    if not (0.0 <= tau < float("inf")):
        raise ValueError("tau must be finite and >= 0")
    return tau


class FramePipeline:
    """The frame pipeline of device I/O, apart from any network: slots of buffers for the frames in flight, and three stages per
    frame, each enqueued on the stream it is given -- `_upload` (the uint8 pair into pinned memory and on to the device),
    `_compute` (the waits, the two views of the pair, `rectify=`, then the class's own work) and `_readback` (the frame's record
    in ONE copy of exactly its bytes) -- with `_result`, the one synchronisation of a frame, `__call__` and `stream` on top.

    What a subclass states: `_device`, where the frames live; `_fields`, the record a frame hands out; `_fill`, which turns the
    uint8 pair in device memory into that record; and, where it has a frame of fixed size to place the image in, `_place` and
    `_room`.  KittiInference puts a network's frame there; SGMInference has none."""

    out_scale = 1                # the maps handed out are at most this many times the room in each direction (HighResInference)
    device_io = True             # what `device_io=None` means for the class
    needs_device_io = None       # the reason why the class refuses device_io=False, if it does
    has_uint16 = True            # False: the record has no uint16 form, `as_uint16=True` is refused
    Frame = None                 # a namedtuple type to hand the fields out in, by name; None: a tuple (one field: itself)

    def __init__(self, device=None, device_io: bool = None, rectify=None):
        if rectify is not None and not all(hasattr(rectify, k) for k in ("src_hw", "dst_hw", "X", "Y", "valid")):
            raise TypeError(f"rectify= must be a geometry.RectifyMaps, got {type(rectify)}")
        if device_io is not None:
            self.device_io = device_io
        if self.needs_device_io and not self.device_io:
            raise ValueError(f"{type(self).__name__} needs device_io=True: {self.needs_device_io}")
        self.rectify = rectify
        self._dev = None if device is None else torch.device(device)
        self._slots = []
        self._copy_stream = None

    @property
    def _device(self):
        """the device the frames live on"""
        return self._dev

    def _room(self):
        """(rows, cols): the largest window a frame can have; the slots' records and the post-filter's buffers are sized for it"""
        raise NotImplementedError

    def _place(self, h, w):
        """(src_y0, dst_y0, rows, cols) of an h x w image (the rectified one, with rectify=).  Here: the window is the image"""
        return 0, 0, h, w

    def _fields(self, rows, cols, as_uint16):
        """the record of a frame whose maps are rows x cols: (name, dtype, shape) in the order they lie in the slot's buffer"""
        raise NotImplementedError

    def _fill(self, s, left, right, h, w, as_uint16):
        """current stream: the (h,w,c) uint8 pair as it lies in device memory (rectified, with rectify=) -> the frame's record:
        lays it out (`s.set_fields`) and writes every field of `s.dev`"""
        raise NotImplementedError

    def _slot(self, i):
        while len(self._slots) <= i:
            rows, cols = self._room()
            self._slots.append(_Slot(self._device, _nbytes(self._fields(rows * self.out_scale, cols * self.out_scale, False))))
        return self._slots[i]

    def _upload(self, s, left_rgb, right_rgb, copy):
        """host: the pair into the slot's pinned buffer; `copy` stream: pinned -> device"""
        left_rgb, right_rgb = np.ascontiguousarray(left_rgb), np.ascontiguousarray(right_rgb)
        if left_rgb.dtype != np.uint8 or right_rgb.dtype != np.uint8 or left_rgb.ndim != 3 \
                or left_rgb.shape[2] not in (3, 4) or left_rgb.shape != right_rgb.shape:
            raise ValueError(f"device_io takes two (H,W,3) or (H,W,4) uint8 images of one shape, got {left_rgb.dtype} "
                             f"{left_rgb.shape} and {right_rgb.dtype} {right_rgb.shape}")
        h, w, c = left_rgb.shape
        if self.rectify is not None and (h, w) != tuple(self.rectify.src_hw):
            raise ValueError(f"rectify= was built for {self.rectify.src_hw[0]} x {self.rectify.src_hw[1]} raw images, got "
                             f"{h} x {w}")
        place = self._place(*((h, w) if self.rectify is None else self.rectify.dst_hw))
        n = h * w * c
        off = s.reserve_input(n)
        s.uploaded.synchronize()                     # the previous copy out of the pinned buffer
        pin = s.in_pin.numpy()
        pin[:n] = left_rgb.reshape(-1)
        pin[off:off + n] = right_rgb.reshape(-1)
        with torch.cuda.stream(copy):
            copy.wait_event(s.computed)              # the previous frame of this slot has read its input
            s.in_dev[:off + n].copy_(s.in_pin[:off + n], non_blocking=True)      # one copy for the pair
            s.uploaded.record(copy)
        s.frame, s.item = _Frame(h, w, c, *place, off), None

    @torch.no_grad()
    def _compute(self, s, compute, as_uint16):
        """`compute` stream: [rectify ->] `_fill` into the slot's device output"""
        from . import ops
        f = s.frame
        h, w, n = f.h, f.w, f.h * f.w * f.c
        with torch.cuda.stream(compute):
            compute.wait_event(s.uploaded)
            compute.wait_event(s.done)               # the previous read-back of this slot's output
            left, right = s.in_dev[:n].view(h, w, f.c), s.in_dev[f.off:f.off + n].view(h, w, f.c)
            if self.rectify is not None:
                h, w = self.rectify.dst_hw
                left, right = ops.rectify_pair(left, right, self.rectify, out=s.rectified(h, w, f.c))
            s.left, s.out_hw = left, (f.rows, f.cols)
            self._fill(s, left, right, h, w, as_uint16)
            s.computed.record(compute)

    def _readback(self, s, copy):
        """`copy` stream: the frame's record, device output -> pinned, in one copy of exactly its bytes"""
        n = s.out_bytes
        with torch.cuda.stream(copy):
            copy.wait_event(s.computed)
            s.out_pin[:n].copy_(s.out_dev[:n], non_blocking=True)
            s.done.record(copy)
        s.copy = copy

    def _rest(self, s, head):
        """host, after the frame's wait: sends for what the frame hands out beyond its record `head` (the fields in the pinned
        buffer) and returns a function that waits for it and gives it as {name: array}.  Here: nothing, an empty dict.
        KittiInference3D: the vertices."""
        return dict

    def _result(self, s):
        """host: the one synchronisation of a frame, then a copy of every field out of the pinned buffer"""
        s.done.synchronize()
        rest = self._rest(s, s.pin)                  # (in flight while the host copies the fields)
        out = {name: v.numpy().copy() for name, v in s.pin.items()}
        out.update(rest())
        if self.Frame is not None:
            return self.Frame(*(out.get(name) for name in self.Frame._fields))
        return tuple(out.values()) if len(out) > 1 else out["disp"]

    def _call_device(self, left_rgb, right_rgb, as_uint16, *more):
        dev = self._device
        cur = torch.cuda.current_stream(dev)
        s = self._slot(0)
        self._upload(s, left_rgb, right_rgb, cur, *more)
        self._compute(s, cur, as_uint16)
        self._readback(s, cur)
        return self._result(s)

    def _check_format(self, as_uint16):
        if as_uint16 and not self.has_uint16:
            raise TypeError(f"{type(self).__name__} hands out no uint16 form of its frames: as_uint16=True is not for it")

    def stream(self, pairs, depth: int = 2, as_uint16: bool = False):
        """Generator over an iterable of (left_rgb, right_rgb) uint8 pairs (sizes may differ as long as each fits the
        frame): yields what `__call__` gives for each pair, byte for byte, in input order, `depth` frames in flight.  A copy
        stream beside the compute stream carries the upload of frame i+1 and the read-back of frame i-1 while frame i
        computes."""
        if not self.device_io:
            raise RuntimeError("stream() needs KittiInference(..., device_io=True)")
        if depth < 1:
            raise ValueError("depth >= 1")
        self._check_format(as_uint16)
        dev = self._device
        compute = torch.cuda.current_stream(dev)
        if self._copy_stream is None:
            self._copy_stream = torch.cuda.Stream(dev)
        copy = self._copy_stream
        copy.wait_stream(compute)
        inflight = collections.deque()               # slots in input order; [slot, read-back enqueued]
        try:
            for i, (left_rgb, right_rgb, *more) in enumerate(pairs):      # (more: what a subclass's `_upload` takes per frame)
                if len(inflight) == depth:               # slot i % depth is the oldest frame's: hand that frame out first
                    old = inflight.popleft()
                    if not old[1]:
                        self._readback(old[0], copy)
                    yield self._result(old[0])
                s = self._slot(i % depth)
                self._upload(s, left_rgb, right_rgb, copy, *more)
                self._compute(s, compute, as_uint16)
                # the read-back of the frame before goes behind this upload on the copy stream: it waits for that frame's
                # compute, and an upload queued behind it would wait too
                if inflight and not inflight[-1][1]:
                    self._readback(inflight[-1][0], copy)
                    inflight[-1][1] = True
                inflight.append([s, False])
            while inflight:
                old = inflight.popleft()
                if not old[1]:
                    self._readback(old[0], copy)
                yield self._result(old[0])
        finally:
            compute.wait_stream(copy)                # later work on the compute stream may reuse slot 0 (`__call__`)

    def __call__(self, left_rgb: np.ndarray, right_rgb: np.ndarray, as_uint16: bool = False):
        self._check_format(as_uint16)
        return self._call_device(left_rgb, right_rgb, as_uint16)


class KittiInference(FramePipeline):
    """`disp = KittiInference(model)(left_rgb, right_rgb)`: my_img.py:89-110 `my()` without the file I/O.

    `model` is a GwcNet (or the nn.DataParallel wrapper the reference builds, my_img.py:37) already on the GPU with its
    weights loaded.  The 2D networks run as ordinary PyTorch-ROCm launches; the cost-volume path (volume -> dres0/1 ->
    3 x cva -> classif3 -> soft-argmin) is captured once for the fixed frame size and replayed (`graph=False`: eager).

    `device_io=True`: normalisation, padding, crop and the uint16 conversion run as HIP kernels; the host only copies the
    uint8 pair into pinned memory and the result out of it.  `stream(pairs)` pipelines successive frames.  `device_io=None`
    (the default) is the class's own default: False here, True for the subclasses that work on the device only.

    `rectify=maps` (keyword, every subclass too; a geometry.RectifyMaps): the pairs handed in are RAW (maps.src_hw) and are
    rectified first -- `ops.rectify_pair` into a per-slot device buffer with device_io, `rectify_pair_host` without -- and
    everything behind (normalisation, placement, the maps handed out) is of the rectified images (maps.dst_hw): the result is
    what rectifying on the host and handing the rectified pair in gives.  None (the default) changes nothing.

    Two layers.  FramePipeline owns what does not depend on a network: the slots, the upload, the head of the compute stage
    (waits, rectify=), the read-back, the result and `stream`.  This class fills its hooks with the network: the model, eager or
    graphed, the (Hc,Wc) frame and the image's placement in it (`_place`, `_room`), and `_fill`: histogram -> table -> frames ->
    model -> `_export`.  What a subclass states: its mask mode, through `_take_mask` (which disparity and which mask
    `_frame_maps` yields); the record a frame hands out, through `_fields`; and how the frame's maps get into that record,
    through `_export`.  A stage behind the network that reads (disparity, mask, window) starts from `_StageMixin`."""

    confidence = False           # True: a confidence map next to every disparity map (mask mode "confidence")
    radius = 1                   # its window, in 1/4-res disparity bins either side of the peak
    mask_mode = None             # None | "confidence" | "lr": what `_frame_maps` yields next to the disparity
    CONF_U16_SCALE = 65535.0      # uint16 scale of the second map (a confidence in [0,1]; a 0 / 1 validity mask)
    device_io = False            # (the host path is the reference's own)
    _mirrored = None             # (2,1,3,Hc,Wc): the mirrored, swapped frames of `_lr_maps`, rewritten whole by every frame

    @property
    def nmaps(self):
        """the network's maps per frame: the disparity[, a second map in [0,1]]"""
        return 1 if self.mask_mode is None else 2

    def __init__(self, model, crop_height: int = 384, crop_width: int = 1248, graph: bool = True, dtype=None,
                 device_io: bool = None, *, rectify=None):
        """dtype: None (fp32) or torch.float16 / torch.bfloat16 -- the reduced-precision path of BASELINE config 5
        ("fp16, hipGraph-captured 3D hourglass"): the captured hot path runs under ops.reduced_precision(dtype)."""
        super().__init__(device_io=device_io, rectify=rectify)
        self.net = model.module if isinstance(model, torch.nn.DataParallel) else model
        self.crop_height, self.crop_width = crop_height, crop_width
        self.graph = graph
        self.dtype = dtype
        self._graphed = None
        if rectify is not None:
            self._place(*rectify.dst_hw)             # the rectified image must fit or cover the frame
        self._frames = None          # (2,3,Hc,Wc): the network's inputs, rewritten whole by every frame
        self.net.eval()

    @property
    def _device(self):
        """the network's"""
        return next(self.net.parameters()).device

    def _room(self):
        return self.crop_height, self.crop_width

    def _place(self, h, w):
        return placement(*self._net_hw(h, w), self.crop_height, self.crop_width)

    def _calib_or_maps(self, calib):
        """calib=, or else the calibration the rectify= maps carry"""
        if calib is None:
            calib = getattr(self.rectify, "calib", None)
            if calib is None:
                raise ValueError(f"{type(self).__name__} needs calib=, or rectify= maps that carry the rectified pair's calibration")
        return calib

    def _max_disp_or_model(self, max_disp):
        """max_disp=, or else the model's `maxdisp`"""
        if max_disp is None:
            max_disp = getattr(self.net, "maxdisp", None)
            if max_disp is None:
                raise ValueError(f"{type(self).__name__} needs max_disp=: the model has no `maxdisp`")
        return max_disp

    def _take_mask(self, mask, mask_min=0.5, radius=1, tau=1.0):
        """The mask mode of the instance, checked and stored: which disparity and which mask a frame yields (`_frame_maps`).
          None          the disparity alone
          "confidence"  the disparity and the window mass within `radius` bins of the peak
          "lr"          the UNFILLED left disparity and the validity map of the cross-check under `tau` (two passes per frame)
        `mask_min` is the threshold the stages behind apply to the mask."""
        if mask not in (None, "confidence", "lr"):
            raise ValueError(f"mask is None, 'confidence' or 'lr', got {mask!r}")
        if int(radius) < 0 or float(mask_min) != float(mask_min):
            raise ValueError("radius >= 0 and mask_min must not be NaN")
        self.mask_mode, self.mask_min = mask, float(mask_min)
        self.radius, self.tau = int(radius), _check_tau(tau)
        self.confidence = mask == "confidence"

    @torch.no_grad()
    def forward_frame(self, left: torch.Tensor, right: torch.Tensor):
        """(1,3,Hc,Wc) x2 on the GPU -> full-resolution disparity (1,1,Hc,Wc); = GwcNet.forward(...)[0] in eval mode.
        With confidence: (disparity, confidence), both (1,1,Hc,Wc)."""
        net = self.net
        fl, fr = net.feature_extraction(left), net.feature_extraction(right)
        guidance = net.guidance(left)["g"]
        args = [fl["gwc_segments"], fr["gwc_segments"]]
        if net.use_concat_volume:
            args += [fl["concat_feature"], fr["concat_feature"]]
        import contextlib
        from . import ops
        kwargs = {"confidence": self.radius} if self.confidence else {}      # the statistics launch is part of the graph
        kwargs.update(self._hot_kwargs())
        live = self._hot_inputs()
        ctx = ops.reduced_precision(self.dtype) if self.dtype is not None else contextlib.nullcontext()
        with ctx:      # (a replay needs no context: the captured launches are already the reduced-precision kernels)
            if self.graph:
                if self._graphed is None:
                    self._graphed = GraphedHotPath(net, *args, **kwargs, **live)
                r = self._graphed(*args, **live)
            else:
                r = net.hot_path(*args, **kwargs, **live)
        if not self.confidence:
            return net.prop(guidance, r["pred4_q"])
        # the leading planes of the statistics as they lie in memory (disparity, unimodal disparity, window mass): one
        # up-sampling launch for all.  A frame is ONE image: only for B == 1 is this slice contiguous (no gather copy)
        assert r["stats4_q"].shape[0] == 1
        up = net.prop.forward_planes(guidance, r["stats4_q"][:, :ops.CONF_MASS + 1], (4.0, 4.0, 1.0))
        return up[:, ops.CONF_DISP:ops.CONF_DISP + 1], up[:, ops.CONF_MASS:ops.CONF_MASS + 1]

    @torch.no_grad()
    def _lr_maps(self, left, right, cols, outputs):
        """the two passes of the left-right check under `self.tau`: the left disparity as the network gave it and the maps of
        `ops.lr_consistency` named in `outputs`"""
        from . import ops
        disp = self.forward_frame(left, right)           # its own tensor: the second replay below does not touch it
        if self._mirrored is None or self._mirrored.shape[1:] != left.shape or self._mirrored.device != left.device:
            self._mirrored = torch.empty((2,) + tuple(left.shape), device=left.device, dtype=torch.float32)
        disp_m = self.forward_frame(*ops.mirror_pair(left.contiguous(), right.contiguous(), out=self._mirrored))
        return disp, ops.lr_consistency(disp.contiguous(), disp_m.contiguous(), self.tau, cols, outputs=outputs)

    def _frame_maps(self, left, right, cols):
        """the `nmaps` maps of one frame as a tuple, by the mask mode; cols: the image's width inside the frame"""
        if self.mask_mode == "lr":
            disp, r = self._lr_maps(left, right, cols, ("valid",))
            return disp, r["valid"]
        maps = self.forward_frame(left, right)
        return maps if self.confidence else (maps,)

    def _hot_kwargs(self):
        """further keywords of `hot_path` that are settings: part of what a graph captures"""
        return {}

    def _hot_inputs(self):
        """further keywords of `hot_path` that are tensors of the frame: static inputs of the graph, copied in at every call"""
        return {}

    def _net_hw(self, h, w):
        """the size at which an h x w image (rectified, with rectify=) enters the network's frame (HighResInference: smaller)"""
        return h, w

    def _net_pair(self, s, left, right, h, w):
        """current stream: the uint8 pair on the device as it enters the frame, with its size (HighResInference: downscaled)"""
        return left, right, h, w

    def _fields(self, rows, cols, as_uint16):
        """the record of a frame whose maps are rows x cols: (name, dtype, shape) in the order they lie in the slot's buffer"""
        dtype = torch.uint16 if as_uint16 else torch.float32
        return [(name, dtype, (rows, cols)) for name in ("disp", "mask")[:self.nmaps]]

    def _fill(self, s, left, right, h, w, as_uint16):
        """current stream: histogram -> table -> frames -> model -> export into the slot's device output"""
        from . import ops
        if self._frames is None:
            self._frames = torch.empty((2, 3, self.crop_height, self.crop_width), device=s.device, dtype=torch.float32)
        left, right, h, w = self._net_pair(s, left, right, h, w)
        lut, _ = ops.frame_lut(ops.frame_histogram(left, right), h * w)
        fl, fr = ops.frame_apply(left, right, lut, self._room(), *s.frame.placement, out=self._frames)
        s.set_fields(self._fields(*s.out_hw, as_uint16))
        self._export(s, self._frame_maps(fl, fr, s.frame.cols), s.dev)

    def _export(self, s, maps, out):
        """current stream: the frame's maps, cropped to the image's window, into `out`, the fields in the slot's device output"""
        from . import ops
        for m, o, scale in zip(maps, out.values(), (256.0, self.CONF_U16_SCALE)):
            if o.dtype == torch.uint16:
                ops.disp_export(m.contiguous(), *s.frame.window, scale=scale, f32=False, u16=True, out_u16=o)
            else:
                ops.disp_export(m.contiguous(), *s.frame.window, out_f32=o)

    def __call__(self, left_rgb: np.ndarray, right_rgb: np.ndarray, as_uint16: bool = False):
        self._check_format(as_uint16)
        if self.device_io:
            return self._call_device(left_rgb, right_rgb, as_uint16)
        if self.rectify is not None:
            left_rgb, right_rgb = rectify_pair_host(left_rgb, right_rgb, self.rectify)
        left, right, h, w = pad_or_crop(normalize_pair(left_rgb, right_rgb), self.crop_height, self.crop_width)
        dev = next(self.net.parameters()).device
        maps = self._frame_maps(left.to(dev), right.to(dev), min(w, self.crop_width))
        if len(maps) == 1:
            disp = crop_back(maps[0].squeeze().cpu().numpy(), h, w, self.crop_height, self.crop_width)
            return (disp * 256).astype("uint16") if as_uint16 else disp           # my_img.py:110
        disp, conf = (crop_back(m.squeeze().cpu().numpy(), h, w, self.crop_height, self.crop_width) for m in maps)
        if as_uint16:      # fp32 products, truncated, as dca_disp_export
            return (disp * 256).astype("uint16"), (conf * np.float32(self.CONF_U16_SCALE)).astype("uint16")
        return disp, conf


class KittiInferenceWithConfidence(KittiInference):
    """`disp, conf = KittiInferenceWithConfidence(model, ..., radius=1)(left_rgb, right_rgb)`: KittiInference with the same
    arguments (host or device I/O, eager or graph, fp32 or reduced precision) whose `__call__` and `stream()` hand out a
    `(disp, conf)` tuple per frame.  `conf` is the probability mass of the final disparity distribution within `radius`
    1/4-res bins of its peak (GwcNet.predict's `confidence`), cropped by the same window as the disparity: float32 in
    [0,1], or uint16(conf * 65535) with as_uint16 (dca_disp_export with scale 65535).  The statistics launch is part of
    the captured hot path; with device I/O both maps come back in one copy and one synchronisation per frame.  The
    disparity is bitwise KittiInference's."""

    def __init__(self, model, *args, radius: int = 1, **kwargs):
        super().__init__(model, *args, **kwargs)
        self._take_mask("confidence", radius=radius)


class KittiInferenceLR(KittiInference):
    """`disp_filled, valid = KittiInferenceLR(model, ..., tau=1.0)(left_rgb, right_rgb)`: KittiInference with the same
    arguments (host or device I/O, eager or graph, fp32 or reduced precision) whose `__call__` and `stream()` hand out a
    `(disp_filled, valid)` tuple per frame (GwcNet.predict_lr's maps of those names; ops.lr_consistency).  Every frame
    takes two passes of the network: the frames as they are, then the mirrored, swapped frames (`ops.mirror_pair` of the
    float32 frames -- with device I/O the ones `frame_apply` wrote: the look-up table does not depend on the pixel
    order, so that is exact), which give the right view's disparity.  With `graph=True` both passes replay the SAME
    captured hot path; the first pass's 1/4-res disparity goes through the up-sampler, which allocates its result, before
    the second replay overwrites the graph's static buffers.  Only the image's own columns take part in the check (`cols`
    = its width inside the frame): the zero padding on the right is never matched against and never a fill source.
    `valid` is float32 1.0 / 0.0, or uint16 65535 / 0 with as_uint16 (dca_disp_export with scale 65535).  With device I/O
    both maps come back in one copy and one synchronisation per frame.  A frame costs about two of KittiInference's."""

    def __init__(self, model, *args, tau: float = 1.0, **kwargs):
        super().__init__(model, *args, **kwargs)
        self._take_mask("lr", tau=tau)

    def _frame_maps(self, left, right, cols):
        """its own case: the FILLED disparity (the classes behind a mask mode take the unfilled one)"""
        _, r = self._lr_maps(left, right, cols, ("valid", "filled"))
        return r["filled"], r["valid"]


class _HintsMixin:
    """The hints of a guided network as an instance holds them: `guide` = (k, c) of `ops.cost_volume`, or
    None for an unguided network; `hints4`, the ONE (1,Hc/4,Wc/4) buffer that every frame rewrites whole; and the two hooks of
    `forward_frame` that hand both to the (graphed) hot path.  Shared by KittiInferenceGuided (hints from outside) and
    KittiInferenceTemporal (hints from the previous frame)."""

    guide = None
    hints4 = None

    def _take_guide(self, guide):
        from .guided import guide_params
        guide_params(type(self).__name__, guide)
        if self.crop_height % 4 or self.crop_width % 4:
            raise ValueError(f"{type(self).__name__}: the frame must be a multiple of 4 in both directions")
        self.guide = (float(guide[0]), float(guide[1]))

    def _hot_kwargs(self):
        return {} if self.guide is None else {"guide": self.guide}

    def _hot_inputs(self):
        return {} if self.guide is None else {"hints4": self.hints4}

    def _hints4_buffer(self, dev):
        if self.hints4 is None:
            self.hints4 = torch.zeros((1, self.crop_height // 4, self.crop_width // 4), device=dev, dtype=torch.float32)
        return self.hints4


SGM_KEYS = ("max_disp", "paths", "P1", "P2", "uniqueness", "min_disp", "lr_tau")


def _check_sgm(name, opts):
    """the options of semi-global matching as a wrapper takes them (SGM_KEYS; the defaults are those of `ops.sgm_disparity`,
    max_disp 192 and lr_tau 1.0) -> (the keywords of `ops.sgm_disparity`, lr_tau or None)"""
    from . import sgm as _sgm
    if not isinstance(opts, dict) or set(opts) - set(SGM_KEYS):
        raise TypeError(f"{name}: the options of semi-global matching are a dict with keys out of {SGM_KEYS}, got {opts!r}")
    kw = dict(max_disp=192, paths=_sgm.SGM_PATHS, P1=_sgm.SGM_P1, P2=_sgm.SGM_P2, uniqueness=_sgm.SGM_UNIQUENESS,
              min_disp=_sgm.SGM_MIN_DISP)
    kw.update({k: v for k, v in opts.items() if k != "lr_tau"})
    kw = dict(zip(kw, _sgm.sgm_scalars(name, ValueError, _sgm.MIN_DIM, _sgm.MIN_DIM, **kw)))
    lr_tau = opts.get("lr_tau", 1.0)
    return kw, None if lr_tau is None else _check_tau(lr_tau)


class _SGM:
    """Per-slot buffers of semi-global matching for h x w images, allocated once: the workspace of `ops.sgm_disparity` and the
    maps it writes -- the left disparity and its validity, with a left-right check also the mirrored right view"""

    def __init__(self, device, h, w, max_disp, lr):
        from . import ops
        self.workspace = ops.sgm_workspace(h, w, max_disp, device)
        names = ("disp", "valid") + (("disp_right_mirrored",) if lr else ())
        self.out = {k: torch.empty((h, w), device=device, dtype=torch.float32) for k in names}


def _sgm_maps(s, left, right, kw, lr_tau):
    """current stream: (disp, valid), both float32 (h,w), of the uint8 pair as it lies in device memory:
    `ops.sgm_disparity` under the keywords `kw`; with `lr_tau` its right view -- read from the same aggregation -- goes through
    `ops.lr_consistency`, the two validities are multiplied and the disparity is +0.0 where the product is 0."""
    from . import ops
    h, w = int(left.shape[0]), int(left.shape[1])
    buf = s.scratch(("sgm", h, w), lambda: _SGM(s.device, h, w, kw["max_disp"], lr_tau is not None))
    r = ops.sgm_disparity(left, right, outputs=tuple(buf.out), out=buf.out, workspace=buf.workspace, **kw)
    disp, valid = r["disp"], r["valid"]
    if lr_tau is not None:
        valid = valid * ops.lr_consistency(disp[None], r["disp_right_mirrored"][None], lr_tau, outputs=("valid",))["valid"][0]
        disp = disp * valid
    return disp, valid


class KittiInferenceGuided(_HintsMixin, KittiInference):
    """`disp = KittiInferenceGuided(model, ...)(left_rgb, right_rgb, hints)`: KittiInference (device I/O; eager or graph, fp32
    or reduced precision, rectify=) whose network is guided by sparse disparity hints: `__call__` and
    `stream(triples)` take a third item per frame.
      lidar=None               the (h,w) float32 hint map of the image (the rectified image, with rectify=): a disparity in
                               pixels, +0.0 where nothing was measured; a numpy array (uploaded beside the pair) or a tensor
                               on the device (read on the current stream)
      lidar=geometry.LidarCalib   the (N,4) float32 scan: staged through a `geometry.LidarProjector` and projected with
                               `ops.lidar_disparity` (hw of the calibration = the image's size)
      sgm=dict(...)            NO third item: the hint map is computed from the pair itself by semi-global matching (DESIGN.md
                               section 6r) on the uint8 images already in device memory, under the options of SGM_KEYS
                               (`ops.sgm_disparity`'s, and lr_tau, default 1.0: its left-right check; None: none); an invalid
                               pixel is +0.0, "nothing measured".  Not together with lidar=.
    `ops.hints_to_quarter` writes the frame's hints through the frame's placement into ONE buffer the instance owns, and
    `forward_frame` hands it to the (graphed) hot path: no allocation per frame.  guide = (k, c) of `ops.cost_volume`.  The
    record handed out is KittiInference's.  Not combined with the other subclasses."""

    device_io = True
    needs_device_io = "the hints are brought to the network's frame on the device"
    sgm = None                   # the keywords of `ops.sgm_disparity`, with sgm=
    sgm_lr_tau = None

    def __init__(self, model, *args, lidar=None, sgm=None, guide=(10.0, 1.0), **kwargs):
        super().__init__(model, *args, **kwargs)
        self._take_guide(guide)
        if lidar is not None and not isinstance(lidar, LidarCalib):
            raise TypeError(f"lidar= must be a geometry.LidarCalib, got {type(lidar)}")
        if sgm is not None:
            if lidar is not None:
                raise ValueError("KittiInferenceGuided: sgm= computes the hints from the pair, lidar= from a scan: give one of them")
            self.sgm, self.sgm_lr_tau = _check_sgm("KittiInferenceGuided", sgm)
        self.lidar = lidar
        self._proj = None            # the LidarProjector, built with the first scan
        self.hints4 = None           # (1,Hc/4,Wc/4): the frame's hints, rewritten whole by every frame

    @torch.no_grad()
    def forward_frame(self, left, right, hints=None):
        """`hints` (1,Hc,Wc) or (Hc,Wc) float32 on the device: the hint map of the frame (a direct call); None: the hints
        `_net_pair` has put into `self.hints4`"""
        if hints is not None:
            from . import ops
            self._hints4_buffer(left.device)
            ops.hints_to_quarter(hints.reshape(1, self.crop_height, self.crop_width).contiguous(),
                                 (self.crop_height, self.crop_width), maxdisp=self.net.maxdisp, out=self.hints4)
        if self.hints4 is None:
            raise RuntimeError("KittiInferenceGuided.forward_frame: no hints yet (hand them in, or go through __call__)")
        return super().forward_frame(left, right)

    def __call__(self, left_rgb, right_rgb, hints=None, as_uint16: bool = False):
        self._check_format(as_uint16)
        self._check_item(hints)
        return self._call_device(left_rgb, right_rgb, as_uint16, hints)

    def _check_item(self, hints):
        if (hints is None) != (self.sgm is not None):
            raise TypeError("KittiInferenceGuided: with sgm= a frame is the pair alone, the hints are computed from it; without, a "
                            "frame is (left, right, hints)")

    def _upload(self, s, left_rgb, right_rgb, copy, hints=None):
        self._check_item(hints)
        super()._upload(s, left_rgb, right_rgb, copy)
        if self.sgm is not None:
            s.item = ("sgm", None)
            return
        hw = (s.frame.h, s.frame.w) if self.rectify is None else tuple(self.rectify.dst_hw)
        if self.lidar is not None:
            if tuple(self.lidar.hw) != hw:
                raise ValueError(f"lidar= projects into {self.lidar.hw[0]} x {self.lidar.hw[1]} images, got {hw[0]} x {hw[1]}")
            s.item = ("scan", hints)
            return
        if isinstance(hints, torch.Tensor):
            if not hints.is_cuda or hints.dtype != torch.float32 or tuple(hints.shape) != hw or not hints.is_contiguous():
                raise ValueError(f"hints must be a contiguous float32 {hw} map, got {hints.dtype} {tuple(hints.shape)}")
            s.item = ("map", hints)
            return
        hints = np.ascontiguousarray(hints)
        if hints.dtype != np.float32 or hints.shape != hw:
            raise ValueError(f"hints must be a float32 {hw} map of the image, got {hints.dtype} {hints.shape}")
        pin, dev = s.scratch(("hints",) + hw, lambda: (torch.empty(hw, dtype=torch.float32).pin_memory(),
                                                       torch.empty(hw, device=s.device, dtype=torch.float32)))
        pin.numpy()[:] = hints       # (the copy that last left this buffer is behind the `uploaded` the parent waited for)
        with torch.cuda.stream(copy):
            dev.copy_(pin, non_blocking=True)
            s.uploaded.record(copy)  # again: the pair and the hints
        s.item = ("map", dev)

    def _net_pair(self, s, left, right, h, w):
        """current stream: also the frame's `hints4`, from the slot's map (or scan) through the slot's placement"""
        from . import ops
        kind, item = s.item
        if kind == "scan":
            if self._proj is None:
                self._proj = LidarProjector(self.lidar, s.device, capacity=max(1 << 18, int(np.asarray(item).shape[0])))
            item = self._proj(item)["disp"]
        elif kind == "sgm":
            item = _sgm_maps(s, left, right, self.sgm, self.sgm_lr_tau)[0]
        ops.hints_to_quarter(item, self._room(), s.frame.placement, maxdisp=self.net.maxdisp,
                             out=self._hints4_buffer(s.device)[0])
        return left, right, h, w


class SGMInference(FramePipeline):
    """`disp, valid = SGMInference(max_disp=192, paths=8, P1=10, P2=120, uniqueness=15, lr_tau=1.0, median=0, speckle=None)(
    left_rgb, right_rgb)`: a disparity map without a network.  It takes NO model.  The uint8 pair is
    uploaded through the slots of FramePipeline (rectified first with rectify=), `ops.sgm_disparity` runs on it as it lies in
    device memory, and with `lr_tau` (None: off) `ops.lr_consistency` cross-checks the left view against `disp_right_mirrored`,
    which is read from the same aggregation: the two validities are multiplied and the disparity is +0.0 where the product is 0.
    Then the post-filter of section 6l on the same stream: `ops.median_filter` (`median` = 3 or 5; 0: off) and
    `ops.speckle_filter` (`speckle` = (max_size, max_diff); None: off) with that validity as the mask.  `disp` is float32 (h,w)
    in pixels, `valid` float32 1.0 / 0.0; both come back in ONE copy of exactly their bytes and one synchronisation per frame;
    `stream(pairs)` pipelines frames as for the other classes.  There is no frame to pad into: the maps are the image's own
    size, images of different sizes may follow each other (the buffers grow to the largest seen), each within the limits of
    `ops.sgm_disparity`.  No uint16 form.  device: where the frames live."""

    needs_device_io = "semi-global matching runs on the device only"
    has_uint16 = False
    mask_min = 0.5               # the post-filter's threshold on the validity

    def __init__(self, max_disp: int = 192, paths: int = 8, P1: int = 10, P2: int = 120, uniqueness: int = 15, lr_tau=1.0,
                 median: int = 0, speckle=None, rectify=None, *, min_disp: int = 1, device="cuda"):
        super().__init__(device=device, rectify=rectify)
        self.sgm, self.lr_tau = _check_sgm("SGMInference", dict(max_disp=max_disp, paths=paths, P1=P1, P2=P2, uniqueness=uniqueness,
                                                                min_disp=min_disp, lr_tau=lr_tau))
        self.median, self.speckle = _check_post(median, speckle)
        self._largest = (7, 7) if rectify is None else tuple(rectify.dst_hw)       # the largest image so far: the room of a frame

    def _room(self):
        return self._largest

    def _fields(self, rows, cols, as_uint16):
        return _disp_valid(rows, cols)

    def _upload(self, s, left_rgb, right_rgb, copy):
        if self.rectify is None and np.ndim(left_rgb) == 3:
            # room for the image's maps in THIS slot, whose previous frame has been handed out (rare: the largest image so far grew)
            h, w = np.shape(left_rgb)[:2]
            self._largest = (max(h, self._largest[0]), max(w, self._largest[1]))
            s.reserve_output(_nbytes(self._fields(*self._largest, False)), drop=("post",))     # (the post-filter's buffers too)
        super()._upload(s, left_rgb, right_rgb, copy)

    def _fill(self, s, left, right, h, w, as_uint16):
        """current stream: semi-global matching [-> left-right check] [-> post-filter] into the slot's device output"""
        s.set_fields(self._fields(h, w, False))
        disp, valid = _sgm_maps(s, left, right, self.sgm, self.lr_tau)
        if self.median or self.speckle is not None:
            # as KittiInferenceFiltered: without a speckle filter, max_size 0 keeps every active pixel
            _post_filter(self, s, disp, valid, (0, h, w), s.dev["disp"], self.speckle or (0, 0.0), False, s.dev["valid"])
        else:
            s.dev["disp"].copy_(disp)
            s.dev["valid"].copy_(valid)


def _check_post(median, speckle):
    """the `median=` / `speckle=` keywords of the wrappers: 0, 3 or 5 and None or (max_size, max_diff)"""
    if isinstance(median, bool) or median not in (0, 3, 5):
        raise ValueError(f"median is 0 (off), 3 or 5, got {median!r}")
    if speckle is not None:
        try:
            size, diff = speckle
            ok = int(size) == size and 0 <= int(size) < 1 << 31 and 0.0 <= float(diff) < float("inf")
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError(f"speckle is None or (max_size, max_diff) with an integer max_size >= 0 and a finite max_diff >= 0, "
                             f"got {speckle!r}")
        speckle = (int(size), float(diff))
    return int(median), speckle


class _Post:
    """Per-slot buffers of the post-filter (`median=`, `speckle=`), allocated once for the frame size: four float32 maps (the
    median's result, the mask cropped to the window, the filtered disparity, the filter's validity) and the union-find
    workspace of `ops.speckle_filter`."""

    def __init__(self, device, crop_height, crop_width):
        from . import ops
        self.maps = torch.empty((4, crop_height * crop_width), device=device, dtype=torch.float32)
        self.workspace = ops.speckle_workspace(crop_height, crop_width, device)


def _post_filter(infer, s, pred, mask, window, out_disp, speckle, fold, out_valid=None):
    """current stream: `infer.median`, then the speckle filter (max_size, max_diff) = `speckle` (None: none), over the window
    (y0, rows, cols) of the frame's disparity `pred`; mask (of pred's shape, or None) with
    `infer.mask_min` decides which pixels are active.  The filtered disparity goes to `out_disp`, the speckle filter's validity
    to `out_valid` if given.  Returns the (pred, mask, window) the following stage reads: the filtered disparity and the
    mask, both the window's own (rows,cols) from here on.  `fold`: the speckle filter's validity multiplies the mask (a
    removed pixel is no measurement), which is sound only where the stage behind applies a mask_min > 0.  Nothing is allocated
    after the slot's first frame, but the product of a fold."""
    from . import ops
    post = s.scratch("post", lambda: _Post(s.device, *infer._room()))
    y0, rows, cols = window
    med, cropped, disp, valid = (post.maps[k, :rows * cols].view(rows, cols) for k in range(4))
    pred = pred.view(pred.shape[-2:])
    if mask is not None:
        mask = mask.view(pred.shape)
        ops.disp_export(mask, y0, rows, cols, out_f32=cropped)
    else:
        cropped = None
    if infer.median:
        pred = ops.median_filter(pred, infer.median, mask, infer.mask_min, window, out=med)
        mask, window = cropped, None
    if speckle is None:                              # the median alone (the callers have one then)
        out_disp.copy_(med)
        return med, cropped, (0, rows, cols)
    r = ops.speckle_filter(pred, speckle[0], speckle[1], mask, infer.mask_min, window, outputs=("disp",),
                           out={"disp": out_disp, "valid": valid if out_valid is None else out_valid}, workspace=post.workspace)
    if fold:
        cropped = r["valid"] if cropped is None else cropped * r["valid"]
    return r["disp"], cropped, (0, rows, cols)


class _StageMixin:
    """What the stages behind the network share (KittiInferenceFiltered, KittiInference3D, KittiInferenceGround and so
    KittiInferenceStixels, KittiInferenceColor): the `median=` / `speckle=` keywords, and ONE preamble, `_stage_maps`, that turns
    the frame's maps into the (pred, mask, window) a stage reads."""

    _validity = False            # True: with rectify=, the maps' validity (`rectify.valid[0]`) is the mask, or multiplies it
    _valid_frame = None          # that validity placed in the frame, float32 (Hc,Wc), built once

    def _take_post(self, median, speckle):
        self.median, self.speckle = _check_post(median, speckle)

    def _validity_in_mask(self, mask_min, speckle=False):
        """the class lets `rectify=`'s validity into the mask (and states with `speckle=True` that it always folds the speckle
        filter's): both are 0 / 1, so a mask_min <= 0 would switch nothing off"""
        self._validity = True
        if self.rectify is not None and not float(mask_min) > 0.0:
            raise ValueError("with rectify= the maps' validity (0 / 1) enters the mask: mask_min must be > 0")
        if speckle and self.speckle is not None and not float(mask_min) > 0.0:
            raise ValueError("with speckle= the filter's validity (0 / 1) enters the mask: mask_min must be > 0")

    def _stage_maps(self, s, maps, out, fold, export=True, speckle=None, out_valid=None):
        """current stream: the frame's maps -> (pred, mask, window), 2-D views.  With `median=` / `speckle=` the post-filter runs
        (`fold`, `out_valid`: `_post_filter`'s; `speckle`: the filter to run in place of the instance's own) and writes the
        disparity it gives into out["disp"]; without, `export` puts the window of the disparity there.  Then `rectify=`'s validity
        enters the mask, where the class has said so: a pixel without a full source footprint is no measurement."""
        from . import ops
        f = s.frame
        pred, mask = _maps2d(maps)
        window = f.window
        speckle = self.speckle if speckle is None else speckle
        filtered = bool(self.median) or speckle is not None
        if filtered:
            pred, mask, window = _post_filter(self, s, pred, mask, window, out["disp"], speckle, fold, out_valid)
        elif export:
            ops.disp_export(pred, *window, out_f32=out["disp"])
        if self._validity and self.rectify is not None:
            valid = self._valid(pred.device, f)
            if filtered:                             # (pred and mask are the window's own from here on)
                valid = valid[f.dst_y0:f.dst_y0 + f.rows, :f.cols].contiguous()
            mask = valid if mask is None else mask * valid
        return pred, mask, window

    def _valid(self, device, f):
        """rectify.valid[0] as a float32 mask placed in the frame like the image; built once (the frame size is fixed)"""
        if self._valid_frame is None or self._valid_frame.device != device:
            frame = np.zeros(self._room(), np.float32)
            frame[f.dst_y0:f.dst_y0 + f.rows, :f.cols] = self.rectify.valid[0][f.src_y0:f.src_y0 + f.rows, :f.cols]
            self._valid_frame = torch.from_numpy(frame).to(device)
        return self._valid_frame


class KittiInferenceFiltered(_StageMixin, KittiInference):
    """`disp, valid = KittiInferenceFiltered(model, ..., median=0, speckle=(200, 2.0), mask=None | "confidence" | "lr")(left_rgb,
    right_rgb)`: KittiInference with device I/O (required: the filters run where the disparity lies) followed by the
    post-filter on the same stream: `ops.median_filter` (`median` = 3 or 5; 0: off), then
    `ops.speckle_filter` (`speckle` = (max_size, max_diff): components of at most max_size pixels of disparities chained
    within max_diff are removed; None: only pixels that are not active are removed), both over the image's own window of
    the padded frame -- the padding is never a neighbour.  `disp` is float32 (h,w), the filtered disparity, +0.0 where a
    pixel was removed; `valid` float32 1.0 / 0.0.  The mask mode decides which pixels are active, with `mask_min`:
      None          every finite pixel of KittiInference's disparity
      "confidence"  KittiInferenceWithConfidence's disparity where the window mass (`radius`) reaches mask_min
      "lr"          the UNFILLED left disparity where the cross-check (`tau`; two passes per frame) holds
    The result is `ops.speckle_filter(ops.median_filter(d, ...), ...)` of the map(s) those classes hand out, bit for bit.
    Buffers are allocated once per slot; both maps come back in one copy and one synchronisation per frame."""

    nmaps = 2
    device_io = True
    needs_device_io = "the filters run on the device, next to the disparity"
    has_uint16 = False

    def __init__(self, model, *args, median: int = 0, speckle=(200, 2.0), mask=None, mask_min: float = 0.5, radius: int = 1,
                 tau: float = 1.0, **kwargs):
        super().__init__(model, *args, **kwargs)
        self._take_mask(mask, mask_min, radius, tau)
        self._take_post(median, speckle)

    def _fields(self, rows, cols, as_uint16):
        return _disp_valid(rows, cols)

    def _export(self, s, maps, out):
        # without a speckle filter, max_size 0 keeps every active pixel: valid = active, and only the others go.  `valid` is
        # handed out itself: nothing behind reads the mask, so nothing is folded into it
        self._stage_maps(s, maps, out, False, speckle=self.speckle or (0, 0.0), out_valid=out["valid"])


class HighResInference(KittiInference):
    """`disp, valid = HighResInference(model, scale=2, crop_height=..., crop_width=..., radius=2, sigma_s=1.0, sigma_r=24.0,
    mask=None | "confidence" | "lr")(left_rgb, right_rgb)`: a pair that is LARGER than the network's frame (a Middlebury-F pair
    is about 2000 x 2964, the frame 384 x 1248) goes through the network at 1 / scale of its size and comes back at its own
    (DESIGN.md section 6m).  With device I/O (required: both resamplers read the uint8 pair where it lies), per frame: one
    upload of the full-resolution pair, `ops.area_downscale_pair` (the reference's INTER_AREA halving for scale 2), the
    unchanged histogram / table / `frame_apply` path on the small pair, the network, the mask of the chosen mode, ONE launch
    of `ops.guided_upsample` straight from the padded frame through its window, guided by the full-resolution left image,
    one read-back.  `crop_height`, `crop_width` are NETWORK-resolution sizes; the small image, ceil(H / scale) x
    ceil(W / scale), must fit the frame.  `disp` is float32 (H,W) in FULL-resolution pixels (the network's values times
    scale): the disparity range becomes scale * maxdisp.  `valid` is float32 1.0 / 0.0: 0 where no tap of the upsampler was
    active (`disp` is +0.0 there).  The taps per mode, with `mask_min`:
      None          every finite disparity > 0 of KittiInference's map
      "confidence"  those whose window mass (`conf_radius`) reaches mask_min
      "lr"          those of the UNFILLED left disparity that pass the cross-check (`tau`; two passes per frame)
    `radius`, `sigma_s`, `sigma_r`, `floor`: `highres.jbu_tables`; the defaults were not tuned on real data.  The result is
    `ops.guided_upsample` of the map(s) the existing class of that mode hands out for the downscaled pair, bit for bit.
    `rectify=maps`: the raw pair is rectified at full resolution first.  With one fp32 sample below 2 GiB per tensor the
    largest is the cost volume, channels x maxdisp / 4 x H / 4 x W / 4 floats at network resolution: at maxdisp 192 that is
    fewer than 279,620 quarter-resolution pixels for the 40-channel volume of GwcNet-G and 174,762 for the 64 channels of
    GwcNet-GC -- network frames up to 1024 x 4368 or 1632 x 2736 (G) and 1024 x 2720 or 1280 x 2176 (GC), so at scale 2
    full-resolution pairs up to 2048 x 8736 (G) and 2048 x 5440 (GC); a Middlebury-F pair at scale 2 (1000 x 1482 ->
    frame 1008 x 1488) fits both."""

    nmaps = 2
    needs_device_io = "the resamplers read the uint8 pair on the device"
    has_uint16 = False
    MASKS = (None, "confidence", "lr")

    def __init__(self, model, scale: int = 2, crop_height: int = 384, crop_width: int = 1248, graph: bool = True, dtype=None,
                 device_io: bool = True, radius: int = 2, sigma_s: float = 1.0, sigma_r: float = 24.0, floor: float = 1e-4,
                 mask=None, mask_min: float = 0.5, conf_radius: int = 1, tau: float = 1.0, *, rectify=None):
        from . import highres
        if isinstance(scale, bool) or not isinstance(scale, int) or not 2 <= scale <= highres.HR_MAX_SCALE:
            raise ValueError(f"HighResInference: scale is an integer in 2..{highres.HR_MAX_SCALE}, got {scale!r}")
        self.scale = self.out_scale = scale             # (`_net_hw` reads it when the parent fits rectify= into the frame)
        super().__init__(model, crop_height, crop_width, graph, dtype, device_io, rectify=rectify)
        self._take_mask(mask, mask_min, conf_radius, tau)       # (`radius` of the parent: the confidence window)
        self.tables = highres.jbu_tables(scale, radius, sigma_s, sigma_r, floor)        # (refuses what it cannot do)
        self._tables_dev = None

    def _net_hw(self, h, w):
        from .highres import small_hw
        hs, ws = small_hw(h, w, self.scale)
        if hs > self.crop_height or ws > self.crop_width:
            raise ValueError(f"a {h} x {w} image is {hs} x {ws} at 1/{self.scale} and does not fit the {self.crop_height} x "
                             f"{self.crop_width} frame")
        return hs, ws

    def _net_pair(self, s, left, right, h, w):
        from . import ops
        hs, ws = self._net_hw(h, w)
        c = left.shape[2]
        s.out_hw = (h, w)                                # the maps come back at the image's own size
        small = ops.area_downscale_pair(left, right, self.scale, out=self._small(s, hs, ws, c))
        return small[0], small[1], hs, ws

    def _small(self, s, hs, ws, c):
        """the slot's downscaled pair, (2,hs,ws,c) uint8, in a buffer with room for the largest the frame takes"""
        buf = s.scratch("small", lambda: torch.empty(2 * self.crop_height * self.crop_width * 4, device=s.device, dtype=torch.uint8))
        return buf[:2 * hs * ws * c].view(2, hs, ws, c)

    def _fields(self, h, w, as_uint16):
        return _disp_valid(h, w)

    def _export(self, s, maps, out):
        from . import highres, ops
        if self._tables_dev is None or self._tables_dev[0].device != s.device:
            self._tables_dev = highres.device_tables(self.tables, s.device)
        f = s.frame
        pred = maps[0].contiguous()
        mask = maps[1].contiguous().view_as(pred) if len(maps) > 1 else None
        guide_lo = self._small(s, f.rows, f.cols, s.left.shape[2])[0]        # (the small image fits the frame: the window is its size)
        ops.guided_upsample(pred, guide_lo, s.left, self.scale, self._tables_dev, f.window, mask, self.mask_min, out=out)


Frame3D = collections.namedtuple("Frame3D", "disp mask depth vertices")


class _Geo:
    """Per-slot buffers of KittiInference3D beyond the frame's record, allocated once for the frame size: `vert`, the vertex
    records with room for the worst case of the frame, on the device and pinned, and the offsets workspace of `ops.point_cloud`."""

    def __init__(self, device, crop_height, crop_width, stride):
        from . import ops
        cap = -(-crop_height // stride) * -(-crop_width // stride)
        self.vert_dev = torch.empty((cap, 4), device=device, dtype=torch.float32)
        self.vert_pin = torch.empty((cap, 4), dtype=torch.float32).pin_memory()
        self.offsets = ops.point_cloud_workspace(crop_height, crop_width, device)[0]


class KittiInference3D(_StageMixin, KittiInference):
    """`disp, mask, depth, vertices = KittiInference3D(model, calib, mask=None | "confidence" | "lr", ...)(left_rgb,
    right_rgb)`: KittiInference with device I/O (required: the colours are the uint8 left image that already lies in device
    memory) followed by the geometry stage on the same stream: `ops.disp_to_depth` and
    `ops.point_cloud` under `calib` (a geometry.StereoCalib of the images as they are handed in; with `rectify=` of the rectified pair, by default the
    maps' own `calib`, and pixels whose source footprint leaves the raw image -- `rectify.valid[0] == 0` -- get depth 0 and no
    vertex: the validity map is the mask, or multiplies it), `min_disp`, `max_depth`,
    `stride` and, with a mask, `mask >= mask_min`.  The disparity and the mask per mode:
      None          KittiInference's disparity, no mask (`mask` of the result is None)
      "confidence"  KittiInferenceWithConfidence's disparity and window mass (`radius`)
      "lr"          the UNFILLED left disparity and the validity map of the cross-check (`tau`; two passes per frame): a
                    filled pixel is a guess, not a measurement, and must not become a point
    `depth` is float32 metres, 0 where no point is; `vertices` a geometry.PLY_VERTEX array of exactly the kept pixels in
    row-major order, in the left camera's frame (`geometry.write_ply` stores it as it is).  All buffers of a frame in
    flight are allocated once per slot.  The read-back is one copy of the maps with the count in front, then -- once that
    count is on the host -- one copy of exactly count * 16 bytes of vertices: ONE more host wait per frame than the other
    classes have, on that frame's own copy only; in `stream()` the later frames keep computing meanwhile, and the vertex copy
    of frame i goes onto the copy stream directly behind that frame's maps.
    `median=3 | 5` and `speckle=(max_size, max_diff)` (keywords, off by default) put the post-filter of
    KittiInferenceFiltered in front of the geometry stage: `disp` is then the filtered disparity, and the speckle filter's
    validity multiplies the mask exactly where `rectify`'s does -- a removed pixel gets depth 0 and no vertex (mask_min
    must be > 0).  With the defaults every result is byte for byte what it is without the keywords."""

    # (`device_io` stays False here: this class has always asked for device_io=True to be written out)
    needs_device_io = "the point colours are read from the uint8 image on the device"
    has_uint16 = False
    Frame = Frame3D

    def __init__(self, model, calib=None, *args, mask=None, mask_min: float = 0.5, min_disp: float = 0.0,
                 max_depth: float = 80.0, stride: int = 1, radius: int = 1, tau: float = 1.0, speckle=None, median: int = 0,
                 **kwargs):
        from . import frame_ops
        super().__init__(model, *args, **kwargs)
        self._take_post(median, speckle)
        calib = self._calib_or_maps(calib)
        self._validity_in_mask(mask_min, speckle=True)
        if int(stride) < 1:
            raise ValueError("stride >= 1")
        frame_ops._geo_scalars("KittiInference3D", calib, mask_min, min_disp, max_depth)       # the operators' ranges, up front
        self._take_mask(mask, mask_min, radius, tau)
        self.calib, self.stride = calib, int(stride)
        self.filters = dict(mask_min=self.mask_min, min_disp=float(min_disp), max_depth=float(max_depth))

    def _fields(self, rows, cols, as_uint16):
        """16 bytes of `count` (2 int64), then the maps (disparity[, mask], depth): one copy brings the maps AND the count"""
        maps = ("disp", "mask", "depth") if self.nmaps == 2 else ("disp", "depth")
        return [("count", torch.int64, (2,))] + [(name, torch.float32, (rows, cols)) for name in maps]

    def _geo(self, s):
        return s.scratch("geo", lambda: _Geo(s.device, self.crop_height, self.crop_width, self.stride))

    def _export(self, s, maps, out):
        from . import ops
        g = self._geo(s)
        pred, mask = _maps2d(maps)
        ops.disp_export(pred, *s.frame.window, out_f32=out["disp"])
        if mask is not None:
            ops.disp_export(mask, *s.frame.window, out_f32=out["mask"])
        # the disparity handed out is the filtered one (the post-filter overwrites the export above); a removed pixel is no
        # measurement: depth 0, no vertex (mask_min > 0 is enforced with speckle=, so the fold always holds).  The mask handed out
        # stays as it is
        pred, mask, window = self._stage_maps(s, (pred, mask), out, True, export=False)
        ops.disp_to_depth(pred, self.calib, window, mask, out_f32=out["depth"], **self.filters)
        ops.point_cloud(pred, self.calib, s.left, mask, window, v0=s.frame.src_y0, stride=self.stride,
                        out=g.vert_dev, workspace=(g.offsets, out["count"]), **self.filters)

    def _rest(self, s, head):
        """the vertex step: the count is on the host, so exactly the written records follow the maps on their copy stream;
        the frame's second host wait is for them"""
        from .geometry import PLY_VERTEX
        g = self._geo(s)
        written = int(head["count"][1])
        with torch.cuda.stream(s.copy):
            if written:
                g.vert_pin[:written].copy_(g.vert_dev[:written], non_blocking=True)
            s.done.record(s.copy)

        def vertices():
            s.done.synchronize()
            return {"vertices": g.vert_pin[:written].numpy().view(PLY_VERTEX).reshape(-1).copy()}
        return vertices


FrameGround = collections.namedtuple("FrameGround", "disp label free_row free_disp bev plane")


class _Ground:
    """Per-slot buffers of KittiInferenceGround beyond the frame's record, allocated once for the frame size: the v-disparity
    histogram and the workspace of `ops.ground_plane`."""

    def __init__(self, device, crop_height, crop_width, max_disp):
        from . import ops
        self.vdisp = torch.empty((crop_height, max_disp), device=device, dtype=torch.int32)
        self.workspace = ops.ground_workspace(crop_height, crop_width, max_disp, device)


class KittiInferenceGround(_StageMixin, KittiInference):
    """`disp, label, free_row, free_disp, bev, plane = KittiInferenceGround(model, calib, mask=None | "confidence" | "lr", ...)(
    left_rgb, right_rgb)`: KittiInference with device I/O (required: the stage runs where the disparity lies) followed by the
    ground stage on the same stream: `ops.ground_plane` -- v-disparity, Hough line, least squares with
    roll -- and `ops.ground_segment` under `calib` (a geometry.StereoCalib of the images as they are handed in; with `rectify=`
    of the rectified pair, by default the maps' own `calib`, and pixels whose source footprint leaves the raw image are no
    measurement: the maps' validity is the mask, or multiplies it; mask_min must be > 0 then).  The disparity and the mask per
    mode are KittiInference3D's: None, "confidence" (`radius`) or "lr" (`tau`; the UNFILLED left disparity, two passes per frame).
    `median=3 | 5` and `speckle=(max_size, max_diff)` (off by default) run the post-filter of
    KittiInferenceFiltered BEFORE the fit: `disp` is then the filtered disparity, a removed pixel is no measurement.
      disp       float32 (h,w)        the disparity the stage read
      label      uint8   (h,w)        0 no data, 1 ground, 2 obstacle, 3 overhang, 4 below ground
      free_row   int32   (w,)         the base row of the lowest obstacle of every column, -1: none; free_disp float32 (w,): its disparity
      bev        int32   (2,NZ,NX)    ground / obstacle pixels per cell of `grid` = (cell, x_half, z_max) in metres
      plane      float64 (16,)        the plane record (`ground.PLANE_FIELDS`; `ground.plane_pose(plane, calib, v0)` gives the camera's
                                      height, pitch and roll; v0 = the image row of the window's first row, 0 for an image
                                      that fits the frame)
    `max_disp`: the histogram's bins, default the model's `maxdisp`; `min_disp`: the smallest valid disparity; `plane`, `segment`:
    dicts of further keywords of `ops.ground_plane` (fit_rows, refine, tol, min_rise, min_votes, min_inliers) and
    `ops.ground_segment` (tol_d, h_ground, h_max, min_run).  All buffers are allocated once per slot; the whole record comes
    back in one copy and one synchronisation per frame."""

    device_io = True
    needs_device_io = "the ground stage runs on the device, next to the disparity"
    has_uint16 = False
    Frame = FrameGround
    PLANE_KEYS = ("fit_rows", "refine", "tol", "min_rise", "min_votes", "min_inliers")
    SEGMENT_KEYS = ("tol_d", "h_ground", "h_max", "min_run")

    def __init__(self, model, calib=None, *args, mask=None, mask_min: float = 0.5, radius: int = 1, tau: float = 1.0, speckle=None,
                 median: int = 0, max_disp=None, min_disp=None, grid=None, plane=None, segment=None, **kwargs):
        from . import ground as G
        super().__init__(model, *args, **kwargs)
        name = type(self).__name__
        self._take_post(median, speckle)
        calib = self._calib_or_maps(calib)
        self._validity_in_mask(mask_min)
        self._take_mask(mask, mask_min, radius, tau)
        max_disp = self._max_disp_or_model(max_disp)
        plane, segment = dict(plane or {}), dict(segment or {})
        if set(plane) - set(self.PLANE_KEYS) or set(segment) - set(self.SEGMENT_KEYS):
            raise ValueError(f"{name}: plane= takes {self.PLANE_KEYS} and segment= takes {self.SEGMENT_KEYS}, got {sorted(plane)} and "
                             f"{sorted(segment)}")
        self.min_disp = G.GROUND_MIN_DISP if min_disp is None else float(min_disp)
        self.grid = G.GROUND_GRID if grid is None else tuple(float(v) for v in grid)
        # the operators' ranges, up front (fit_rows is checked against the frame; an image may be smaller)
        p = dict(rows_range=plane.get("fit_rows"), min_rise=G.GROUND_MIN_RISE, min_votes=None, refine=G.GROUND_REFINE,
                 min_inliers=G.GROUND_MIN_INLIERS, tol=G.GROUND_TOL)
        p.update({k: v for k, v in plane.items() if k != "fit_rows"})
        G.plane_scalars(name, ValueError, self.crop_height, self.crop_width, max_disp, min_disp=self.min_disp, **p)
        G.calib_scalars(name, ValueError, calib)
        g = dict(tol_d=G.GROUND_TOL_D, h_ground=G.GROUND_H_GROUND, h_max=G.GROUND_H_MAX, min_run=G.GROUND_MIN_RUN)
        g.update(segment)
        self._cells = G.segment_scalars(name, ValueError, max_disp, self.min_disp, grid=self.grid, **g)[-1][3:]       # (NX, NZ)
        self.calib, self.max_disp, self.plane_kw, self.segment_kw = calib, int(max_disp), plane, segment

    def _fields(self, rows, cols, as_uint16):
        """the doubles first, the bytes last: every field lies at a multiple of its element size"""
        NX, NZ = self._cells
        return [("plane", torch.float64, (16,)), ("disp", torch.float32, (rows, cols)), ("free_row", torch.int32, (cols,)),
                ("free_disp", torch.float32, (cols,)), ("bev", torch.int32, (2, NZ, NX)), ("label", torch.uint8, (rows, cols))]

    def _export(self, s, maps, out):
        from . import ops
        pred, frame = self._plane(s, maps, out)
        names = ("label", "free_row", "free_disp", "bev")
        ops.ground_segment(pred, out["plane"], self.calib, grid=self.grid, outputs=names, out={k: out[k] for k in names}, **frame,
                           **self.segment_kw)

    def _plane(self, s, maps, out):
        """current stream: the filters, then `ops.ground_plane` into out["plane"] (and the disparity it read into out["disp"]);
        returns that disparity and the frame keywords (max_disp, mask, mask_min, window, min_disp) of the stage behind"""
        from . import ops
        g = s.scratch("ground", lambda: _Ground(s.device, self.crop_height, self.crop_width, self.max_disp))
        # the filters run before the fit; a removed pixel is +0.0, below every min_disp > 0, and leaves the mask where it has one
        pred, mask, window = self._stage_maps(s, maps, out, self.mask_min > 0.0)
        frame = dict(max_disp=self.max_disp, mask=mask, mask_min=self.mask_min, window=window, min_disp=self.min_disp)
        ops.ground_plane(pred, calib=self.calib, v0=s.frame.src_y0, workspace=g.workspace,
                         out={"plane": out["plane"], "vdisp": g.vdisp[:s.frame.rows]}, **frame, **self.plane_kw)
        return pred, frame


FrameStixels = collections.namedtuple("FrameStixels", "disp plane count stixels energy")


class KittiInferenceStixels(KittiInferenceGround):
    """`disp, plane, count, stixels, energy = KittiInferenceStixels(model, calib, mask=None | "confidence" | "lr", ...)(left_rgb,
    right_rgb)`: KittiInferenceGround's mask source, filters (`median=`, `speckle=`) and plane fit (`plane=`), followed on the
    same stream by `ops.stixels` instead of the per-pixel segmentation: the image is cut into columns of
    `width` pixels and cells of `row_step` rows, and every column bottom-up into ground / object / sky segments.
      disp     float32 (h,w)                       the disparity the stage read
      plane    float64 (16,)                       the plane record (`ground.PLANE_FIELDS`)
      count    int32   (w // width,)               the segments of every column (also beyond max_segments); 0: no road plane
      stixels  int32   (w // width, max_segments, 4)   bottom-up: first and last row of `disp`, class 0 / 1 / 2, disparity in
                                                   sixteenths (-1: none); zero beyond `count`
      energy   int64   (w // width,)               the column's least energy
    `stixel.stixels_metric(stixels, count, plane, calib, width)` gives X, Z and the heights of foot and head in metres.
    `stixel=`: a dict of further keywords of `ops.stixels` (min_valid, params).  A few hundred records per frame instead of a
    label per pixel; the whole record comes back in one copy and one synchronisation per frame."""

    needs_device_io = "the stixel stage runs on the device, next to the disparity"
    Frame = FrameStixels
    STIXEL_KEYS = ("min_valid", "params")

    def __init__(self, model, calib=None, *args, width=None, row_step=None, max_segments=None, stixel=None, **kwargs):
        from . import stixel as S
        if "grid" in kwargs or "segment" in kwargs:
            raise TypeError(f"{type(self).__name__} has no per-pixel segmentation: grid= and segment= belong to KittiInferenceGround")
        super().__init__(model, calib, *args, **kwargs)
        name = type(self).__name__
        stixel = dict(stixel or {})
        if set(stixel) - set(self.STIXEL_KEYS):
            raise ValueError(f"{name}: stixel= takes {self.STIXEL_KEYS}, got {sorted(stixel)}")
        # the operator's ranges, up front, for the frame (an image may be smaller: the operator checks it again)
        _, self.width, self.row_step, _, self.max_segments, _, _, _ = S.grid_scalars(
            name, ValueError, self.crop_height, self.crop_width, self.max_disp, S.STIXEL_WIDTH if width is None else width,
            S.STIXEL_ROW_STEP if row_step is None else row_step, stixel.get("min_valid", S.STIXEL_MIN_VALID),
            S.STIXEL_MAX_SEGMENTS if max_segments is None else max_segments, self.min_disp)
        S.energy_params(name, ValueError, stixel.get("params"))
        self.stixel_kw = stixel

    def _fields(self, rows, cols, as_uint16):
        """the 8-byte fields first: every field lies at a multiple of its element size"""
        CS = cols // self.width
        return [("plane", torch.float64, (16,)), ("energy", torch.int64, (CS,)), ("disp", torch.float32, (rows, cols)),
                ("count", torch.int32, (CS,)), ("stixels", torch.int32, (CS, self.max_segments, 4))]

    def _export(self, s, maps, out):
        from . import ops
        pred, frame = self._plane(s, maps, out)
        ws = s.scratch("stixel", lambda: ops.stixel_workspace(self.crop_height, self.crop_width, s.device, self.width, self.row_step))
        names = ("count", "stixels", "energy")
        ops.stixels(pred, out["plane"], width=self.width, row_step=self.row_step, max_segments=self.max_segments, outputs=names,
                    out={k: out[k] for k in names}, workspace=ws, **frame, **self.stixel_kw)


FrameTemporal = collections.namedtuple("FrameTemporal", "disp var age")


class _Temporal:
    """What KittiInferenceTemporal keeps between the frames of a sequence, for images whose window is rows x cols: the state
    (disp, var, age), the prediction (pred, var, age, hints) and the workspace of `ops.disp_reproject`.  Allocated once."""

    def __init__(self, device, rows, cols):
        from . import ops
        f32 = dict(device=device, dtype=torch.float32)
        self.state = {"disp": torch.zeros((rows, cols), **f32), "var": torch.zeros((rows, cols), **f32),
                      "age": torch.zeros((rows, cols), device=device, dtype=torch.uint8)}
        self.pred = {"pred": torch.zeros((rows, cols), **f32), "var": torch.zeros((rows, cols), **f32),
                     "age": torch.zeros((rows, cols), device=device, dtype=torch.uint8), "hints": torch.zeros((rows, cols), **f32)}
        self.workspace = ops.temporal_workspace(rows, cols, device)


class KittiInferenceTemporal(_HintsMixin, KittiInference):
    """`disp, var, age = KittiInferenceTemporal(model, calib, ...)(left_rgb, right_rgb, pose)`: KittiInference with device I/O
    (required: the state lives where the disparity lies) over a SEQUENCE: `__call__` and
    `stream(triples)` take the camera's world pose as a third item per frame -- a (4,4) or (3,4) array, camera coordinates ->
    world coordinates, of the rectified left camera (`geometry.read_kitti_poses`, `geometry.oxts_poses`) -- and every frame
    does, on the compute stream, in input order:
      1. `ops.disp_reproject`: the state of the frame before, warped by the ego-motion between the two poses into this image;
      2. with guide=(k, c): `ops.hints_to_quarter` of the prediction's `hints` into the instance's `hints4` buffer, which guides
         the network as LiDAR hints guide KittiInferenceGuided's (zero hints, the first frame's, are the unguided network bit
         for bit);
      3. the network (eager or graph, fp32 or reduced precision; mask=None | "confidence" | "lr" as KittiInference3D has them);
      4. `ops.temporal_fuse` of prediction and measurement into the new state.
    calib: the geometry.StereoCalib of the images as they are handed in; with `rectify=` of the rectified pair, by default the
    maps' own.  meas_var: the variance of a measurement in px^2, a scalar; q, occl, hint_min_age, min_disp, max_disp (default the
    model's maxdisp): `ops.disp_reproject`'s; gate, var_max: `ops.temporal_fuse`'s; None means the named default of temporal.py
    (meas_var 0.25, q 0, gate 3, occl (1, 1, 1.0), hint_min_age 1, min_disp 1/16, var_max inf).  pose=None, an image of another size, or
    `reset()` drops the state: that frame is a first frame.  The state lives in two buffer sets and a workspace that the
    instance owns, allocated with the first frame of a size; a frame hands out
      disp float32 (h,w)   the fused disparity, +0.0: nothing     var float32 (h,w)   its variance in px^2
      age  uint8   (h,w)   the frames since the pixel's filter started
    in one copy and one synchronisation.  The reprojection takes the pose by value and is launched eagerly, in front of the
    graph.  No accuracy is claimed for guide=: the repository ships no trained weights.  Not combined with the other subclasses."""

    device_io = True
    needs_device_io = "the state of the sequence lives on the device, next to the disparity"
    has_uint16 = False
    Frame = FrameTemporal

    def __init__(self, model, calib=None, *args, guide=None, meas_var: float = None, q: float = None, gate: float = None,
                 occl=None, hint_min_age: int = None, mask=None, mask_min: float = 0.5, radius: int = 1, tau: float = 1.0,
                 min_disp: float = None, max_disp: float = None, var_max: float = None, **kwargs):
        from . import temporal as T
        super().__init__(model, *args, **kwargs)
        name = type(self).__name__
        calib = self._calib_or_maps(calib)
        self._take_mask(mask, mask_min, radius, tau)
        if guide is not None:
            if mask == "lr":
                raise ValueError(f"{name}: guide= is not combined with mask='lr' (the second, mirrored pass has no hints of its own)")
            self._take_guide(guide)
        max_disp = self._max_disp_or_model(max_disp)
        pick = lambda v, default: default if v is None else v      # noqa: E731
        self.reproject_kw = dict(max_disp=float(max_disp), min_disp=float(pick(min_disp, T.TEMPORAL_MIN_DISP)),
                                 occl=tuple(pick(occl, T.TEMPORAL_OCCL)), q=float(pick(q, T.TEMPORAL_Q)),
                                 hint_min_age=pick(hint_min_age, T.TEMPORAL_HINT_MIN_AGE))
        self.fuse_kw = dict(meas_var=float(pick(meas_var, T.TEMPORAL_MEAS_VAR)), min_disp=self.reproject_kw["min_disp"],
                            gate=float(pick(gate, T.TEMPORAL_GATE)), var_max=float(pick(var_max, T.TEMPORAL_VAR_MAX)))
        # the operators' ranges, up front
        T.reproject_matrix(calib, np.eye(4))
        T.reproject_scalars(name, ValueError, self.crop_height, self.crop_width, np.eye(3, 4), T._doffs(name, ValueError, calib, None),
                            min_ratio=T.TEMPORAL_MIN_RATIO, **self.reproject_kw)
        T.fuse_scalars(name, ValueError, **self.fuse_kw)
        self.calib = calib
        self._sets = {}              # (rows, cols) -> _Temporal
        self._last = None            # (the pose, (src_y0, rows, cols)) of the frame that wrote the state; None: no state

    def reset(self):
        """drops the state: the next frame is a first frame"""
        self._last = None

    def __call__(self, left_rgb, right_rgb, pose, as_uint16: bool = False):
        self._check_format(as_uint16)
        return self._call_device(left_rgb, right_rgb, as_uint16, pose)

    def _upload(self, s, left_rgb, right_rgb, copy, pose):
        """host, in input order: also the frame's matrix G from the pose before and this one (None: a first frame)"""
        from . import temporal as T
        from .geometry import _pose44, relative_pose
        if pose is not None:
            pose = _pose44(pose, type(self).__name__)
        super()._upload(s, left_rgb, right_rgb, copy)
        src_y0 = s.frame.src_y0
        key = (src_y0, s.frame.rows, s.frame.cols)
        if pose is not None and self._last is not None and self._last[1] == key:
            # the window's row 0 is image row src_y0: the principal point moves up by as much
            cal = self.calib if src_y0 == 0 else type(self.calib)(self.calib.f, self.calib.baseline, self.calib.cx,
                                                                 self.calib.cy - src_y0, self.calib.doffs)
            s.item = T.reproject_matrix(cal, relative_pose(self._last[0], pose))
        self._last = None if pose is None else (pose, key)

    def _set(self, s):
        rows, cols = s.frame.rows, s.frame.cols
        if (rows, cols) not in self._sets:
            self._sets[(rows, cols)] = _Temporal(s.device, rows, cols)
        return self._sets[(rows, cols)]

    def _net_pair(self, s, left, right, h, w):
        """current stream, in front of the network: the prediction from the state of the frame before, and the frame's `hints4`"""
        from . import ops
        t = self._set(s)
        if s.item is not None:
            names = ("pred", "var", "age") + (("hints",) if self.guide is not None else ())
            ops.disp_reproject(t.state, s.item, self.calib, outputs=names, out={k: t.pred[k] for k in names}, workspace=t.workspace,
                               **self.reproject_kw)
        if self.guide is not None:
            if s.item is not None:
                ops.hints_to_quarter(t.pred["hints"], (self.crop_height, self.crop_width), (0,) + s.frame.window,
                                     maxdisp=self.net.maxdisp, out=self._hints4_buffer(s.device)[0])
            else:
                self._hints4_buffer(s.device).zero_()
        return left, right, h, w

    def _fields(self, rows, cols, as_uint16):
        """the floats first, the bytes last: every field lies at a multiple of its element size"""
        return [("disp", torch.float32, (rows, cols)), ("var", torch.float32, (rows, cols)), ("age", torch.uint8, (rows, cols))]

    def _export(self, s, maps, out):
        """current stream, behind the network: prediction and measurement into the state, the state into the record"""
        from . import ops
        t = self._set(s)
        meas = maps[0].contiguous()
        mask = maps[1].contiguous() if len(maps) > 1 else None
        ops.temporal_fuse(t.pred if s.item is not None else None, meas, window=s.frame.window, mask=mask, mask_min=self.mask_min,
                          out=t.state, **self.fuse_kw)
        for k, v in t.state.items():
            out[k].copy_(v, non_blocking=True)


FrameOdometry = collections.namedtuple("FrameOdometry", "disp var age pose motion count residual status")


class _Odometry:
    """What KittiInferenceOdometry keeps between the frames of a sequence beside _Temporal's, for windows of rows x cols: two
    grey pyramids (the previous and the current left image, swapped per frame), the disparity pyramid of the state, the
    estimate's record, matrices and workspace, and the world pose.  Allocated once."""

    def __init__(self, device, rows, cols, levels):
        from . import odometry as OD
        n = OD.pyramid_len(rows, cols, levels)
        self.grey = [torch.empty(n, device=device, dtype=torch.uint8) for _ in range(2)]
        self.cur = 0                                         # the index of the pyramid the NEXT frame writes
        self.dpyr = torch.empty(n, device=device, dtype=torch.float32)
        self.rec = torch.zeros(OD.REC_LEN, device=device, dtype=torch.float64)
        self.g = torch.zeros(24, device=device, dtype=torch.float32)
        self.sums = torch.zeros(OD.SUMS, device=device, dtype=torch.int64)
        self.world = torch.zeros(12, device=device, dtype=torch.float64)
        self.window = None                                   # the window's pixels where the image is wider than it
        self.have_rec = False                                # the record holds the motion of the frame before


class KittiInferenceOdometry(KittiInferenceTemporal):
    """`frame = KittiInferenceOdometry(model, calib, ...)(left_rgb, right_rgb)`: KittiInferenceTemporal for a sequence WITHOUT
    poses: a stereo-2015 pair, a Middlebury sequence, a user's own rig.  `__call__` and `stream(pairs)`
    take (left, right); the motion of the left camera since the frame before is estimated on the device from that frame's
    disparity state and the two left images, and every frame does, on the compute stream, in input order, in front of the network:
      1. `ops.grey_pyramid` of the current left image (the window of it that the state covers), from the uint8 frame in device memory;
      2. `ops.ego_motion` against the pyramids kept from the frame before, started from the motion of the frame before
         (init="last": constant velocity; a failed or missing one: the identity) or always from the identity (init="identity");
      3. `ops.disp_reproject` with the matrix G the estimate left ON THE DEVICE -- the host never sees it;
    then KittiInferenceTemporal's own work (guide= included) with that prediction, and behind the fuse
      4. `ops.disp_pyramid` of the new state, the swap of the image pyramids, and `ops.pose_chain`:
         T_world <- T_world T_cur_from_prev^-1 on the device.
    A failed estimate (too few textured pixels with disparity, a singular system) leaves G as NaN: the prediction is empty, the
    fuse starts every pixel again from the measurement, the world pose stays.  The first frame, an image of another size and
    `reset()` start a sequence: no estimate runs, the world pose is the identity.  levels, iters, grad_min, huber, min_pixels,
    min_ratio: `ops.ego_motion`'s (None: the named defaults of odometry.py); the window must not exceed 2^20 pixels.  A frame
    hands out, in its single read-back (the doubles first in the record),
      FrameOdometry(disp, var, age,            KittiInferenceTemporal's
                    pose (4,4) float64,        the camera in the world of the sequence's first frame
                    motion (4,4) float64,      T_cur_from_prev in metres; the identity on a first frame or after a failure
                    count, residual, status)   of the estimate's last iteration; status 0 ok, 1 failed
    `pose=` may still be passed per frame (`infer(left, right, pose=T)`, or a third item in `stream`): the estimate does not run,
    the frame's disp, var and age are KittiInferenceTemporal's bit for bit for the same calls, `pose` is the given pose, `motion`
    the relative pose to the given pose before (the identity without one), status 0 and count 0; later estimated frames chain
    on from the given pose."""

    Frame = FrameOdometry

    def __init__(self, model, calib=None, *args, levels: int = None, iters: int = None, init: str = "last", grad_min: int = None,
                 huber: float = None, min_pixels: int = None, min_ratio: float = None, **kwargs):
        from . import odometry as OD
        super().__init__(model, calib, *args, **kwargs)
        name = type(self).__name__
        if init not in ("last", "identity"):
            raise ValueError(f"{name}: init is 'last' or 'identity', got {init!r}")
        pick = lambda v, default: default if v is None else v      # noqa: E731
        self.init = init
        self.ego_kw = dict(levels=pick(levels, OD.ODOMETRY_LEVELS), iters=pick(iters, OD.ODOMETRY_ITERS),
                           min_disp=self.reproject_kw["min_disp"], max_disp=self.reproject_kw["max_disp"],
                           min_ratio=pick(min_ratio, OD.ODOMETRY_MIN_RATIO), grad_min=pick(grad_min, OD.ODOMETRY_GRAD_MIN),
                           huber=pick(huber, OD.ODOMETRY_HUBER), min_pixels=pick(min_pixels, OD.ODOMETRY_MIN_PIXELS))
        levels = OD._levels(name, ValueError, 1 << OD.MAX_LEVELS, 1 << OD.MAX_LEVELS, self.ego_kw["levels"], None)
        res = OD.ego_scalars(name, ValueError, 1 << (levels - 1), 1 << (levels - 1), self.calib, **self.ego_kw)   # the ranges, up front
        self.ego_kw["levels"], self.ego_kw["iters"] = res[0], res[1]
        self._osets = {}             # (rows, cols) -> _Odometry
        self._okey = None            # (h, w, src_y0, rows, cols) of the frame before; None: no sequence runs
        self._given = None           # the pose given with the frame before (pose=), or None

    def reset(self):
        super().reset()
        self._okey = self._given = None

    def __call__(self, left_rgb, right_rgb, pose=None, as_uint16: bool = False):
        return super().__call__(left_rgb, right_rgb, pose, as_uint16)

    def _fields(self, rows, cols, as_uint16):
        from .odometry import FRAME_LEN
        return [("odo", torch.float64, (FRAME_LEN,))] + super()._fields(rows, cols, as_uint16)

    def _upload(self, s, left_rgb, right_rgb, copy, pose=None):
        """host, in input order: what this frame is -- a first frame, an estimated one, or one with a given pose"""
        from . import odometry as OD
        from .geometry import _pose44, relative_pose
        name = type(self).__name__
        if pose is not None:
            pose = _pose44(pose, name)
        hw = np.shape(left_rgb)[:2] if self.rectify is None else tuple(self.rectify.dst_hw)
        if len(hw) == 2:                                     # (anything else: the parent's refusal)
            _, _, rows, cols = self._place(*hw)
            if rows * cols > OD.MAX_PIXELS:
                raise ValueError(f"{name}: the window of {rows} x {cols} pixels exceeds the estimate's {OD.MAX_PIXELS}")
            OD._levels(name, ValueError, rows, cols, self.ego_kw["levels"], None)
        super()._upload(s, left_rgb, right_rgb, copy, pose)
        f = s.frame
        key = (f.h, f.w, f.src_y0, f.rows, f.cols)
        running = self._okey == key
        if pose is not None:
            motion = relative_pose(self._given, pose) if running and self._given is not None else np.eye(4)
            s.odo = ("given", np.concatenate([pose.reshape(-1), motion.reshape(-1), [0.0, 0.0, 0.0]]))
        else:
            s.odo = ("estimate" if running else "first", None)
        self._okey, self._given = key, pose

    def _oset(self, s):
        key = (s.frame.rows, s.frame.cols)
        if key not in self._osets:
            self._osets[key] = _Odometry(s.device, *key, self.ego_kw["levels"])
        return self._osets[key]

    def _window_calib(self, s):
        """the window's row 0 is image row src_y0: the principal point moves up by as much"""
        c, y0 = self.calib, s.frame.src_y0
        return c if y0 == 0 else type(c)(c.f, c.baseline, c.cx, c.cy - y0, c.doffs)

    def _net_pair(self, s, left, right, h, w):
        """current stream, in front of the network: the pyramid of this image, the estimate, then the parent's prediction"""
        from . import ops
        f, o = s.frame, self._oset(s)
        img = left[f.src_y0:f.src_y0 + f.rows, :f.cols]
        if not img.is_contiguous():                          # an image wider than the frame: the window's pixels, packed
            if o.window is None or o.window.shape != img.shape:
                o.window = torch.empty(img.shape, device=s.device, dtype=torch.uint8)
            o.window.copy_(img)
            img = o.window
        ops.grey_pyramid(img, self.ego_kw["levels"], out=o.grey[o.cur])
        if s.odo[0] == "estimate":
            ops.ego_motion(o.grey[1 - o.cur], o.grey[o.cur], o.dpyr, (f.rows, f.cols), self._window_calib(s),
                           init=o.rec if self.init == "last" and o.have_rec else None, out={"rec": o.rec, "g": o.g},
                           workspace=o.sums, **self.ego_kw)
            s.item = o.g[:12].view(3, 4)                     # the parent hands it to `ops.disp_reproject`, which reads it on the device
        return super()._net_pair(s, left, right, h, w)

    def _export(self, s, maps, out):
        """current stream, behind the fuse: the pyramid of the new state, the swap, the world pose into the record"""
        from . import ops
        super()._export(s, maps, out)
        o = self._oset(s)
        ops.disp_pyramid(self._set(s).state["disp"], self.ego_kw["levels"], self.ego_kw["min_disp"], out=o.dpyr)
        o.cur = 1 - o.cur
        if s.odo[0] == "given":
            # through the slot's pinned record (the host has taken the slot's previous frame out of it): no pageable copy
            s.pin["odo"].copy_(torch.from_numpy(s.odo[1]))
            out["odo"].copy_(s.pin["odo"], non_blocking=True)
            o.world.copy_(out["odo"][:12], non_blocking=True)
        else:
            ops.pose_chain(o.rec if s.odo[0] == "estimate" else None, o.world, out=out["odo"])
        o.have_rec = s.odo[0] == "estimate"

    def _result(self, s):
        s.done.synchronize()
        out = {name: v.numpy().copy() for name, v in s.pin.items()}
        odo = out["odo"]
        return FrameOdometry(out["disp"], out["var"], out["age"], odo[:16].reshape(4, 4), odo[16:32].reshape(4, 4), int(odo[32]),
                             float(odo[33]), int(odo[34]))


class KittiInferenceColor(_StageMixin, KittiInference):
    """`disp, rgb = KittiInferenceColor(model, cmap="kitti", max_disp=None, mask=None | "confidence" | "lr", ...)(left_rgb,
    right_rgb)`: KittiInference with device I/O (required: the picture is made where the disparity lies) followed by one
    launch of `ops.disp_colorize` on the same stream.  `disp` is float32 (h,w), bitwise
    KittiInference's; `rgb` is uint8 (h,w,3), the same window (`color_png` stores it as it is).
      cmap       "kitti": the KITTI devkit's disp_to_color; "gray"
      max_disp   None: the model's `maxdisp`; a number: t = min(d / max_disp, 1); "auto": every frame is ranged over its own
                 valid pixels by `ops.disp_range` on the device, and the launch reads the pair from device memory
      mask       None; "confidence": KittiInferenceWithConfidence's window mass (`radius`), pixels below `mask_min` are black;
                 "lr": the validity map of the left-right check (`tau`; two passes per frame), invalid pixels are black and the
                 disparity is the UNFILLED one
    Pixels whose disparity is not finite or not > 0 are black.  Both maps come back in one copy and one synchronisation per
    frame.  `median=3 | 5` and `speckle=(max_size, max_diff)` (keywords, off by default) run the
    post-filter of KittiInferenceFiltered first: `disp` is then the filtered disparity and a removed pixel is black."""

    device_io = True
    needs_device_io = "the map is coloured on the device, next to the disparity"
    has_uint16 = False

    def __init__(self, model, *args, cmap: str = "kitti", max_disp=None, mask=None, mask_min: float = 0.5, radius: int = 1,
                 tau: float = 1.0, speckle=None, median: int = 0, **kwargs):
        super().__init__(model, *args, **kwargs)
        self._take_post(median, speckle)
        if cmap not in ("kitti", "gray"):
            raise ValueError(f"cmap is 'kitti' or 'gray', got {cmap!r}")
        self._take_mask(mask, mask_min, radius, tau)
        max_disp = self._max_disp_or_model(max_disp)
        if max_disp != "auto":
            max_disp = float(max_disp)
            if not 0.0 < max_disp < float("inf"):
                raise ValueError(f"max_disp is 'auto' or a positive, finite number, got {max_disp}")
        self.cmap, self.max_disp = cmap, max_disp

    def _fields(self, rows, cols, as_uint16):
        """the float32 disparity, its uint8 RGB picture behind it at byte 4 rows cols: one copy brings both"""
        return [("disp", torch.float32, (rows, cols)), ("rgb", torch.uint8, (rows, cols, 3))]

    def _export(self, s, maps, out):
        from . import ops
        # with the filters the disparity handed out is the filtered one (a removed pixel is +0.0: black).  With mask_min <= 0 the
        # mask switches nothing off, so the filter's validity (0 / 1) must not enter it either
        pred, mask, (y0, rows, cols) = self._stage_maps(s, maps, out, self.mask_min > 0.0)
        scale = {"max_disp": self.max_disp}
        if self.max_disp == "auto":
            scale = {"range": ops.disp_range(pred, (y0, rows, cols), mask, self.mask_min)}
        ops.disp_colorize(pred, y0, rows, cols, cmap=self.cmap, mask=mask, mask_min=self.mask_min, out=out["rgb"], **scale)


def color_png(path: str, rgb: np.ndarray) -> None:
    """8-bit RGB PNG of a colour image as KittiInferenceColor / `ops.disp_colorize` / `ops.disp_error_image(u8=True)` hand
    it out: uint8 (h,w,3)."""
    from PIL import Image
    rgb = np.asarray(rgb)
    if rgb.dtype != np.uint8 or rgb.ndim != 3 or rgb.shape[2] != 3:
        raise ValueError(f"color_png takes a uint8 (h,w,3) image, got {rgb.dtype} {rgb.shape}")
    Image.fromarray(np.ascontiguousarray(rgb), "RGB").save(path, format="PNG")


def confidence_png(path: str, conf: np.ndarray) -> None:
    """16-bit PNG of a confidence map: uint16(conf * 65535) for float input (as `as_uint16=True` gives it), 65535 = certain."""
    from PIL import Image
    conf = np.asarray(conf)
    if conf.dtype != np.uint16:
        conf = (conf.astype(np.float32) * np.float32(KittiInference.CONF_U16_SCALE)).astype("uint16")
    Image.fromarray(conf).save(path, format="PNG")
