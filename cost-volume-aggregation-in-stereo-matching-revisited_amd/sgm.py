"""Semi-global matching on a census cost -- a disparity source that needs no weights -- on the host, numpy only: the restatement
of include/dca_hip.h (dca_sgm_census, dca_sgm_disparity) that the kernels of csrc/sgm.hip equal bit for bit
(tests/test_gpu_sgm.py), vectorised over bins and scanlines, and the documented CPU path for a user without a ROCm device; below
it the operators themselves, `sgm_census`, `sgm_disparity` and `sgm_workspace` (`ops.sgm_*`), which take device tensors and
have no CPU fallback.  DESIGN.md section 6r.

One rectified pair of uint8 images, (H,W) grey or (H,W,3) / (H,W,4) interleaved.  Everything is integer arithmetic: the census
(9 x 7, 62 bits), the Hamming cost, the path recursion with the penalties P1 <= P2, the sum S over 4 or 8 paths (it fits uint16
without saturation), the winner with its uniqueness test and the sub-pixel step in sixteenths of a pixel; the one float32
operation is the exact division float(q) / 16."""
from __future__ import annotations

import numpy as np
import torch

from ._call import _C, _L, _chk, _ptr, _stream
from .frame_ops import _out, _out_dict, _req_dev, _req_u8_pair

MIN_DIM = 7                                    # DCA_SGM_MIN_DIM: the census window fits once
MAX_DIM = 8192                                 # DCA_SGM_MAX_DIM
MIN_DISP = 8                                   # DCA_SGM_MIN_DISP: the least max_disp
MAX_DISP = 256                                 # DCA_SGM_MAX_DISP: the largest
MAX_P = 4095                                   # DCA_SGM_MAX_P: 8 (62 + 4095) < 2^16
CENSUS_BITS = 62                               # DCA_SGM_CENSUS_BITS
COST_OUT = 62                                  # DCA_SGM_COST_OUT: the cost of a bin whose right pixel lies outside the image
MAX_VOLUME = 1 << 30                           # H W D stays below
SGM_OUTPUTS = ("disp", "valid", "cost", "disp_right", "disp_right_mirrored")
SGM_DEFAULT_OUTPUTS = SGM_OUTPUTS[:3]
PATHS = ((0, 1), (0, -1), (1, 0), (-1, 0), (1, 1), (1, -1), (-1, 1), (-1, -1))      # predecessor offsets (dy, dx); the first four: paths=4

# defaults
SGM_PATHS = 8
SGM_P1 = 10
SGM_P2 = 120
SGM_UNIQUENESS = 15
SGM_MIN_DISP = 1

_NONE = 1 << 20                                # a bin that is not there: above every S
_POP8 = np.array([bin(i).count("1") for i in range(256)], np.uint8)


def sgm_scalars(name, err, H, W, max_disp, paths=SGM_PATHS, P1=SGM_P1, P2=SGM_P2, uniqueness=SGM_UNIQUENESS, min_disp=SGM_MIN_DISP):
    """the scalars of `sgm_disparity` within the ranges of include/dca_hip.h -> (D, paths, P1, P2, uniqueness, min_disp) as
    ints; `err`: the exception a refusal raises"""
    vals = (max_disp, paths, P1, P2, uniqueness, min_disp)
    try:
        whole = all(not isinstance(v, bool) and int(v) == v for v in vals)
    except (TypeError, ValueError):
        whole = False
    if not whole:
        raise err(f"{name}: max_disp, paths, P1, P2, uniqueness and min_disp are whole numbers, got {vals!r}")
    D, paths, P1, P2, u, min_disp = (int(v) for v in vals)
    if not (MIN_DIM <= H <= MAX_DIM and MIN_DIM <= W <= MAX_DIM):
        raise err(f"{name}: {MIN_DIM} <= H, W <= {MAX_DIM}, got {H} x {W}")
    if not MIN_DISP <= D <= MAX_DISP:
        raise err(f"{name}: max_disp is an integer in [{MIN_DISP}, {MAX_DISP}], got {max_disp}")
    if H * W * D >= MAX_VOLUME:
        raise err(f"{name}: H * W * max_disp stays below 2^30, got {H} x {W} x {D}")
    if paths not in (4, 8):
        raise err(f"{name}: paths is 4 or 8, got {paths}")
    if not 1 <= P1 <= P2 <= MAX_P:
        raise err(f"{name}: 1 <= P1 <= P2 <= {MAX_P}, got P1 {P1} and P2 {P2}")
    if not 0 <= u <= 99:
        raise err(f"{name}: uniqueness is an integer in [0, 99], got {uniqueness}")
    if not 0 <= min_disp <= D - 1:
        raise err(f"{name}: min_disp is an integer in [0, max_disp - 1], got {min_disp}")
    return D, paths, P1, P2, u, min_disp


def _output_names(name, err, outputs):
    names = SGM_DEFAULT_OUTPUTS if outputs is None else tuple(outputs)
    if not names or any(k not in SGM_OUTPUTS for k in names):
        raise err(f"{name}: outputs are chosen from {SGM_OUTPUTS}, got {names}")
    return names


def grey_host(img):
    """a uint8 image (H,W) or (H,W,3) / (H,W,4) -> its grey values (H,W) int64: g = (77 R + 150 G + 29 B + 128) >> 8; a grey
    image as it is, a fourth channel ignored"""
    a = np.asarray(img)
    if a.dtype != np.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] not in (3, 4)) or a.size == 0:
        raise ValueError(f"census_host: expected a uint8 (H,W), (H,W,3) or (H,W,4) image, got {a.dtype} {a.shape}")
    if a.ndim == 2:
        return a.astype(np.int64)
    r, g, b = (a[..., k].astype(np.int64) for k in range(3))
    return (77 * r + 150 * g + 29 * b + 128) >> 8


def census_host(img):
    """the census of one image -> (H,W) uint64: 62 bits, the neighbours of the 9 x 7 window row-major with the centre skipped,
    the first at bit 61; a bit is 1 iff the neighbour lies inside the image and is darker than the centre"""
    g = grey_host(img)
    H, W = g.shape
    pad = np.full((H + 6, W + 8), 255, np.int64)             # outside: darker than no centre
    pad[3:3 + H, 4:4 + W] = g
    bits = np.zeros((H, W), np.uint64)
    for dy in range(7):
        for dx in range(9):
            if (dy, dx) != (3, 4):
                bits = (bits << np.uint64(1)) | (pad[dy:dy + H, dx:dx + W] < g).astype(np.uint64)
    return bits


def popcount64(a):
    """the number of set bits of every uint64 of `a` -> int64"""
    a = np.ascontiguousarray(a, np.uint64)
    return _POP8[a.view(np.uint8).reshape(a.shape + (8,))].sum(axis=-1, dtype=np.int64)


def cost_volume_host(cL, cR, D):
    """C (H,W,D) int64: popcount(cL(y,x) ^ cR(y,x-d)) for x - d >= 0, COST_OUT otherwise"""
    H, W = cL.shape
    C = np.full((H, W, D), COST_OUT, np.int64)
    for d in range(min(D, W)):
        C[:, d:, d] = popcount64(cL[:, d:] ^ cR[:, :W - d])
    return C


def _step(c, prev, P1, P2):
    """one step of the recursion on n scanlines at once: c, prev (n,D) -> L (n,D)"""
    m = prev.min(axis=1, keepdims=True)
    best = np.minimum(prev, m + P2)
    best[:, 1:] = np.minimum(best[:, 1:], prev[:, :-1] + P1)
    best[:, :-1] = np.minimum(best[:, :-1], prev[:, 1:] + P1)
    return c + best - m


def path_host(C, r, P1, P2):
    """L_r (H,W,D) int64 of the predecessor offset r = (dy, dx): L_r(p) = C(p) where p - r lies outside the image"""
    dy, dx = r
    H, W, _ = C.shape
    L = np.empty_like(C)
    if dy == 0:
        xs = range(W) if dx > 0 else range(W - 1, -1, -1)
        for i, x in enumerate(xs):
            L[:, x] = C[:, x] if i == 0 else _step(C[:, x], L[:, x - dx], P1, P2)
        return L
    ys = range(H) if dy > 0 else range(H - 1, -1, -1)
    for i, y in enumerate(ys):
        L[y] = C[y]
        if i == 0:
            continue
        prev = L[y - dy]
        if dx == 0:
            L[y] = _step(C[y], prev, P1, P2)
        elif dx > 0:                                         # the predecessor of column x is column x - 1: none for x = 0
            L[y, 1:] = _step(C[y, 1:], prev[:-1], P1, P2)
        else:
            L[y, :-1] = _step(C[y, :-1], prev[1:], P1, P2)
    return L


def aggregate_host(C, paths, P1, P2):
    """S (H,W,D) int64: the sum of L_r over the first `paths` offsets of PATHS"""
    S = np.zeros_like(C)
    for r in PATHS[:paths]:
        S += path_host(C, r, P1, P2)
    return S


def _winner(V, nk):
    """V (H,W,D) int64 with _NONE in the bins that are not present, nk (H,W) or a scalar: the number present -> (d*, s, q):
    the lowest argmin, its value, 16 d* + the sub-pixel step"""
    D = V.shape[-1]
    ds = np.argmin(V, axis=-1)                               # the first minimum
    take = lambda k: np.take_along_axis(V, np.clip(k, 0, D - 1)[..., None], axis=-1)[..., 0]
    s, sm, sp = take(ds), take(ds - 1), take(ds + 1)
    den = sm + sp - 2 * s
    ok = (ds > 0) & (ds < nk - 1) & (den > 0)
    off = np.where(ok, (16 * (sm - sp) + 17 * den) // np.maximum(2 * den, 1) - 8, 0)
    return ds, s, 16 * ds + off


def _sixteenths(q):
    return q.astype(np.float32) / np.float32(16.0)


def sgm_host(left, right, max_disp, paths=SGM_PATHS, P1=SGM_P1, P2=SGM_P2, uniqueness=SGM_UNIQUENESS, min_disp=SGM_MIN_DISP,
             outputs=None):
    """Semi-global matching of one rectified uint8 pair (definitions: include/dca_hip.h, dca_sgm_disparity).  Returns a dict with
    the keys of `outputs` (default the first three of SGM_OUTPUTS), each (H,W):
      disp                 float32  q / 16 where valid, +0.0 elsewhere
      valid                float32  1.0 / 0.0: the uniqueness test passes and d* >= min_disp
      cost                 int32    S(p, d*), for every pixel
      disp_right           float32  the right view's disparity from the same S, in the right image's coordinates; every pixel
      disp_right_mirrored  float32  the same with column i at index W-1-i (the second argument of `ops.lr_consistency`)"""
    name = "sgm_host"
    names = _output_names(name, ValueError, outputs)
    L, R = np.asarray(left), np.asarray(right)
    if L.shape != R.shape:
        raise ValueError(f"{name}: expected two uint8 images of one shape, got {L.shape} and {R.shape}")
    try:
        cL, cR = census_host(L), census_host(R)
    except ValueError as e:
        raise ValueError(str(e).replace("census_host", name)) from None
    H, W = cL.shape
    D, paths, P1, P2, u, min_disp = sgm_scalars(name, ValueError, H, W, max_disp, paths, P1, P2, uniqueness, min_disp)
    S = aggregate_host(cost_volume_host(cL, cR, D), paths, P1, P2)
    assert S.max() < 1 << 16
    res = {}
    if set(names) & {"disp", "valid", "cost"}:
        ds, s, q = _winner(S, D)
        k = np.arange(D)
        other = np.where(np.abs(k - ds[..., None]) > 1, S, _NONE).min(axis=-1)
        ok = (other * (100 - u) >= 100 * s) & (ds >= min_disp)
        res["disp"] = np.where(ok, _sixteenths(q), np.float32(0))
        res["valid"] = ok.astype(np.float32)
        res["cost"] = s.astype(np.int32)
    if set(names) & {"disp_right", "disp_right_mirrored"}:
        SR = np.full_like(S, _NONE)
        for k in range(min(D, W)):
            SR[:, :W - k, k] = S[:, k:, k]
        _, _, q = _winner(SR, np.minimum(D, W - np.arange(W))[None, :])
        res["disp_right"] = _sixteenths(q)
        res["disp_right_mirrored"] = np.ascontiguousarray(res["disp_right"][:, ::-1])
    return {k: res[k] for k in SGM_OUTPUTS if k in names}


# ------------------------------------------------------------------------------------------------
# The operators on the device (csrc/sgm.hip), by the conventions of frame_ops.py: arguments are validated once, here; a refusal
# names the operator; a tensor that is not on a ROCm device is an error; no launch synchronises; with `out` and `workspace`
# passed in nothing is allocated either (hipGraph capture).  ops.py re-exports them.
# ------------------------------------------------------------------------------------------------
_SGM_KINDS = {"disp": torch.float32, "valid": torch.float32, "cost": torch.int32, "disp_right": torch.float32,
              "disp_right_mirrored": torch.float32}
assert (MIN_DIM, MAX_DIM, MIN_DISP, MAX_DISP, MAX_P, CENSUS_BITS, COST_OUT) == tuple(
    _C[k] for k in ("DCA_SGM_MIN_DIM", "DCA_SGM_MAX_DIM", "DCA_SGM_MIN_DISP", "DCA_SGM_MAX_DISP", "DCA_SGM_MAX_P",
                    "DCA_SGM_CENSUS_BITS", "DCA_SGM_COST_OUT")), "sgm.py restates other constants than include/dca_hip.h defines"


def _sgm_pair(name, left, right):
    """two uint8 images of one shape on one ROCm device, (H,W) or (H,W,3) / (H,W,4) -> (H, W, C), C = 1 for grey"""
    if isinstance(left, torch.Tensor) and left.dim() == 2:
        _req_dev(left, name, "the left image", torch.uint8)
        _req_dev(right, name, "the right image", torch.uint8, like=left)
        if left.shape != right.shape or left.numel() == 0:
            raise RuntimeError(f"{name}: expected two uint8 images of one shape, got {tuple(left.shape)} and {tuple(right.shape)}")
        return int(left.shape[0]), int(left.shape[1]), 1
    shape = _req_u8_pair(left, right, name)
    _req_dev(right, name, "the right image", torch.uint8, like=left)
    return shape


def sgm_workspace_bytes(H, W, max_disp):
    """the bytes `sgm_disparity` needs between its launches: the census of both images (2,H,W) uint64 and S (H,W,D) uint16"""
    return 16 * int(H) * int(W) + 2 * int(H) * int(W) * int(max_disp)


def sgm_workspace(H, W, max_disp, device):
    """the uint8 workspace of `sgm_disparity(..., workspace=)` for H x W images and `max_disp` bins.  A call writes every byte
    before it reads it; nothing has to be cleared."""
    sgm_scalars("sgm_workspace", RuntimeError, int(H), int(W), max_disp)
    return torch.empty((sgm_workspace_bytes(H, W, max_disp),), device=device, dtype=torch.uint8)


def sgm_census(left_u8, right_u8, out=None):
    """The census of a rectified uint8 pair, (H,W) grey or (H,W,3) / (H,W,4), ONE launch -> (2,H,W) int64 on the device, the
    left image first; the 62 bits of include/dca_hip.h (dca_sgm_census) are the low bits of every word.  out: the buffer to
    write into."""
    name = "sgm_census"
    H, W, C = _sgm_pair(name, left_u8, right_u8)
    sgm_scalars(name, RuntimeError, H, W, MIN_DISP)
    out = _out(name, "out", out, torch.int64, (2, H, W), left_u8)
    with torch.cuda.device_of(left_u8):
        _chk(_L().dca_sgm_census(_ptr(left_u8), _ptr(right_u8), _ptr(out), H, W, C, _stream()), "dca_sgm_census")
    return out


def sgm_disparity(left_u8, right_u8, max_disp, paths=SGM_PATHS, P1=SGM_P1, P2=SGM_P2, uniqueness=SGM_UNIQUENESS,
                  min_disp=SGM_MIN_DISP, outputs=None, out=None, workspace=None):
    """Semi-global matching of a rectified uint8 pair on the device, (H,W) grey or (H,W,3) / (H,W,4) as `ops.rectify_pair` and
    `ops.area_downscale_pair` give them (definitions: include/dca_hip.h, dca_sgm_disparity): the 9 x 7 census of both images, the
    Hamming cost over `max_disp` bins (8 .. 256, any integer), `paths` = 4 or 8 paths with the penalties 1 <= P1 <= P2 <= 4095,
    the winner with the uniqueness margin `uniqueness` (per cent, 0 .. 99; 0: off) and a sub-pixel step in sixteenths; a winner
    below `min_disp` is no measurement.  Returns a dict of (H,W) device tensors, those named in `outputs` (default the first
    three of SGM_OUTPUTS; the others are neither computed nor written):
      disp                 float32  the left disparity in pixels, +0.0 where invalid (`ops.hints_to_quarter`'s "nothing measured")
      valid                float32  1.0 / 0.0
      cost                 int32    the winner's aggregated cost, for every pixel
      disp_right           float32  the right view's disparity, read from the same aggregation, in its own coordinates
      disp_right_mirrored  float32  the same, column i at index W-1-i: the second argument of `ops.lr_consistency`
    out: a dict of buffers for some or all of them; workspace: `sgm_workspace(H, W, max_disp, device)`.  One launch for the census,
    one per path, one per view; no host wait; with `out` and `workspace` nothing is allocated.  Bitwise reproducible: integers,
    and no atomic."""
    name = "sgm_disparity"
    names = _output_names(name, RuntimeError, outputs)
    scalars = None
    if isinstance(left_u8, torch.Tensor) and left_u8.dim() in (2, 3):      # the scalars first: refused on any device
        scalars = sgm_scalars(name, RuntimeError, int(left_u8.shape[0]), int(left_u8.shape[1]), max_disp, paths, P1, P2,
                              uniqueness, min_disp)
    H, W, C = _sgm_pair(name, left_u8, right_u8)             # (refuses whatever the branch above did not see)
    D, paths, P1, P2, u, min_disp = scalars
    res = _out_dict(name, _SGM_KINDS, (), names, out, lambda k: (H, W), left_u8)
    need = sgm_workspace_bytes(H, W, D)
    if workspace is None:
        workspace = torch.empty((need,), device=left_u8.device, dtype=torch.uint8)
    _req_dev(workspace, name, "workspace", torch.uint8, like=left_u8)
    if workspace.numel() < need or workspace.data_ptr() % 8:
        raise RuntimeError(f"{name}: workspace must hold at least {need} bytes at a multiple of 8 (`sgm_workspace`), got "
                           f"{workspace.numel()}")
    with torch.cuda.device_of(left_u8):
        _chk(_L().dca_sgm_disparity(_ptr(left_u8), _ptr(right_u8), _ptr(workspace), *(_ptr(res.get(k)) for k in SGM_OUTPUTS),
                                    H, W, C, D, paths, P1, P2, u, min_disp, _stream()), "dca_sgm_disparity")
    return res
