"""Autograd operators of the DCANet hot path, each a thin host wrapper over the C ABI of
libdca_hip.so (include/dca_hip.h).  PyTorch is used for device memory, streams and autograd graph
bookkeeping only; every arithmetic step on the path runs in a hand-written HIP kernel.

There is no CPU / eager fallback: tensors must be fp32 on a ROCm device and the library must load.
"""
from __future__ import annotations

import ctypes
import math
import os
import threading
from typing import Optional

import torch

from . import _lib
from . import geometry as _geometry

_C = _lib.CONSTANTS       # the integer #define DCA_* of include/dca_hip.h
_vp = ctypes.c_void_p


def _L():
    return _lib.load()


def _ptr(t: Optional[torch.Tensor]):
    return _vp(t.data_ptr()) if t is not None else None


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_raw_device = getattr(torch._C, "_cuda_getDevice", None)


def _stream():
    """torch's CURRENT stream on the current device as a hipStream_t (every launch goes there).  The raw C accessors
    cost ~0.3 us against ~9 us for torch.cuda.current_stream() -- there are ~1000 launches per training step."""
    if _raw_stream is not None and _raw_device is not None:
        return _vp(_raw_stream(_raw_device()))
    return _vp(torch.cuda.current_stream().cuda_stream)


def _chk(rc: int, name: str):
    if rc != 0:
        raise RuntimeError(f"{name} failed with hipError_t {rc}")


def _req(t: torch.Tensor, name: str, packed_ok: bool = False) -> torch.Tensor:
    if getattr(t, "_dca_px2", None) is not None and not packed_ok:
        raise RuntimeError(f"{name}: got a tensor in the packed px2 operand format (only the f16x2 3x3x3 stride-1 convolution "
                           "reads it; ask the producer for an fp32 result)")
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(
            f"{name}: the DCANet hot path runs only as HIP kernels on a ROCm device (got "
            f"{'a ' + str(t.device) + ' tensor' if isinstance(t, torch.Tensor) else type(t)}); there is no CPU fallback")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name}: expected float32, got {t.dtype}")
    t = t.contiguous()
    if t.data_ptr() % 16:
        t = t.clone(memory_format=torch.contiguous_format)
    return t


def _opt(t, name):
    return None if t is None else _req(t, name)


# ------------------------------------------------------------------------------------------------
# cost volumes
# ------------------------------------------------------------------------------------------------
class _GwcVolume(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ref, tgt, maxdisp, num_groups):
        ref, tgt = _req(ref, "build_gwc_volume"), _req(tgt, "build_gwc_volume")
        B, C, H, W = ref.shape
        vol = torch.empty((B, num_groups, maxdisp, H, W), device=ref.device, dtype=torch.float32)
        with torch.cuda.device_of(ref):
            _chk(_L().dca_gwc_volume_fwd(_ptr(ref), _ptr(tgt), _ptr(vol), B, C, H, W, maxdisp, num_groups, _stream()),
                 "dca_gwc_volume_fwd")
        ctx.save_for_backward(ref, tgt)
        ctx.meta = (maxdisp, num_groups)
        return vol

    @staticmethod
    def backward(ctx, gvol):
        ref, tgt = ctx.saved_tensors
        maxdisp, G = ctx.meta
        gvol = _req(gvol, "build_gwc_volume.backward")
        B, C, H, W = ref.shape
        gref, gtgt = torch.empty_like(ref), torch.empty_like(tgt)
        with torch.cuda.device_of(ref):
            _chk(_L().dca_gwc_volume_bwd(_ptr(gvol), _ptr(ref), _ptr(tgt), _ptr(gref), _ptr(gtgt), B, C, H, W,
                                         maxdisp, G, _stream()), "dca_gwc_volume_bwd")
        return gref, gtgt, None, None


class _ConcatVolume(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ref, tgt, maxdisp):
        ref, tgt = _req(ref, "build_concat_volume"), _req(tgt, "build_concat_volume")
        B, C, H, W = ref.shape
        vol = torch.empty((B, 2 * C, maxdisp, H, W), device=ref.device, dtype=torch.float32)
        with torch.cuda.device_of(ref):
            _chk(_L().dca_concat_volume_fwd(_ptr(ref), _ptr(tgt), _ptr(vol), B, C, H, W, maxdisp, _stream()),
                 "dca_concat_volume_fwd")
        ctx.meta = (B, C, H, W, maxdisp)
        return vol

    @staticmethod
    def backward(ctx, gvol):
        B, C, H, W, maxdisp = ctx.meta
        gvol = _req(gvol, "build_concat_volume.backward")
        gref = torch.empty((B, C, H, W), device=gvol.device, dtype=torch.float32)
        gtgt = torch.empty_like(gref)
        with torch.cuda.device_of(gvol):
            _chk(_L().dca_concat_volume_bwd(_ptr(gvol), _ptr(gref), _ptr(gtgt), B, C, H, W, maxdisp, _stream()),
                 "dca_concat_volume_bwd")
        return gref, gtgt, None


def gwc_volume(ref, tgt, maxdisp, num_groups):
    return _GwcVolume.apply(ref, tgt, int(maxdisp), int(num_groups))


class _CostVolume(torch.autograd.Function):
    """Fused builder (csrc/volume_fused.hip): gwc volume from 1-3 channel segments per side + optional concat volume,
    one output tensor, fp32 or the reduced-precision storage type."""

    @staticmethod
    def forward(ctx, maxdisp, num_groups, out_dtype, nseg, has_concat, *tensors):
        refs = [_req(t, "cost_volume.ref") for t in tensors[:nseg]]
        tgts = [_req(t, "cost_volume.tgt") for t in tensors[nseg:2 * nseg]]
        cref = _req(tensors[2 * nseg], "cost_volume.cref") if has_concat else None
        ctgt = _req(tensors[2 * nseg + 1], "cost_volume.ctgt") if has_concat else None
        B, _, H, W = refs[0].shape
        segC = [t.shape[1] for t in refs]
        Cc = cref.shape[1] if has_concat else 0
        for r_, t_ in zip(refs, tgts):
            assert r_.shape == t_.shape and r_.shape[0] == B and tuple(r_.shape[2:]) == (H, W)
        vol = torch.empty((B, num_groups + 2 * Cc, maxdisp, H, W), device=refs[0].device, dtype=out_dtype)
        rp = (ctypes.c_void_p * nseg)(*[t.data_ptr() for t in refs])
        tp = (ctypes.c_void_p * nseg)(*[t.data_ptr() for t in tgts])
        sc = (ctypes.c_int * nseg)(*segC)
        code = 0 if out_dtype == torch.float32 else LP_DTYPES[out_dtype]
        # fp32 volume without concat part: the builder emits the per-channel maxima the first f16x2 convolution scales by
        vmax = _cslots(num_groups, vol.device) if (CONV_X2 and AMAX_EMIT and code == 0 and Cc == 0 and B * H <= CSLOTS) else None
        with torch.cuda.device_of(vol):
            _chk(_L().dca_cost_volume_fwd(rp, tp, sc, nseg, _ptr(cref), _ptr(ctgt), Cc, _ptr(vol), B, H, W, maxdisp,
                                          num_groups, code, _ptr(vmax), _stream()), "dca_cost_volume_fwd")
        ctx.save_for_backward(*refs, *tgts)
        ctx.meta = (maxdisp, num_groups, nseg, segC, Cc, (B, H, W))
        return _tag_cmax(vol, vmax, B * H)   # no read pass in front of dres0's first convolution

    @staticmethod
    def backward(ctx, gvol):
        maxdisp, G, nseg, segC, Cc, (B, H, W) = ctx.meta
        refs, tgts = ctx.saved_tensors[:nseg], ctx.saved_tensors[nseg:]
        gvol = _req(gvol, "cost_volume.backward")
        ref = refs[0] if nseg == 1 else torch.cat(refs, 1)
        tgt = tgts[0] if nseg == 1 else torch.cat(tgts, 1)
        gg = gvol if Cc == 0 else gvol[:, :G].contiguous()
        gref, gtgt = torch.empty_like(ref), torch.empty_like(tgt)
        lib = _L()
        with torch.cuda.device_of(gvol):
            _chk(lib.dca_gwc_volume_bwd(_ptr(gg), _ptr(ref), _ptr(tgt), _ptr(gref), _ptr(gtgt), B, ref.shape[1], H, W,
                                        maxdisp, G, _stream()), "dca_gwc_volume_bwd")
            grads = list(gref.split(segC, 1)) + list(gtgt.split(segC, 1))
            if Cc:
                gc = gvol[:, G:].contiguous()
                gcr = torch.empty((B, Cc, H, W), device=gvol.device, dtype=torch.float32)
                gct = torch.empty_like(gcr)
                _chk(lib.dca_concat_volume_bwd(_ptr(gc), _ptr(gcr), _ptr(gct), B, Cc, H, W, maxdisp, _stream()),
                     "dca_concat_volume_bwd")
                grads += [gcr, gct]
        return (None, None, None, None, None) + tuple(grads)


def cost_volume(ref, tgt, maxdisp, num_groups, cref=None, ctgt=None, out_dtype=torch.float32):
    """build_gwc_volume(ref, tgt) [cat build_concat_volume(cref, ctgt)] as ONE (B, G + 2*Cc, D, H, W) tensor.  `ref` /
    `tgt` may be tuples of channel segments (the extractor's l2 / l3 / l4 maps) that are read in place.  Falls back to
    the separate builders + torch.cat when W % 4 != 0, and for the fp32 volume also when D % 4 != 0 (the fused kernel takes
    any D; the fp32 routing is left as it was).  The reduced-precision volume has the fused builder only: any D, W % 4 == 0."""
    refs = tuple(ref) if isinstance(ref, (tuple, list)) else (ref,)
    tgts = tuple(tgt) if isinstance(tgt, (tuple, list)) else (tgt,)
    W = refs[0].shape[-1]
    C = sum(t.shape[1] for t in refs)
    cpg = C // num_groups if num_groups else 0
    ok = (W % 4 == 0 and (maxdisp % 4 == 0 or out_dtype != torch.float32) and len(refs) <= 3 and cpg in (1, 2, 4, 8, 16)
          and C % num_groups == 0 and all(t.shape[1] % cpg == 0 for t in refs))
    if not ok:
        if out_dtype != torch.float32:
            raise RuntimeError("cost_volume: the reduced-precision volume needs W % 4 == 0")
        r1 = refs[0] if len(refs) == 1 else torch.cat(refs, 1)
        t1 = tgts[0] if len(tgts) == 1 else torch.cat(tgts, 1)
        vol = gwc_volume(r1, t1, maxdisp, num_groups)
        return vol if cref is None else torch.cat((vol, concat_volume(cref, ctgt, maxdisp)), 1)
    extra = () if cref is None else (cref, ctgt)
    return _CostVolume.apply(int(maxdisp), int(num_groups), out_dtype, len(refs), cref is not None, *refs, *tgts, *extra)


def concat_volume(ref, tgt, maxdisp):
    return _ConcatVolume.apply(ref, tgt, int(maxdisp))


# ------------------------------------------------------------------------------------------------
# softmax(dim=1) / soft-argmin / disparity regression on (B, K, *spatial)
# ------------------------------------------------------------------------------------------------
class _SoftArgmin(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mode):
        x = _req(x, "softargmin")
        B, K = x.shape[0], x.shape[1]
        HW = x[0, 0].numel()
        out = torch.empty_like(x) if mode == 0 else torch.empty((B, 1) + tuple(x.shape[2:]), device=x.device,
                                                                dtype=torch.float32)
        with torch.cuda.device_of(x):
            _chk(_L().dca_softargmin_fwd(_ptr(x), _ptr(out), B, K, HW, mode, _stream()), "dca_softargmin_fwd")
        ctx.mode = mode
        ctx.save_for_backward(out if mode == 0 else x)
        return out

    @staticmethod
    def backward(ctx, g):
        (aux,) = ctx.saved_tensors
        g = _req(g, "softargmin.backward")
        B, K = aux.shape[0], aux.shape[1]
        HW = aux[0, 0].numel()
        gx = torch.empty_like(aux)
        with torch.cuda.device_of(aux):
            _chk(_L().dca_softargmin_bwd(_ptr(aux), _ptr(g), _ptr(gx), B, K, HW, ctx.mode, _stream()),
                 "dca_softargmin_bwd")
        return gx, None


def softmax_dim1(x):
    return _SoftArgmin.apply(x, 0)


def softargmin(x):
    """disparity_regression(softmax(x, 1), K) fused: (B,K,...) logits -> (B,1,...)."""
    return _SoftArgmin.apply(x, 1)


def regression(x):
    """disparity_regression(x, K) for an arbitrary x: sum_k k*x[:,k], keepdim."""
    return _SoftArgmin.apply(x, 2)


# planes of `softargmin_stats` (include/dca_hip.h)
CONF_DISP, CONF_DUNI, CONF_MASS, CONF_ENT, CONF_STD, CONF_PLANES = (
    _C[f"DCA_CONF_{n}"] for n in ("DISP", "DUNI", "MASS", "ENT", "STD", "PLANES"))


def _req_no_grad(name, *tensors):
    if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in tensors):
        raise RuntimeError(f"{name} is inference only (no backward): call it under torch.no_grad() or detach its inputs")


def softargmin_stats(logits, radius=1):
    """(B,K,*spatial) logits -> (B,5,*spatial): per pixel the soft-argmin (plane CONF_DISP, bitwise `softargmin`), the
    soft-argmin (CONF_DUNI) and the probability mass (CONF_MASS) of the window |k - argmax| <= radius, the entropy
    normalised by log K (CONF_ENT) and the standard deviation (CONF_STD) of the soft-max distribution over dim 1
    (definitions: include/dca_hip.h).  radius >= K means the whole range.  Inference only."""
    _req_no_grad("softargmin_stats", logits)
    x = _req(logits, "softargmin_stats")
    radius = int(radius)
    if x.dim() < 3 or x.numel() == 0 or radius < 0:
        raise RuntimeError(f"softargmin_stats: expected non-empty (B,K,*spatial) logits and radius >= 0, got "
                           f"{tuple(x.shape)} and radius {radius}")
    B, K = x.shape[0], x.shape[1]
    HW = x[0, 0].numel()
    out = torch.empty((B, CONF_PLANES) + tuple(x.shape[2:]), device=x.device, dtype=torch.float32)
    with torch.cuda.device_of(x):
        _chk(_L().dca_softargmin_stats(_ptr(x), _ptr(out), B, K, HW, min(radius, K), _stream()), "dca_softargmin_stats")
    return out


class _UpSoftArgmin(torch.autograd.Function):
    """trilinear x s up-sampling + softmax(dim 1) + disparity regression, fused (gwcnet_dca_g.py:261-264)."""

    @staticmethod
    def forward(ctx, logits, scale):
        logits = _req(logits, "up_softargmin")
        B, n, hc, wc = logits.shape
        disp = torch.empty((B, 1, scale * hc, scale * wc), device=logits.device, dtype=torch.float32)
        with torch.cuda.device_of(logits):
            _chk(_L().dca_up_softargmin_fwd(_ptr(logits), _ptr(disp), B, n, hc, wc, scale, _stream()),
                 "dca_up_softargmin_fwd")
        ctx.save_for_backward(logits)
        ctx.scale = scale
        return disp

    @staticmethod
    def backward(ctx, g):
        (logits,) = ctx.saved_tensors
        g = _req(g, "up_softargmin.backward")
        B, n, hc, wc = logits.shape
        s = ctx.scale
        g1 = torch.empty((B, n, s * hc, s * wc), device=logits.device, dtype=torch.float32)
        gl = torch.empty_like(logits)
        with torch.cuda.device_of(logits):
            _chk(_L().dca_up_softargmin_bwd(_ptr(logits), _ptr(g), _ptr(g1), _ptr(gl), B, n, hc, wc, s, _stream()),
                 "dca_up_softargmin_bwd")
        return gl, None


def up_softargmin(logits, scale):
    """(B,n,hc,wc) logits -> (B,1,s*hc,s*wc) expected disparity over s*n bins; falls back to the unfused kernels
    for n > 64 or scales other than 2 / 4 / 8."""
    if logits.shape[1] > 64 or logits.shape[1] < 2 or scale not in (2, 4, 8):
        return softargmin(trilinear_upsample(logits.unsqueeze(1), scale).squeeze(1))
    return _UpSoftArgmin.apply(logits, int(scale))


# ------------------------------------------------------------------------------------------------
# 3D convolutions
# ------------------------------------------------------------------------------------------------
def _round_up(a, m):
    return (a + m - 1) // m * m


# 3x3x3 stride-1 convolutions run on the bf16 matrix pipe with the exact three-way bf16 split of both operands
# ("bf16x3", conv3d_bf16x3.hip): fp32-grade accuracy (measured error vs fp64 slightly BELOW the fp32 MFMA kernel's)
# at 1.3-1.75x the speed on every shape the networks use, 1/4 to 1/16 resolution (tools/x3_vs_fp32.py).
# DCA_CONV=fp32 forces the fp32 MFMA kernel everywhere.
# DCA_CONV: "x2" (default) = 3x3x3 stride-1 convolutions and their weight gradients on the f16x2 split kernels
# (conv3d_f16x2.hip: two f16 terms per operand, three products, power-of-two operand scaling from the tensor's max |.|);
# "x3" = the bf16x3 split kernels for them; "fp32" = fp32 MFMA kernels everywhere.
_CONV_MODE = os.environ.get("DCA_CONV", "x2")
CONV_X3 = _CONV_MODE != "fp32"
CONV_X2 = _CONV_MODE == "x2"
WGRAD_S2_X2 = os.environ.get("DCA_WGRAD_S2", "x2") != "fp32"   # stride-2 / transposed weight gradient on the f16x2 split (A/B)
DECONV_X3 = os.environ.get("DCA_DECONV", "x3") != "fp32"
C1_WGRAD_FUSED = os.environ.get("DCA_C1_WGRAD", "fused") != "expand"   # logit heads: weight gradient without the 27-plane tensor (A/B)
CONV_S2_X2 = os.environ.get("DCA_CONV_S2", "x2") != "fp32"     # the stride-2 convolution itself on the f16x2 split (A/B)
BN_FUSE = os.environ.get("DCA_BN_FUSE", "1") != "0"        # BatchNorm batch statistics from the conv epilogue (training)   # the transposed-convolution member of the family alone (A/B timing)
C1_BWD_FUSE = os.environ.get("DCA_C1_BWD", "fused") != "split"      # 1x1x1 conv + BatchNorm backward as one launch (A/B)
SKIP_FOLD = os.environ.get("DCA_SKIP_FOLD", "1") != "0"    # cva skip BatchNorm folded into the block's output BatchNorm (A/B)
_X3_MIN_WORKGROUPS = 1


# ---- operand scales of the f16x2 kernels --------------------------------------------------------------------------------
# Every CHANNEL of an operand is scaled by its own power of two (csrc/dca_common.h).  What travels with a tensor object:
#   t._dca_cmax = (slots, nslots, version): per-channel maxima the kernel that WROTE t emitted (BatchNorm apply / backward,
#                 the f16x2 convolution's fused epilogue): slots[c * CSLOTS + s], s < nslots.  No zero-initialisation.
#   t._dca_exps = (exps, version): the per-channel scale exponents (C ints) once somebody derived them (the weight-packing
#                 kernel of the first convolution over t does, on the way).
#   t._dca_px2  = (exps,): t is NOT fp32 data but the packed px2 image of an fp32 tensor of t's shape (the two scaled f16
#                 terms, [term][C/8][D][H][W][8]), written by a BatchNorm kernel for the f16x2 convolution that consumes it.
#   t._dca_twin = (twin, version): the packed px2 image of the fp32 tensor t, written beside t by its BatchNorm
#                 (pack_out="both"); it lives exactly as long as t.
# `version` = t._version at tagging time: an in-place change of t invalidates the tag (_tag_ok is the one statement of that
# rule).  Tags are attached by the autograd Function that launches the producing kernel, inside its forward / backward -- an
# attribute set on an output there is still on what apply() returns -- and only through the four _tag_* setters.  Tensors
# without a tag get one read pass (dca_cmax_f32).
AMAX_STATS = {"tagged": 0, "computed": 0, "packed": 0}
CSLOTS = _C["DCA_AMAX_CSLOTS"]
AMAX_EMIT = os.environ.get("DCA_AMAX_EMIT", "1") != "0"    # 0: no producer-side maxima, every operand gets its read pass (A/B)
PACK = os.environ.get("DCA_PACK", "1") != "0"              # 0: no packed px2 operands, fp32 tensors everywhere (A/B)


def _cslots(C, device):
    """uninitialised per-channel slot words for a tensor with C channels (None when producer-side maxima are switched off)"""
    if not AMAX_EMIT:
        return None
    return torch.empty((C * CSLOTS,), device=device, dtype=torch.int32)


def _ver(t):
    """version counter of t, or None for an inference tensor (torch.inference_mode(): such a tensor does not track
    versions -- and cannot be changed in place outside inference mode, so its tag stays valid)"""
    return None if t.is_inference() else t._version


def _tag_cmax(t, slots, nslots):
    if slots is not None:
        t._dca_cmax = (slots, int(nslots), _ver(t))
    return t


def _tag_px2(t, exps):
    t._dca_px2 = (exps,)
    return t


def _tag_exps(t, exps):
    t._dca_exps = (exps, _ver(t))


def _tag_twin(t, twin):
    t._dca_twin = (twin, _ver(t))


def _tag_ok(t, name):
    """the versioned tag `name` of t if it is valid -- stamped with t's current version, payload on t's device -- else None"""
    tag = getattr(t, name, None)
    if tag is not None and tag[-1] == _ver(t) and tag[0].device == t.device:
        return tag
    return None


def _copy_tags(src, dst):
    """the valid operand tags of src on dst, a view of the same values (the alias output of _Conv3d)"""
    cmax, exps, twin = _tag_ok(src, "_dca_cmax"), _tag_ok(src, "_dca_exps"), _tag_ok(src, "_dca_twin")
    if cmax is not None:
        _tag_cmax(dst, cmax[0], cmax[1])
    if exps is not None:
        _tag_exps(dst, exps[0])
    if twin is not None:
        _tag_twin(dst, twin[0])


def _is_packed(t):
    return getattr(t, "_dca_px2", None) is not None


def _twin_of(t):
    """the packed px2 twin of the fp32 tensor t (written together with t by the BatchNorm apply pass), or None"""
    tag = _tag_ok(t, "_dca_twin")
    return None if tag is None else tag[0]


def _slots_of(t):
    """(slots, nslots) of the fp32 tensor t (N, C, ...): the producer's if t carries valid ones, else one read pass"""
    tag = _tag_ok(t, "_dca_cmax")
    if tag is not None:
        AMAX_STATS["tagged"] += 1
        return tag[0], tag[1]
    AMAX_STATS["computed"] += 1
    N, C = t.shape[0], t.shape[1]
    S = t[0, 0].numel()
    slots = torch.empty((C * CSLOTS,), device=t.device, dtype=torch.int32)
    lib = _L()
    _chk(lib.dca_cmax_f32(_ptr(t), N, C, S, _ptr(slots), _stream()), "dca_cmax_f32")
    nslots = lib.dca_bn_num_chunks(C, S)
    _tag_cmax(t, slots, nslots)
    return slots, nslots


def _exps_cached(t):
    if _is_packed(t):
        return t._dca_px2[0]
    tag = _tag_ok(t, "_dca_exps")
    return None if tag is None else tag[0]


def _exps_of(t):
    """per-channel scale exponents (C ints on the device) of operand t: packed tensor -> its own; cached; else from the slots"""
    ex = _exps_cached(t)
    if ex is not None:
        return ex
    slots, nslots = _slots_of(t)
    C = t.shape[1]
    ex = torch.empty((C,), device=t.device, dtype=torch.int32)
    _chk(_L().dca_cmax_exps(_ptr(slots), nslots, C, _ptr(ex), _stream()), "dca_cmax_exps")
    _tag_exps(t, ex)
    return ex


def pack_x2(x):
    """the packed px2 image of an fp32 tensor (N, C % 8 == 0, D, H, W) with exponents from its per-channel maxima (tests,
    micro-benchmarks; in the network the BatchNorm kernels write this format themselves)"""
    x = _req(x, "pack_x2")
    N, C = x.shape[0], x.shape[1]
    S = x[0, 0].numel()
    ex = _exps_of(x)
    xp = torch.empty_like(x)
    _chk(_L().dca_bn_apply_pack(_ptr(x), None, _ptr(ex), _ptr(xp), N, C, S, 1.0, None, None, None, None, None, _stream()),
         "dca_bn_apply_pack")
    return _tag_px2(xp, ex)


def _x3_eligible(x, x2, ksize, stride, transposed, A, B):
    if not CONV_X3 or ksize != 3 or stride != 1 or transposed or x2 is not None:
        return False
    N, _, D, H, W = x.shape
    tiles = N * ((D + 3) // 4) * ((H + 7) // 8) * ((W + 15) // 16) * ((B + 31) // 32)
    return tiles >= _X3_MIN_WORKGROUPS and max(A, B) * D * H * W * 4 < 0x7ffffff0


def _dx3_eligible(x, x2, ksize, stride, transposed, A, B):
    """transposed 3x3x3 stride-2 convs on the bf16x3 kernel of deconv3d_x3.hip: <= 32 output channels, coarse width
    divisible by 4, 16-byte aligned input"""
    if not CONV_X3 or not DECONV_X3 or not transposed or ksize != 3 or stride != 2 or x2 is not None or B > 32 or A > 64:
        return False
    N, _, D, H, W = x.shape
    return W % 4 == 0 and x.data_ptr() % 16 == 0 and max(A, 8) * D * H * W * 4 < 0x7ffffff0 and 256 * D * H * W * 4 < 0x7ffffff0


def _s2x2_eligible(x, x2, ksize, stride, transposed, A, B, scale, res_pre, slope):
    """3x3x3 stride-2 convs on the f16x2 kernel of conv3d_s2_f16x2.hip: plain output or the inference epilogue (folded
    BatchNorm, activation, res_post; no res_pre), fine width divisible by 4, 16-byte aligned input, enough tiles to fill the
    chip (small volumes stay on the fp32 MFMA kernel)"""
    if not (CONV_X2 and CONV_X3 and CONV_S2_X2) or ksize != 3 or stride != 2 or transposed or x2 is not None:
        return False
    if res_pre is not None or A > 256 or A <= 4:
        return False
    N, _, D, H, W = x.shape
    Do, Ho, Wo = (D + 1) // 2, (H + 1) // 2, (W + 1) // 2
    tiles = N * ((Do + 1) // 2) * ((Ho + 3) // 4) * ((Wo + 31) // 32) * ((B + 63) // 64)
    return (W % 4 == 0 and x.data_ptr() % 16 == 0 and tiles >= _X3_MIN_WORKGROUPS
            and (A + 3) * D * H * W * 4 < 0x7ffffff0 and (B + 63) * Do * Ho * Wo * 4 < 0x7ffffff0)


def _c1x3_eligible(x, x2, ksize, A, C1, y):
    """1x1x1 convs on the bf16x3 kernel of conv1_x3.hip (fp32-grade, LDS-free): channel layouts it is built for, voxel
    count divisible by 4, 16-byte aligned tensors"""
    if not CONV_X3 or ksize != 1:
        return False
    C2 = 0 if x2 is None else x2.shape[1]
    if (C1, C2) not in ((32, 0), (64, 0), (32, 32)) or A != C1 + C2:
        return False
    S = x[0, 0].numel()
    ptrs = [x.data_ptr(), y.data_ptr()] + ([] if x2 is None else [x2.data_ptr()])
    return S % 4 == 0 and all(p % 16 == 0 for p in ptrs) and 64 * S * 4 < 0x7ffffff0


def _conv_family(x, x2, A, B, ksize, stride, transposed, scale=None, res_pre=None, slope=1.0, y=None):
    """the kernel family that serves y = conv(x [, x2]) -- "x2" (conv3d_f16x2.hip), "x3" (conv3d_bf16x3.hip), "s2x2"
    (conv3d_s2_f16x2.hip), "dx3" (deconv3d_x3.hip), "c1x3" (conv1_x3.hip), else "mfma": the fp32 kernels of conv3d_mfma.hip,
    which take every shape.  The only caller of the *_eligible predicates; y (the output tensor) is read for ksize 1 only."""
    if _x3_eligible(x, x2, ksize, stride, transposed, A, B):
        return "x2" if CONV_X2 else "x3"
    if _s2x2_eligible(x, x2, ksize, stride, transposed, A, B, scale, res_pre, slope):
        return "s2x2"
    if _dx3_eligible(x, x2, ksize, stride, transposed, A, B):
        return "dx3"
    return "c1x3" if _c1x3_eligible(x, x2, ksize, A, x.shape[1], y) else "mfma"


def _c1_bwd_route(x, x2, weight, res_pre=None):
    """how the backward of a 1x1x1 convolution with a BatchNorm behind it runs -- "fused" (conv1_bwd_fused.hip: the BatchNorm
    backward stops after its reduction and hands dz on, ONE launch forms dy in registers and gives dx [, dx2] and dw) or
    "split" (the BatchNorm writes dy; backward-data and weight gradient per input through _conv_family / _wgrad_family).
    Asked once, in the forward, by convbn3d / convbn3d_pair: the BatchNorm and the convolution node get the same answer."""
    if not C1_BWD_FUSE or res_pre is not None or weight.dim() != 5 or weight.shape[2] != 1 or not torch.is_grad_enabled():
        return "split"
    C1, C2 = x.shape[1], (0 if x2 is None else x2.shape[1])
    if weight.shape[0] != 32 or (C1, C2) not in ((32, 0), (32, 32)) or weight.shape[1] != C1 + C2:
        return "split"
    tensors = (x, weight) if x2 is None else (x, x2, weight)
    if not all(t.is_cuda and t.dtype == torch.float32 and t.requires_grad for t in tensors):
        return "split"      # the launch produces every gradient
    if x2 is not None and x2.shape != x.shape:
        return "split"
    S = x[0, 0].numel()
    return "fused" if (S % 4 == 0 and x.shape[0] * 32 * S * 4 < 0x7ffff000) else "split"


def _c1_bwd_fused(dz, x, x2, weight):
    """(dx, dx2 or None, dw) of the 1x1x1 convolution whose BatchNorm handed its dz on (tag _dca_lazy, _BnAct.backward)"""
    tag = getattr(dz, "_dca_lazy", None)
    if tag is None:
        raise RuntimeError("conv3d.backward: expected the gradient the BatchNorm behind this 1x1x1 convolution hands on "
                           "(the tag was lost on the way through autograd)")
    y, stats, dgb, slope, training = tag
    if y.shape != dz.shape or y.shape[0] != x.shape[0] or y.shape[2:] != x.shape[2:]:
        raise RuntimeError("conv3d.backward: the BatchNorm's gradient does not belong to this convolution")
    N, C1 = x.shape[0], x.shape[1]
    C2 = 0 if x2 is None else x2.shape[1]
    S = x[0, 0].numel()
    lib = _L()
    part = torch.empty((lib.dca_conv1_bwd_fused_workspace(N, S, int(x2 is not None)),), device=x.device, dtype=torch.float32)
    gx = torch.empty_like(x)
    gx2 = None if x2 is None else torch.empty_like(x2)
    gw = torch.empty_like(weight)
    _chk(lib.dca_conv1_bwd_fused(_ptr(dz), _ptr(y), _ptr(stats), _ptr(dgb), float(slope), int(training), _ptr(x), _ptr(x2),
                                 _ptr(weight), _ptr(part), _ptr(gx), _ptr(gx2), _ptr(gw), C1 + C2, 1, N, C1, C2,
                                 weight.shape[0], S, _stream()), "dca_conv1_bwd_fused")
    return gx, gx2, gw


class _SkipBn:
    """The skip branch of a block on the folded route (_skip_fold_route): the raw output y of its 1x1x1 convolution, that
    output's batch-statistics partials (or None) and the slope-1 BatchNorm still to be applied to it.  Handed to `convbn3d` as
    res_pre, where the block's output BatchNorm applies it in registers (_BnSkipAct); it is never a tensor."""
    __slots__ = ("y", "part", "bn", "into")

    def __init__(self, y, part, bn, into):
        self.y, self.part, self.bn, self.into = y, part, bn, into


def _skip_fold_route(x, conv_b, bn_b, slope_b, bn_out):
    """how act(BN_out(.) + BN_b(conv_b(x))) runs, BN_b a slope-1 BatchNorm whose only reader is BN_out's res_pre -- "fold":
    BN_b is not applied on its own, the apply and backward passes of BN_out form it in registers and its backward reduction
    rides in BN_out's (_BnSkipAct: a read of y_r for the skip's maxima instead of the pass that writes the skip tensor, and no
    pass that re-reads g for BN_b's sums), or "apply":
    two `_BnAct` nodes.  The folded kernels exist for what the training step runs: batch statistics of both BatchNorms under
    grad, fp32, the packed px2 output with its fp32 copy (pack_out="both", promised by the caller with `bn_out`), and a
    1x1x1 convolution whose backward takes BN_b's dz as it is (_c1_bwd_route).  Asked once, by convbn3d_pair."""
    if not (SKIP_FOLD and PACK and CONV_X2 and bn_out is not None and torch.is_grad_enabled() and _lp_dtype() is None):
        return "apply"
    C = bn_b.num_features
    if not (bn_b.training and bn_out.training) or bn_out.num_features != C or C % 8 or float(slope_b) != 1.0:
        return "apply"
    if x.dtype != torch.float32 or bn_b.weight is None or bn_b.bias is None:
        return "apply"
    return "fold" if _c1_bwd_route(x, None, conv_b.weight) == "fused" else "apply"


def _k3s1(weight, stride, transposed, x2, head=False):
    """a 3x3x3 stride-1 convolution of one input, not transposed, that is not a logit head (Cout > 1): what the packed px2
    operands, the twin and the alias output exist for.  head=True: that is one (Cout == 1) instead."""
    return x2 is None and not transposed and int(stride) == 1 and weight.shape[2] == 3 and (weight.shape[0] == 1) == head


def _x2_pairs(xp, yp, W):
    """may the f16x2 3x3x3 stride-1 weight-gradient kernel read these two operands (packed px2 or not) at width W?  An fp32
    operand needs W % 4 == 0 there; at any other width only two packed ones pair."""
    return W % 4 == 0 or (xp and yp)


def _wgrad_family(x, dy, Cx, Cy, ksize, stride):
    """the kernel that serves the weight gradient of fine tensor x and dy: "x2" (conv3d_wgrad_f16x2.hip), "x3"
    (conv3d_wgrad_bf16x3.hip), "s2x2" (conv3d_wgrad_s2_f16x2.hip: stride-2 / transposed convolution), else "mfma"
    (conv3d_wgrad.hip, exact fp32, every shape).  Raises for a packed px2 operand that "x2" cannot take."""
    Di, Hi, Wi = x.shape[2:]
    Do, Ho, Wo = dy.shape[2:]
    xp, yp = _is_packed(x), _is_packed(dy)
    split = (CONV_X3 and ksize == 3 and x.data_ptr() % 16 == 0 and dy.data_ptr() % 16 == 0
             and max(Cx, Cy) * Di * Hi * Wi * 4 < 0x7ffffff0)
    if split and CONV_X2 and stride == 1 and _x2_pairs(xp, yp, Wi):
        return "x2"
    if xp or yp:
        raise RuntimeError("weight gradient: a packed px2 operand can only feed the f16x2 3x3x3 stride-1 kernel")
    if split and stride == 1 and Wi % 4 == 0:
        return "x3"
    if (split and CONV_X2 and WGRAD_S2_X2 and stride == 2 and Wi % 4 == 0 and Wo % 4 == 0
            and (Do, Ho, Wo) == ((Di + 1) // 2, (Hi + 1) // 2, (Wi + 1) // 2)):
        return "s2x2"
    return "mfma"


def _slice_width(ksize, stride, transposed, B):
    """output channels one launch of dca_conv3d_forward produces (include/dca_hip.h)"""
    if ksize == 1 or transposed:
        return 32
    return 32 if (stride == 1 and B <= 32) else 64


def _prep_weight(w_src, A, B, K, src_ab, flip, ksize, stride, transposed, b_off=0, Bn=None):
    """wt[tap][Apad][Bpad] for the output-channel slice [b_off, b_off+Bn) (padding rules of include/dca_hip.h)."""
    Bn = B if Bn is None else Bn
    if ksize == 1:
        Apad = 32 if A <= 32 else 64
        Bpad = 32
    else:
        Apad = _round_up(A, 8)
        Bpad = 32 if (transposed or (stride == 1 and Bn <= 32)) else 64
    def build():
        wt = torch.empty((K, Apad, Bpad), device=w_src.device, dtype=torch.float32)
        _chk(_L().dca_conv3d_prep_weight(_ptr(w_src), _ptr(wt), A, Bn, Apad, Bpad, K, int(src_ab), int(flip), B, b_off,
                                         _stream()), "dca_conv3d_prep_weight")
        return wt
    return _memo(("prep", A, B, K, int(src_ab), int(flip), Apad, Bpad, b_off, Bn), (w_src,), build,
                 (0, A, Bn, Apad, Bpad, K, int(src_ab), int(flip), B, b_off)), Apad


def _x2_weights(prefix, x, w_src, A, B, src_ab, flip, cached_key):
    """(wx, xexps) for ONE launch of the f16x2-family convolution `prefix` ("dca_conv3d_x2" / "dca_conv3d_s2x2") over operand
    x.  The weights are packed per launch: the image folds the operand's per-channel exponents in (dca_hip.h).  Exponents x
    already carries are used (counted under AMAX_STATS[cached_key]); otherwise the packing kernel derives them from the
    operand's slots on the way and they stay on the tensor for later users (the weight gradient of this convolution, other
    convolutions over the same tensor)."""
    lib = _L()
    wx = torch.empty((getattr(lib, prefix + "_weight_bytes")(A, B) // 2,), device=x.device, dtype=torch.int16)
    xexps = _exps_cached(x)
    if xexps is not None:
        AMAX_STATS[cached_key] += 1
        slots, nslots = None, 0
    else:
        slots, nslots = _slots_of(x)
        xexps = torch.empty((A,), device=x.device, dtype=torch.int32)
    _chk(getattr(lib, prefix + "_prep_weight")(_ptr(w_src), _ptr(wx), A, B, int(src_ab), int(flip), _ptr(slots), nslots,
                                               _ptr(xexps), _stream()), prefix + "_prep_weight")
    if slots is not None:
        _tag_exps(x, xexps)
    return wx, xexps


def _x3_weights(w_src, A, B, src_ab, flip):
    """the bf16x3 fragments of a 3x3x3 weight (conv3d_bf16x3.hip and deconv3d_x3.hip read the same image), memoised"""
    def build():
        w3 = torch.empty((_L().dca_conv3d_x3_weight_bytes(A, B) // 2,), device=w_src.device, dtype=torch.int16)
        _chk(_L().dca_conv3d_x3_prep_weight(_ptr(w_src), _ptr(w3), A, B, int(src_ab), int(flip), _stream()),
             "dca_conv3d_x3_prep_weight")
        return w3
    return _memo(("x3prep", A, B, int(src_ab), int(flip)), (w_src,), build, (1, A, B, 0, 0, 27, int(src_ab), int(flip), B, 0))


def _out_dims(dims, ksize, stride, transposed):
    if ksize == 1 or stride == 1:
        return tuple(dims)
    if transposed:
        return tuple(2 * d for d in dims)
    return tuple((d + 1) // 2 for d in dims)


def _conv_sliced(x, x2, w_src, A, B, K, src_ab, flip, ksize, stride, transposed, scale=None, shift=None, slope=1.0,
                 res_pre=None, res_post=None, want_stats=False, emit_amax=False):
    """y = conv(x [, x2]) with A contraction channels and B output channels, as ceil(B / slice) launches that each
    write their channel slice of y (w_src is the PyTorch weight; src_ab / flip as in dca_conv3d_prep_weight).
    want_stats (no epilogue then): returns (y, part) where part holds the BatchNorm batch-statistics partials of y emitted
    by the convolution kernel itself (B * nchunk * 4 doubles, csrc/bn_fused_stats.h), or (y, None) when the kernel serving
    this shape has no such form.  x may be a packed px2 operand (f16x2 kernels only); emit_amax: tag y with its per-channel
    maxima where the kernel serving this shape can emit them (inference chains conv -> conv)"""
    N, C1, Di, Hi, Wi = x.shape
    Do, Ho, Wo = _out_dims((Di, Hi, Wi), ksize, stride, transposed)
    y = torch.empty((N, B, Do, Ho, Wo), device=x.device, dtype=torch.float32)
    packed = _is_packed(x)
    family = _conv_family(x, x2, A, B, ksize, stride, transposed, scale, res_pre, slope, y)
    if packed and family != "x2":
        raise RuntimeError("conv3d: a packed px2 operand can only feed the f16x2 3x3x3 stride-1 convolution")
    lib = _L()
    partials = lambda nchunk: torch.empty((B * nchunk * 4,), device=x.device, dtype=torch.float64)   # bn_fused_stats.h
    part = None
    if family == "x2":
        wx, xexps = _x2_weights("dca_conv3d_x2", x, w_src, A, B, src_ab, flip, "packed" if packed else "tagged")
        if want_stats:
            part = partials(lib.dca_conv3d_x2_stats_chunks(N, B, Di, Hi, Wi))
            _chk(lib.dca_conv3d_x2_forward_stats(_ptr(x), int(packed), _ptr(xexps), _ptr(wx), _ptr(y), _ptr(part), N, A, B,
                                                 Di, Hi, Wi, _stream()), "dca_conv3d_x2_forward_stats")
        else:
            ycm = _cslots(B, x.device) if emit_amax else None
            _chk(lib.dca_conv3d_x2_forward(_ptr(x), int(packed), _ptr(xexps), _ptr(wx), _ptr(y), _ptr(scale), _ptr(shift),
                                           _ptr(res_pre), _ptr(res_post), float(slope), _ptr(ycm), N, A, B, Di, Hi, Wi,
                                           _stream()), "dca_conv3d_x2_forward")
            _tag_cmax(y, ycm, lib.dca_conv3d_x2_stats_chunks(N, B, Di, Hi, Wi))
    elif family == "x3":
        wx = _x3_weights(w_src, A, B, src_ab, flip)
        if want_stats:
            part = partials(lib.dca_conv3d_x3_stats_chunks(N, B, Di, Hi, Wi))
            _chk(lib.dca_conv3d_x3_forward_stats(_ptr(x), _ptr(wx), _ptr(y), _ptr(part), N, A, B, Di, Hi, Wi, _stream()),
                 "dca_conv3d_x3_forward_stats")
        else:
            _chk(lib.dca_conv3d_x3_forward(_ptr(x), _ptr(wx), _ptr(y), _ptr(scale), _ptr(shift), _ptr(res_pre),
                                           _ptr(res_post), float(slope), N, A, B, Di, Hi, Wi, _stream()),
                 "dca_conv3d_x3_forward")
    elif family == "s2x2":
        wx, xexps = _x2_weights("dca_conv3d_s2x2", x, w_src, A, B, src_ab, flip, "tagged")
        nsl = lib.dca_conv3d_s2x2_out_slots(N, B, Di, Hi, Wi)
        ycm = _cslots(B, x.device) if (emit_amax and nsl <= CSLOTS) else None
        _chk(lib.dca_conv3d_s2x2_forward(_ptr(x), _ptr(xexps), _ptr(wx), _ptr(y), _ptr(scale), _ptr(shift), float(slope),
                                         _ptr(res_post), _ptr(ycm), N, A, B, Di, Hi, Wi, _stream()), "dca_conv3d_s2x2_forward")
        if ycm is not None:
            _tag_cmax(y, ycm, nsl)
    elif family == "dx3":
        wx = _x3_weights(w_src, A, B, src_ab, flip)
        if want_stats:
            part = partials(lib.dca_deconv3d_x3_stats_chunks(N, Di, Hi, Wi))
            _chk(lib.dca_deconv3d_x3_forward_stats(_ptr(x), _ptr(wx), _ptr(y), _ptr(part), N, A, B, Di, Hi, Wi,
                                                   _stream()), "dca_deconv3d_x3_forward_stats")
        else:
            _chk(lib.dca_deconv3d_x3_forward(_ptr(x), _ptr(wx), _ptr(y), _ptr(scale), _ptr(shift), _ptr(res_pre),
                                             _ptr(res_post), float(slope), N, A, B, Di, Hi, Wi, _stream()),
                 "dca_deconv3d_x3_forward")
    elif family == "c1x3":
        S = Do * Ho * Wo
        C2 = 0 if x2 is None else x2.shape[1]
        if want_stats:
            part = partials(lib.dca_conv1_x3_stats_chunks(N, S))
        for b0 in range(0, B, 32):
            bn = min(32, B - b0)

            def build_c1(b0=b0, bn=bn):
                wf = torch.empty((lib.dca_conv1_x3_weight_bytes(A) // 2,), device=x.device, dtype=torch.int16)
                _chk(lib.dca_conv1_x3_prep_weight(_ptr(w_src), _ptr(wf), A, bn, int(src_ab), B, b0, _stream()),
                     "dca_conv1_x3_prep_weight")
                return wf
            wf = _memo(("c1x3prep", A, B, int(src_ab), b0, bn), (w_src,), build_c1,
                       (2, A, bn, 0, 0, 1, int(src_ab), 0, B, b0))
            if part is not None:
                _chk(lib.dca_conv1_x3_forward_stats(_ptr(x), _ptr(x2), _ptr(wf), _ptr(y), _ptr(part), N, C1, C2, bn, B, b0,
                                                    S, _stream()), "dca_conv1_x3_forward_stats")
            else:
                _chk(lib.dca_conv1_x3_forward(_ptr(x), _ptr(x2), _ptr(wf), _ptr(y), _ptr(scale), _ptr(shift),
                                              _ptr(res_pre), _ptr(res_post), float(slope), N, C1, C2, bn, B, b0, S,
                                              _stream()), "dca_conv1_x3_forward")
    else:
        width = _slice_width(ksize, stride, transposed, B)
        for b0 in range(0, B, width):
            bn = min(width, B - b0)
            wt, Apad = _prep_weight(w_src, A, B, K, src_ab, flip, ksize, stride, transposed, b0, bn)
            _chk(lib.dca_conv3d_forward(_ptr(x), _ptr(x2), _ptr(wt), _ptr(y), _ptr(scale), _ptr(shift), _ptr(res_pre),
                                        _ptr(res_post), float(slope), N, A, C1, bn, Apad, B, b0, Di, Hi, Wi, Do, Ho, Wo,
                                        ksize, stride, int(transposed), _stream()), "dca_conv3d_forward")
    return (y, part) if want_stats else y


def conv3d_prepared(x, wt, A, Apad, B, ksize, stride, transposed):
    """single launch with an already laid-out weight (used by bench.py to time the bare kernel)"""
    N = x.shape[0]
    Di, Hi, Wi = x.shape[2:]
    Do, Ho, Wo = _out_dims((Di, Hi, Wi), ksize, stride, transposed)
    y = torch.empty((N, B, Do, Ho, Wo), device=x.device, dtype=torch.float32)
    _chk(_L().dca_conv3d_forward(_ptr(x), None, _ptr(wt), _ptr(y), None, None, None, None, 1.0, N, A, A, B, Apad, B, 0,
                                 Di, Hi, Wi, Do, Ho, Wo, ksize, stride, int(transposed), _stream()),
         "dca_conv3d_forward")
    return y


def _conv_forward_impl(x, x2, weight, stride, transposed, scale=None, shift=None, slope=1.0, res_pre=None,
                       res_post=None, want_stats=False, emit_amax=False):
    ksize = weight.shape[2]
    K = ksize ** 3
    if transposed:
        Cin, Cout = weight.shape[0], weight.shape[1]
        src_ab = 1
    else:
        Cout, Cin = weight.shape[0], weight.shape[1]
        src_ab = 0
    assert x.shape[1] + (x2.shape[1] if x2 is not None else 0) == Cin, "conv3d: channel mismatch"
    return _conv_sliced(x, x2, weight, Cin, Cout, K, src_ab, 0, ksize, stride, transposed, scale, shift, slope,
                        res_pre, res_post, want_stats, emit_amax)


def _wgrad(x, dy, dw_view_ptr_tensor, dst_offset, Cx, Cy, ksize, stride, s_cy, s_cx):
    """dw[cy*s_cy + cx*s_cx + k] (+dst_offset floats) = sum dy[cy] * x[cx] (see dca_hip.h); x / dy may be packed px2
    operands (3x3x3 stride 1 on the f16x2 kernel only)."""
    N = x.shape[0]
    Di, Hi, Wi = x.shape[2:]
    Do, Ho, Wo = dy.shape[2:]
    dst = _vp(dw_view_ptr_tensor.data_ptr() + 4 * dst_offset)
    lib = _L()
    family = _wgrad_family(x, dy, Cx, Cy, ksize, stride)
    workspace = lambda nws: torch.empty((nws,), device=x.device, dtype=torch.float32)
    if family == "x2":
        xex, yex = _exps_of(x), _exps_of(dy)
        part = workspace(lib.dca_conv3d_wgrad_x2_workspace(N, Cx, Cy, Di, Hi, Wi))
        _chk(lib.dca_conv3d_wgrad_x2(_ptr(x), int(_is_packed(x)), _ptr(xex), _ptr(dy), int(_is_packed(dy)), _ptr(yex),
                                     _ptr(part), dst, N, Cx, Cy, Di, Hi, Wi, s_cy, s_cx, _stream()), "dca_conv3d_wgrad_x2")
    elif family == "x3":
        part = workspace(lib.dca_conv3d_wgrad_x3_workspace(N, Cx, Cy, Di, Hi, Wi))
        _chk(lib.dca_conv3d_wgrad_x3(_ptr(x), _ptr(dy), _ptr(part), dst, N, Cx, Cy, Di, Hi, Wi, s_cy, s_cx, _stream()),
             "dca_conv3d_wgrad_x3")
    elif family == "s2x2":
        # stride-2 convolution / transposed convolution: x = the fine tensor, dy = the coarse one (conv3d_wgrad_s2_f16x2.hip)
        xex, yex = _exps_of(x), _exps_of(dy)
        part = workspace(lib.dca_conv3d_wgrad_s2_x2_workspace(N, Cx, Cy, Di, Hi, Wi))
        _chk(lib.dca_conv3d_wgrad_s2_x2(_ptr(x), _ptr(xex), _ptr(dy), _ptr(yex), _ptr(part), dst, N, Cx, Cy, Di, Hi, Wi,
                                        s_cy, s_cx, _stream()), "dca_conv3d_wgrad_s2_x2")
    else:
        part = workspace(lib.dca_conv3d_wgrad_workspace(N, Cx, Cy, Do, Ho, Wo, ksize, stride))
        _chk(lib.dca_conv3d_wgrad(_ptr(x), _ptr(dy), _ptr(part), dst, N, Cx, Cy, Di, Hi, Wi, Do, Ho, Wo, ksize, stride,
                                  s_cy, s_cx, _stream()), "dca_conv3d_wgrad")


class _Conv3dC1(torch.autograd.Function):
    """nn.Conv3d(C, 1, 3, padding=1, bias=False): the logit heads.  The 27 taps become a GEMM axis so forward and
    weight gradient run on the 1x1x1 matrix-core kernels (see include/dca_hip.h); C must be 32 or 64."""

    @staticmethod
    def forward(ctx, x, weight):
        x, weight = _req(x, "conv3d"), _req(weight, "conv3d.weight")
        N, C, D, H, W = x.shape
        with torch.cuda.device_of(x):
            T = _conv_sliced(x, None, weight, C, 27, 1, 1, 0, 1, 1, False)      # wt[ci][tap] = w[0, ci, tap]; (N,27,D,H,W)
            y = torch.empty((N, 1, D, H, W), device=x.device, dtype=torch.float32)
            _chk(_L().dca_conv3d_c1_gather(_ptr(T), _ptr(y), N, D, H, W, _stream()), "dca_conv3d_c1_gather")
        ctx.save_for_backward(x, weight)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dy = _req(dy, "conv3d.backward")
        N, C, D, H, W = x.shape
        gx = gw = None
        lib = _L()
        with torch.cuda.device_of(x):
            if ctx.needs_input_grad[0]:
                gx = torch.empty_like(x)
                _chk(lib.dca_conv3d_c1_bwd_data(_ptr(dy), _ptr(weight), _ptr(gx), N, C, D, H, W, _stream()),
                     "dca_conv3d_c1_bwd_data")
            if ctx.needs_input_grad[1]:
                gw = torch.empty_like(weight)
                if (C1_WGRAD_FUSED and W % 4 == 0 and x.data_ptr() % 16 == 0 and dy.data_ptr() % 16 == 0
                        and x.numel() * 4 < 0x7ffffff0):
                    # the tap-shifted views of dy are built inside the weight-gradient kernel: no 27-plane tensor
                    nws = lib.dca_conv3d_wgrad_workspace(N, C, 27, D, H, W, 1, 1)
                    part = torch.empty((nws,), device=x.device, dtype=torch.float32)
                    _chk(lib.dca_conv3d_c1_wgrad(_ptr(x), _ptr(dy), _ptr(part), _ptr(gw), N, C, D, H, W, _stream()),
                         "dca_conv3d_c1_wgrad")
                else:
                    G = torch.empty((N, 27, D, H, W), device=x.device, dtype=torch.float32)
                    _chk(lib.dca_conv3d_c1_expand(_ptr(dy), _ptr(G), N, D, H, W, _stream()), "dca_conv3d_c1_expand")
                    _wgrad(x, G, gw, 0, C, 27, 1, 1, 1, 27)                      # dw[ci*27 + tap]
        return gx, gw


class _Conv3d(torch.autograd.Function):
    """Conv3d (k=3 pad=1 stride 1|2, or k=1) / ConvTranspose3d (k=3 s=2 p=1 op=1), bias=False.
    Optional second input x2 = implicit channel concat for the 1x1x1 `fuse` conv."""

    @staticmethod
    def forward(ctx, x, x2, weight, stride, transposed, want_stats=False, alias=False, packed_dy=False, lazy_dy=False):
        """want_stats: returns (y, part) -- part = the BatchNorm batch-statistics partials of y from the convolution
        kernel's own epilogue (not differentiable; csrc/bn_fused_stats.h), empty where the kernel serving this shape
        cannot produce them.
        alias (3x3x3 stride 1 only): one more output, x itself, for the OTHER consumers of x -- their summed gradient comes
        back as that output's gradient and is added inside this convolution's backward-data launch (epilogue `+ res_post`)
        instead of by autograd's separate accumulation pass."""
        x, weight = _req(x, "conv3d", packed_ok=True), _req(weight, "conv3d.weight")
        x2 = _opt(x2, "conv3d.x2")
        if _is_packed(x) and alias:
            raise RuntimeError("conv3d: alias output of a packed px2 operand")
        ctx.save_for_backward(x, x2, weight)
        ctx.meta = (stride, transposed)
        ctx.alias = bool(alias)
        ctx.set_materialize_grads(False)             # an unused output's gradient arrives as None, not as a tensor of zeros
        ctx.x_px2 = getattr(x, "_dca_px2", None)    # save_for_backward keeps the tensor, not its Python attributes
        ctx.packed_dy = bool(packed_dy)              # the gradient of y arrives as a packed px2 operand (_BnAct, pack_dy)
        ctx.lazy_dy = bool(lazy_dy)                  # it arrives as the BatchNorm's own dz, tagged (_BnAct, lazy_dy)
        ctx.x_exps = None
        # a packed twin of x (written beside it by its BatchNorm): this convolution and its weight gradient read the twin
        Cout, Cin = weight.shape[:2]
        twin = PACK and _k3s1(weight, stride, transposed, x2) and _conv_family(x, None, Cin, Cout, 3, 1, False) == "x2"
        xt = _twin_of(x) if twin else None
        ctx.x_twin = xt
        xin = x if xt is None else xt
        with torch.cuda.device_of(x):
            out = _conv_forward_impl(xin, x2, weight, stride, transposed, want_stats=want_stats)   # y, or (y, part)
            ctx.x_exps = _exps_cached(xin)             # forward and weight gradient scale x by the same exponents
        if want_stats:
            part = out[1] if out[1] is not None else torch.empty((0,), device=x.device, dtype=torch.float64)
            ctx.mark_non_differentiable(part)
            out = (out[0], part)
        if alias:
            xa = x.view_as(x)
            _copy_tags(x, xa)
            out = (out + (xa,)) if want_stats else (out, xa)
        return out

    @staticmethod
    def backward(ctx, dy, *rest):
        x, x2, weight = ctx.saved_tensors
        xw = x                                      # the operand of the weight gradient
        if ctx.x_twin is not None:
            xw = ctx.x_twin                         # (tagged px2 when it was written)
        elif ctx.x_px2 is not None:
            _tag_px2(x, ctx.x_px2[0])
        elif ctx.x_exps is not None and _exps_cached(x) is None:
            _tag_exps(x, ctx.x_exps)
        stride, transposed = ctx.meta
        g_alias = _opt(rest[-1], "conv3d.backward") if (ctx.alias and rest) else None
        if dy is None:       # y was not used: nothing flows through the convolution, only past it (alias)
            return g_alias, None, None, None, None, None, None, None, None
        if ctx.packed_dy and not _is_packed(dy):
            raise RuntimeError("conv3d.backward: expected the packed px2 gradient of the BatchNorm behind this convolution "
                               "(the tag was lost on the way through autograd)")
        dy = _req(dy, "conv3d.backward", packed_ok=True)
        if ctx.x_twin is not None and not _x2_pairs(True, _is_packed(dy), x.shape[-1]):
            # the twin cannot be paired with this dy (an fp32 x of such a width never gets a packed one: _pack_dy_ok): the
            # weight gradient reads the fp32 x and takes the kernel that serves this width; the forward read the twin, which
            # holds the same values
            xw = x
        ksize = weight.shape[2]
        K = ksize ** 3
        gx = gx2 = gw = None
        need_x, need_x2, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        with torch.cuda.device_of(x):
            if transposed:
                Cin, Cout = weight.shape[0], weight.shape[1]
                if need_x:  # stride-2 conv of dy with Wt read as a Conv3d weight [Cin][Cout][K]
                    gx = _conv_sliced(dy, None, weight, Cout, Cin, K, 0, 0, 3, 2, False)
                if need_w:
                    gw = torch.empty_like(weight)
                    _wgrad(dy, x, gw, 0, Cout, Cin, 3, 2, Cout * K, K)
            elif ksize == 3:
                Cout, Cin = weight.shape[0], weight.shape[1]
                if need_x:
                    if stride == 1:   # dy's max-|.| word: tag or one pass; + the other consumers' gradient of x (alias)
                        gx = _conv_sliced(dy, None, weight, Cout, Cin, K, 1, 1, 3, 1, False, res_post=g_alias)
                        g_alias = None
                    else:
                        gx = _conv_sliced(dy, None, weight, Cout, Cin, K, 1, 0, 3, 2, True)
                        if gx.shape != x.shape:
                            raise RuntimeError("stride-2 conv backward needs even input dims")
                if need_w:
                    gw = torch.empty_like(weight)
                    _wgrad(xw, dy, gw, 0, Cin, Cout, 3, stride, Cin * K, K)
            else:
                Cout, Cin = weight.shape[0], weight.shape[1]
                w2 = weight.reshape(Cout, Cin)
                C1 = x.shape[1]
                if Cout not in (32, 64):
                    raise RuntimeError("1x1x1 conv backward-data needs 32 or 64 output channels")
                if ctx.lazy_dy:
                    gx, gx2, gw = _c1_bwd_fused(dy, x, x2, weight)
                    need_x = need_x2 = need_w = False
                if need_x:
                    wa = w2[:, :C1].contiguous()
                    gx = _conv_sliced(dy, None, wa, Cout, C1, 1, 1, 0, 1, 1, False)
                if x2 is not None and need_x2:
                    wb = w2[:, C1:].contiguous()
                    gx2 = _conv_sliced(dy, None, wb, Cout, Cin - C1, 1, 1, 0, 1, 1, False)
                if need_w:
                    gw = torch.empty_like(weight)
                    _wgrad(x, dy, gw, 0, C1, Cout, 1, 1, Cin, 1)
                    if x2 is not None:
                        _wgrad(x2, dy, gw, C1, Cin - C1, Cout, 1, 1, Cin, 1)
        if g_alias is not None:      # alias on a path without the fused form
            gx = g_alias if gx is None else gx + g_alias
        return gx, gx2, gw, None, None, None, None, None, None


class _ConvPair(torch.autograd.Function):
    """Two convolutions of ONE input -- A: 3x3x3 stride 2, B: 1x1x1 (`cost_agg.conv1` and `cost_agg.redir` of
    Multi_Aggregation, models/augment/cva.py:16-23) -- as one autograd node, so that the gradient of the shared input is
    formed inside the second backward-data launch (epilogue `+ res_post`) instead of by autograd's separate accumulation add
    (three passes over a 1/4-resolution tensor).  Same kernels, same values: (a + b) is one fp32 addition either way."""

    @staticmethod
    def forward(ctx, x, wa, wb, want_stats, lazy_b=False):
        """lazy_b: the gradient of the 1x1x1 branch arrives as its BatchNorm's own dz, tagged (_BnAct, lazy_dy)"""
        x, wa, wb = _req(x, "conv_pair"), _req(wa, "conv_pair.weight_a"), _req(wb, "conv_pair.weight_b")
        ctx.save_for_backward(x, wa, wb)
        ctx.lazy_b = bool(lazy_b)
        with torch.cuda.device_of(x):
            if want_stats:
                ya, pa = _conv_forward_impl(x, None, wa, 2, False, want_stats=True)
                yb, pb = _conv_forward_impl(x, None, wb, 1, False, want_stats=True)
            else:
                ya, pa = _conv_forward_impl(x, None, wa, 2, False), None
                yb, pb = _conv_forward_impl(x, None, wb, 1, False), None
        none = lambda: torch.empty((0,), device=x.device, dtype=torch.float64)
        pa, pb = (none() if pa is None else pa), (none() if pb is None else pb)
        ctx.mark_non_differentiable(pa, pb)
        return ya, pa, yb, pb

    @staticmethod
    def backward(ctx, dya, _dpa, dyb, _dpb):
        x, wa, wb = ctx.saved_tensors
        dya, dyb = _req(dya, "conv_pair.backward"), _req(dyb, "conv_pair.backward")
        Ca, Cin, Cb = wa.shape[0], wa.shape[1], wb.shape[0]
        if Cb not in (32, 64):
            raise RuntimeError("1x1x1 conv backward-data needs 32 or 64 output channels")
        with torch.cuda.device_of(x):
            if ctx.lazy_b:
                gb, _, gwb = _c1_bwd_fused(dyb, x, None, wb)
            else:
                gb = _conv_sliced(dyb, None, wb.reshape(Cb, Cin).contiguous(), Cb, Cin, 1, 1, 0, 1, 1, False)
                gwb = None
            gx = _conv_sliced(dya, None, wa, Ca, Cin, 27, 1, 0, 3, 2, True, res_post=gb)     # d(x) = A^T dya + B^T dyb
            if gx.shape != x.shape:
                raise RuntimeError("stride-2 conv backward needs even input dims")
            gwa = torch.empty_like(wa)
            _wgrad(x, dya, gwa, 0, Cin, Ca, 3, 2, Cin * 27, 27)
            if gwb is None:
                gwb = torch.empty_like(wb)
                _wgrad(x, dyb, gwb, 0, Cin, Cb, 1, 1, Cin, 1)
        return gx, gwa, gwb, None, None


PAIR_FUSE = os.environ.get("DCA_PAIR_FUSE", "1") != "0"


def convbn3d_pair(x, conv_a, bn_a, slope_a, conv_b, bn_b, slope_b, pack_a=False, skip_into=None):
    """(act(BN_a(conv_a(x))), act(BN_b(conv_b(x)))) for conv_a = Conv3d(k3, s2, p1), conv_b = Conv3d(k1) over the SAME x;
    training path: one autograd node for the two convolutions (`_ConvPair`), otherwise two `convbn3d` calls.
    pack_a: the first result has one consumer, a 3x3x3 stride-1 convolution (see convbn3d, pack_out)
    skip_into: the caller promises that the second result has ONE reader, the res_pre of a `convbn3d` call with this
    BatchNorm module and pack_out="both".  On the folded route (_skip_fold_route) the second result is then a `_SkipBn`
    record for that call instead of a tensor."""
    inference = (not bn_a.training and not bn_b.training and not torch.is_grad_enabled())
    ok = (PAIR_FUSE and not inference and _lp_dtype() is None and conv_a.kernel_size[0] == 3 and conv_a.stride[0] == 2
          and conv_b.kernel_size[0] == 1 and conv_b.weight.shape[0] in (32, 64) and x.dtype == torch.float32
          and not isinstance(conv_a, torch.nn.ConvTranspose3d) and all(d % 2 == 0 for d in x.shape[2:]))
    if not ok:
        return convbn3d(x, conv_a, bn_a, slope_a, pack_out=pack_a), convbn3d(x, conv_b, bn_b, slope_b)
    stats = bool(BN_FUSE and bn_a.training and bn_b.training)
    fold = _skip_fold_route(x, conv_b, bn_b, slope_b, skip_into) == "fold"
    lazy = fold or _c1_bwd_route(x, None, conv_b.weight) == "fused"
    ya, pa, yb, pb = _ConvPair.apply(x, conv_a.weight, conv_b.weight, stats, lazy)
    za = bn_act(ya, bn_a, slope_a, stats_part=pa if pa.numel() else None, pack_out=pack_a)
    if fold:
        return za, _SkipBn(yb, pb if pb.numel() else None, bn_b, skip_into)
    zb = bn_act(yb, bn_b, slope_b, stats_part=pb if pb.numel() else None, lazy_dy=lazy)
    return za, zb


def conv3d(x, weight, stride=1, transposed=False, x2=None):
    if _k3s1(weight, stride, transposed, x2, head=True) and weight.shape[1] in (32, 64):
        return _Conv3dC1.apply(x, weight)
    return _Conv3d.apply(x, x2, weight, int(stride), bool(transposed))


def conv3d_fused_inference(x, weight, stride, transposed, scale, shift, slope, res_pre=None, res_post=None, x2=None):
    """Forward-only conv with the affine (folded BatchNorm) + activation + residual epilogue fused."""
    x, weight = _req(x, "conv3d"), _req(weight, "conv3d.weight")
    with torch.cuda.device_of(x):
        return _conv_forward_impl(x, _opt(x2, "x2"), weight, int(stride), bool(transposed), _opt(scale, "scale"),
                                  _opt(shift, "shift"), slope, _opt(res_pre, "res_pre"), _opt(res_post, "res_post"),
                                  emit_amax=CONV_X2 and AMAX_EMIT)


# ------------------------------------------------------------------------------------------------
# BatchNorm3d + activation + residual
# ------------------------------------------------------------------------------------------------
def bn_stats_vector(y, gamma, beta, running_mean, running_var, training, momentum, eps, part=None, zexps=None,
                    rpre=None, rpost=None):
    """[mean | invstd | scale | shift] (4*C floats); updates the running stats in place when training.
    part: partial statistics the producing convolution already emitted (dca_*_forward_stats), or None.
    zexps (training only): C ints that receive the scale exponents of z = act(BN(y) + res_pre) + res_post for the packed px2
    output; rpre / rpost = (slots, nslots) of the residual tensors (their per-channel maxima enter the bound)."""
    rps, rpn = rpre if rpre is not None else (None, 0)
    rqs, rqn = rpost if rpost is not None else (None, 0)
    N, C = y.shape[0], y.shape[1]
    S = y[0, 0].numel()
    stats = torch.empty((4 * C,), device=y.device, dtype=torch.float32)
    lib = _L()
    if training:
        if part is not None:     # one self-centred partial {K, n, s, q} per (channel, workgroup) of the producing conv
            _chk(lib.dca_bn_finalize_centered(_ptr(part), part.numel() // (4 * C), _ptr(gamma), _ptr(beta),
                                              _ptr(running_mean), _ptr(running_var), float(momentum), float(eps),
                                              _ptr(stats), _ptr(zexps), _ptr(rps), rpn, _ptr(rqs), rqn, C, _stream()),
                 "dca_bn_finalize_centered")
            return stats
        nchunk = lib.dca_bn_num_chunks(C, S)
        part = torch.empty((C * nchunk * 2 + C,), device=y.device, dtype=torch.float64)   # partial sums + C shifts
        _chk(lib.dca_bn_stats(_ptr(y), _ptr(part), N, C, S, _stream()), "dca_bn_stats")
        _chk(lib.dca_bn_finalize(_ptr(part), nchunk, float(N * S), _ptr(gamma), _ptr(beta), _ptr(running_mean),
                                 _ptr(running_var), float(momentum), float(eps), 1, _ptr(stats), _ptr(zexps), _ptr(rps), rpn,
                                 _ptr(rqs), rqn, C, _stream()), "dca_bn_finalize")
    else:
        assert zexps is None
        _chk(lib.dca_bn_finalize(None, 0, float(N * S), _ptr(gamma), _ptr(beta), _ptr(running_mean),
                                 _ptr(running_var), float(momentum), float(eps), 0, _ptr(stats), None, None, 0, None, 0, C,
                                 _stream()), "dca_bn_finalize")
    return stats


def bn_eval_affine(bn):
    """[mean | invstd | scale | shift] of an eval-mode BatchNorm (running statistics), 4*C floats."""
    C = bn.num_features

    def build():
        stats = torch.empty((4 * C,), device=bn.running_mean.device, dtype=torch.float32)
        _chk(_L().dca_bn_finalize(None, 0, 1.0, _ptr(bn.weight), _ptr(bn.bias), _ptr(bn.running_mean),
                                  _ptr(bn.running_var), 0.1, float(bn.eps), 0, _ptr(stats), None, None, 0, None, 0, C, _stream()),
             "dca_bn_finalize")
        return stats
    src = tuple(t for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var) if t is not None)
    return _memo(("bnfold", float(bn.eps)), src, build)


class _BnAct(torch.autograd.Function):
    """z = act(BN(y) + res_pre) + res_post with nn.BatchNorm3d semantics.
    pack_z:  1: z is written in the packed px2 operand format (for ONE consumer: an f16x2 convolution) instead of fp32;
             2: both -- the fp32 z for all readers and a packed twin (it rides on z: _dca_twin) for the f16x2 convolution
             among them and its weight gradient.
    pack_dy: backward writes the gradient of y in the packed px2 format (y's producer is an f16x2 convolution: its
             backward-data and weight-gradient kernels are the only readers)."""

    @staticmethod
    def forward(ctx, y, gamma, beta, running_mean, running_var, training, momentum, eps, slope, res_pre, res_post,
                part=None, zmax=None, pack_z=False, pack_dy=False, lazy_dy=False):
        """zmax: per-channel slot words that receive max |z| (see _cslots); z is tagged with them here"""
        y = _req(y, "batch_norm")
        res_pre, res_post = _opt(res_pre, "res_pre"), _opt(res_post, "res_post")
        N, C = y.shape[0], y.shape[1]
        S = y[0, 0].numel()
        lib = _L()
        pack_z = int(pack_z) if (training and C % 8 == 0) else 0
        pack_dy = bool(pack_dy and res_pre is None and C % 8 == 0)
        ctx.lazy_dy = bool(lazy_dy and res_pre is None and not pack_dy)
        with torch.cuda.device_of(y):
            zexps = torch.empty((C,), device=y.device, dtype=torch.int32) if pack_z else None
            rpre = _slots_of(res_pre) if (pack_z and res_pre is not None) else None
            rpost = _slots_of(res_post) if (pack_z and res_post is not None) else None
            stats = bn_stats_vector(y, gamma, beta, running_mean, running_var, training, momentum, eps, part, zexps, rpre, rpost)
            ymax = torch.empty((C * CSLOTS,), device=y.device, dtype=torch.int32) if pack_dy else None
            z = torch.empty_like(y)
            if pack_z:
                zp = z if pack_z == 1 else torch.empty_like(y)
                _chk(lib.dca_bn_apply_pack(_ptr(y), _ptr(stats), _ptr(zexps), _ptr(zp), N, C, S, float(slope), _ptr(ymax),
                                           _ptr(res_pre), _ptr(res_post), _ptr(z) if pack_z == 2 else None,
                                           _ptr(zmax) if pack_z == 2 else None, _stream()), "dca_bn_apply_pack")
                ymax_slots = lib.dca_bn_pack_chunks(C, S)
                _tag_px2(zp, zexps)
                if pack_z == 2:
                    _tag_twin(z, zp)
            else:
                _chk(lib.dca_bn_apply(_ptr(y), _ptr(stats), _ptr(res_pre), _ptr(res_post), _ptr(z), N, C, S, float(slope),
                                      _ptr(zmax), _ptr(ymax), _stream()), "dca_bn_apply")
                ymax_slots = lib.dca_bn_num_chunks(C, S)
        ctx.save_for_backward(y, stats, res_pre if slope != 1.0 else None, ymax)
        ctx.meta = (training, slope, res_pre is not None, res_post is not None, pack_dy, ymax_slots)
        return z if pack_z == 1 else _tag_cmax(z, zmax, ymax_slots)    # max |z| sits in as many slots as max |y| would

    @staticmethod
    def backward(ctx, dz):
        y, stats, res_pre, ymax = ctx.saved_tensors
        training, slope, has_pre, has_post, pack_dy, ymax_slots = ctx.meta
        dz = _req(dz, "batch_norm.backward")
        N, C = y.shape[0], y.shape[1]
        S = y[0, 0].numel()
        lib = _L()
        with torch.cuda.device_of(y):
            nchunk = lib.dca_bn_num_chunks(C, S)
            part = torch.empty((C * nchunk * 2,), device=y.device, dtype=torch.float64)
            dgb = torch.empty((4 * C,), device=y.device, dtype=torch.float32)
            g_out = None
            if ctx.lazy_dy:
                # reduce and finalize only: the 1x1x1 convolution that produced y forms dy itself (_c1_bwd_fused) from dz,
                # which travels on as an alias of its own carrying what that launch needs
                _chk(lib.dca_bn_backward_reduce(_ptr(dz), _ptr(y), _ptr(stats), _ptr(part), _ptr(dgb), N, C, S, float(slope),
                                                int(training), _stream()), "dca_bn_backward_reduce")
                dy = dz.view_as(dz)
                dy._dca_lazy = (y, stats, dgb, slope, training)
            elif pack_dy:
                dyexps = torch.empty((C,), device=y.device, dtype=torch.int32)
                gmax = torch.empty((C * CSLOTS,), device=y.device, dtype=torch.int32)
                dy = torch.empty_like(y)
                _chk(lib.dca_bn_backward_pack(_ptr(dz), _ptr(y), _ptr(stats), _ptr(part), _ptr(dgb), _ptr(dy), _ptr(dyexps),
                                              _ptr(gmax), _ptr(ymax), ymax_slots if ymax is not None else 0, N, C, S,
                                              float(slope), int(training), _stream()), "dca_bn_backward_pack")
                _tag_px2(dy, dyexps)
            else:
                dy = torch.empty_like(y)
                want_g = has_pre and slope != 1.0 and ctx.needs_input_grad[9]
                g_out = torch.empty_like(y) if want_g else None
                dm = _cslots(C, y.device) if CONV_X2 else None     # per-channel max |dy| for the convolution's backward kernels
                _chk(lib.dca_bn_backward(_ptr(dz), _ptr(y), _ptr(res_pre), _ptr(stats), _ptr(part), _ptr(dgb), _ptr(dy),
                                         _ptr(g_out), N, C, S, float(slope), int(training), _ptr(dm), _stream()),
                     "dca_bn_backward")
                _tag_cmax(dy, dm, nchunk)
        g_pre = None
        if has_pre and ctx.needs_input_grad[9]:
            g_pre = g_out if g_out is not None else dz
        g_post = dz if (has_post and ctx.needs_input_grad[10]) else None
        return dy, dgb[:C], dgb[C:2 * C], None, None, None, None, None, None, g_pre, g_post, None, None, None, None, None


class _BnSkipAct(torch.autograd.Function):
    """z = act(BN(y) + BN_r(y_r)) + res_post, both BatchNorms over batch statistics, BN_r a plain affine (slope 1, no
    residuals) that only this node reads: the folded route of _skip_fold_route.  One apply pass writes the fp32 z and its
    packed twin (_BnAct, pack_z 2) with BN_r formed in registers (its per-channel maxima, which the twin's exponents need
    beforehand, come from a read pass over y_r: half the traffic of the apply pass it replaces); backward's reduce pass carries BN_r's sums, its apply pass
    writes dy and g, and g travels on as the lazy dz of the 1x1x1 convolution that produced y_r (as _BnAct, lazy_dy).
    Saves y, y_r and the two statistics vectors -- no tensor of the skip's shape beyond the convolution outputs themselves."""

    @staticmethod
    def forward(ctx, y, gamma, beta, running_mean, running_var, momentum, eps, part, y_r, gamma_r, beta_r, running_mean_r,
                running_var_r, momentum_r, eps_r, part_r, slope, res_post, zmax):
        y, y_r = _req(y, "batch_norm"), _req(y_r, "batch_norm.skip")
        res_post = _opt(res_post, "res_post")
        if y_r.shape != y.shape:
            raise RuntimeError("batch_norm: the skip branch does not have the output's shape")
        N, C = y.shape[0], y.shape[1]
        S = y[0, 0].numel()
        lib = _L()
        with torch.cuda.device_of(y):
            stats_r = bn_stats_vector(y_r, gamma_r, beta_r, running_mean_r, running_var_r, True, momentum_r, eps_r, part_r)
            # max |skip| per channel -- what the skip's own apply pass would have tagged it with -- from a read pass over y_r:
            # the packed twin gets the exponents of the two-node route, bit for bit
            nchunk = lib.dca_bn_num_chunks(C, S)
            rslots = torch.empty((C * CSLOTS,), device=y.device, dtype=torch.int32)
            _chk(lib.dca_bn_skip_max(_ptr(y_r), _ptr(stats_r), N, C, S, _ptr(rslots), _stream()), "dca_bn_skip_max")
            zexps = torch.empty((C,), device=y.device, dtype=torch.int32)
            rpost = _slots_of(res_post) if res_post is not None else None
            stats = bn_stats_vector(y, gamma, beta, running_mean, running_var, True, momentum, eps, part, zexps,
                                    (rslots, nchunk), rpost)
            z, zp = torch.empty_like(y), torch.empty_like(y)
            _chk(lib.dca_bn_apply_pack_skip(_ptr(y), _ptr(stats), _ptr(zexps), _ptr(zp), N, C, S, float(slope), None, _ptr(y_r),
                                            _ptr(stats_r), _ptr(res_post), _ptr(z), _ptr(zmax), _stream()),
                 "dca_bn_apply_pack_skip")
            _tag_px2(zp, zexps)
            _tag_twin(z, zp)
        ctx.save_for_backward(y, stats, y_r, stats_r)
        ctx.meta = (slope, res_post is not None)
        return _tag_cmax(z, zmax, lib.dca_bn_pack_chunks(C, S))

    @staticmethod
    def backward(ctx, dz):
        y, stats, y_r, stats_r = ctx.saved_tensors
        slope, has_post = ctx.meta
        dz = _req(dz, "batch_norm.backward")
        N, C = y.shape[0], y.shape[1]
        S = y[0, 0].numel()
        lib = _L()
        with torch.cuda.device_of(y):
            nchunk = lib.dca_bn_num_chunks(C, S)
            part, part_r = (torch.empty((C * nchunk * 2,), device=y.device, dtype=torch.float64) for _ in range(2))
            dgb, dgb_r = (torch.empty((4 * C,), device=y.device, dtype=torch.float32) for _ in range(2))
            dy, g = torch.empty_like(y), torch.empty_like(y)
            dm = _cslots(C, y.device)                       # per-channel max |dy| for the convolution's backward kernels
            _chk(lib.dca_bn_backward_skip(_ptr(dz), _ptr(y), _ptr(y_r), _ptr(stats), _ptr(stats_r), _ptr(part), _ptr(part_r),
                                          _ptr(dgb), _ptr(dgb_r), _ptr(dy), _ptr(g), N, C, S, float(slope), 1, _ptr(dm),
                                          _stream()), "dca_bn_backward_skip")
            _tag_cmax(dy, dm, nchunk)
            g._dca_lazy = (y_r, stats_r, dgb_r, 1.0, True)  # what _c1_bwd_fused reads, as _BnAct.backward hands it on
        g_post = dz if (has_post and ctx.needs_input_grad[17]) else None
        return (dy, dgb[:C], dgb[C:2 * C], None, None, None, None, None, g, dgb_r[:C], dgb_r[C:2 * C], None, None, None, None,
                None, None, g_post, None)


_tls = threading.local()


class frozen_weights:
    """Inference helper: inside this context the caller promises that parameters and BatchNorm buffers do not change, so
    the per-call weight re-layouts (dca_conv3d_prep_weight / dca_conv3d_x3_prep_weight) and folded eval-mode BatchNorm
    affines are computed once per tensor and reused (the usual weight pre-packing of inference engines; ~80 tiny launches
    = 0.5 ms of an 8.5 ms forward at 544x960).  Never active outside the context, per thread, dropped at exit; bypassed
    while a stream capture is running (a graph must contain its own prep kernels)."""

    def __enter__(self):
        self.prev = getattr(_tls, "frozen", None)
        _tls.frozen = {}
        return self

    def __exit__(self, *exc):
        _tls.frozen = self.prev
        return False


_PLAN_RECORDER = None   # PrepackPlan being recorded (process-wide, see the class)
_PLAN_ACTIVE = None     # {cache key: packed tensor} of the active PrepackPlan


class PrepackPlan:
    """Training helper: the weight re-layouts of a whole step as ONE launch (dca_conv3d_prep_many).

        plan = ops.PrepackPlan()
        with plan.recording():          # one ordinary step: notes every (parameter, layout) the step asks for
            step()
        plan.finalize()
        loop:   with plan.active(): step_forward_backward(); optimizer.step(); plan.refresh()

    `refresh()` re-packs all recorded layouts from the current parameter values; inside `active()` the convolutions pick
    the pre-packed images up instead of launching their own prep kernels.  Only layouts whose source is a leaf tensor
    that owns its storage (a parameter) are planned; anything else keeps packing per call.  The recording / active
    state is per PROCESS, not per thread: backward-data layouts are requested from the autograd engine's thread."""

    def __init__(self):
        self.entries = {}      # cache key -> (packed tensor, descriptor tuple, source tensors)
        self.table = None
        self.n = 0

    def recording(self):
        plan = self

        class _Rec:
            def __enter__(self_inner):
                global _PLAN_RECORDER
                self_inner.prev, _PLAN_RECORDER = _PLAN_RECORDER, plan

            def __exit__(self_inner, *exc):
                global _PLAN_RECORDER
                _PLAN_RECORDER = self_inner.prev
                return False
        return _Rec()

    def finalize(self):
        import struct
        rows = []
        for out, desc, tensors in self.entries.values():
            kind, A, Bn, Apad, Bpad, K, src_ab, flip, Btotal, b_off = desc
            nch = (A + 15) // 16
            rows.append(struct.pack("<QQ12iq", tensors[0].data_ptr(), out.data_ptr(), kind, A, Bn, Apad, Bpad, K, src_ab,
                                    flip, Btotal, b_off, nch, 0, out.numel()))
        self.n = len(rows)
        if self.n:
            dev = next(iter(self.entries.values()))[0].device
            self.table = torch.frombuffer(bytearray(b"".join(rows)), dtype=torch.uint8).to(dev)
        return self

    def refresh(self):
        if self.n:
            _chk(_L().dca_conv3d_prep_many(_ptr(self.table), self.n, _stream()), "dca_conv3d_prep_many")

    def active(self):
        plan = self

        class _Act:
            def __enter__(self_inner):
                global _PLAN_ACTIVE
                self_inner.prev = _PLAN_ACTIVE
                _PLAN_ACTIVE = {k: out for k, (out, _, _t) in plan.entries.items()}

            def __exit__(self_inner, *exc):
                global _PLAN_ACTIVE
                _PLAN_ACTIVE = self_inner.prev
                return False
        return _Act()


def _memo(key, tensors, build, desc=None):
    """build() once per (key, identity of `tensors`) inside a frozen_weights() / PrepackPlan.active() context; plain
    build() otherwise (a PrepackPlan being recorded also notes `desc`, the dca_conv3d_prep_many descriptor)"""
    rec = _PLAN_RECORDER
    if rec is not None:
        out = build()
        t = tensors[0] if tensors else None
        if desc is not None and t is not None and t.is_leaf and t._base is None:
            rec.entries[(key,) + tuple((id(x), x.data_ptr()) for x in tensors)] = (out, desc, tensors)
        return out
    act = _PLAN_ACTIVE
    if act is not None and desc is not None:
        hit = act.get((key,) + tuple((id(x), x.data_ptr()) for x in tensors))
        if hit is not None:
            return hit
    cache = getattr(_tls, "frozen", None)
    if cache is None or (tensors and tensors[0].is_cuda and torch.cuda.is_current_stream_capturing()):
        return build()
    k = (key,) + tuple((id(t), t.data_ptr()) for t in tensors)
    hit = cache.get(k)
    if hit is None:
        hit = cache[k] = (build(), tensors)   # keeps the source tensors alive, so ids cannot be recycled
    return hit[0]


class batched_bn_counters:
    """Inside this context the `num_batches_tracked += 1` of every train-mode BatchNorm (nn.BatchNorm3d semantics) is
    deferred and applied at exit as ONE multi-tensor add instead of ~50 one-element kernel launches per step."""

    def __enter__(self):
        self.prev = getattr(_tls, "pending", None)
        _tls.pending = []
        return self

    def __exit__(self, *exc):
        pending, _tls.pending = _tls.pending, self.prev
        if pending:
            torch._foreach_add_(pending, 1)
        return False


def bn_act(y, bn, slope=1.0, res_pre=None, res_post=None, stats_part=None, pack_out=False, pack_dy=False, lazy_dy=False):
    """Applies the nn.BatchNorm3d module `bn` (parameters/buffers only; its forward is never called).
    stats_part: batch-statistics partial sums of y from the producing convolution (`_Conv3d` with want_stats), if it made them.
    pack_out: True -- the result has ONE consumer, an f16x2 3x3x3 stride-1 convolution: write it in the packed px2 operand
    format instead of fp32; "both" -- several consumers, ONE of them such a convolution: fp32 result plus a packed twin that
    this convolution and its weight gradient pick up (training BatchNorm only; plain fp32 otherwise).  The packed forms do
    not depend on the width; at W % 4 != 0 the twin's reader gets an fp32 gradient (_pack_dy_ok) and takes the fp32 tensor
    for its weight gradient (_Conv3d.backward), the forward still reads the twin.  pack_dy: see _BnAct.
    lazy_dy: y's only producer is a 1x1x1 convolution node that was told the same (_c1_bwd_route == "fused"): backward runs
    the reduction only and hands dz on, tagged, for that node's one fused launch.  Never set by a caller that owns y."""
    momentum = 0.1 if bn.momentum is None else bn.momentum
    training = bn.training or bn.running_mean is None
    if _lp_dtype() is not None:
        raise RuntimeError("ops.reduced_precision is inference only: call the model in eval mode under torch.no_grad()")
    C = y.shape[1]
    pack_z = 0
    if pack_out and PACK and CONV_X2 and training and C % 8 == 0 and torch.is_grad_enabled():
        pack_z = 2 if pack_out == "both" else 1
    pack_dy = bool(pack_dy and PACK and CONV_X2 and res_pre is None and C % 8 == 0)
    zm = _cslots(C, y.device) if (CONV_X2 and pack_z != 1) else None    # per-channel max |z|: the next convolution's operand scales
    z = _BnAct.apply(y, bn.weight, bn.bias, bn.running_mean, bn.running_var, training, momentum, bn.eps, float(slope),
                     res_pre, res_post, stats_part if training else None, zm, pack_z, pack_dy,
                     bool(lazy_dy and res_pre is None))
    _bn_count(bn)
    return z


def _bn_count(bn):
    """the `num_batches_tracked += 1` of a train-mode BatchNorm (deferred inside batched_bn_counters)"""
    if bn.training and bn.num_batches_tracked is not None:
        pending = getattr(_tls, "pending", None)
        if pending is not None:
            pending.append(bn.num_batches_tracked)
        else:
            bn.num_batches_tracked.add_(1)


def bn_skip_act(y, bn, slope, skip, res_post=None, stats_part=None):
    """act(BN(y) + BN_r(y_r)) + res_post for a `_SkipBn` record `skip` (the folded route, decided in convbn3d_pair): fp32
    result with its packed twin, as bn_act(..., res_pre=<the applied skip>, pack_out="both") gives; both modules' running
    statistics and counters move as on the two-node route."""
    if skip.into is not bn:
        raise RuntimeError("bn_skip_act: this skip branch was folded for another BatchNorm (convbn3d_pair, skip_into)")
    br = skip.bn
    mom = lambda b: 0.1 if b.momentum is None else b.momentum
    zm = _cslots(y.shape[1], y.device)
    z = _BnSkipAct.apply(y, bn.weight, bn.bias, bn.running_mean, bn.running_var, mom(bn), bn.eps, stats_part, skip.y,
                         br.weight, br.bias, br.running_mean, br.running_var, mom(br), br.eps, skip.part, float(slope),
                         res_post, zm)
    _bn_count(br)
    _bn_count(bn)
    return z


class reduced_precision:
    """Inference-only context (BASELINE configs 2 "bf16" / 5 "fp16"): inside it the fused conv + BatchNorm inference
    launches of the 3x3x3 stride-1 convolutions use `dtype` (torch.bfloat16 / torch.float16) operands with ONE native
    MFMA product per multiply and fp32 accumulation (csrc/conv3d_lp.hip) instead of the fp32-grade six-product split.
    Softmax, soft-argmin, BatchNorm folding, the context injection's arg-max / region softmax and the 32 -> 1 logit
    heads stay fp32.  Per thread; never active outside the context; training (autograd) raises."""

    def __init__(self, dtype):
        if dtype not in LP_DTYPES:
            raise ValueError("reduced_precision: torch.bfloat16 or torch.float16")
        self.dtype = dtype

    def __enter__(self):
        self.prev = getattr(_tls, "lp", None)
        _tls.lp = self.dtype
        return self

    def __exit__(self, *exc):
        _tls.lp = self.prev
        return False


def _lp_dtype():
    return getattr(_tls, "lp", None)


def _pack_dy_ok(x, x2, conv, transposed, stride, res_pre):
    """may the gradient of this convolution's output travel as a packed px2 operand?  (its only readers are then the f16x2
    backward-data and weight-gradient kernels of this very convolution)"""
    if not (PACK and res_pre is None and _k3s1(conv.weight, stride, transposed, x2)):
        return False
    Cout, Cin = conv.weight.shape[0], conv.weight.shape[1]
    if Cout % 8 or _conv_family(x, None, Cin, Cout, 3, 1, False) != "x2":
        return False
    return _x2_pairs(_is_packed(x), True, x.shape[-1]) and (_is_packed(x) or x.data_ptr() % 16 == 0)


def convbn3d(x, conv, bn, slope=1.0, res_pre=None, res_post=None, x2=None, alias=False, pack_out=False):
    """`convbn_3d` (models/submodule.py:121-124) + activation + residual adds, on the HIP kernels.

    conv: nn.Conv3d / nn.ConvTranspose3d (bias=False), bn: nn.BatchNorm3d -- used as parameter holders.
    Inference (eval BN, no grad): one fused launch (BN folded into the conv epilogue).  Otherwise conv ->
    batch statistics -> apply, each with a HIP backward.
    pack_out: the caller promises that the result has ONE consumer and that it is a 3x3x3 stride-1 convolution through this
    function: in training the BatchNorm apply pass then writes the packed px2 operand format (csrc/dca_common.h) instead
    of fp32 (never with residuals); "both": fp32 plus a packed twin for the one such convolution among several consumers
    (bn_act; residuals allowed).  Silently fp32
    wherever the packed form does not apply: eval / no-grad, channel counts that are not multiples of 8, DCA_PACK=0 or
    another kernel family.  Any width works: an operand that cannot be paired in the f16x2 weight-gradient kernel (an fp32
    tensor or gradient at W % 4 != 0 beside a packed one) is read as fp32 by the kernel that serves that width."""
    transposed = isinstance(conv, torch.nn.ConvTranspose3d)
    stride = conv.stride[0]
    if isinstance(res_pre, _SkipBn):
        # the folded route (training under grad, fp32: _skip_fold_route); the caller promised pack_out="both"
        if pack_out != "both" or alias:
            raise RuntimeError("convbn3d: a folded skip branch needs pack_out='both' (convbn3d_pair, skip_into)")
        if BN_FUSE and conv.weight.shape[0 if not transposed else 1] > 1:
            y, part = _Conv3d.apply(x, x2, conv.weight, int(stride), bool(transposed), True)
        else:
            y, part = conv3d(x, conv.weight, stride, transposed, x2), None
        return bn_skip_act(y, bn, slope, res_pre, res_post, part if (part is not None and part.numel()) else None)
    if alias:
        # alias=True: returns (z, x') with x' = x for the other consumers of x (see _Conv3d.forward); plain (z, x) where the
        # fused form does not apply
        fuse = (PAIR_FUSE and torch.is_grad_enabled() and x.requires_grad and _k3s1(conv.weight, stride, transposed, x2)
                and _lp_dtype() is None and x.dtype == torch.float32)
        if not fuse:
            return convbn3d(x, conv, bn, slope, res_pre, res_post, x2), x
        stats = bool(BN_FUSE and bn.training)
        pdy = _pack_dy_ok(x, None, conv, False, 1, res_pre)
        out = _Conv3d.apply(x, None, conv.weight, 1, False, stats, True, pdy)
        y, part, xa = (out[0], out[1], out[2]) if stats else (out[0], None, out[1])
        z = bn_act(y, bn, slope, res_pre, res_post, part if (part is not None and part.numel()) else None,
                   pack_out=pack_out, pack_dy=pdy)
        return z, xa
    if not bn.training and not torch.is_grad_enabled():
        lp = _lp_dtype()
        if lp is not None and not transposed and stride == 1 and conv.kernel_size[0] == 3 and x2 is None:
            with torch.cuda.device_of(x):
                stats = bn_eval_affine(bn)
            C = bn.num_features
            return conv3d_lp(x, conv.weight, lp, stats[2 * C:3 * C], stats[3 * C:], slope, res_pre, res_post,
                             out_dtype=x.dtype)
        xx = _req(x, "convbn3d")
        with torch.cuda.device_of(xx):
            stats = bn_eval_affine(bn)
        C = bn.num_features
        return conv3d_fused_inference(xx, conv.weight, stride, transposed, stats[2 * C:3 * C], stats[3 * C:], slope,
                                      res_pre, res_post, x2)
    if BN_FUSE and bn.training and conv.weight.shape[0 if not transposed else 1] > 1 and _lp_dtype() is None:
        # the convolution kernel emits the batch statistics of its own output where it has such a form (the bf16x3 family):
        # no separate pass over y
        pdy = _pack_dy_ok(x, x2, conv, transposed, stride, res_pre)
        lazy = not transposed and _c1_bwd_route(x, x2, conv.weight, res_pre) == "fused"
        y, part = _Conv3d.apply(x, x2, conv.weight, int(stride), bool(transposed), True, False, pdy, lazy)
        return bn_act(y, bn, slope, res_pre, res_post, part if part.numel() else None, pack_out=pack_out, pack_dy=pdy,
                      lazy_dy=lazy)
    if not transposed and _lp_dtype() is None and _c1_bwd_route(x, x2, conv.weight, res_pre) == "fused":
        y = _Conv3d.apply(x, x2, conv.weight, int(stride), False, False, False, False, True)   # eval-mode BatchNorm under grad
        return bn_act(y, bn, slope, res_pre, res_post, lazy_dy=True)
    if _is_packed(x) and _pack_dy_ok(x, x2, conv, transposed, stride, res_pre):
        # DCA_BN_FUSE=0: the alias node before this layer packs its output all the same, and a packed x pairs only with a
        # packed gradient in the weight-gradient kernel at W % 4 != 0 (_x2_pairs): hand it one, as the branch above does
        y = _Conv3d.apply(x, x2, conv.weight, int(stride), bool(transposed), False, False, True)
        return bn_act(y, bn, slope, res_pre, res_post, pack_dy=True)
    y = conv3d(x, conv.weight, stride, transposed, x2)
    return bn_act(y, bn, slope, res_pre, res_post)


# ------------------------------------------------------------------------------------------------
# pooling / interpolation
# ------------------------------------------------------------------------------------------------
class _AvgPool3d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = _req(x, "avg_pool3d")
        N, C, D, H, W = x.shape
        y = torch.empty((N, C, (D + 1) // 2, (H + 1) // 2, (W + 1) // 2), device=x.device, dtype=torch.float32)
        with torch.cuda.device_of(x):
            _chk(_L().dca_avgpool3d_fwd(_ptr(x), _ptr(y), N * C, D, H, W, _stream()), "dca_avgpool3d_fwd")
        ctx.shape = tuple(x.shape)
        return y

    @staticmethod
    def backward(ctx, gy):
        gy = _req(gy, "avg_pool3d.backward")
        N, C, D, H, W = ctx.shape
        gx = torch.empty(ctx.shape, device=gy.device, dtype=torch.float32)
        with torch.cuda.device_of(gy):
            _chk(_L().dca_avgpool3d_bwd(_ptr(gy), _ptr(gx), None, None, N * C, D, H, W, _stream()), "dca_avgpool3d_bwd")
        return gx


class _PoolFork(torch.autograd.Function):
    """(AvgPool3d(3, 2, 1)(x), x) as ONE autograd node: the second output is x itself, for a second consumer (a cva block
    pools its input AND feeds it to the `fuse` convolution, models/augment/cva.py:62-69).  Backward adds that consumer's
    gradient inside the pooling backward kernel (`res`) instead of leaving the sum to autograd's accumulation pass."""

    @staticmethod
    def forward(ctx, x, third):
        x = _req(x, "avg_pool3d")
        N, C, D, H, W = x.shape
        y = torch.empty((N, C, (D + 1) // 2, (H + 1) // 2, (W + 1) // 2), device=x.device, dtype=torch.float32)
        with torch.cuda.device_of(x):
            _chk(_L().dca_avgpool3d_fwd(_ptr(x), _ptr(y), N * C, D, H, W, _stream()), "dca_avgpool3d_fwd")
        ctx.shape = tuple(x.shape)
        ctx.set_materialize_grads(False)
        if third:       # a third consumer of x (the block's `cost0 + augmented_cost`): its gradient joins inside the same kernel
            return y, x.view_as(x), x.view_as(x)
        return y, x.view_as(x)

    @staticmethod
    def backward(ctx, gy, gx2, gx3=None):
        extra = [g for g in (gx2, gx3) if g is not None]
        if gy is None:
            return (extra[0] + extra[1] if len(extra) == 2 else (extra[0] if extra else None)), None
        gy = _req(gy, "avg_pool3d.backward")
        res = _opt(extra[0], "avg_pool3d.backward") if extra else None
        res2 = _opt(extra[1], "avg_pool3d.backward") if len(extra) == 2 else None
        N, C, D, H, W = ctx.shape
        gx = torch.empty(ctx.shape, device=gy.device, dtype=torch.float32)
        with torch.cuda.device_of(gy):
            _chk(_L().dca_avgpool3d_bwd(_ptr(gy), _ptr(gx), _ptr(res), _ptr(res2), N * C, D, H, W, _stream()),
                 "dca_avgpool3d_bwd")
        return gx, None


def avg_pool3d_fork(x, third=False):
    """(avg_pool3d_k3s2p1(x), x'[, x'']) with x' = x'' = x for further consumers whose gradients are added inside the pooling
    backward kernel (training path; plain pooling and x itself otherwise)"""
    if PAIR_FUSE and torch.is_grad_enabled() and x.requires_grad and x.dtype == torch.float32:
        outs = _PoolFork.apply(x, bool(third))
        for o in outs[1:]:
            _copy_tags(x, o)        # the aliases are x: its per-channel maxima / packed twin stay valid (residual bounds)
        return outs
    return (avg_pool3d_k3s2p1(x), x, x) if third else (avg_pool3d_k3s2p1(x), x)


class _Trilinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, scale):
        x = _req(x, "interpolate")
        N, C, D, H, W = x.shape
        y = torch.empty((N, C, D * scale, H * scale, W * scale), device=x.device, dtype=torch.float32)
        with torch.cuda.device_of(x):
            _chk(_L().dca_trilinear_fwd(_ptr(x), _ptr(y), N * C, D, H, W, scale, _stream()), "dca_trilinear_fwd")
        ctx.meta = (tuple(x.shape), scale)
        return y

    @staticmethod
    def backward(ctx, gy):
        shape, scale = ctx.meta
        gy = _req(gy, "interpolate.backward")
        N, C, D, H, W = shape
        gx = torch.empty(shape, device=gy.device, dtype=torch.float32)
        with torch.cuda.device_of(gy):
            _chk(_L().dca_trilinear_bwd(_ptr(gy), _ptr(gx), N * C, D, H, W, scale, _stream()), "dca_trilinear_bwd")
        return gx, None


def avg_pool3d_k3s2p1(x):
    return _AvgPool3d.apply(x)


def trilinear_upsample(x, scale):
    return _Trilinear.apply(x, int(scale))


# ------------------------------------------------------------------------------------------------
# DCA: context injection and disparity attention
# ------------------------------------------------------------------------------------------------
class _ContextInject(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, preds):
        x, preds = _req(x, "context_inject"), _req(preds, "context_inject.preds")
        B, C, n = x.shape[:3]
        HW = x.shape[3] * x.shape[4]
        key = torch.empty_like(x)
        kstar = torch.empty((B, HW), device=x.device, dtype=torch.int32)
        e = torch.empty((B, HW), device=x.device, dtype=torch.float32)
        pm = torch.empty_like(e)
        denom = torch.empty((B, n), device=x.device, dtype=torch.float32)
        part = torch.empty((B * ((HW + 255) // 256) * n,), device=x.device, dtype=torch.float32)
        with torch.cuda.device_of(x):
            _chk(_L().dca_context_inject_fwd(_ptr(x), _ptr(preds), _ptr(key), _ptr(kstar), _ptr(e), _ptr(pm),
                                             _ptr(denom), _ptr(part), B, C, n, HW, _stream()), "dca_context_inject_fwd")
        ctx.save_for_backward(x, preds, kstar, e, pm, denom)
        ctx.mark_non_differentiable(kstar)
        return key, kstar

    @staticmethod
    def backward(ctx, dkey, _unused):
        x, preds, kstar, e, pm, denom = ctx.saved_tensors
        dkey = _req(dkey, "context_inject.backward")
        B, C, n = x.shape[:3]
        HW = x.shape[3] * x.shape[4]
        dx, dpreds = torch.empty_like(x), torch.empty_like(preds)
        dw = torch.empty_like(e)
        T = torch.empty_like(denom)
        part = torch.empty((B * ((HW + 255) // 256) * n,), device=x.device, dtype=torch.float32)
        with torch.cuda.device_of(x):
            _chk(_L().dca_context_inject_bwd(_ptr(dkey), _ptr(x), _ptr(preds), _ptr(kstar), _ptr(e), _ptr(pm),
                                             _ptr(denom), _ptr(dx), _ptr(dpreds), _ptr(dw), _ptr(T), _ptr(part), B, C,
                                             n, HW, _stream()), "dca_context_inject_bwd")
        return dx, dpreds


class _DispAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v):
        q, k, v = _req(q, "attention.q"), _req(k, "attention.k"), _req(v, "attention.v")
        B, C, n = q.shape[:3]
        HW = q.shape[3] * q.shape[4]
        out = torch.empty_like(q)
        with torch.cuda.device_of(q):
            _chk(_L().dca_disp_attention_fwd(_ptr(q), _ptr(k), _ptr(v), _ptr(out), B, C, n, HW, _stream()),
                 "dca_disp_attention_fwd")
        ctx.save_for_backward(q, k, v)
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v = ctx.saved_tensors
        dout = _req(dout, "attention.backward")
        B, C, n = q.shape[:3]
        HW = q.shape[3] * q.shape[4]
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        with torch.cuda.device_of(q):
            _chk(_L().dca_disp_attention_bwd(_ptr(q), _ptr(k), _ptr(v), _ptr(dout), _ptr(dq), _ptr(dk), _ptr(dv), B,
                                             C, n, HW, _stream()), "dca_disp_attention_bwd")
        return dq, dk, dv


def context_inject(x, preds):
    """SemanticLevelContext's feats_sl + inputs (semantic_level.py:96-126); returns (key_feats, kstar)."""
    return _ContextInject.apply(x, preds)


def disparity_attention(q, k, v):
    """softmax(q k^T / sqrt(8)) v along the disparity axis of every pixel, heads of 8 channels
    (SelfAttention_bn.py:70-94).  Limits of the kernels: channels % 8 == 0 and at most 64 disparity bins."""
    if q.dim() != 5 or q.shape[1] % 8 or q.shape[2] > 64:
        raise RuntimeError(f"disparity_attention: needs (B, C % 8 == 0, n <= 64, H, W) tensors, got {tuple(q.shape)} "
                           "(n = maxdisp/8 with the down-sampling cva, maxdisp/4 without)")
    return _DispAttention.apply(q, k, v)


# ------------------------------------------------------------------------------------------------
# convex x4 up-sampling and the stereo focal loss (csrc/heads2d.hip)
# ------------------------------------------------------------------------------------------------
class _ConvexUp4(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mask_logits, disp):
        mask_logits, disp = _req(mask_logits, "convex_upsample4.mask"), _req(disp, "convex_upsample4.disp")
        B, C, h, w = mask_logits.shape
        if C != 144 or tuple(disp.shape) != (B, 1, h, w):
            raise RuntimeError(f"convex_upsample4: expected mask (B,144,h,w) and disp (B,1,h,w), got "
                               f"{tuple(mask_logits.shape)} and {tuple(disp.shape)}")
        up = torch.empty((B, 1, 4 * h, 4 * w), device=disp.device, dtype=torch.float32)
        with torch.cuda.device_of(disp):
            _chk(_L().dca_convex_up4_fwd(_ptr(mask_logits), _ptr(disp), _ptr(up), B, h, w, _stream()),
                 "dca_convex_up4_fwd")
        ctx.save_for_backward(mask_logits, disp)
        return up

    @staticmethod
    def backward(ctx, gup):
        mask_logits, disp = ctx.saved_tensors
        gup = _req(gup, "convex_upsample4.backward")
        B, _, h, w = mask_logits.shape
        gl, gd = torch.empty_like(mask_logits), torch.empty_like(disp)
        wk = torch.empty((B, 9, h, w), device=disp.device, dtype=torch.float32)
        with torch.cuda.device_of(disp):
            _chk(_L().dca_convex_up4_bwd(_ptr(mask_logits), _ptr(disp), _ptr(gup), _ptr(gl), _ptr(gd), _ptr(wk), B, h, w,
                                         _stream()), "dca_convex_up4_bwd")
        return gl, gd


def convex_upsample4(mask_logits, disp):
    """PropgationNet_4x.forward after its conv (models/submodule.py:366-373): (B,144,h,w), (B,1,h,w) -> (B,1,4h,4w)."""
    return _ConvexUp4.apply(mask_logits, disp)


CONF_MAX_PLANES = _C["DCA_CONF_MAX_PLANES"]


def convex_upsample4_planes(mask_logits, planes, scales):
    """`convex_upsample4` for P = 1..8 planes through one read of the mask: (B,144,h,w), (B,P,h,w), P floats ->
    (B,P,4h,4w), plane p = convex combination of scales[p] * planes[:, p] over the 3x3 neighbourhood.  A plane with scale 4
    is bitwise `convex_upsample4` of that plane.  Neighbours outside the map are 0 for every plane, so any plane falls
    towards 0 in the cells along the frame border, as the disparity does.  Inference only."""
    _req_no_grad("convex_upsample4_planes", mask_logits, planes)
    mask_logits, planes = _req(mask_logits, "convex_upsample4_planes.mask"), _req(planes, "convex_upsample4_planes.planes")
    scales = [float(v) for v in scales]
    if mask_logits.dim() != 4 or planes.dim() != 4:
        raise RuntimeError(f"convex_upsample4_planes: expected mask (B,144,h,w) and planes (B,P,h,w), got "
                           f"{tuple(mask_logits.shape)} and {tuple(planes.shape)}")
    B, C, h, w = mask_logits.shape
    P = planes.shape[1]
    if C != 144 or tuple(planes.shape) != (B, P, h, w) or not 1 <= P <= CONF_MAX_PLANES or len(scales) != P \
            or planes.numel() == 0:
        raise RuntimeError(f"convex_upsample4_planes: expected mask (B,144,h,w), planes (B,P,h,w) with 1 <= P <= "
                           f"{CONF_MAX_PLANES} and P scales, got {tuple(mask_logits.shape)}, {tuple(planes.shape)} and "
                           f"{len(scales)} scales")
    up = torch.empty((B, P, 4 * h, 4 * w), device=planes.device, dtype=torch.float32)
    sc = (ctypes.c_float * P)(*scales)       # host array, copied into the launch's arguments
    with torch.cuda.device_of(planes):
        _chk(_L().dca_convex_up4_planes(_ptr(mask_logits), _ptr(planes), ctypes.cast(sc, _vp), _ptr(up), B, P, h, w,
                                        _stream()), "dca_convex_up4_planes")
    return up


class _FocalLevels(torch.autograd.Function):
    """sum_l w_l * StereoFocalLoss.loss_per_level(est_l, gt) for estimates of ONE resolution; `gt` is already pooled."""

    @staticmethod
    def forward(ctx, gt, coef, weights, *ests):
        ests = [_req(e, "focal_loss.est") for e in ests]
        gt = _req(gt, "focal_loss.gt")
        B, K = ests[0].shape[0], ests[0].shape[1]
        HW = ests[0][0, 0].numel()
        n = len(ests)
        if n > 8 or K > 256 or K < 2 or any(e.shape != ests[0].shape for e in ests) or gt.numel() != B * HW:
            raise RuntimeError("focal_loss: at most 8 equally shaped (B,K<=256,H,W) estimates per call and a ground truth "
                               "pooled to (B,1,H,W)")
        lib = _L()
        work = torch.empty((lib.dca_focal_loss_workspace(n, B, HW),), device=gt.device, dtype=torch.float64)
        out = torch.empty((n + 1,), device=gt.device, dtype=torch.float32)
        eptr = (ctypes.c_void_p * n)(*[e.data_ptr() for e in ests])
        wts = (ctypes.c_float * n)(*[float(w) for w in weights])
        with torch.cuda.device_of(gt):
            _chk(lib.dca_focal_loss_fwd(eptr, wts, n, _ptr(gt), _ptr(work), _ptr(out), B, K, HW, float(coef), _stream()),
                 "dca_focal_loss_fwd")
        ctx.save_for_backward(gt, work, *ests)
        ctx.meta = (float(coef), [float(w) for w in weights])
        return out[n]

    @staticmethod
    def backward(ctx, gloss):
        gt, work, *ests = ctx.saved_tensors
        coef, weights = ctx.meta
        n = len(ests)
        B, K = ests[0].shape[0], ests[0].shape[1]
        HW = ests[0][0, 0].numel()
        gloss = _req(gloss.reshape(1), "focal_loss.backward")
        gests = [torch.empty_like(e) for e in ests]
        eptr = (ctypes.c_void_p * n)(*[e.data_ptr() for e in ests])
        gptr = (ctypes.c_void_p * n)(*[g.data_ptr() for g in gests])
        wts = (ctypes.c_float * n)(*weights)
        with torch.cuda.device_of(gt):
            _chk(_L().dca_focal_loss_bwd(eptr, gptr, wts, n, _ptr(gt), _ptr(work), _ptr(gloss), B, K, HW, coef, _stream()),
                 "dca_focal_loss_bwd")
        return (None, None, None) + tuple(gests)


def focal_loss_levels(ests, gt_pooled, weights, focal_coefficient):
    """Weighted stereo focal loss (models/loss.py:206-240) of several estimates that share one resolution."""
    return _FocalLevels.apply(gt_pooled, float(focal_coefficient), tuple(float(w) for w in weights), *ests)


# ------------------------------------------------------------------------------------------------
# Reduced-precision inference (BASELINE configs 2 / 5): bf16 or fp16 storage, one MFMA product, fp32 accumulation
# ------------------------------------------------------------------------------------------------
LP_DTYPES = {torch.bfloat16: _C["DCA_BF16"], torch.float16: _C["DCA_FP16"]}


def _req_lp(t, name, lp):
    """contiguous ROCm tensor that is either fp32 or the 2-byte type `lp`"""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name}: the DCANet hot path runs only as HIP kernels on a ROCm device; there is no CPU fallback")
    if t.dtype not in (torch.float32, lp):
        raise RuntimeError(f"{name}: expected float32 or {lp}, got {t.dtype}")
    t = t.contiguous()
    if t.data_ptr() % 16:
        t = t.clone(memory_format=torch.contiguous_format)
    return t


def conv3d_lp(x, weight, lp, scale=None, shift=None, slope=1.0, res_pre=None, res_post=None, out_dtype=None,
              src_ab=0, flip=0):
    """3x3x3 stride-1 convolution with `lp` (torch.bfloat16 / torch.float16) operands and fp32 accumulation; the folded
    BatchNorm affine, activation and residual adds run in fp32 in the epilogue.  x may be fp32 (rounded on the fly) or
    `lp`; the result (and the residuals) are `out_dtype` = `lp` (default) or fp32.  Forward only."""
    code = LP_DTYPES[lp]
    out_dtype = lp if out_dtype is None else out_dtype
    x = _req_lp(x, "conv3d_lp", lp)
    weight = _req(weight, "conv3d_lp.weight")
    if torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad):
        raise RuntimeError("conv3d_lp: the reduced-precision path is inference only (wrap the call in torch.no_grad())")
    N, Cin, D, H, W = x.shape
    Cout = weight.shape[1] if src_ab else weight.shape[0]
    assert (weight.shape[0] if src_ab else weight.shape[1]) == Cin and tuple(weight.shape[2:]) == (3, 3, 3)
    lib = _L()
    for r in (res_pre, res_post):
        if r is not None and (r.dtype != out_dtype or tuple(r.shape) != (N, Cout, D, H, W)):
            raise RuntimeError("conv3d_lp: residuals must have the output's shape and dtype")
    res_pre = None if res_pre is None else _req_lp(res_pre, "conv3d_lp.res_pre", lp)
    res_post = None if res_post is None else _req_lp(res_post, "conv3d_lp.res_post", lp)
    with torch.cuda.device_of(x):
        def build():
            wx = torch.empty((lib.dca_conv3d_lp_weight_bytes(Cin, Cout) // 2,), device=x.device, dtype=torch.int16)
            _chk(lib.dca_conv3d_lp_prep_weight(_ptr(weight), _ptr(wx), Cin, Cout, int(src_ab), int(flip), code, _stream()),
                 "dca_conv3d_lp_prep_weight")
            return wx
        wx = _memo(("lpprep", Cin, Cout, int(src_ab), int(flip), code), (weight,), build)
        y = torch.empty((N, Cout, D, H, W), device=x.device, dtype=out_dtype)
        _chk(lib.dca_conv3d_lp_forward(_ptr(x), _ptr(wx), _ptr(y), _ptr(_opt(scale, "scale")), _ptr(_opt(shift, "shift")),
                                       _ptr(res_pre), _ptr(res_post), float(slope), N, Cin, Cout, D, H, W, code,
                                       int(x.dtype == torch.float32), int(out_dtype == torch.float32), _stream()),
             "dca_conv3d_lp_forward")
    return y


def conv1x1_lp(x, weight, lp, x2=None, scale=None, shift=None, slope=1.0, res_pre=None, res_post=None, out_dtype=None):
    """1x1x1 convolution (Cout <= 32) over one or two `lp` inputs (implicit channel concat), fp32 accumulation, fused
    affine + activation + residual epilogue; result `lp` (default) or fp32.  weight: (Cout, C1 + C2[,1,1,1]) fp32."""
    code = LP_DTYPES[lp]
    out_dtype = lp if out_dtype is None else out_dtype
    x = _req_lp(x, "conv1x1_lp", lp)
    x2 = None if x2 is None else _req_lp(x2, "conv1x1_lp.x2", lp)
    if x.dtype != lp or (x2 is not None and x2.dtype != lp):
        raise RuntimeError(f"conv1x1_lp: inputs must be {lp}")
    weight = _req(weight, "conv1x1_lp.weight")
    N, C1 = x.shape[0], x.shape[1]
    C2 = 0 if x2 is None else x2.shape[1]
    Cout = weight.shape[0]
    S = x[0, 0].numel()
    assert weight[0].numel() == C1 + C2, "conv1x1_lp: channel mismatch"
    if Cout > 32 or S % 4:
        raise RuntimeError("conv1x1_lp: at most 32 output channels and a voxel count divisible by 4")
    lib = _L()
    oshape = (N, Cout) + tuple(x.shape[2:])
    for r in (res_pre, res_post):
        if r is not None and (r.dtype != out_dtype or tuple(r.shape) != oshape):
            raise RuntimeError("conv1x1_lp: residuals must have the output's shape and dtype")
    res_pre = None if res_pre is None else _req_lp(res_pre, "conv1x1_lp.res_pre", lp)
    res_post = None if res_post is None else _req_lp(res_post, "conv1x1_lp.res_post", lp)
    with torch.cuda.device_of(x):
        def build():
            wf = torch.empty((lib.dca_conv1_lp_weight_bytes(C1, C2) // 2,), device=x.device, dtype=torch.int16)
            _chk(lib.dca_conv1_lp_prep_weight(_ptr(weight), _ptr(wf), Cout, C1, C2, code, _stream()),
                 "dca_conv1_lp_prep_weight")
            return wf
        wf = _memo(("lp1prep", Cout, C1, C2, code), (weight,), build)
        y = torch.empty(oshape, device=x.device, dtype=out_dtype)
        _chk(lib.dca_conv1_lp_forward(_ptr(x), _ptr(x2), _ptr(wf), _ptr(y), _ptr(_opt(scale, "scale")),
                                      _ptr(_opt(shift, "shift")), _ptr(res_pre), _ptr(res_post), float(slope), N, C1, C2,
                                      Cout, S, code, int(out_dtype == torch.float32), _stream()), "dca_conv1_lp_forward")
    return y


def _lp_code(t):
    return LP_DTYPES[t.dtype]


def avg_pool3d_lp(x):
    """AvgPool3d(3, 2, 1) of a 2-byte (N,C,D,H,W) tensor -> fp32 (the 1/8-resolution interior of a DCA block is fp32)."""
    x = _req_lp(x, "avg_pool3d_lp", x.dtype)
    N, C, D, H, W = x.shape
    y = torch.empty((N, C, (D + 1) // 2, (H + 1) // 2, (W + 1) // 2), device=x.device, dtype=torch.float32)
    with torch.cuda.device_of(x):
        _chk(_L().dca_avgpool3d_lp_fwd(_ptr(x), _ptr(y), N * C, D, H, W, _lp_code(x), _stream()), "dca_avgpool3d_lp_fwd")
    return y


def trilinear_up2_lp(x, lp):
    """x2 trilinear up-sampling of an fp32 tensor, written in the 2-byte type `lp`."""
    x = _req(x, "trilinear_up2_lp")
    N, C, D, H, W = x.shape
    y = torch.empty((N, C, 2 * D, 2 * H, 2 * W), device=x.device, dtype=lp)
    with torch.cuda.device_of(x):
        _chk(_L().dca_trilinear_up2_lp_fwd(_ptr(x), _ptr(y), N * C, D, H, W, LP_DTYPES[lp], _stream()),
             "dca_trilinear_up2_lp_fwd")
    return y


def conv3d_s2_lp(x, weight, scale, shift, slope, exact=False):
    """3x3x3 stride-2 conv + folded BN + activation reading a 2-byte x, fp32 result.  Default: weights rounded to x's
    type, one MFMA product (csrc/conv3d_s2_lp.hip); exact=True keeps the fp32 MFMA arithmetic (csrc/conv3d_mfma.hip)."""
    x = _req_lp(x, "conv3d_s2_lp", x.dtype)
    weight = _req(weight, "conv3d_s2_lp.weight")
    N, Cin, D, H, W = x.shape
    Cout = weight.shape[0]
    Do, Ho, Wo = (D + 1) // 2, (H + 1) // 2, (W + 1) // 2
    lib = _L()
    code = _lp_code(x)
    with torch.cuda.device_of(x):
        y = torch.empty((N, Cout, Do, Ho, Wo), device=x.device, dtype=torch.float32)
        if exact:
            wt, Apad = _prep_weight(weight, Cin, Cout, 27, 0, 0, 3, 2, False)
            _chk(lib.dca_conv3d_forward_mixed(_ptr(x), _ptr(wt), _ptr(y), _ptr(scale), _ptr(shift), None, None,
                                              float(slope), N, Cin, Cout, Apad, D, H, W, Do, Ho, Wo, 0, code, _stream()),
                 "dca_conv3d_forward_mixed")
            return y

        def build():
            wx = torch.empty((lib.dca_conv3d_s2_lp_weight_bytes(Cin) // 2,), device=x.device, dtype=torch.int16)
            _chk(lib.dca_conv3d_s2_lp_prep_weight(_ptr(weight), _ptr(wx), Cin, Cout, code, _stream()),
                 "dca_conv3d_s2_lp_prep_weight")
            return wx
        wx = _memo(("lps2", Cin, Cout, code), (weight,), build)
        _chk(lib.dca_conv3d_s2_lp_forward(_ptr(x), _ptr(wx), _ptr(y), _ptr(_opt(scale, "scale")), _ptr(_opt(shift, "shift")),
                                          float(slope), N, Cin, Cout, D, H, W, code, _stream()), "dca_conv3d_s2_lp_forward")
    return y


def deconv3d_lp(x, weight, lp, scale, shift, slope, res_pre=None, res_post=None, exact=False):
    """ConvTranspose3d(3, s2, p1, op1) + folded BN + residuals + activation: fp32 x -> 2-byte result / residuals.
    Default: operands rounded to `lp`, one MFMA product (csrc/deconv3d_lp.hip); exact=True keeps the fp32 MFMA
    arithmetic and only writes / reads the 2-byte tensors (csrc/conv3d_mfma.hip)."""
    x = _req(x, "deconv3d_lp")
    weight = _req(weight, "deconv3d_lp.weight")
    N, Cin, D, H, W = x.shape
    Cout = weight.shape[1]
    oshape = (N, Cout, 2 * D, 2 * H, 2 * W)
    for r in (res_pre, res_post):
        if r is not None and (r.dtype != lp or tuple(r.shape) != oshape):
            raise RuntimeError("deconv3d_lp: residuals must have the output's shape and dtype")
    res_pre = None if res_pre is None else _req_lp(res_pre, "deconv3d_lp.res_pre", lp)
    res_post = None if res_post is None else _req_lp(res_post, "deconv3d_lp.res_post", lp)
    lib = _L()
    code = LP_DTYPES[lp]
    with torch.cuda.device_of(x):
        y = torch.empty(oshape, device=x.device, dtype=lp)
        if exact or Cin > 64 or Cout > 32:
            wt, Apad = _prep_weight(weight, Cin, Cout, 27, 1, 0, 3, 2, True)
            _chk(lib.dca_conv3d_forward_mixed(_ptr(x), _ptr(wt), _ptr(y), _ptr(scale), _ptr(shift), _ptr(res_pre),
                                              _ptr(res_post), float(slope), N, Cin, Cout, Apad, D, H, W, 2 * D, 2 * H, 2 * W,
                                              1, code, _stream()), "dca_conv3d_forward_mixed")
            return y

        def build():
            wx = torch.empty((lib.dca_conv3d_lp_weight_bytes(Cin, Cout) // 2,), device=x.device, dtype=torch.int16)
            _chk(lib.dca_conv3d_lp_prep_weight(_ptr(weight), _ptr(wx), Cin, Cout, 1, 0, code, _stream()),
                 "dca_conv3d_lp_prep_weight")
            return wx
        wx = _memo(("lpdeconv", Cin, Cout, code), (weight,), build)
        _chk(lib.dca_deconv3d_lp_forward(_ptr(x), _ptr(wx), _ptr(y), _ptr(_opt(scale, "scale")), _ptr(_opt(shift, "shift")),
                                         _ptr(res_pre), _ptr(res_post), float(slope), N, Cin, Cout, D, H, W, code, _stream()),
             "dca_deconv3d_lp_forward")
    return y


def conv3d_c1_lp(x, weight):
    """nn.Conv3d(C, 1, 3, padding=1, bias=False) logit head on a 2-byte x: the 27 taps become the output axis of the
    reduced-precision 1x1x1 GEMM (fp32 accumulation, fp32 tap tensor), then the fp32 27-tap shifted gather."""
    lp = x.dtype
    weight = _req(weight, "conv3d_c1_lp.weight")
    N, C, D, H, W = x.shape
    w27 = _memo(("c1lp",), (weight,), lambda: weight[0].reshape(C, 27).t().contiguous())
    T = conv1x1_lp(x, w27, lp, out_dtype=torch.float32)
    y = torch.empty((N, 1, D, H, W), device=x.device, dtype=torch.float32)
    with torch.cuda.device_of(x):
        _chk(_L().dca_conv3d_c1_gather(_ptr(T), _ptr(y), N, D, H, W, _stream()), "dca_conv3d_c1_gather")
    return y


# ------------------------------------------------------------------------------------------------
# Evaluation step (main_dca.py:143-246 `mytest`): disparity metrics, region confusion matrices, run state
# (csrc/eval_metrics.hip; state layout in include/dca_hip.h).  No launch synchronises; all buffers are torch's.
# ------------------------------------------------------------------------------------------------
EVAL_REC = _C["DCA_EVAL_REC"]
EVAL_STATE_HEAD = _C["DCA_EVAL_STATE_HEAD"]
EVAL_MAX_CLASSES = _C["DCA_EVAL_MAX_CLASSES"]


def disp_metrics(pred, gt, maxdisp, mask=None):
    """Per-image error statistics of a (padded) prediction against the ground truth in one pass: pred (B,Hp,Wp) or
    (B,1,Hp,Wp) with Hp >= H, Wp >= W (rows padded on top, columns on the right: the crop of main_dca.py:171-174 is
    done by addressing), gt (B,H,W), mask bool (B,H,W) or None (gt > 0 & gt < maxdisp).  Returns (B,8) float64:
    #mask, #(gt>0), sum e, sum smooth_l1(e), #(e>1), #(e>2), #(e>3), #(e>3 & e/|gt|>0.05), e = |pred - gt| in fp32."""
    pred, gt = _req(pred, "disp_metrics"), _req(gt, "disp_metrics")
    if pred.dim() == 4 and pred.shape[1] == 1:
        pred = pred[:, 0]
    if pred.dim() != 3 or gt.dim() != 3 or pred.shape[0] != gt.shape[0]:
        raise RuntimeError(f"disp_metrics: expected pred (B,Hp,Wp) and gt (B,H,W), got {tuple(pred.shape)} and {tuple(gt.shape)}")
    (B, Hp, Wp), (H, W) = pred.shape, gt.shape[1:]
    if Hp < H or Wp < W:
        raise RuntimeError("disp_metrics: the prediction is smaller than the ground truth")
    if mask is not None:
        if not isinstance(mask, torch.Tensor) or not mask.is_cuda:
            raise RuntimeError("disp_metrics: the mask must be on the ROCm device; there is no CPU fallback")
        if mask.dtype != torch.bool or mask.shape != gt.shape:
            raise RuntimeError("disp_metrics: expected a bool mask of the ground truth's shape")
        mask = mask.contiguous()
    rec = torch.empty((B, EVAL_REC), device=gt.device, dtype=torch.float64)
    with torch.cuda.device_of(gt):
        ws = torch.empty(_L().dca_disp_metrics_workspace(B, H, W), device=gt.device, dtype=torch.uint8)
        _chk(_L().dca_disp_metrics(_ptr(pred), _ptr(gt), _ptr(mask), _ptr(rec), _ptr(ws), B, H, W, Hp - H, Wp - W,
                                   float(maxdisp), _stream()), "dca_disp_metrics")
    return rec


def region_confusion(volumes, gt):
    """Confusion matrices of 1..3 region-probability volumes (B,C,hp,wp) (or (B,1,C,hp,wp)) at 1/8 resolution against
    label = floor(adaptive_avg_pool2d(gt / 8, (H//8, W//8))), gt (B,H,W); prediction = arg-max over C at row
    i + (hp - H//8), column j.  Returns (len(volumes), C, C) int64, rows = label, columns = prediction."""
    if isinstance(volumes, torch.Tensor):
        volumes = [volumes]
    vols = []
    for v in volumes:
        v = _req(v, "region_confusion")
        vols.append(v[:, 0] if v.dim() == 5 and v.shape[1] == 1 else v)
    gt = _req(gt, "region_confusion")
    if not 1 <= len(vols) <= 3 or any(v.dim() != 4 or v.shape != vols[0].shape for v in vols):
        raise RuntimeError("region_confusion: expected 1 to 3 volumes (B,C,hp,wp) of one shape")
    (B, C, hp, wp), (H, W) = vols[0].shape, gt.shape[1:]
    if gt.dim() != 3 or gt.shape[0] != B or H < 8 or W < 8 or hp < H // 8 or wp < W // 8 or C > EVAL_MAX_CLASSES:
        raise RuntimeError(f"region_confusion: volumes {tuple(vols[0].shape)} do not fit the ground truth {tuple(gt.shape)} "
                           f"(C <= {EVAL_MAX_CLASSES})")
    cm = torch.empty((len(vols), C, C), device=gt.device, dtype=torch.int64)
    p = [_ptr(v) for v in vols] + [None] * (3 - len(vols))
    with torch.cuda.device_of(gt):
        _chk(_L().dca_region_confusion(p[0], p[1], p[2], _ptr(gt), _ptr(cm), len(vols), B, C, hp, wp, H, W, _stream()),
             "dca_region_confusion")
    return cm


def eval_state(num_classes, device):
    """zeroed run state of `eval_accumulate` (float64; layout: include/dca_hip.h)"""
    n = _L().dca_eval_state_len(int(num_classes))
    if n <= 0:
        raise RuntimeError(f"eval_state: 1 <= num_classes <= {EVAL_MAX_CLASSES}")
    return torch.zeros(n, device=device, dtype=torch.float64)


def eval_accumulate(state, rec, cm, gt_shape):
    """Adds one batch -- rec of `disp_metrics`, cm of `region_confusion` -- to the run state, in place."""
    for t, dt, name in ((state, torch.float64, "state"), (rec, torch.float64, "rec"), (cm, torch.int64, "cm")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"eval_accumulate: {name} must be on the ROCm device; there is no CPU fallback")
        if t.dtype != dt or not t.is_contiguous():
            raise RuntimeError(f"eval_accumulate: {name} must be a contiguous {dt} tensor")
    nvol, C = cm.shape[0], cm.shape[1]
    if state.numel() != _L().dca_eval_state_len(C) or rec.dim() != 2 or rec.shape[1] != EVAL_REC or cm.shape[2] != C:
        raise RuntimeError("eval_accumulate: state / rec / cm do not fit together")
    with torch.cuda.device_of(state):
        _chk(_L().dca_eval_accumulate(_ptr(rec), _ptr(cm), _ptr(state), rec.shape[0], nvol, C, int(gt_shape[-2]),
                                      int(gt_shape[-1]), _stream()), "dca_eval_accumulate")
    return state


CONF_MAX_BINS = _C["DCA_CONF_MAX_BINS"]
CONF_ERR_SCALE = _C["DCA_CONF_ERR_SCALE"]     # the error sums of `conf_histogram` are in units of 2^-20 pixels


def conf_histogram(conf, pred, gt, state, maxdisp):
    """Adds the pixels of one batch to a risk-coverage state, in place: conf, pred, gt float32 of one shape, state
    (nbins,3) int64 on the device.  Per confidence bin min(nbins-1, int(clamp(conf,0,1) * nbins)): the count of pixels
    with 0 < gt < maxdisp and a confidence that is not NaN, the sum of trunc(|pred - gt| * 2^20) and the count of
    |pred - gt| > 3.  Integer atomics only: bitwise reproducible.  One launch, no synchronisation."""
    conf, pred, gt = (_req(t, "conf_histogram") for t in (conf, pred, gt))
    if conf.shape != pred.shape or conf.shape != gt.shape or conf.numel() == 0:
        raise RuntimeError(f"conf_histogram: conf, pred and gt must have one non-empty shape, got {tuple(conf.shape)}, "
                           f"{tuple(pred.shape)} and {tuple(gt.shape)}")
    if not isinstance(state, torch.Tensor) or not state.is_cuda:
        raise RuntimeError("conf_histogram: the state must be on the ROCm device; there is no CPU fallback")
    if any(t.device != conf.device for t in (pred, gt, state)):
        raise RuntimeError(f"conf_histogram: conf, pred, gt and the state must be on one device, got {conf.device}, "
                           f"{pred.device}, {gt.device} and {state.device}")
    if state.dtype != torch.int64 or not state.is_contiguous() or state.dim() != 2 or state.shape[1] != 3 \
            or not 2 <= state.shape[0] <= CONF_MAX_BINS:
        raise RuntimeError(f"conf_histogram: the state must be a contiguous int64 (nbins,3) tensor, 2 <= nbins <= "
                           f"{CONF_MAX_BINS}, got {state.dtype} {tuple(state.shape)}")
    with torch.cuda.device_of(conf):
        _chk(_L().dca_conf_histogram(_ptr(conf), _ptr(pred), _ptr(gt), _ptr(state), 1, conf.numel(), state.shape[0],
                                     float(maxdisp), _stream()), "dca_conf_histogram")
    return state


# ------------------------------------------------------------------------------------------------
# Left-right consistency (csrc/lr_consistency.hip): inference only, no counterpart in the reference
# ------------------------------------------------------------------------------------------------
LR_MAX_W = _C["DCA_LR_MAX_W"]
LR_OUTPUTS = ("diff", "valid", "filled", "disp_right")


def _req_f32_same(name, a, b, what):
    """two contiguous float32 tensors of one non-empty shape on one ROCm device, as they are (no copy is made)"""
    for t in (a, b):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"{name}: {what} must be on the ROCm device; there is no CPU fallback")
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise RuntimeError(f"{name}: {what} must be contiguous float32 tensors, got {t.dtype}"
                               f"{'' if t.is_contiguous() else ' (not contiguous)'}")
    if a.shape != b.shape or a.device != b.device or a.numel() == 0:
        raise RuntimeError(f"{name}: {what} must have one non-empty shape on one device, got {tuple(a.shape)} on {a.device} "
                           f"and {tuple(b.shape)} on {b.device}")


def mirror_pair(left, right, out=None):
    """(left, right) (...,H,W) float32 -> (flipW(right), flipW(left)), bit copies, one launch: the mirrored, swapped pair on
    which the unchanged network computes the RIGHT view's disparity in mirrored coordinates (include/dca_hip.h).
    out: a contiguous float32 (2, *left.shape) buffer to write into (allocated when None); the results are its two halves."""
    _req_no_grad("mirror_pair", left, right)
    _req_f32_same("mirror_pair", left, right, "left and right")
    if left.dim() < 2:
        raise RuntimeError(f"mirror_pair: expected (...,H,W) images, got {tuple(left.shape)}")
    if out is None:
        out = torch.empty((2,) + tuple(left.shape), device=left.device, dtype=torch.float32)
    _req_dev(out, "mirror_pair", "out", torch.float32, (2,) + tuple(left.shape))
    if out.device != left.device or out.untyped_storage().data_ptr() in (left.untyped_storage().data_ptr(),
                                                                         right.untyped_storage().data_ptr()):
        raise RuntimeError("mirror_pair: out must be a buffer of its own on the images' device (the flip is not in place)")
    H, W = int(left.shape[-2]), int(left.shape[-1])
    with torch.cuda.device_of(left):
        _chk(_L().dca_mirror_pair(_ptr(left), _ptr(right), _ptr(out[0]), _ptr(out[1]), left.numel() // (H * W), H, W,
                                  _stream()), "dca_mirror_pair")
    return out[0], out[1]


def lr_consistency(disp_left, disp_right_mirrored, tau=1.0, cols=None, outputs=None):
    """Cross-check of a left disparity map against the right view's, invalidation and background fill, ONE launch
    (definitions: include/dca_hip.h, dca_lr_consistency).  disp_left, disp_right_mirrored: (B,1,H,W) or (B,H,W) float32;
    the second is what the network gives on `mirror_pair(left, right)`: right-image column i at index W-1-i.  tau: finite,
    >= 0.  cols (default W): only columns [0, cols) of either image take part (a frame zero-padded on the right).
    Returns a dict of maps shaped like the input: `diff` (|d - r|, +inf out of view), `valid` (1.0 / 0.0), `filled`
    (valid pixels bit for bit; invalid ones from the nearest valid neighbours in the row, the smaller of the two) and
    `disp_right` (the right view's disparity in its own coordinates).  outputs: the names wanted (default all four;
    `valid` is always computed) -- the others are neither computed nor written.  W <= 8192.  Bitwise reproducible."""
    _req_no_grad("lr_consistency", disp_left, disp_right_mirrored)
    _req_f32_same("lr_consistency", disp_left, disp_right_mirrored, "the two disparity maps")
    shape = tuple(disp_left.shape)
    if len(shape) not in (3, 4) or (len(shape) == 4 and shape[1] != 1):
        raise RuntimeError(f"lr_consistency: expected (B,1,H,W) or (B,H,W) disparity maps, got {shape}")
    B, H, W = shape[0], shape[-2], shape[-1]
    tau = float(tau)
    if not (0.0 <= tau < math.inf):
        raise RuntimeError(f"lr_consistency: tau must be finite and >= 0, got {tau}")
    cols = W if cols is None else int(cols)
    if not 1 <= cols <= W or W > LR_MAX_W:
        raise RuntimeError(f"lr_consistency: 1 <= cols <= W <= {LR_MAX_W}, got cols {cols} and W {W}")
    names = LR_OUTPUTS if outputs is None else tuple(outputs)
    if any(n not in LR_OUTPUTS for n in names):
        raise RuntimeError(f"lr_consistency: outputs are chosen from {LR_OUTPUTS}, got {names}")
    res = {n: torch.empty(shape, device=disp_left.device, dtype=torch.float32) for n in LR_OUTPUTS
           if n in names or n == "valid"}
    with torch.cuda.device_of(disp_left):
        _chk(_L().dca_lr_consistency(_ptr(disp_left), _ptr(disp_right_mirrored), *(_ptr(res.get(n)) for n in LR_OUTPUTS),
                                     B, H, W, cols, tau, _stream()), "dca_lr_consistency")
    return res


# ------------------------------------------------------------------------------------------------
# Self-supervised loss (csrc/selfsup.hip): view synthesis + edge-aware smoothness, all levels of a
# step in one launch per direction.  The smoothness term is the reference's util.py:76-86; the rest has no counterpart.
# ------------------------------------------------------------------------------------------------
SELFSUP_MAX_LEVELS = _C["DCA_SELFSUP_MAX_LEVELS"]
SELFSUP_TILE = (_C["DCA_SELFSUP_TILE_H"], _C["DCA_SELFSUP_TILE_W"])
SELFSUP_SUMS = _C["DCA_SELFSUP_SUMS"]
SELFSUP_OUT = _C["DCA_SELFSUP_OUT"]
SELFSUP_MAX_SAMPLE = (1 << 31) - 1          # 3 H W, the elements of one sample's image: offsets inside a sample are 32-bit


def _selfsup_check(left, right, disps, weights, valid, scalars):
    """validates the arguments of `selfsup_loss`; returns (B, H, W, weights as floats, valid_u8)"""
    name = "selfsup_loss"
    for t, what in ((left, "left"), (right, "right")):
        _req_dev(t, name, f"the {what} image", torch.float32)
    if left.dim() != 4 or left.shape[1] != 3 or left.shape != right.shape or left.device != right.device:
        raise RuntimeError(f"{name}: expected two (B,3,H,W) images of one shape on one device, got {tuple(left.shape)} and "
                           f"{tuple(right.shape)}")
    B, _, H, W = (int(s) for s in left.shape)
    if B < 1 or H < 3 or W < 3:
        raise RuntimeError(f"{name}: the 3x3 windows need B >= 1, H >= 3 and W >= 3, got {tuple(left.shape)}")
    if 3 * H * W > SELFSUP_MAX_SAMPLE or W > 1 << 24 or B > 65535:
        raise RuntimeError(f"{name}: 3 H W <= {SELFSUP_MAX_SAMPLE} (offsets inside a sample are 32-bit), W <= 2^24 and "
                           f"B <= 65535, got {tuple(left.shape)}")
    disps = list(disps)
    if not 1 <= len(disps) <= SELFSUP_MAX_LEVELS or len(weights) != len(disps):
        raise RuntimeError(f"{name}: 1 to {SELFSUP_MAX_LEVELS} disparity maps with one weight each, got {len(disps)} maps and "
                           f"{len(weights)} weights")
    for d in disps:
        _req_dev(d, name, "a disparity map", torch.float32)
        if tuple(d.shape) not in ((B, H, W), (B, 1, H, W)) or d.device != left.device:
            raise RuntimeError(f"{name}: expected ({B},{H},{W}) or ({B},1,{H},{W}) disparity maps on {left.device}, got "
                               f"{tuple(d.shape)} on {d.device}")
    valid_u8 = 0
    if valid is not None:
        if not isinstance(valid, torch.Tensor) or not valid.is_cuda or valid.device != left.device:
            raise RuntimeError(f"{name}: valid must be on the images' ROCm device; there is no CPU fallback")
        if valid.dtype not in (torch.float32, torch.bool) or not valid.is_contiguous() or valid.numel() != B * H * W \
                or tuple(valid.shape) not in ((B, H, W), (B, 1, H, W)):
            raise RuntimeError(f"{name}: valid must be a contiguous float32 or bool ({B},{H},{W}) tensor, got {valid.dtype} "
                               f"{tuple(valid.shape)}")
        if valid.requires_grad:
            raise RuntimeError(f"{name}: valid carries no gradient")
        valid_u8 = int(valid.dtype == torch.bool)
    alpha, lam, c1, c2 = scalars
    if not (0.0 <= alpha <= 1.0) or not (c1 > 0.0 and c2 > 0.0) or lam != lam:
        raise RuntimeError(f"{name}: 0 <= alpha <= 1, c1 > 0, c2 > 0 and a lam that is a number, got alpha {alpha}, lam {lam}, "
                           f"c1 {c1}, c2 {c2}")
    return B, H, W, [float(w) for w in weights], valid_u8


class _SelfSupLoss(torch.autograd.Function):
    """sum_l w_l (photo_scale photo_l + lam smooth_l) and the detached (L,3) per-level (photo, smooth, sum M)"""

    @staticmethod
    def forward(ctx, left, right, valid, weights, scalars, photo_scale, *disps):
        B, H, W, weights, valid_u8 = _selfsup_check(left, right, disps, weights, valid, scalars)
        n = len(disps)
        tiles = -(-H // SELFSUP_TILE[0]) * -(-W // SELFSUP_TILE[1])
        work = torch.empty((n * B * tiles * SELFSUP_SUMS,), device=left.device, dtype=torch.float64)
        out = torch.empty((n * SELFSUP_OUT + 1,), device=left.device, dtype=torch.float32)
        dptr = (ctypes.c_void_p * n)(*[d.data_ptr() for d in disps])
        wts = (ctypes.c_float * n)(*weights)
        with torch.cuda.device_of(left):
            _chk(_L().dca_selfsup_loss_fwd(_ptr(left), _ptr(right), dptr, wts, n, _ptr(valid), valid_u8, _ptr(work), _ptr(out),
                                           B, H, W, *scalars, photo_scale, _stream()), "dca_selfsup_loss_fwd")
        ctx.save_for_backward(left, right, valid, out, *disps)
        ctx.meta = (B, H, W, weights, valid_u8, scalars, photo_scale)
        stats = out[:n * SELFSUP_OUT].view(n, SELFSUP_OUT)[:, :3]
        ctx.mark_non_differentiable(stats)
        return out[n * SELFSUP_OUT], stats

    @staticmethod
    def backward(ctx, gloss, _gstats):
        left, right, valid, out, *disps = ctx.saved_tensors
        B, H, W, weights, valid_u8, scalars, photo_scale = ctx.meta
        n = len(disps)
        gloss = _req(gloss.reshape(1), "selfsup_loss.backward")
        gds = [torch.empty_like(d) for d in disps]
        dptr = (ctypes.c_void_p * n)(*[d.data_ptr() for d in disps])
        gptr = (ctypes.c_void_p * n)(*[g.data_ptr() for g in gds])
        wts = (ctypes.c_float * n)(*weights)
        with torch.cuda.device_of(left):
            _chk(_L().dca_selfsup_loss_bwd(_ptr(left), _ptr(right), dptr, gptr, wts, n, _ptr(valid), valid_u8, _ptr(out),
                                           _ptr(gloss), B, H, W, *scalars, photo_scale, _stream()), "dca_selfsup_loss_bwd")
        return (None,) * 6 + tuple(gds)


def selfsup_loss(left, right, disps, weights, valid=None, alpha=0.85, lam=0.1, c1=1e-4, c2=9e-4, photo_scale=1.0):
    """Self-supervised stereo loss of up to 8 disparity maps in one launch per direction (definitions: include/dca_hip.h,
    dca_selfsup_loss_fwd): sum_l weights[l] (photo_l + lam smooth_l), where photo_l compares `left` with `right` warped
    along the row by disps[l] (alpha SSIM over 3x3 windows + (1 - alpha) L1, at interior pixels that are in view and
    `valid`) and smooth_l is the reference's edge-aware `loss_disp_smoothness` (util.py:76-86).
    left, right: (B,3,H,W) float32, used as given; disps: (B,H,W) or (B,1,H,W) contiguous float32, full-resolution pixels;
    valid: (B,H,W) float32 or bool, no gradient, default all ones; photo_scale: 1, or 0 for the smoothness term alone.
    3 H W < 2^31 per sample.  Returns (loss, stats): a 0-dim float32 tensor with a gradient to the disparity maps only,
    and the detached (L,3) float32 per-level (photo, smooth, sum M) for logging.  Bitwise reproducible; no host
    synchronisation; graph-capturable."""
    scalars = (float(alpha), float(lam), float(c1), float(c2))
    return _SelfSupLoss.apply(left, right, valid, tuple(float(w) for w in weights), scalars, float(photo_scale), *disps)


# ------------------------------------------------------------------------------------------------
# Inference frame I/O (my_img.py:47-110 around the model call): per-plane normalisation as histogram -> table -> look-up,
# placement in the zero-padded frame, export of the cropped disparity (csrc/frame_io.hip).  No launch synchronises.
# ------------------------------------------------------------------------------------------------
def _req_dev(t, name, what, dtype, shape=None):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name}: {what} must be on the ROCm device; there is no CPU fallback")
    if t.dtype != dtype or not t.is_contiguous():
        raise RuntimeError(f"{name}: {what} must be a contiguous {dtype} tensor, got {t.dtype}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise RuntimeError(f"{name}: {what} must have shape {tuple(shape)}, got {tuple(t.shape)}")
    return t


def _req_u8_pair(left, right, name):
    _req_dev(left, name, "the left image", torch.uint8)
    _req_dev(right, name, "the right image", torch.uint8)
    if left.dim() != 3 or left.shape[2] not in (3, 4) or left.shape != right.shape or left.numel() == 0:
        raise RuntimeError(f"{name}: expected two (H,W,3) or (H,W,4) uint8 images of one shape, got {tuple(left.shape)} and "
                           f"{tuple(right.shape)}")
    if left.shape[0] * left.shape[1] >= 1 << 31:
        raise RuntimeError(f"{name}: H * W must stay below 2^31")
    return tuple(int(s) for s in left.shape)


def frame_histogram(left_u8, right_u8):
    """Histograms of the colour planes of two interleaved (H,W,C) uint8 images, C = 3 or 4 (a fourth channel is ignored).
    Returns (2,3,256) int32 counts (image, plane, value); bitwise reproducible."""
    H, W, C = _req_u8_pair(left_u8, right_u8, "frame_histogram")
    hist = torch.empty((2, 3, 256), device=left_u8.device, dtype=torch.int32)
    with torch.cuda.device_of(left_u8):
        _chk(_L().dca_frame_hist(_ptr(left_u8), _ptr(right_u8), _ptr(hist), H, W, C, _stream()), "dca_frame_hist")
    return hist


def frame_lut(hist, n_pixels):
    """hist of `frame_histogram` and the pixel count H*W -> (lut (2,3,256) float32, stats (2,3,2) float64 = mean, std):
    lut[i,c,v] = float32((v - mean) / std) in fp64 with the population std (my_img.py:59-68);
    inference.lut_from_histogram is its numpy restatement, equal bit for bit."""
    _req_dev(hist, "frame_lut", "hist", torch.int32, (2, 3, 256))
    if not 0 < int(n_pixels) < 1 << 31:
        raise RuntimeError("frame_lut: 0 < n_pixels < 2^31")
    lut = torch.empty((2, 3, 256), device=hist.device, dtype=torch.float32)
    stats = torch.empty((2, 3, 2), device=hist.device, dtype=torch.float64)
    with torch.cuda.device_of(hist):
        _chk(_L().dca_frame_lut(_ptr(hist), int(n_pixels), _ptr(lut), _ptr(stats), _stream()), "dca_frame_lut")
    return lut, stats


def frame_apply(left_u8, right_u8, lut, frame_hw, src_y0, dst_y0, rows, cols, out=None):
    """Table look-up and placement: the rows x cols window of the (H,W,C) uint8 images starting at source row src_y0,
    column 0, goes through lut (2,3,256) into the planar frames at row dst_y0, column 0; every other frame element
    becomes +0.0.  out: (2,3,Hc,Wc) float32, written whole (allocated when None).  Returns the (1,3,Hc,Wc) views
    (left, right) of it, the tensors `GwcNet.forward` takes."""
    H, W, C = _req_u8_pair(left_u8, right_u8, "frame_apply")
    Hc, Wc = int(frame_hw[0]), int(frame_hw[1])
    _req_dev(lut, "frame_apply", "lut", torch.float32, (2, 3, 256))
    src_y0, dst_y0, rows, cols = int(src_y0), int(dst_y0), int(rows), int(cols)
    if Hc <= 0 or Wc <= 0 or min(src_y0, dst_y0, rows, cols) < 0 or src_y0 + rows > H or cols > W or dst_y0 + rows > Hc \
            or cols > Wc:
        raise RuntimeError(f"frame_apply: the {rows} x {cols} window (source row {src_y0}, frame row {dst_y0}) does not fit "
                           f"the {H} x {W} source or the {Hc} x {Wc} frame")
    if out is None:
        out = torch.empty((2, 3, Hc, Wc), device=left_u8.device, dtype=torch.float32)
    _req_dev(out, "frame_apply", "out", torch.float32, (2, 3, Hc, Wc))
    with torch.cuda.device_of(left_u8):
        _chk(_L().dca_frame_apply(_ptr(left_u8), _ptr(right_u8), _ptr(lut), _ptr(out[0]), _ptr(out[1]), H, W, C, Hc, Wc,
                                  src_y0, dst_y0, rows, cols, _stream()), "dca_frame_apply")
    return out[0:1], out[1:2]


def disp_export(pred, y0, h, w, scale=256.0, f32=True, u16=False, out_f32=None, out_u16=None):
    """The h x w window of the prediction (Hc,Wc) / (1,1,Hc,Wc) starting at row y0, column 0 (my_img.py:105-108), as
    float32 (bit copy) and / or uint16(pred * scale) (my_img.py:110; truncated, saturated to [0, 65535], NaN -> 0).
    Returns (float32 (h,w) or None, uint16 (h,w) or None); out_f32 / out_u16: buffers of that shape to write into."""
    if not isinstance(pred, torch.Tensor) or not pred.is_cuda:
        raise RuntimeError("disp_export: the prediction must be on the ROCm device; there is no CPU fallback")
    if pred.dtype != torch.float32 or not pred.is_contiguous() or pred.dim() < 2 or pred.numel() == 0 \
            or pred.numel() != pred.shape[-2] * pred.shape[-1]:
        raise RuntimeError(f"disp_export: expected a contiguous float32 (Hc,Wc) prediction, got {pred.dtype} {tuple(pred.shape)}")
    Hc, Wc = int(pred.shape[-2]), int(pred.shape[-1])
    y0, h, w = int(y0), int(h), int(w)
    if y0 < 0 or h <= 0 or w <= 0 or y0 + h > Hc or w > Wc or Hc * Wc >= 1 << 31:
        raise RuntimeError(f"disp_export: the {h} x {w} window at row {y0} does not fit the {Hc} x {Wc} prediction")
    if not (f32 or u16):
        raise RuntimeError("disp_export: nothing to export (f32 and u16 are both off)")
    of = ou = None
    if f32:
        of = torch.empty((h, w), device=pred.device, dtype=torch.float32) if out_f32 is None else \
            _req_dev(out_f32, "disp_export", "out_f32", torch.float32, (h, w))
    if u16:
        ou = torch.empty((h, w), device=pred.device, dtype=torch.uint16) if out_u16 is None else \
            _req_dev(out_u16, "disp_export", "out_u16", torch.uint16, (h, w))
    with torch.cuda.device_of(pred):
        _chk(_L().dca_disp_export(_ptr(pred), _ptr(of), _ptr(ou), Hc, Wc, y0, h, w, float(scale), _stream()),
             "dca_disp_export")
    return of, ou


# ------------------------------------------------------------------------------------------------
# Rectification of a raw pair in front of the frame I/O (csrc/rectify.hip): one launch gathers both
# images through the fixed-point maps of a geometry.RectifyMaps.  No launch synchronises.
# ------------------------------------------------------------------------------------------------
RECT_MAX_SRC = _C["DCA_RECT_MAX_SRC"]


def _overlap(a, b):
    return a.data_ptr() < b.data_ptr() + b.numel() * b.element_size() and \
        b.data_ptr() < a.data_ptr() + a.numel() * a.element_size()


def rectify_pair(left_u8, right_u8, maps, out=None):
    """The raw (Hs,Ws,C) uint8 pair, C = 3 or 4, through `maps` (a geometry.RectifyMaps with src_hw == (Hs,Ws)) -> the two
    rectified (Hd,Wd,C) uint8 images, one launch: bilinear with 5 fractional bits per axis, zero outside the source, a
    fourth channel 255 (definitions: include/dca_hip.h, dca_rectify_pair; geometry.rectify_pair_host is the numpy
    restatement, equal bit for bit).  out: a (2,Hd,Wd,C) uint8 buffer or a pair of (Hd,Wd,C) buffers to write into, which
    must not overlap the inputs or each other.  With `out` given and the maps already on the device (their first use uploads
    them) nothing is allocated and the host never waits: the launch can be captured into a hipGraph."""
    name = "rectify_pair"
    Hs, Ws, C = _req_u8_pair(left_u8, right_u8, name)
    if not hasattr(maps, "device_maps") or not hasattr(maps, "src_hw"):
        raise RuntimeError(f"{name}: maps must be a geometry.RectifyMaps, got {type(maps)}")
    if (Hs, Ws) != tuple(maps.src_hw):
        raise RuntimeError(f"{name}: the maps were built for {maps.src_hw[0]} x {maps.src_hw[1]} images, got {Hs} x {Ws}")
    if left_u8.device != right_u8.device:
        raise RuntimeError(f"{name}: the two images must be on one device")
    Hd, Wd = maps.dst_hw
    if max(Hs, Ws) > RECT_MAX_SRC or Hs * Ws * C >= 1 << 31 or Hd * Wd * C >= 1 << 31:
        raise RuntimeError(f"{name}: the source may be at most {RECT_MAX_SRC} x {RECT_MAX_SRC} and every image must stay "
                           "below 2^31 bytes")
    if out is None:
        out = torch.empty((2, Hd, Wd, C), device=left_u8.device, dtype=torch.uint8)
    if not isinstance(out, (torch.Tensor, tuple, list)) or len(out) != 2:
        raise RuntimeError(f"{name}: out must be a (2,{Hd},{Wd},{C}) uint8 buffer or a pair of ({Hd},{Wd},{C}) buffers")
    ol, orr = out[0], out[1]
    for t, what in ((ol, "out[0]"), (orr, "out[1]")):
        _req_dev(t, name, what, torch.uint8, (Hd, Wd, C))
        if t.device != left_u8.device:
            raise RuntimeError(f"{name}: {what} must be on the images' device")
        if _overlap(t, left_u8) or _overlap(t, right_u8):
            raise RuntimeError(f"{name}: {what} must not alias an input image")
    if _overlap(ol, orr):
        raise RuntimeError(f"{name}: out[0] and out[1] must not alias each other")
    dmaps, plane = maps.device_maps(left_u8.device)
    with torch.cuda.device_of(left_u8):
        _chk(_L().dca_rectify_pair(_ptr(left_u8), _ptr(right_u8), _ptr(dmaps), plane, _ptr(ol), _ptr(orr), Hs, Ws, Hd, Wd, C,
                                   _stream()), "dca_rectify_pair")
    return ol, orr


# ------------------------------------------------------------------------------------------------
# Training inputs (dataloader/datasets.py:221-254, 270-317 after the decode): photometric augmentation as one byte table
# per image, crop, occlusion patch, normalisation, ground-truth crop and mask (csrc/train_io.hip).  No launch synchronises;
# dcanet_amd.training holds the numpy restatements and the TrainInput / TrainStep classes built on these.
# ------------------------------------------------------------------------------------------------
def _req_window(name, H, W, y1, x1, th, tw):
    y1, x1, th, tw = int(y1), int(x1), int(th), int(tw)
    if min(y1, x1) < 0 or min(th, tw) <= 0 or y1 + th > H or x1 + tw > W:
        raise RuntimeError(f"{name}: the {th} x {tw} window at ({y1}, {x1}) does not fit the {H} x {W} source")
    return y1, x1, th, tw


def train_luma_sum(left_u8, right_u8, bg):
    """Sum of PIL's convert("L") of each image after its byte table bg (2,256) uint8 (gamma o brightness): (2,) int64,
    S[i] = sum over pixels of (19595 R' + 38470 G' + 7471 B' + 32768) >> 16 with X' = bg[i][X]."""
    H, W, C = _req_u8_pair(left_u8, right_u8, "train_luma_sum")
    _req_dev(bg, "train_luma_sum", "bg", torch.uint8, (2, 256))
    S = torch.empty(2, device=left_u8.device, dtype=torch.int64)
    with torch.cuda.device_of(left_u8):
        _chk(_L().dca_train_luma_sum(_ptr(left_u8), _ptr(right_u8), _ptr(bg), _ptr(S), H, W, C, _stream()),
             "dca_train_luma_sum")
    return S


def train_tables(S, n_pixels, bg, contrast, norm):
    """S of `train_luma_sum`, the pixel count, bg (2,256) uint8, the two contrast factors and norm (2,3,256) float32 ->
    (U (2,256) uint8 = contrast o bg, T (2,3,256) float32 = norm o U); training.contrast_table restates the blend."""
    _req_dev(S, "train_tables", "S", torch.int64, (2,))
    _req_dev(bg, "train_tables", "bg", torch.uint8, (2, 256))
    _req_dev(norm, "train_tables", "norm", torch.float32, (2, 3, 256))
    f0, f1 = float(contrast[0]), float(contrast[1])
    if not 0 < int(n_pixels) < 1 << 31 or not (math.isfinite(f0) and math.isfinite(f1)):
        raise RuntimeError("train_tables: 0 < n_pixels < 2^31 and finite contrast factors")
    U = torch.empty((2, 256), device=S.device, dtype=torch.uint8)
    T = torch.empty((2, 3, 256), device=S.device, dtype=torch.float32)
    with torch.cuda.device_of(S):
        _chk(_L().dca_train_tables(_ptr(S), int(n_pixels), _ptr(bg), f0, f1, _ptr(norm), _ptr(U), _ptr(T), _stream()),
             "dca_train_tables")
    return U, T


def train_patch_colour(right_u8, U, y1, x1, th, tw):
    """Per channel floor(mean of U[1][byte]) over the th x tw window at (y1, x1) of the right image: (3,) uint8, the
    colour of the occlusion patch (datasets.py:306)."""
    H, W, C = _req_u8_pair(right_u8, right_u8, "train_patch_colour")
    _req_dev(U, "train_patch_colour", "U", torch.uint8, (2, 256))
    y1, x1, th, tw = _req_window("train_patch_colour", H, W, y1, x1, th, tw)
    sums = torch.empty(3, device=U.device, dtype=torch.int64)
    colour = torch.empty(3, device=U.device, dtype=torch.uint8)
    with torch.cuda.device_of(U):
        _chk(_L().dca_train_patch_colour(_ptr(right_u8), _ptr(U), _ptr(sums), _ptr(colour), H, W, C, y1, x1, th, tw,
                                         _stream()), "dca_train_patch_colour")
    return colour


def train_crop_norm(left_u8, right_u8, T, y1, x1, out_left, out_right, patch=None, norm=None, colour=None):
    """The th x tw window at (y1, x1) of both (H,W,C) uint8 images through T (2,3,256) into out_left, out_right
    (3,th,tw) float32 -- contiguous views, e.g. slot b of a (B,3,th,tw) batch.  patch = (r0, r1, c0, c1): rows r0:r1,
    columns c0:c1 of the RIGHT crop become norm[1][ch][colour[ch]] (norm (2,3,256), colour (3,) uint8 on the device)."""
    H, W, C = _req_u8_pair(left_u8, right_u8, "train_crop_norm")
    _req_dev(T, "train_crop_norm", "T", torch.float32, (2, 3, 256))
    _req_dev(out_left, "train_crop_norm", "out_left", torch.float32)
    if out_left.dim() != 3 or out_left.shape[0] != 3:
        raise RuntimeError(f"train_crop_norm: out_left must be (3,th,tw), got {tuple(out_left.shape)}")
    th, tw = int(out_left.shape[1]), int(out_left.shape[2])
    _req_dev(out_right, "train_crop_norm", "out_right", torch.float32, (3, th, tw))
    y1, x1, th, tw = _req_window("train_crop_norm", H, W, y1, x1, th, tw)
    py0 = px0 = ph = pw = 0
    if patch is not None:
        r0, r1, c0, c1 = (int(v) for v in patch)
        if not (0 <= r0 <= r1 <= th and 0 <= c0 <= c1 <= tw):
            raise RuntimeError(f"train_crop_norm: the patch rows {r0}:{r1}, columns {c0}:{c1} leave the {th} x {tw} crop")
        py0, px0, ph, pw = r0, c0, r1 - r0, c1 - c0
    if ph > 0 and pw > 0:
        _req_dev(norm, "train_crop_norm", "norm", torch.float32, (2, 3, 256))
        _req_dev(colour, "train_crop_norm", "colour", torch.uint8, (3,))
    else:
        py0 = px0 = ph = pw = 0
        norm = colour = None
    with torch.cuda.device_of(left_u8):
        _chk(_L().dca_train_crop_norm(_ptr(left_u8), _ptr(right_u8), _ptr(T), _ptr(norm), _ptr(colour), _ptr(out_left),
                                      _ptr(out_right), H, W, C, y1, x1, th, tw, py0, px0, ph, pw, _stream()),
             "dca_train_crop_norm")
    return out_left, out_right


def train_disp_crop(disp, y1, x1, maxdisp, out_gt, out_mask, flip_rows=False, scale=1.0, inf_to_zero=False):
    """disp (H,W) float32 or uint16 on the device -> out_gt (th,tw) float32 = the window at (y1, x1) * scale and out_mask
    (th,tw) bool = gt > 0 & gt < maxdisp (main_dca.py:127).  flip_rows: the source is a bottom-up PFM payload;
    inf_to_zero: +inf -> 0 (the Middlebury loaders)."""
    if not isinstance(disp, torch.Tensor) or not disp.is_cuda:
        raise RuntimeError("train_disp_crop: the disparity must be on the ROCm device; there is no CPU fallback")
    if disp.dtype not in (torch.float32, torch.uint16) or disp.dim() != 2 or not disp.is_contiguous() or disp.numel() == 0:
        raise RuntimeError(f"train_disp_crop: expected a contiguous (H,W) float32 or uint16 disparity, got {disp.dtype} "
                           f"{tuple(disp.shape)}")
    H, W = int(disp.shape[0]), int(disp.shape[1])
    if H * W >= 1 << 31:
        raise RuntimeError("train_disp_crop: H * W must stay below 2^31")
    _req_dev(out_gt, "train_disp_crop", "out_gt", torch.float32)
    if out_gt.dim() != 2:
        raise RuntimeError(f"train_disp_crop: out_gt must be (th,tw), got {tuple(out_gt.shape)}")
    th, tw = int(out_gt.shape[0]), int(out_gt.shape[1])
    _req_dev(out_mask, "train_disp_crop", "out_mask", torch.bool, (th, tw))
    y1, x1, th, tw = _req_window("train_disp_crop", H, W, y1, x1, th, tw)
    with torch.cuda.device_of(disp):
        _chk(_L().dca_train_disp_crop(_ptr(disp), int(disp.dtype == torch.uint16), _ptr(out_gt), _ptr(out_mask), H, W, y1, x1,
                                      th, tw, int(bool(flip_rows)), float(scale), int(bool(inf_to_zero)), float(maxdisp),
                                      _stream()), "dca_train_disp_crop")
    return out_gt, out_mask


# ------------------------------------------------------------------------------------------------
# Geometry from calibrated disparity (csrc/geometry.hip): metric depth and a compacted, coloured point
# cloud from the maps the pipeline already holds on the device.  Inference only, no counterpart in the reference.  No launch
# synchronises; with every buffer passed in nothing is allocated either (hipGraph capture).
# ------------------------------------------------------------------------------------------------
PC_TILE = _C["DCA_PC_TILE"]
PC_RECORD_BYTES = _C["DCA_PC_RECORD_BYTES"]
GEO_MIN_DISP = 0.0           # default filters: any non-negative disparity ...
GEO_MAX_DEPTH = 80.0         # ... up to the range the KITTI depth benchmark evaluates (metres)


def _geo_frame(name, pred, mask, window):
    """the (Hc,Wc) / (1,1,Hc,Wc) prediction, the optional mask of its shape and the window (y0, rows, cols), default whole"""
    _req_no_grad(name, pred, mask)
    _req_dev(pred, name, "the prediction", torch.float32)
    if pred.dim() < 2 or pred.numel() == 0 or pred.numel() != pred.shape[-2] * pred.shape[-1]:
        raise RuntimeError(f"{name}: expected a (Hc,Wc) prediction of one frame, got {tuple(pred.shape)}")
    if mask is not None:
        _req_f32_same(name, pred, mask, "the prediction and the mask")
    Hc, Wc = int(pred.shape[-2]), int(pred.shape[-1])
    y0, rows, cols = (0, Hc, Wc) if window is None else (int(v) for v in window)
    if y0 < 0 or rows <= 0 or cols <= 0 or y0 + rows > Hc or cols > Wc or Hc * Wc >= 1 << 31:
        raise RuntimeError(f"{name}: the {rows} x {cols} window at row {y0} does not fit the {Hc} x {Wc} prediction")
    return Hc, Wc, y0, rows, cols


def _geo_scalars(name, calib, mask_min, min_disp, max_depth):
    """(f, fb, cx, cy, doffs, min_disp, max_depth, mask_min) as floats, within the ranges of include/dca_hip.h"""
    try:
        f, fb, cx, cy, doffs = (float(getattr(calib, k)) for k in ("f", "fb", "cx", "cy", "doffs"))
    except (AttributeError, TypeError, ValueError) as e:
        raise RuntimeError(f"{name}: calib must be a geometry.StereoCalib (f, fb, cx, cy, doffs): {e}") from None
    mask_min, min_disp, max_depth = float(mask_min), float(min_disp), float(max_depth)
    if not (0.0 < f < math.inf and 0.0 < fb < math.inf and all(math.isfinite(v) for v in (cx, cy, doffs))):
        raise RuntimeError(f"{name}: the calibration must be finite with f > 0 and f * baseline > 0")
    if not 0.0 <= min_disp < math.inf:
        raise RuntimeError(f"{name}: min_disp must be finite and >= 0, got {min_disp}")
    if not 0.0 < max_depth < math.inf:
        raise RuntimeError(f"{name}: max_depth must be finite and > 0, got {max_depth}")
    if math.isnan(mask_min):
        raise RuntimeError(f"{name}: mask_min must not be NaN")
    return f, fb, cx, cy, doffs, min_disp, max_depth, mask_min


def disp_to_depth(pred, calib, window=None, mask=None, mask_min=0.5, min_disp=GEO_MIN_DISP, max_depth=GEO_MAX_DEPTH,
                  f32=True, u16=False, scale=256.0, out_f32=None, out_u16=None):
    """Dense metric depth of the window (y0, rows, cols) of a disparity map (Hc,Wc) / (1,1,Hc,Wc), one launch:
    Z = calib.fb / (d + calib.doffs) where d >= min_disp, 0 < Z <= max_depth and (mask is None or mask >= mask_min),
    +0.0 elsewhere (the KITTI depth convention; definitions: include/dca_hip.h).  mask: float32, shaped like pred.
    Returns (float32 (rows,cols) or None, uint16 (rows,cols) = trunc(Z * scale) saturated, or None); out_f32 / out_u16:
    buffers of that shape to write into."""
    Hc, Wc, y0, rows, cols = _geo_frame("disp_to_depth", pred, mask, window)
    f, fb, cx, cy, doffs, min_disp, max_depth, mask_min = _geo_scalars("disp_to_depth", calib, mask_min, min_disp, max_depth)
    if not (f32 or u16):
        raise RuntimeError("disp_to_depth: nothing to compute (f32 and u16 are both off)")
    if u16 and not 0.0 < float(scale) < math.inf:
        raise RuntimeError(f"disp_to_depth: scale must be finite and > 0, got {scale}")
    of = ou = None
    if f32:
        of = torch.empty((rows, cols), device=pred.device, dtype=torch.float32) if out_f32 is None else \
            _req_dev(out_f32, "disp_to_depth", "out_f32", torch.float32, (rows, cols))
    if u16:
        ou = torch.empty((rows, cols), device=pred.device, dtype=torch.uint16) if out_u16 is None else \
            _req_dev(out_u16, "disp_to_depth", "out_u16", torch.uint16, (rows, cols))
    with torch.cuda.device_of(pred):
        _chk(_L().dca_disp_to_depth(_ptr(pred), _ptr(mask), _ptr(of), _ptr(ou), Hc, Wc, y0, rows, cols, fb, doffs, min_disp,
                                    max_depth, mask_min, float(scale), _stream()), "dca_disp_to_depth")
    return of, ou


def point_cloud_tiles(rows, cols):
    """workgroups of the compaction of a rows x cols window: ceil(rows * cols / PC_TILE)"""
    tiles = int(_L().dca_point_cloud_tiles(int(rows), int(cols)))
    if tiles <= 0:
        raise RuntimeError(f"point_cloud: a {rows} x {cols} window is empty or has 2^31 pixels or more")
    return tiles


def point_cloud_workspace(rows, cols, device):
    """(tile_offsets int32 (tiles + 1,), count int64 (2,)) for `point_cloud(..., workspace=)` on windows up to rows x cols"""
    return (torch.empty(point_cloud_tiles(rows, cols) + 1, device=device, dtype=torch.int32),
            torch.empty(2, device=device, dtype=torch.int64))


def point_cloud(pred, calib, rgb=None, mask=None, window=None, v0=0, stride=1, cap=None, out=None, workspace=None,
                mask_min=0.5, min_disp=GEO_MIN_DISP, max_depth=GEO_MAX_DEPTH):
    """The kept pixels of the window (y0, rows, cols) of a disparity map (Hc,Wc) / (1,1,Hc,Wc) as a compacted point cloud in
    the left camera's frame, in row-major window order, three launches and no atomics: bitwise reproducible, order included
    (definitions: include/dca_hip.h, dca_point_cloud).  A pixel (r, c) is kept under the filters of `disp_to_depth` and
    r % stride == c % stride == 0; its image coordinates are (u, v) = (c, v0 + r).  rgb: the (H,W,3) / (H,W,4) uint8 source
    image, read at (v0 + r, c); None: white.  mask: float32, shaped like pred.
    Returns (vertices, count, tile_offsets):
      vertices      (cap,4) float32: x, y, z and the colour bytes r, g, b, 255 in the fourth column -- 16-byte records, the
                    body of a binary PLY file (`geometry.write_ply`); only the first count[1] rows are written
      count         (2,) int64 on the device: kept pixels, records written = min(kept, cap)
      tile_offsets  (tiles + 1,) int32 on the device: kept pixels before every tile of PC_TILE window pixels, then the total
    cap: room in vertices, default the worst case ceil(rows / stride) * ceil(cols / stride), or out's.  out: a (cap,4)
    float32 buffer; workspace: `point_cloud_workspace(...)` of a window at least this large.  With both given nothing is
    allocated and the host never waits: the launches can be captured into a hipGraph."""
    name = "point_cloud"
    Hc, Wc, y0, rows, cols = _geo_frame(name, pred, mask, window)
    f, fb, cx, cy, doffs, min_disp, max_depth, mask_min = _geo_scalars(name, calib, mask_min, min_disp, max_depth)
    v0, stride = int(v0), int(stride)
    if stride < 1 or v0 < 0:
        raise RuntimeError(f"{name}: stride >= 1 and v0 >= 0, got stride {stride} and v0 {v0}")
    C = Hs = Ws = 0
    if rgb is not None:
        _req_dev(rgb, name, "rgb", torch.uint8)
        if rgb.dim() != 3 or rgb.shape[2] not in (3, 4) or rgb.device != pred.device or rgb.shape[0] * rgb.shape[1] >= 1 << 31:
            raise RuntimeError(f"{name}: rgb must be a (H,W,3) or (H,W,4) uint8 image on the prediction's device, got "
                               f"{tuple(rgb.shape)}")
        Hs, Ws, C = (int(s) for s in rgb.shape)
        if v0 + rows > Hs or cols > Ws:
            raise RuntimeError(f"{name}: the {rows} x {cols} window at image row {v0} does not fit the {Hs} x {Ws} image")
    tiles = point_cloud_tiles(rows, cols)
    if out is not None:
        _req_dev(out, name, "out", torch.float32)
        if out.dim() != 2 or out.shape[1] != 4 or out.device != pred.device or out.data_ptr() % PC_RECORD_BYTES:
            raise RuntimeError(f"{name}: out must be a 16-byte aligned (cap,4) float32 buffer on the prediction's device, got "
                               f"{tuple(out.shape)}")
        if cap is not None and int(cap) > out.shape[0]:
            raise RuntimeError(f"{name}: cap {cap} exceeds the {out.shape[0]} records of out")
    if cap is None:
        cap = out.shape[0] if out is not None else -(-rows // stride) * -(-cols // stride)
    cap = int(cap)
    if cap < 0:
        raise RuntimeError(f"{name}: cap >= 0, got {cap}")
    if out is None:
        out = torch.empty((cap, 4), device=pred.device, dtype=torch.float32)
    if workspace is None:
        workspace = point_cloud_workspace(rows, cols, pred.device)
    offs, count = workspace
    _req_dev(offs, name, "workspace[0] (tile_offsets)", torch.int32)
    _req_dev(count, name, "workspace[1] (count)", torch.int64, (2,))
    if offs.dim() != 1 or offs.numel() < tiles + 1 or offs.device != pred.device or count.device != pred.device:
        raise RuntimeError(f"{name}: workspace[0] must hold {tiles + 1} int32 on the prediction's device, got {tuple(offs.shape)}")
    with torch.cuda.device_of(pred):
        _chk(_L().dca_point_cloud(_ptr(pred), _ptr(mask), _ptr(rgb), C, Hs, Ws, _ptr(out) if cap else None, cap, _ptr(offs),
                                  _ptr(count), Hc, Wc, y0, rows, cols, v0, stride, f, fb, cx, cy, doffs, min_disp, max_depth,
                                  mask_min, _stream()), "dca_point_cloud")
    return out[:cap], count, offs[:tiles + 1]


# ------------------------------------------------------------------------------------------------
# Sparse ground truth from a LiDAR scan (csrc/lidar.hip): the points of one scan, projected into the
# rectified left image through a z-buffer and a hidden-point test.  No counterpart in the reference.  No launch
# synchronises; with `out` and `workspace` passed in nothing is allocated either.
# ------------------------------------------------------------------------------------------------
LIDAR_MAX_RADIUS = _C["DCA_LIDAR_MAX_RADIUS"]
_LIDAR_KINDS = {"disp": torch.float32, "depth": torch.float32, "disp_u16": torch.uint16, "count": torch.int64}


def lidar_disparity(points, calib, n=None, occl=_geometry.LIDAR_OCCL, min_depth=_geometry.LIDAR_MIN_DEPTH,
                    max_depth=_geometry.LIDAR_MAX_DEPTH, min_disp=_geometry.LIDAR_MIN_DISP,
                    max_disp=_geometry.LIDAR_MAX_DISP, outputs=("disp",), out=None, workspace=None):
    """One LiDAR scan -> sparse ground-truth maps in the rectified left image, three launches (definitions:
    include/dca_hip.h, dca_lidar_disparity; `geometry.lidar_disparity_host` is the numpy restatement, equal bit for bit).
    points: (N,S) float32 on the device, S >= 3 (a KITTI scan: S = 4); the leading n rows (default all) and their first three
    columns are read.  calib: a geometry.LidarCalib.  A point is kept with min_depth <= z <= max_depth inside the image;
    the nearest point of a pixel wins (integer atomicMin on the depth's bits: the same bits for every order of the points);
    occl = (rx, ry, rel) drops a pixel whose z exceeds (1 + rel) times the smallest z within rx columns and ry rows,
    (0, 0, rel) switches that off; a pixel is written where min_disp <= d < max_disp, d = fb / z - doffs.
    Returns a dict with the keys of `outputs`:
      disp      (H,W) float32: d, +0.0 where there is no measurement (the KITTI convention)
      depth     (H,W) float32: z in metres, +0.0 elsewhere
      disp_u16  (H,W) uint16: the KITTI disparity PNG payload, trunc(d * 256 + 0.5) saturated, >= 1 where written, 0 elsewhere
      count     (2,) int64 on the device: pixels written, points kept
    out: a dict of buffers for some or all of them; workspace: an int32 buffer of at least H * W words (the z-buffer)."""
    name = "lidar_disparity"
    _req_no_grad(name, points)
    _req_dev(points, name, "points", torch.float32)
    if points.dim() != 2:
        raise RuntimeError(f"{name}: expected (N,S) points, got {tuple(points.shape)}")
    N, S = int(points.shape[0]), int(points.shape[1])
    n, rx, ry, rel, fb, doffs, min_depth, max_depth, min_disp, max_disp, outputs = _geometry._lidar_scalars(
        name, RuntimeError, calib, N, S, n, occl, min_depth, max_depth, min_disp, max_disp, outputs)
    H, W = calib.hw
    dev = points.device
    out = {} if out is None else out
    if not isinstance(out, dict) or set(out) - set(_LIDAR_KINDS):
        raise RuntimeError(f"{name}: out must be a dict with keys out of {tuple(_LIDAR_KINDS)}")
    res = {}
    for key in outputs:
        shape = (2,) if key == "count" else (H, W)
        if key in out:
            res[key] = _req_dev(out[key], name, f"out[{key!r}]", _LIDAR_KINDS[key], shape)
            if res[key].device != dev:
                raise RuntimeError(f"{name}: out[{key!r}] must be on the points' device")
        else:
            res[key] = torch.empty(shape, device=dev, dtype=_LIDAR_KINDS[key])
    if workspace is None:
        workspace = torch.empty(H * W, device=dev, dtype=torch.int32)
    _req_dev(workspace, name, "workspace", torch.int32)
    if workspace.numel() < H * W or workspace.device != dev:
        raise RuntimeError(f"{name}: workspace must hold {H * W} int32 on the points' device, got {workspace.numel()}")
    m = [float(v) for v in calib.M.reshape(-1)]
    with torch.cuda.device_of(points):
        _chk(_L().dca_lidar_disparity(_ptr(points) if N else None, N, S, n, *m, H, W, fb, doffs, min_depth, max_depth, min_disp,
                                      max_disp, rx, ry, rel, _ptr(res.get("disp")), _ptr(res.get("depth")),
                                      _ptr(res.get("disp_u16")), _ptr(res.get("count")), _ptr(workspace), _stream()),
             "dca_lidar_disparity")
    return res


# ------------------------------------------------------------------------------------------------
# Disparity post-filter (csrc/postfilter.hip): speckle removal -- connected components of similar
# disparity, the small ones dropped -- and a small masked median.  Inference only, no counterpart in the reference;
# `postfilter.speckle_filter_host` / `median_filter_host` are the numpy restatements, equal bit for bit.  No launch
# synchronises; with `out` and `workspace` passed in nothing is allocated either (hipGraph capture).
# ------------------------------------------------------------------------------------------------
SPECKLE_TILE = (_C["DCA_SPK_TILE_H"], _C["DCA_SPK_TILE_W"])
SPECKLE_OUTPUTS = ("disp", "valid", "size")
_SPECKLE_KINDS = {"disp": torch.float32, "valid": torch.float32, "size": torch.int32}
POSTFILTER_MAX_BATCH = 65535


def _pf_frame(name, disp, mask, mask_min, window):
    """the maps (Hc,Wc) / (B,Hc,Wc) / (B,1,Hc,Wc), the optional mask of their shape and the window (y0, rows, cols), default
    whole, as `_geo_frame` takes them for one frame -> (B, Hc, Wc, y0, rows, cols, mask_min, the outputs' shape)"""
    _req_no_grad(name, disp, mask)
    _req_dev(disp, name, "the disparity", torch.float32)
    shape = tuple(disp.shape)
    if len(shape) not in (2, 3, 4) or (len(shape) == 4 and shape[1] != 1) or disp.numel() == 0:
        raise RuntimeError(f"{name}: expected (Hc,Wc), (B,Hc,Wc) or (B,1,Hc,Wc) disparity maps, got {shape}")
    if mask is not None:
        _req_f32_same(name, disp, mask, "the disparity and the mask")
    mask_min = float(mask_min)
    if mask is not None and math.isnan(mask_min):
        raise RuntimeError(f"{name}: mask_min must not be NaN")
    Hc, Wc = shape[-2:]
    B = disp.numel() // (Hc * Wc)
    try:
        y0, rows, cols = (0, Hc, Wc) if window is None else (int(v) for v in window)
    except (TypeError, ValueError):
        raise RuntimeError(f"{name}: window is (y0, rows, cols), got {window!r}") from None
    if y0 < 0 or rows <= 0 or cols <= 0 or y0 + rows > Hc or cols > Wc:
        raise RuntimeError(f"{name}: the {rows} x {cols} window at row {y0} does not fit the {Hc} x {Wc} map")
    if Hc * Wc >= 1 << 31 or rows * cols >= 1 << 31 or B > POSTFILTER_MAX_BATCH:
        raise RuntimeError(f"{name}: a map must have fewer than 2^31 pixels (label offsets are 32-bit) and a batch at most "
                           f"{POSTFILTER_MAX_BATCH} maps, got {B} x {Hc} x {Wc}")
    return B, Hc, Wc, y0, rows, cols, mask_min, shape[:-2] + (rows, cols)


def speckle_workspace(rows, cols, device, batch=1):
    """(label, count): the two int32 buffers of batch * rows * cols words for `speckle_filter(..., workspace=)` on windows up
    to rows x cols; a call writes every word it reads, nothing has to be cleared between calls"""
    n = int(batch) * int(rows) * int(cols)
    if n <= 0 or int(rows) * int(cols) >= 1 << 31:
        raise RuntimeError(f"speckle_workspace: a {rows} x {cols} window, batch {batch}, is empty or has 2^31 pixels or more")
    return torch.empty(n, device=device, dtype=torch.int32), torch.empty(n, device=device, dtype=torch.int32)


def speckle_filter(disp, max_size, max_diff, mask=None, mask_min=0.5, window=None, fill=0.0, outputs=None, out=None,
                   workspace=None):
    """Speckle filter of disparity maps (Hc,Wc) / (B,Hc,Wc) / (B,1,Hc,Wc), images independent, over the window (y0, rows, cols)
    of every map (definitions: include/dca_hip.h, dca_speckle_filter).  A window pixel is active iff it is finite and (mask is
    None or mask >= mask_min); two 4-neighbours are joined iff both are active and |a - b| <= max_diff in float32 (equality
    joins; chained, a ramp with small steps is one component).  max_size: an integer >= 0; components of at most max_size
    pixels are removed (0: the identity on active pixels).  Returns a dict of (rows,cols) maps per image:
      disp   float32  the input bit for bit where valid, `fill` elsewhere (+0.0: "no measurement")
      valid  float32  1.0 where active and size > max_size, 0.0 elsewhere
      size   int32    the pixel's component size, 0 for an inactive pixel
    outputs: the names wanted (default all three; `valid` is always computed) -- the others are neither computed nor written.
    out: a dict of buffers for some or all of them; workspace: `speckle_workspace(...)` of a window and batch at least this
    large.  With both given nothing is allocated and the host never waits: the four launches can be captured into a
    hipGraph.  Bitwise reproducible: tile-local union-find in LDS, a merge across tile edges with integer atomics."""
    name = "speckle_filter"
    B, Hc, Wc, y0, rows, cols, mask_min, shape = _pf_frame(name, disp, mask, mask_min, window)
    try:
        ok = int(max_size) == max_size and 0 <= int(max_size) < 1 << 31 and 0.0 <= float(max_diff) < math.inf
        max_diff, fill = float(max_diff), float(fill)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise RuntimeError(f"{name}: max_size must be an integer >= 0, max_diff finite and >= 0 and fill a number, got "
                           f"{max_size!r}, {max_diff!r} and {fill!r}")
    names = SPECKLE_OUTPUTS if outputs is None else tuple(outputs)
    if any(n not in SPECKLE_OUTPUTS for n in names):
        raise RuntimeError(f"{name}: outputs are chosen from {SPECKLE_OUTPUTS}, got {names}")
    out = {} if out is None else out
    if not isinstance(out, dict) or set(out) - set(SPECKLE_OUTPUTS):
        raise RuntimeError(f"{name}: out must be a dict with keys out of {SPECKLE_OUTPUTS}")
    dev = disp.device
    res = {}
    for key in SPECKLE_OUTPUTS:
        if key not in names and key != "valid":
            continue
        if key in out:
            res[key] = _req_dev(out[key], name, f"out[{key!r}]", _SPECKLE_KINDS[key], shape)
            if res[key].device != dev:
                raise RuntimeError(f"{name}: out[{key!r}] must be on the disparity's device")
        else:
            res[key] = torch.empty(shape, device=dev, dtype=_SPECKLE_KINDS[key])
    if workspace is None:
        workspace = speckle_workspace(rows, cols, dev, B)
    try:
        label, count = workspace
    except (TypeError, ValueError):
        raise RuntimeError(f"{name}: workspace is the (label, count) pair of `speckle_workspace`") from None
    for t, what in ((label, "workspace[0] (label)"), (count, "workspace[1] (count)")):
        _req_dev(t, name, what, torch.int32)
        if t.numel() < B * rows * cols or t.device != dev:
            raise RuntimeError(f"{name}: {what} must hold {B * rows * cols} int32 on the disparity's device, got {t.numel()}")
    if label.data_ptr() == count.data_ptr():
        raise RuntimeError(f"{name}: workspace[0] and workspace[1] must be two buffers")
    with torch.cuda.device_of(disp):
        _chk(_L().dca_speckle_filter(_ptr(disp), _ptr(mask), _ptr(res.get("disp")), _ptr(res["valid"]), _ptr(res.get("size")),
                                     _ptr(label), _ptr(count), B, Hc, Wc, y0, rows, cols, int(max_size), max_diff, mask_min,
                                     fill, _stream()), "dca_speckle_filter")
    return res


def median_filter(disp, ksize, mask=None, mask_min=0.5, window=None, out=None):
    """Masked ksize x ksize median (ksize 3 or 5) of disparity maps (Hc,Wc) / (B,Hc,Wc) / (B,1,Hc,Wc) over the window
    (y0, rows, cols), one launch (definitions: include/dca_hip.h, dca_median_filter).  For an active centre (finite, and
    mask is None or mask >= mask_min) the candidates are the active pixels of the neighbourhood inside the window -- no
    border replication -- and the result is the one of rank (n - 1) // 2, the lower median for even n, an input value bit
    for bit (-0.0 < +0.0); an inactive centre is copied unchanged.  Returns float32 (rows,cols) per image; out: a buffer
    of that shape to write into (not the input)."""
    name = "median_filter"
    B, Hc, Wc, y0, rows, cols, mask_min, shape = _pf_frame(name, disp, mask, mask_min, window)
    if isinstance(ksize, bool) or ksize not in (3, 5):
        raise RuntimeError(f"{name}: ksize is 3 or 5, got {ksize!r}")
    if out is None:
        out = torch.empty(shape, device=disp.device, dtype=torch.float32)
    _req_dev(out, name, "out", torch.float32, shape)
    if out.device != disp.device or out.untyped_storage().data_ptr() == disp.untyped_storage().data_ptr():
        raise RuntimeError(f"{name}: out must be a buffer of its own on the disparity's device (the filter is not in place)")
    with torch.cuda.device_of(disp):
        _chk(_L().dca_median_filter(_ptr(disp), _ptr(mask), _ptr(out), B, Hc, Wc, y0, rows, cols, int(ksize), mask_min,
                                    _stream()), "dca_median_filter")
    return out


# ------------------------------------------------------------------------------------------------
# Pictures of a disparity map (csrc/visualize.hip): the KITTI error map of a prediction against the
# ground truth (utils/visualization.py:31-55) and the colour-coded disparity map, uint8 RGB on the device.  No launch
# synchronises; definitions: include/dca_hip.h.
# ------------------------------------------------------------------------------------------------
CMAPS = {"gray": _C["DCA_CMAP_GRAY"], "kitti": _C["DCA_CMAP_KITTI"]}


def disp_error_image(pred, gt, abs_thres=3.0, rel_thres=0.05, legend=True, f32=True, u8=False, out_f32=None, out_u8=None):
    """The KITTI error map of a (padded) prediction against the ground truth in one launch (the reference's
    disp_error_image_func.forward, utils/visualization.py:31-55): pred (B,Hp,Wp) or (B,1,Hp,Wp) with Hp >= H, Wp >= W (rows
    padded on top, columns on the right, cropped by addressing as in `disp_metrics`), gt (B,H,W).  Returns (float32 planar
    (B,3,H,W) in [0,1] -- the reference's result -- or None, uint8 interleaved (B,H,W,3) or None); out_f32 / out_u8: buffers
    of those shapes to write into.  legend: the colour key in the top-left corner (the reference always draws it)."""
    name = "disp_error_image"
    pred, gt = _req(pred, name), _req(gt, name)
    if pred.dim() == 4 and pred.shape[1] == 1:
        pred = pred[:, 0]
    if pred.dim() != 3 or gt.dim() != 3 or pred.shape[0] != gt.shape[0] or gt.numel() == 0:
        raise RuntimeError(f"{name}: expected pred (B,Hp,Wp) and gt (B,H,W), got {tuple(pred.shape)} and {tuple(gt.shape)}")
    (B, Hp, Wp), (H, W) = pred.shape, gt.shape[1:]
    if Hp < H or Wp < W:
        raise RuntimeError(f"{name}: the prediction is smaller than the ground truth")
    if B * Hp * Wp >= 1 << 31:
        raise RuntimeError(f"{name}: B * Hp * Wp must stay below 2^31")
    abs_thres, rel_thres = float(abs_thres), float(rel_thres)
    if not (0.0 < abs_thres < math.inf and 0.0 < rel_thres < math.inf):
        raise RuntimeError(f"{name}: abs_thres and rel_thres must be positive and finite, got {abs_thres} and {rel_thres}")
    if not (f32 or u8):
        raise RuntimeError(f"{name}: nothing to compute (f32 and u8 are both off)")
    of = ou = None
    if f32:
        of = torch.empty((B, 3, H, W), device=gt.device, dtype=torch.float32) if out_f32 is None else \
            _req_dev(out_f32, name, "out_f32", torch.float32, (B, 3, H, W))
    if u8:
        ou = torch.empty((B, H, W, 3), device=gt.device, dtype=torch.uint8) if out_u8 is None else \
            _req_dev(out_u8, name, "out_u8", torch.uint8, (B, H, W, 3))
    with torch.cuda.device_of(gt):
        _chk(_L().dca_disp_error_image(_ptr(pred), _ptr(gt), _ptr(of), _ptr(ou), B, H, W, Hp - H, Wp - W, abs_thres, rel_thres,
                                       1 if legend else 0, _stream()), "dca_disp_error_image")
    return of, ou


def _vis_maps(name, disp, mask, batched):
    """the float32 map(s) and the optional mask of the same shape: (B, Hc, Wc) of a batch, or of ONE frame (B = 1)"""
    _req_no_grad(name, disp, mask)
    _req_dev(disp, name, "the disparity", torch.float32)
    if disp.dim() < 2 or disp.numel() == 0:
        raise RuntimeError(f"{name}: expected a (Hc,Wc) map{' or a (B,Hc,Wc) batch' if batched else ''}, got {tuple(disp.shape)}")
    Hc, Wc = int(disp.shape[-2]), int(disp.shape[-1])
    B = disp.numel() // (Hc * Wc)
    if not batched and B != 1:
        raise RuntimeError(f"{name}: expected the (Hc,Wc) map of one frame, got {tuple(disp.shape)}")
    if mask is not None:
        _req_f32_same(name, disp, mask, "the disparity and the mask")
    if B > 65535 or B * Hc * Wc >= 1 << 31:
        raise RuntimeError(f"{name}: at most 65535 maps and fewer than 2^31 pixels")
    return B, Hc, Wc


def _vis_mask_min(name, mask, mask_min):
    mask_min = float(mask_min)
    if mask is not None and math.isnan(mask_min):
        raise RuntimeError(f"{name}: mask_min must not be NaN")
    return mask_min


def disp_range(disp, window=None, mask=None, mask_min=0.5):
    """(lo, hi) of the valid pixels of the window (y0, rows, cols) (default: everything) of every map of disp (Hc,Wc) /
    (B,Hc,Wc) / (B,1,Hc,Wc): finite, > 0 and, with a float32 mask shaped like disp, mask >= mask_min.  Returns (B,2)
    float32 on the device, (0, 0) for a map without a valid pixel; two launches, nothing is read back; bitwise
    reproducible."""
    name = "disp_range"
    B, Hc, Wc = _vis_maps(name, disp, mask, True)
    y0, rows, cols = (0, Hc, Wc) if window is None else (int(v) for v in window)
    if y0 < 0 or rows <= 0 or cols <= 0 or y0 + rows > Hc or cols > Wc:
        raise RuntimeError(f"{name}: the {rows} x {cols} window at row {y0} does not fit the {Hc} x {Wc} map")
    mask_min = _vis_mask_min(name, mask, mask_min)
    out = torch.empty((B, 2), device=disp.device, dtype=torch.float32)
    with torch.cuda.device_of(disp):
        ws = torch.empty(_L().dca_disp_range_workspace(B, rows, cols), device=disp.device, dtype=torch.uint8)
        _chk(_L().dca_disp_range(_ptr(disp), _ptr(mask), _ptr(out), _ptr(ws), B, Hc, Wc, y0, rows, cols, mask_min, _stream()),
             "dca_disp_range")
    return out


def disp_colorize(disp, y0, rows, cols, max_disp=None, range=None, cmap="kitti", mask=None, mask_min=0.5, out=None):
    """The rows x cols window at row y0, column 0 of ONE map (Hc,Wc) / (1,1,Hc,Wc) as a colour image, one launch: uint8
    (rows,cols,3) on the device.  Exactly one of max_disp (a host number: t = min(d / max_disp, 1), the KITTI devkit's
    scaling) and range (the (1,2) / (2,) device tensor (lo, hi) of `disp_range`: auto-ranging without a read-back) must be
    given.  cmap: "kitti" (the devkit's disp_to_color) or "gray".  Pixels that are not finite, not > 0 or, with a float32 mask
    shaped like disp, below mask_min are black.  out: a (rows,cols,3) uint8 buffer to write into."""
    name = "disp_colorize"
    if cmap not in CMAPS:
        raise ValueError(f"{name}: cmap is one of {sorted(CMAPS)}, got {cmap!r}")
    _, Hc, Wc = _vis_maps(name, disp, mask, False)
    y0, rows, cols = int(y0), int(rows), int(cols)
    if y0 < 0 or rows <= 0 or cols <= 0 or y0 + rows > Hc or cols > Wc:
        raise RuntimeError(f"{name}: the {rows} x {cols} window at row {y0} does not fit the {Hc} x {Wc} map")
    if (max_disp is None) == (range is None):
        raise RuntimeError(f"{name}: give exactly one of max_disp and range")
    if range is not None:
        _req_dev(range, name, "range", torch.float32)
        if range.numel() != 2 or range.device != disp.device:
            raise RuntimeError(f"{name}: range must hold (lo, hi) on the map's device, got {tuple(range.shape)}")
        max_disp = 0.0
    elif not 0.0 < float(max_disp) < math.inf:
        raise RuntimeError(f"{name}: max_disp must be positive and finite, got {max_disp}")
    mask_min = _vis_mask_min(name, mask, mask_min)
    if out is None:
        out = torch.empty((rows, cols, 3), device=disp.device, dtype=torch.uint8)
    _req_dev(out, name, "out", torch.uint8, (rows, cols, 3))
    with torch.cuda.device_of(disp):
        _chk(_L().dca_disp_colorize(_ptr(disp), _ptr(mask), _ptr(range), _ptr(out), Hc, Wc, y0, rows, cols, float(max_disp),
                                    mask_min, CMAPS[cmap], _stream()), "dca_disp_colorize")
    return out
