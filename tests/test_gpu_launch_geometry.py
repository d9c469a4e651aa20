"""Size queries and launches agree on the device.

The host allocates the weight-gradient slabs (`part`), the BatchNorm statistics partials (`stat_part`) and the per-channel
output maxima (`y_cmax`) from a size query of the C ABI, and the launch indexes them with its own grid: both come from one
geometry function per kernel (csrc/*.hip).  Here every such buffer is allocated with exactly the queried size and a guard
tail of a sentinel bit pattern behind it, the C ABI is called directly (ops._L()), and the tail must stay untouched while
the result equals, bit for bit, what `ops` produces for the same inputs.

Two shapes per kernel: the smallest with partial tiles in every dimension (32 -> 32 channels at D, H, W = 5, 9, 20; 32 -> 64
at fine 6, 10, 24 for stride 2), and a small one whose tile count exceeds the workgroups the grid rule allows, so that both
sides of the rule's `min` are taken; the query is checked to return the cap there and to stay below it at the other."""
import pytest
import torch

import dcanet_amd  # noqa: F401
from dcanet_amd import ops
from dcanet_amd.ops import _chk, _ptr, _stream

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 0x7FA5A5A5     # a NaN as fp32 and, twice, as fp64: nothing a kernel writes here
GUARD = 1 << 16           # sentinel words behind the queried size (more than one weight-gradient slab of 27 * 1024 floats)
SMALL, SMALL_S2 = (5, 9, 20), (6, 10, 24)


def _guarded(n, dtype):
    """(all words, the n elements of dtype the query asked for): sentinel everywhere, GUARD words behind the n elements"""
    k = torch.empty((), dtype=dtype).element_size() // 4
    words = torch.full((n * k + GUARD,), SENTINEL, device=DEV, dtype=torch.int32)
    return words, words[:n * k].view(dtype)


def _tail_untouched(words):
    return bool((words[-GUARD:] == SENTINEL).all())


def _rand(seed, *shape):
    return torch.randn(shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))


def _ncu():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def _cdiv(a, b):
    return (a + b - 1) // b


# ---- weight-gradient slabs -------------------------------------------------------------------------------------------------
# family: f16x2 / bf16x3 split kernels (stride 1), the stride-2 f16x2 kernel, and the generic fp32 kernel in its three forms
@pytest.mark.parametrize("family,N,Cx,Cy,dims,capped", [
    ("x2", 1, 32, 32, SMALL, False), ("x2", 1, 32, 32, (17, 30, 60), True),            # tiles 2 x 4 x 16: 9 * 8 * 4 = 288 > 256
    ("x3", 1, 32, 32, SMALL, False), ("x3", 1, 32, 32, (17, 30, 60), True),
    ("s2x2", 1, 32, 64, SMALL_S2, False), ("s2x2", 2, 32, 64, (9, 73, 72), True),      # coarse 5 x 37 x 36, tiles 1 x 4 x 16: 300
    ("k3s1", 1, 32, 32, SMALL, False), ("k3s1", 2, 32, 32, (17, 30, 60), True),        # tiles 2 x 4 x 32: 2 * 144
    ("k3s2", 1, 32, 64, SMALL_S2, False), ("k3s2", 2, 32, 64, (9, 73, 72), True),      # coarse tiles 1 x 2 x 32: 2 * 190
    ("k1", 1, 32, 32, SMALL, False), ("k1", 5, 32, 32, (17, 30, 60), True),            # 256 voxels per tile: 5 * 120 > 512
])
def test_wgrad_part_is_the_queried_size(monkeypatch, family, N, Cx, Cy, dims, capped):
    lib = ops._L()
    ksize, stride = {"x2": (3, 1), "x3": (3, 1), "s2x2": (3, 2), "k3s1": (3, 1), "k3s2": (3, 2), "k1": (1, 1)}[family]
    K = ksize ** 3
    odims = tuple((d + 1) // 2 for d in dims) if stride == 2 else dims
    x, dy = _rand(1, N, Cx, *dims), _rand(2, N, Cy, *odims)
    s_cy, s_cx = Cx * K, K
    nCT = _cdiv(Cx, 32) * _cdiv(Cy, 32)
    if family == "x2":
        nws, workers = lib.dca_conv3d_wgrad_x2_workspace(N, Cx, Cy, *dims), max(1, _ncu() // nCT)
    elif family == "x3":
        monkeypatch.setattr(ops, "CONV_X2", False)
        nws, workers = lib.dca_conv3d_wgrad_x3_workspace(N, Cx, Cy, *dims), max(1, _ncu() // nCT)
    elif family == "s2x2":
        nws = lib.dca_conv3d_wgrad_s2_x2_workspace(N, Cx, Cy, *dims)
        workers = max(1, _ncu() // (_cdiv(Cx, 32) * _cdiv(Cy, 64)))
    else:
        monkeypatch.setattr(ops, "CONV_X3", False)
        nws = lib.dca_conv3d_wgrad_workspace(N, Cx, Cy, *odims, ksize, stride)
        workers = max(1, 256 * (2 if ksize == 1 else 1) // nCT)      # this kernel's rule does not ask the device
    cap = workers * nCT * K * 1024
    assert 0 < nws <= cap and (nws == cap) == capped
    words, part = _guarded(nws, torch.float32)
    dw = torch.empty((Cy, Cx, K), device=DEV)
    if family == "x2":
        _chk(lib.dca_conv3d_wgrad_x2(_ptr(x), 0, _ptr(ops._exps_of(x)), _ptr(dy), 0, _ptr(ops._exps_of(dy)), _ptr(part),
                                     _ptr(dw), N, Cx, Cy, *dims, s_cy, s_cx, _stream()), "dca_conv3d_wgrad_x2")
    elif family == "x3":
        _chk(lib.dca_conv3d_wgrad_x3(_ptr(x), _ptr(dy), _ptr(part), _ptr(dw), N, Cx, Cy, *dims, s_cy, s_cx, _stream()),
             "dca_conv3d_wgrad_x3")
    elif family == "s2x2":
        _chk(lib.dca_conv3d_wgrad_s2_x2(_ptr(x), _ptr(ops._exps_of(x)), _ptr(dy), _ptr(ops._exps_of(dy)), _ptr(part),
                                        _ptr(dw), N, Cx, Cy, *dims, s_cy, s_cx, _stream()), "dca_conv3d_wgrad_s2_x2")
    else:
        _chk(lib.dca_conv3d_wgrad(_ptr(x), _ptr(dy), _ptr(part), _ptr(dw), N, Cx, Cy, *dims, *odims, ksize, stride, s_cy,
                                  s_cx, _stream()), "dca_conv3d_wgrad")
    assert _tail_untouched(words)
    want = torch.empty_like(dw)
    ops._wgrad(x, dy, want, 0, Cx, Cy, ksize, stride, s_cy, s_cx)
    assert torch.equal(dw, want)


# ---- BatchNorm statistics partials of the forwards ---------------------------------------------------------------------------
@pytest.mark.parametrize("family,N,dims,capped", [
    ("x2", 1, SMALL, False), ("x2", 3, (18, 38, 60), True),            # tiles 4 x 8 x 16: 3 * 5 * 5 * 4 = 300 > 256
    ("x3", 1, SMALL, False), ("x3", 3, (18, 38, 60), True),
    ("c1", 1, SMALL, False), ("c1", 3, (43, 64, 127), True),           # 512 voxels per workgroup: 3 * 2731 groups of 128 > 4 * 2048
    ("deconv", 1, (3, 5, 12), False), ("deconv", 2, (11, 38, 68), True),   # input tiles 2 x 8 x 16: 2 * 6 * 5 * 5 = 300
])
def test_stat_part_is_the_queried_size(monkeypatch, family, N, dims, capped):
    lib = ops._L()
    A = B = 32
    S = dims[0] * dims[1] * dims[2]
    x = _rand(3, N, A, *dims)
    if family == "x3":
        monkeypatch.setattr(ops, "CONV_X2", False)
    if family in ("x2", "x3"):
        w, conv = _rand(4, B, A, 3, 3, 3), (27, 0, 0, 3, 1, False)
        nchunk = getattr(lib, f"dca_conv3d_{family}_stats_chunks")(N, B, *dims)
        cap = min(_ncu(), ops.CSLOTS) if family == "x2" else _ncu()
    elif family == "c1":
        w, conv = _rand(4, B, A, 1, 1, 1), (1, 0, 0, 1, 1, False)
        nchunk, cap = lib.dca_conv1_x3_stats_chunks(N, S), 2048
    else:
        w, conv = _rand(4, A, B, 3, 3, 3), (27, 1, 0, 3, 2, True)
        nchunk, cap = lib.dca_deconv3d_x3_stats_chunks(N, *dims), _ncu()
    assert 0 < nchunk <= cap and (nchunk == cap) == capped
    words, part = _guarded(B * nchunk * 4, torch.float64)
    y = torch.empty((N, B) + tuple(2 * d if family == "deconv" else d for d in dims), device=DEV)
    if family == "x2":
        wx, xexps = ops._x2_weights("dca_conv3d_x2", x, w, A, B, 0, 0, "tagged")
        _chk(lib.dca_conv3d_x2_forward_stats(_ptr(x), 0, _ptr(xexps), _ptr(wx), _ptr(y), _ptr(part), N, A, B, *dims,
                                             _stream()), "dca_conv3d_x2_forward_stats")
    elif family == "x3":
        wx = ops._x3_weights(w, A, B, 0, 0)
        _chk(lib.dca_conv3d_x3_forward_stats(_ptr(x), _ptr(wx), _ptr(y), _ptr(part), N, A, B, *dims, _stream()),
             "dca_conv3d_x3_forward_stats")
    elif family == "c1":
        wf = torch.empty((lib.dca_conv1_x3_weight_bytes(A) // 2,), device=DEV, dtype=torch.int16)
        _chk(lib.dca_conv1_x3_prep_weight(_ptr(w), _ptr(wf), A, B, 0, B, 0, _stream()), "dca_conv1_x3_prep_weight")
        _chk(lib.dca_conv1_x3_forward_stats(_ptr(x), None, _ptr(wf), _ptr(y), _ptr(part), N, A, 0, B, B, 0, S, _stream()),
             "dca_conv1_x3_forward_stats")
    else:
        wx = ops._x3_weights(w, A, B, 1, 0)
        _chk(lib.dca_deconv3d_x3_forward_stats(_ptr(x), _ptr(wx), _ptr(y), _ptr(part), N, A, B, *dims, _stream()),
             "dca_deconv3d_x3_forward_stats")
    assert _tail_untouched(words)
    want_y, want_part = ops._conv_sliced(x, None, w, A, B, *conv, want_stats=True)
    assert want_part is not None and want_part.numel() == part.numel()
    assert torch.equal(y, want_y) and torch.equal(part, want_part)


# ---- per-channel output maxima of the f16x2 forwards -------------------------------------------------------------------------
# y_cmax is [channel][CSLOTS] words of which the launch fills the first `query` of every channel: exactly those
@pytest.mark.parametrize("family,N,B,dims,capped", [
    ("x2", 1, 32, SMALL, False), ("x2", 3, 32, (18, 38, 60), True),
    ("s2x2", 1, 64, SMALL_S2, False), ("s2x2", 5, 64, (9, 73, 68), True),   # coarse 5 x 37 x 34, tiles 2 x 4 x 32: 5 * 3 * 10 * 2
])
def test_y_cmax_slots_are_the_queried_ones(family, N, B, dims, capped):
    lib = ops._L()
    A = 32
    x, w = _rand(5, N, A, *dims), _rand(6, B, A, 3, 3, 3)
    words, _ = _guarded(B * ops.CSLOTS, torch.int32)
    if family == "x2":
        nsl = lib.dca_conv3d_x2_stats_chunks(N, B, *dims)
        y = torch.empty((N, B) + dims, device=DEV)
        wx, xexps = ops._x2_weights("dca_conv3d_x2", x, w, A, B, 0, 0, "tagged")
        _chk(lib.dca_conv3d_x2_forward(_ptr(x), 0, _ptr(xexps), _ptr(wx), _ptr(y), None, None, None, None, 1.0, _ptr(words),
                                       N, A, B, *dims, _stream()), "dca_conv3d_x2_forward")
    else:
        nsl = lib.dca_conv3d_s2x2_out_slots(N, B, *dims)
        y = torch.empty((N, B) + tuple((d + 1) // 2 for d in dims), device=DEV)
        wx, xexps = ops._x2_weights("dca_conv3d_s2x2", x, w, A, B, 0, 0, "tagged")
        _chk(lib.dca_conv3d_s2x2_forward(_ptr(x), _ptr(xexps), _ptr(wx), _ptr(y), None, None, 1.0, None, _ptr(words), N, A, B,
                                         *dims, _stream()), "dca_conv3d_s2x2_forward")
    cap = max(1, _ncu() // _cdiv(B, 32 if family == "x2" else 64))
    assert 0 < nsl <= cap and (nsl == cap) == capped
    slots = words[:B * ops.CSLOTS].view(B, ops.CSLOTS)
    assert _tail_untouched(words)
    assert bool((slots[:, nsl:] == SENTINEL).all()) and bool((slots[:, :nsl] != SENTINEL).all())
    want = ops._conv_sliced(x, None, w, A, B, 27, 0, 0, 3, 1 if family == "x2" else 2, False, emit_amax=True)
    want_slots, want_n, _ = want._dca_cmax
    assert want_n == nsl and torch.equal(y, want)
    assert torch.equal(slots[:, :nsl], want_slots.view(B, ops.CSLOTS)[:, :nsl])
