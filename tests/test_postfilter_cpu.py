"""Disparity post-filter, the parts that need no GPU: the numpy restatements of dcanet_amd/postfilter.py -- what the kernels
of csrc/postfilter.hip must equal bit for bit (tests/test_gpu_postfilter.py) -- against closed forms, against scipy's
connected components and against a per-pixel brute force; the entry points are bound and refuse bad arguments before
anything touches a device; the operators refuse what they cannot do."""
import ctypes
import math

import numpy as np
import pytest
import torch

from _postfilter_cases import TH, TW, component_census, flipped, median_cases, scene, speckle_cases
from dcanet_amd.postfilter import median_filter_host, order_key, speckle_filter_host


def _window_of(c):
    y0, rows, cols = c.window if c.window is not None else (0,) + c.d.shape
    d = c.d[y0:y0 + rows, :cols]
    active = np.isfinite(d) & (True if c.mask is None else c.mask[y0:y0 + rows, :cols] >= 0.5)
    return d, active


@pytest.mark.parametrize("case", speckle_cases(), ids=lambda c: c.name)
def test_speckle_restatement_follows_its_definition(case):
    d, active = _window_of(case)
    ref = speckle_filter_host(case.d, case.max_size, case.max_diff, mask=case.mask, window=case.window)
    assert ref["size"].dtype == np.int32 and ref["valid"].dtype == ref["disp"].dtype == np.float32
    assert ref["size"].shape == ref["valid"].shape == ref["disp"].shape == d.shape
    assert np.array_equal(ref["size"] > 0, active)                          # an inactive pixel has size 0, an active one >= 1
    keep = active & (ref["size"] > case.max_size)
    assert np.array_equal(ref["valid"], keep.astype(np.float32))
    assert np.array_equal(ref["disp"][keep].view(np.uint32), d[keep].view(np.uint32))
    assert np.array_equal(ref["disp"][~keep].view(np.uint32), np.zeros(int((~keep).sum()), np.uint32))      # +0.0
    filled = speckle_filter_host(case.d, case.max_size, case.max_diff, mask=case.mask, window=case.window, fill=-1.0)
    assert (filled["disp"][~keep] == -1).all() and np.array_equal(filled["valid"], ref["valid"])
    census = component_census(ref["size"], active)
    print(case.name, d.shape, census if len(census) < 12 else f"{len(census)} sizes", "kept", int(keep.sum()), "removed",
          int((active & ~keep).sum()))
    if case.sizes is not None:
        assert census == case.sizes
    only = speckle_filter_host(case.d, case.max_size, case.max_diff, mask=case.mask, window=case.window, outputs=("size",))
    assert set(only) == {"size", "valid"}


def test_speckle_closed_forms():
    by = {c.name: c for c in speckle_cases()}
    # the snake: one component through every vertical tile edge on every even row; its size in closed form
    H, W = 2 * TH + 3, 2 * TW + 5
    snake = (H + 1) // 2 * W + (H + 1) // 2 - 1
    for name in ("snake", "snake, rest masked"):
        c = by[name]
        ref = speckle_filter_host(c.d, c.max_size, c.max_diff, mask=c.mask)
        assert c.d.shape == (H, W) and (ref["size"][c.d == 10] == snake).all() and (ref["valid"][c.d == 10] == 1).all()
        assert not ref["valid"][c.d == 50].any()
        assert (ref["size"][c.d == 50] == (0 if c.mask is not None else W - 1)).all()
        gone = speckle_filter_host(c.d, snake, c.max_diff, mask=c.mask)       # size > max_size: the boundary
        assert not gone["valid"].any()
    # the constant frame: n - 1 keeps all, n removes all
    kept, removed = by["constant, kept"], by["constant, removed"]
    n = kept.d.size
    assert kept.max_size == n - 1 and removed.max_size == n and kept.d.shape == (3 * TH, 3 * TW + 1)
    assert speckle_filter_host(kept.d, n - 1, 0.0)["valid"].all() and not speckle_filter_host(kept.d, n, 0.0)["valid"].any()
    # the checkerboard: max_size 0 is the identity, 1 removes everything
    c = by["checkerboard, identity"]
    ident = speckle_filter_host(c.d, 0, 1.0)
    assert ident["valid"].all() and ident["disp"].tobytes() == c.d.tobytes() and (ident["size"] == 1).all()
    assert not speckle_filter_host(c.d, 1, 1.0)["valid"].any()
    # ramps: chained; columns; equality joins
    c = by["ramp 0.75, chained"]
    assert (speckle_filter_host(c.d, 0, 1.0)["size"] == c.d.size).all()
    c = by["ramp 1.25, columns"]
    assert (speckle_filter_host(c.d, 0, 1.0)["size"] == c.d.shape[0]).all()
    c = by["ramp 0.5, equality"]
    assert (speckle_filter_host(c.d, 0, 0.5)["size"] == c.d.size).all()
    assert (speckle_filter_host(c.d, 0, np.nextafter(np.float32(0.5), np.float32(0)))["size"] == c.d.shape[0]).all()
    # values that are no numbers are inactive; -0.0 is a number
    c = by["specials"]
    ref = speckle_filter_host(c.d, 0, 1.0, fill=-1.0)
    bad = ~np.isfinite(c.d)
    assert bad.sum() == 3 * c.d.shape[0]
    assert (ref["size"][bad] == 0).all() and (ref["valid"][bad] == 0).all() and (ref["disp"][bad] == -1).all()
    zero = np.signbit(c.d) & (c.d == 0)
    assert zero.sum() == c.d.shape[0] and (ref["size"][zero] == c.d.shape[0] * (c.d.shape[1] - 60)).all()
    assert np.array_equal(ref["disp"][zero].view(np.uint32), np.full(int(zero.sum()), 0x80000000, np.uint32))
    # the window: the padding around it joins its border pixels, and is never read
    c = by["window"]
    d, mask = scene(37, 83, 1)
    inside = speckle_filter_host(c.d, 50, 1.0, mask=c.mask, window=c.window)
    alone = speckle_filter_host(d, 50, 1.0, mask=mask)
    whole = speckle_filter_host(c.d, 50, 1.0, mask=c.mask)
    for k in alone:
        assert inside[k].tobytes() == alone[k].tobytes(), k
    y0, rows, cols = c.window
    assert (whole["size"][y0:y0 + rows, :cols] > inside["size"]).any(), "the padding does not join the window's border"


@pytest.mark.parametrize("case", speckle_cases(), ids=lambda c: c.name)
def test_speckle_restatement_against_scipy(case):
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    sparse = pytest.importorskip("scipy.sparse")
    d, active = _window_of(case)
    rows, cols = d.shape
    idx = np.arange(rows * cols).reshape(rows, cols)
    u, v = [], []
    with np.errstate(invalid="ignore", over="ignore"):
        for a, b in ((np.s_[:, :-1], np.s_[:, 1:]), (np.s_[:-1], np.s_[1:])):
            join = active[a] & active[b] & (np.abs(d[a] - d[b]) <= np.float32(case.max_diff))
            u.append(idx[a][join])
            v.append(idx[b][join])
    u, v = np.concatenate(u), np.concatenate(v)
    graph = sparse.coo_matrix((np.ones(len(u), np.int8), (u, v)), shape=(rows * cols,) * 2)
    _, comp = csgraph.connected_components(graph, directed=False)
    size = np.where(active, np.bincount(comp)[comp].reshape(rows, cols), 0).astype(np.int32)
    ref = speckle_filter_host(case.d, case.max_size, case.max_diff, mask=case.mask, window=case.window)
    assert np.array_equal(ref["size"], size)
    # a batch: the images are independent
    both = speckle_filter_host(flipped(case.d), case.max_size, case.max_diff, mask=flipped(case.mask), window=case.window)
    assert both["size"].shape == (2, rows, cols) and np.array_equal(both["size"][0], size)
    if case.window is None:
        assert np.array_equal(both["size"][1], size[:, ::-1])


def _median_brute(d, ksize, mask, window):
    y0, rows, cols = window if window is not None else (0,) + d.shape
    R = ksize // 2
    out = np.empty((rows, cols), np.float32)
    act = lambda r, c: bool(np.isfinite(d[y0 + r, c]) and (mask is None or mask[y0 + r, c] >= 0.5))
    evens = lonely = 0
    for r in range(rows):
        for c in range(cols):
            if not act(r, c):
                out[r, c] = d[y0 + r, c]
                continue
            cand = [d[y0 + rr, cc] for rr in range(max(r - R, 0), min(r + R, rows - 1) + 1)
                    for cc in range(max(c - R, 0), min(c + R, cols - 1) + 1) if act(rr, cc)]
            cand.sort(key=lambda v: int(order_key(np.float32(v).view(np.uint32))))
            out[r, c] = cand[(len(cand) - 1) // 2]
            evens += len(cand) % 2 == 0
            lonely += len(cand) == 1
    return out, evens, lonely


@pytest.mark.parametrize("ksize", [3, 5])
@pytest.mark.parametrize("case", median_cases(), ids=lambda c: c[0])
def test_median_restatement_against_brute_force(case, ksize):
    name, d, mask, window = case
    want, evens, lonely = _median_brute(d, ksize, mask, window)
    got = median_filter_host(d, ksize, mask=mask, window=window)
    assert got.dtype == np.float32 and got.shape == want.shape
    assert got.tobytes() == want.tobytes()                                  # NaN payloads and the zeros' signs included
    print(name, ksize, "even n:", evens, "single candidate:", lonely)
    assert evens > 0
    if name == "special 5x7":
        if ksize == 3:
            assert lonely > 0 and got[1, 3] == 9                            # all eight neighbours inactive: the centre itself
        assert np.signbit(got[got == 0]).any() and not np.signbit(got[got == 0]).all()
    batch = median_filter_host(flipped(d), ksize, mask=flipped(mask), window=window)
    assert batch.shape == (2,) + want.shape and batch[0].tobytes() == want.tobytes()


def test_order_key_is_a_total_order_with_minus_zero_below_plus_zero():
    v = np.array([-np.inf, -3.5, -1e-45, -0.0, 0.0, 1e-45, 2.0, np.inf], np.float32)
    k = order_key(v.view(np.uint32)).astype(np.int64)
    assert (np.diff(k) > 0).all()
    assert speckle_filter_host(np.zeros((1, 1), np.float32), 0, 0.0)["size"][0, 0] == 1


def test_postfilter_entry_points_are_bound_and_refuse_bad_arguments():
    """hipErrorInvalidValue (1) without touching a device"""
    from dcanet_amd import _lib, ops
    lib = _lib.load()
    assert ops.SPECKLE_TILE == (TH, TW) == (_lib.CONSTANTS["DCA_SPK_TILE_H"], _lib.CONSTANTS["DCA_SPK_TILE_W"])
    assert _lib.ABI_VERSION == 21 and lib.dca_abi_version() == 21
    for name in ("dca_speckle_filter", "dca_median_filter"):
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    p, q, r, s, t, u = (ctypes.c_void_p(16 * k) for k in range(1, 7))
    spk = lambda d=p, valid=r, label=t, count=u, B=1, Hc=8, Wc=8, y0=0, rows=8, cols=8, max_size=1, max_diff=1.0, mask=None, \
        mask_min=0.5: lib.dca_speckle_filter(d, mask, q, valid, s, label, count, B, Hc, Wc, y0, rows, cols, max_size, max_diff,
                                             mask_min, 0.0, None)
    for bad in (dict(d=None), dict(valid=None), dict(label=None), dict(count=None), dict(B=0), dict(B=65536), dict(Hc=0),
                dict(y0=-1), dict(y0=1), dict(rows=0), dict(cols=9), dict(cols=0), dict(max_size=-1), dict(max_diff=-0.5),
                dict(max_diff=math.nan), dict(max_diff=math.inf), dict(mask=q, mask_min=math.nan),
                dict(Hc=1 << 16, Wc=1 << 15, rows=8, cols=8)):
        assert spk(**bad) == 1, bad
    med = lambda d=p, out=q, B=1, Hc=8, Wc=8, y0=0, rows=8, cols=8, ksize=3, mask=None, mask_min=0.5: \
        lib.dca_median_filter(d, mask, out, B, Hc, Wc, y0, rows, cols, ksize, mask_min, None)
    for bad in (dict(d=None), dict(out=None), dict(out=p), dict(ksize=1), dict(ksize=4), dict(ksize=7), dict(B=0),
                dict(rows=9), dict(y0=4, rows=5), dict(cols=-1), dict(mask=r, mask_min=math.nan)):
        assert med(**bad) == 1, bad


def test_postfilter_operators_refuse_what_they_cannot_do():
    from dcanet_amd import ops
    a = torch.zeros(4, 8)
    for call in (lambda t, **kw: ops.speckle_filter(t, 10, 1.0, **kw), lambda t, **kw: ops.median_filter(t, 3, **kw)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call(a)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call(a.view(1, 1, 4, 8), window=(0, 4, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.speckle_filter(a.double(), 10, 1.0)
    with pytest.raises(RuntimeError):
        ops.speckle_workspace(0, 8, "cpu")
    with pytest.raises(RuntimeError):
        ops.speckle_workspace(1 << 16, 1 << 15, "cpu")
    with pytest.raises(RuntimeError, match="inference only"):
        ops.speckle_filter(a.clone().requires_grad_(), 10, 1.0)
    with pytest.raises(RuntimeError, match="inference only"):
        ops.median_filter(a.clone().requires_grad_(), 3)
    assert ops.SPECKLE_OUTPUTS == ("disp", "valid", "size")
    for bad in (dict(ksize=4), dict(ksize=1), dict(ksize=3, window=(0, 5, 8)), dict(ksize=3, mask_min=math.nan, mask=a)):
        with pytest.raises(ValueError):
            median_filter_host(a.numpy(), **bad)
    for bad in (dict(max_size=-1, max_diff=1.0), dict(max_size=1, max_diff=-1.0), dict(max_size=1, max_diff=math.nan),
                dict(max_size=1, max_diff=1.0, window=(2, 3, 8)), dict(max_size=1, max_diff=1.0, outputs=("nope",))):
        with pytest.raises(ValueError):
            speckle_filter_host(a.numpy(), **bad)
    with pytest.raises(ValueError):
        speckle_filter_host(a.double().numpy(), 1, 1.0)


def test_filtered_wrappers_host_logic():
    """KittiInferenceFiltered takes KittiInference's arguments plus the filters' and hands out two maps; the 3D and colour
    classes take `speckle=` and `median=` and leave them off by default"""
    from dcanet_amd.inference import KittiInference, KittiInference3D, KittiInferenceColor, KittiInferenceFiltered
    net = torch.nn.Linear(1, 1)
    net.maxdisp = 192
    f = KittiInferenceFiltered(net, 64, 128, graph=False, device_io=True)
    assert isinstance(f, KittiInference) and f.nmaps == 2 and (f.crop_height, f.crop_width) == (64, 128)
    assert f.speckle == (200, 2.0) and f.median == 0 and f.mask_mode is None and f.confidence is False
    g = KittiInferenceFiltered(net, median=5, speckle=None, mask="confidence", radius=2, device_io=True)
    assert g.median == 5 and g.speckle is None and g.confidence is True and g.radius == 2
    assert KittiInferenceFiltered(net, mask="lr", tau=2.0, device_io=True).tau == 2.0
    for bad in (dict(median=4), dict(median=1), dict(speckle=(200,)), dict(speckle=(-1, 2.0)), dict(speckle=(200, -1.0)),
                dict(speckle=(200, math.nan)), dict(speckle=(2.5, 1.0)), dict(mask="nope"), dict(mask_min=math.nan),
                dict(tau=-1.0), dict(radius=-1)):
        with pytest.raises(ValueError):
            KittiInferenceFiltered(net, device_io=True, **bad)
    with pytest.raises(ValueError):
        KittiInferenceFiltered(net, device_io=False)
    calib = type("C", (), dict(f=700.0, fb=380.0, cx=600.0, cy=180.0, doffs=0.0))()
    d3 = KittiInference3D(net, calib, device_io=True)
    assert d3.speckle is None and d3.median == 0
    d3 = KittiInference3D(net, calib, device_io=True, speckle=(100, 1.0), median=3)
    assert d3.speckle == (100, 1.0) and d3.median == 3 and d3.nmaps == 1
    col = KittiInferenceColor(net)
    assert col.speckle is None and col.median == 0
    assert KittiInferenceColor(net, speckle=(50, 1.5)).speckle == (50, 1.5)
    for cls, args in ((KittiInference3D, (net, calib)), (KittiInferenceColor, (net,))):
        for bad in (dict(median=2), dict(speckle=(1, 2, 3)), dict(speckle=(0, math.inf))):
            with pytest.raises(ValueError):
                cls(*args, device_io=True, **bad)
