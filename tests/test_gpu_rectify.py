"""Rectification on the MI355X (csrc/rectify.hip, ops.rectify_pair, KittiInference(rectify=)): the kernel
against the numpy restatement of tests/_rectify_reference.py bit for bit, its argument checks, its replay from a hipGraph, and
the way through the inference classes -- a raw pair with rectify= against the host-rectified pair without."""
import numpy as np
import pytest
import torch

import _rectify_reference as REF
from oracle import dcanet_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _maps(case):
    """the package's maps of a shared case, built by the constructor a user would call"""
    from dcanet_amd.geometry import RectifyMaps
    src, dst, c, kind = case
    if kind == "kitti":
        return RectifyMaps.from_kitti_raw(REF.kitti_raw_text())
    X, Y, mats = REF.case_maps(case)
    return RectifyMaps.from_fixed(X, Y, src) if mats is None else RectifyMaps.from_matrices(*mats, src, dst)


def _bytes(t):
    return t.cpu().numpy().tobytes()


# ---- the kernel ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", REF.CASES, ids=REF.case_id)
def test_rectify_pair_equals_the_reference_bitwise(case):
    """both views; fresh outputs, `out=` (sentinel bytes around it stay), an input and an output at byte offset 1 (the scalar
    path), and a second call (no atomics: equal bytes)"""
    from dcanet_amd import ops
    src, dst, c, kind = case
    maps = _maps(case)
    left, right = REF.case_images(case)
    want = REF.remap_pair(left, right, maps.X, maps.Y)
    L, R = _dev(left), _dev(right)
    got = ops.rectify_pair(L, R, maps)
    assert len(got) == 2
    for g, w in zip(got, want):
        assert g.dtype == torch.uint8 and tuple(g.shape) == dst + (c,) and _bytes(g) == w.tobytes()
    again = ops.rectify_pair(L, R, maps)
    assert _bytes(again[0]) == _bytes(got[0]) and _bytes(again[1]) == _bytes(got[1])
    n = dst[0] * dst[1] * c
    # out= as one (2,Hd,Wd,C) buffer inside a larger one filled with a sentinel
    flat = torch.full((2 * n + 32,), 77, dtype=torch.uint8, device=DEV)
    out = flat[16:16 + 2 * n].view(2, *dst, c)
    ol, orr = ops.rectify_pair(L, R, maps, out=out)
    assert ol.data_ptr() == out.data_ptr() and orr.data_ptr() == out[1].data_ptr()
    assert _bytes(out[0]) == want[0].tobytes() and _bytes(out[1]) == want[1].tobytes()
    assert (flat[:16] == 77).all() and (flat[16 + 2 * n:] == 77).all()
    # bases that are not 16-byte (not even 4-byte) aligned: inputs and outputs at byte offset 1
    m = left.size
    fin = torch.zeros(2 * m + 64, dtype=torch.uint8, device=DEV)
    fin[1:1 + m] = L.view(-1)
    fin[m + 7:2 * m + 7] = R.view(-1)
    lv, rv = fin[1:1 + m].view(*src, c), fin[m + 7:2 * m + 7].view(*src, c)
    fout = torch.full((2 * n + 64,), 77, dtype=torch.uint8, device=DEV)
    off = ((n + 8) & ~3) + 1
    o0, o1 = fout[1:1 + n].view(*dst, c), fout[off:off + n].view(*dst, c)
    assert lv.data_ptr() % 16 and o0.data_ptr() % 4 == 1 and o1.data_ptr() % 4 == 1
    ops.rectify_pair(lv, rv, maps, out=(o0, o1))
    assert _bytes(o0) == want[0].tobytes() and _bytes(o1) == want[1].tobytes()
    assert fout[0] == 77 and (fout[1 + n:off] == 77).all() and (fout[off + n:] == 77).all()


def test_rectify_pair_refuses_before_launch():
    from dcanet_amd import ops
    from dcanet_amd.geometry import RectifyMaps
    case = REF.CASES[0]
    maps = _maps(case)
    left, right = REF.case_images(case)
    L, R = _dev(left), _dev(right)
    with pytest.raises(RuntimeError, match="rectify_pair"):
        ops.rectify_pair(L[:-1].contiguous(), R[:-1].contiguous(), maps)                    # not the maps' source size
    with pytest.raises(RuntimeError, match="rectify_pair"):
        ops.rectify_pair(L[..., :2].contiguous(), R[..., :2].contiguous(), maps)             # C = 2
    with pytest.raises(RuntimeError, match="rectify_pair"):
        ops.rectify_pair(L, torch.from_numpy(right), maps)                                   # a CPU tensor
    with pytest.raises(RuntimeError, match="rectify_pair"):
        ops.rectify_pair(L, R[:, ::2], maps)                                                 # not contiguous
    with pytest.raises(RuntimeError, match="rectify_pair"):
        ops.rectify_pair(L.int(), R.int(), maps)                                             # dtype
    with pytest.raises(RuntimeError, match="rectify_pair"):
        ops.rectify_pair(L, R, (maps.X, maps.Y))                                             # not a RectifyMaps
    # aliasing: an identity-sized map whose output could be the input
    same = RectifyMaps.from_fixed(np.zeros((2, 37, 53), np.int32), np.zeros((2, 37, 53), np.int32), (37, 53))
    with pytest.raises(RuntimeError, match="alias"):
        ops.rectify_pair(L, R, same, out=(L, torch.empty_like(R)))
    with pytest.raises(RuntimeError, match="alias"):
        ops.rectify_pair(L, R, same, out=(torch.empty_like(L), R))
    buf = torch.empty((37, 53, 3), dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="alias"):
        ops.rectify_pair(L, R, same, out=(buf, buf))
    with pytest.raises(RuntimeError, match="rectify_pair"):
        ops.rectify_pair(L, R, maps, out=torch.empty((2, 29, 45, 4), dtype=torch.uint8, device=DEV))      # wrong shape
    torch.cuda.synchronize()


def test_rectify_pair_replays_from_a_hipgraph():
    from dcanet_amd import ops
    case = REF.CASES[0]
    src, dst, c, _ = case
    maps = _maps(case)
    rs = np.random.RandomState(31)
    L = torch.empty(src + (c,), dtype=torch.uint8, device=DEV)
    R = torch.empty(src + (c,), dtype=torch.uint8, device=DEV)
    out = torch.zeros((2,) + dst + (c,), dtype=torch.uint8, device=DEV)
    first = rs.randint(0, 256, (2,) + src + (c,)).astype(np.uint8)
    L.copy_(_dev(first[0])), R.copy_(_dev(first[1]))
    ops.rectify_pair(L, R, maps, out=out)                    # uploads the maps: nothing is allocated from here on
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.rectify_pair(L, R, maps, out=out)
    for _ in range(2):
        pair = rs.randint(0, 256, (2,) + src + (c,)).astype(np.uint8)
        L.copy_(_dev(pair[0])), R.copy_(_dev(pair[1]))
        out.zero_()
        g.replay()
        want = REF.remap_pair(pair[0], pair[1], maps.X, maps.Y)
        assert _bytes(out[0]) == want[0].tobytes() and _bytes(out[1]) == want[1].tobytes()
        eager = ops.rectify_pair(L, R, maps)
        assert _bytes(eager[0]) == want[0].tobytes() and _bytes(eager[1]) == want[1].tobytes()


# ---- the inference classes ---------------------------------------------------------------------------------------------------------
RAW, RECT, FRAME = (70, 140), (60, 120), dict(crop_height=64, crop_width=128)
_MODEL = []


def _model():
    if not _MODEL:
        from dcanet_amd.models.gwcnet_dca_g import GwcNet
        m = GwcNet(32)
        m.load_state_dict(O.seeded_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}), strict=True)
        _MODEL.append(m.to(DEV).eval())
    return _MODEL[0]


def _wrap_maps():
    from dcanet_amd.geometry import RectifyMaps
    return RectifyMaps.from_matrices(*REF.smooth_matrices(RAW, RECT), RAW, RECT)


def _raw_pairs(seed, n):
    rng = np.random.default_rng(seed)
    return [(rng.integers(0, 256, RAW + (3,), dtype=np.uint8), rng.integers(0, 256, RAW + (3,), dtype=np.uint8)) for _ in range(n)]


@pytest.mark.timeout(900)
def test_kitti_inference_with_rectify_equals_host_rectified_input(monkeypatch):
    """raw pair + rectify= == reference-rectified pair without, bit for bit: both feed identical bytes to identical launches"""
    from dcanet_amd.geometry import RectifyMaps
    from dcanet_amd.inference import KittiInference
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)      # MIOpen convolutions of the 2D networks; restored
    model, maps = _model(), _wrap_maps()
    assert 0.3 < maps.valid.mean() < 1.0
    with_rect = KittiInference(model, device_io=True, rectify=maps, **FRAME)
    plain = KittiInference(model, device_io=True, **FRAME)
    pairs = _raw_pairs(3, 3)
    refs = [REF.remap_pair(l, r, maps.X, maps.Y) for l, r in pairs]
    want = [plain(*ref) for ref in refs]
    assert want[0].shape == RECT and want[0].std() > 0.1 and not np.array_equal(want[0], want[1])
    for (l, r), w in zip(pairs, want):
        got = with_rect(l, r)
        assert got.shape == RECT and got.dtype == np.float32 and got.tobytes() == w.tobytes()
    got16 = with_rect(*pairs[0], as_uint16=True)
    assert got16.dtype == np.uint16 and np.array_equal(got16, plain(*refs[0], as_uint16=True))
    for depth in (2, 1):
        for g, w in zip(with_rect.stream(iter(pairs), depth=depth), want):
            assert g.tobytes() == w.tobytes()
    for g, ref in zip(with_rect.stream(pairs, depth=2, as_uint16=True), refs):
        assert g.dtype == np.uint16 and np.array_equal(g, plain(*ref, as_uint16=True))
    # a four-channel raw pair: the fourth channel is ignored by everything behind
    l4, r4 = (np.concatenate([a, np.full(RAW + (1,), 9, np.uint8)], 2) for a in pairs[0])
    assert with_rect(l4, r4).tobytes() == want[0].tobytes()
    # the host path rectifies with the numpy restatement
    host = KittiInference(model, rectify=maps, **FRAME)
    assert host(*pairs[0]).tobytes() == KittiInference(model, **FRAME)(*refs[0]).tobytes()
    # the identity map changes nothing
    K, D, Rr, P = REF.identity_matrices(RECT)
    ident = KittiInference(model, device_io=True, rectify=RectifyMaps.from_matrices(K, D, Rr, P, RECT, RECT), **FRAME)
    assert ident(*refs[0]).tobytes() == want[0].tobytes()
    with pytest.raises(ValueError, match="70 x 140"):
        with_rect(*refs[0])                                  # an already rectified pair: not the maps' source size
    assert plain(*refs[1]).tobytes() == want[1].tobytes()    # the un-rectified path is what it was


@pytest.mark.timeout(900)
def test_kitti_inference_3d_with_rectify_masks_invalid_pixels(monkeypatch):
    from dcanet_amd import ops
    from dcanet_amd.geometry import PLY_VERTEX
    from dcanet_amd.inference import KittiInference3D, placement
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    model, maps = _model(), _wrap_maps()
    calib = maps.calib
    l, r = _raw_pairs(9, 1)[0]
    ref_l, ref_r = REF.remap_pair(l, r, maps.X, maps.Y)
    plain = KittiInference3D(model, calib, mask=None, device_io=True, **FRAME)(ref_l, ref_r)
    # no mask to split the pixels: the depth of the median disparity does
    kw = dict(max_depth=float(np.float32(calib.fb) / np.float32(np.median(plain.disp))))
    plain = KittiInference3D(model, calib, mask=None, device_io=True, **kw, **FRAME)(ref_l, ref_r)
    assert 0 < len(plain.vertices) < RECT[0] * RECT[1]
    got = KittiInference3D(model, calib, mask=None, device_io=True, rectify=maps, **kw, **FRAME)(l, r)
    valid = maps.valid[0].astype(bool)
    assert got.mask is None and got.disp.tobytes() == plain.disp.tobytes()                   # handed out unmasked
    assert (got.depth[~valid] == 0).all()
    assert got.depth.tobytes() == np.where(valid, plain.depth, np.float32(0)).tobytes()
    keep = (plain.depth > 0) & valid
    assert 0 < keep.sum() < (plain.depth > 0).sum()
    # the records are those of the unmasked cloud at the valid pixels, in order; colours from the rectified left image
    assert got.vertices.dtype == PLY_VERTEX
    assert got.vertices.tobytes() == plain.vertices[valid[plain.depth > 0]].tobytes()
    rr, cc = np.nonzero(keep)
    for j, name in enumerate(("red", "green", "blue")):
        assert np.array_equal(got.vertices[name], ref_l[rr, cc, j])
    # the count of the operator itself with the valid map passed as the mask
    src_y0, dst_y0, rows, cols = placement(*RECT, 64, 128)
    pred = torch.zeros((64, 128), device=DEV)
    pred[dst_y0:dst_y0 + rows, :cols] = _dev(plain.disp)
    vmask = torch.zeros((64, 128), device=DEV)
    vmask[dst_y0:dst_y0 + rows, :cols] = _dev(maps.valid[0].astype(np.float32))
    _, count, _ = ops.point_cloud(pred, calib, _dev(ref_l), vmask, (dst_y0, rows, cols), v0=src_y0, **kw)
    assert int(count[0]) == len(got.vertices) == int(keep.sum())
    # calib defaults to the maps' own; without either, and with a mask_min that lets validity 0 through, it is refused
    assert KittiInference3D(model, rectify=maps, device_io=True, **FRAME).calib == maps.calib
    with pytest.raises(ValueError, match="calib"):
        KittiInference3D(model, device_io=True, **FRAME)
    with pytest.raises(ValueError, match="mask_min"):
        KittiInference3D(model, rectify=maps, device_io=True, mask_min=0.0, **FRAME)
