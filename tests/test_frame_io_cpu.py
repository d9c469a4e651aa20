"""Host side of the device frame I/O (dcanet_amd.inference, csrc/frame_io.hip): the numpy restatement of the table
kernel against `normalize_pair`, the placement rule against `pad_or_crop`, the fixed ImageNet table against its torch
restatement, and what the library refuses without a GPU."""
import numpy as np
import pytest
import torch


def _ulp_distance(a, b):
    """distance in float32 representable values (finite inputs)"""
    def key(x):
        i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)      # sign-magnitude -> monotone integers; -0.0 and +0.0 coincide
    return np.abs(key(a) - key(b))


def _smooth(rs, h, w):
    y, x = np.mgrid[0:h, 0:w]
    img = np.stack([120 + 90 * np.sin(x / 37.0 + c) * np.cos(y / 23.0 - c) for c in range(3)], -1)
    return np.clip(img + rs.normal(0, 6, img.shape), 0, 255).astype(np.uint8)


def _images():
    rs = np.random.RandomState(5)
    for h, w in ((37, 121), (50, 100), (64, 128), (375, 1242), (400, 1300), (1, 7)):
        yield f"random {h}x{w}", rs.randint(0, 256, (h, w, 3)).astype(np.uint8), rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
    yield "low contrast", rs.randint(100, 104, (60, 90, 3)).astype(np.uint8), rs.randint(100, 104, (60, 90, 3)).astype(np.uint8)
    yield "smooth", _smooth(rs, 375, 1242), _smooth(rs, 375, 1242)
    near = (rs.rand(90, 140, 3) < 0.03).astype(np.uint8) * 255
    near2 = np.where(rs.rand(90, 140, 3) < 0.5, 1, 254).astype(np.uint8)
    yield "near binary", near, near2


def table_normalize(left, right):
    """`normalize_pair` through histogram -> lut_from_histogram -> look-up: what the three device kernels compute"""
    from dcanet_amd.inference import lut_from_histogram
    h, w = left.shape[:2]
    hist = np.stack([[np.bincount(img[:, :, c].ravel(), minlength=256) for c in range(3)] for img in (left, right)])
    lut, stats = lut_from_histogram(hist, h * w)
    out = np.stack([lut[i, c][img[:, :, c]] for i, img in enumerate((left, right)) for c in range(3)])
    return out, lut, stats


@pytest.mark.parametrize("name,left,right", list(_images()), ids=[n for n, _, _ in _images()])
def test_table_form_equals_normalize_pair_within_one_ulp(name, left, right):
    from dcanet_amd.inference import normalize_pair
    with np.errstate(all="ignore"):
        want = normalize_pair(left, right)
    got, lut, stats = table_normalize(left, right)
    assert got.dtype == np.float32 and got.shape == want.shape and lut.dtype == np.float32 and stats.dtype == np.float64
    assert np.array_equal(np.isnan(got), np.isnan(want))
    fin = np.isfinite(want)
    assert np.array_equal(fin, np.isfinite(got))
    d = _ulp_distance(got[fin], want[fin])
    print(f"{name}: max ulp distance {d.max() if d.size else 0}, {int((d > 0).sum())} of {d.size} elements differ")
    assert d.size == 0 or d.max() <= 1
    for i, img in enumerate((left, right)):
        for c in range(3):
            assert stats[i, c, 0] == np.mean(img[:, :, c])          # exact integer sum, one division


def test_constant_plane_is_nan_on_both_sides():
    from dcanet_amd.inference import normalize_pair
    rs = np.random.RandomState(1)
    left, right = rs.randint(0, 256, (20, 30, 3)).astype(np.uint8), rs.randint(0, 256, (20, 30, 3)).astype(np.uint8)
    left[:, :, 1] = 77
    with np.errstate(all="ignore"):
        want = normalize_pair(left, right)
    got, lut, stats = table_normalize(left, right)
    assert np.isnan(want[1]).all() and np.isnan(got[1]).all() and stats[0, 1, 1] == 0.0 and stats[0, 1, 0] == 77.0
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isfinite(got[[0, 2, 3, 4, 5]]).all()


PLACEMENTS = [(50, 100, 64, 128), (64, 128, 64, 128), (64, 100, 64, 128), (50, 128, 64, 128), (1, 7, 64, 128),
              (80, 150, 64, 128), (81, 128, 64, 128), (64, 150, 64, 128), (375, 1242, 384, 1248), (400, 1300, 384, 1248),
              (37, 121, 40, 123)]


@pytest.mark.parametrize("h,w,Hc,Wc", PLACEMENTS)
def test_placement_equals_pad_or_crop(h, w, Hc, Wc):
    from dcanet_amd.inference import crop_back, pad_or_crop, placement
    rs = np.random.RandomState(h * 1000 + w)
    data = rs.randn(6, h, w).astype(np.float32)
    left, right, h2, w2 = pad_or_crop(data, Hc, Wc)
    src_y0, dst_y0, rows, cols = placement(h, w, Hc, Wc)
    frame = np.zeros((6, Hc, Wc), np.float32)
    frame[:, dst_y0:dst_y0 + rows, 0:cols] = data[:, src_y0:src_y0 + rows, 0:cols]
    assert left.shape == (1, 3, Hc, Wc) and (h2, w2) == (h, w)
    assert frame[0:3].tobytes() == left.numpy()[0].tobytes() and frame[3:6].tobytes() == right.numpy()[0].tobytes()
    # the exported window (row dst_y0, rows x cols) is crop_back's
    disp = rs.rand(Hc, Wc).astype(np.float32)
    assert np.array_equal(disp[dst_y0:dst_y0 + rows, 0:cols], crop_back(disp, h, w, Hc, Wc))


@pytest.mark.parametrize("h,w", [(80, 100), (50, 150), (65, 127), (63, 129)])
def test_placement_refuses_mixed_cases(h, w):
    from dcanet_amd.inference import placement
    with pytest.raises(ValueError):
        placement(h, w, 64, 128)


def test_imagenet_lut_equals_torch_restatement():
    from dcanet_amd.inference import imagenet_lut
    lut = imagenet_lut()
    assert lut.shape == (2, 3, 256) and lut.dtype == torch.float32 and lut.is_contiguous() and torch.equal(lut[0], lut[1])
    rs = np.random.RandomState(2)
    img = torch.from_numpy(rs.randint(0, 256, (97, 131, 3)).astype(np.uint8))
    mean = torch.tensor([0.485, 0.456, 0.406]).view(3, 1, 1)
    std = torch.tensor([0.229, 0.224, 0.225]).view(3, 1, 1)
    want = img.permute(2, 0, 1).float().div(255).sub(mean).div(std)
    got = torch.stack([lut[0, c][img[:, :, c].long()] for c in range(3)])
    assert got.numpy().tobytes() == want.numpy().tobytes()


def test_library_refuses_bad_arguments_without_a_gpu():
    import ctypes
    from dcanet_amd import _lib
    lib = _lib.load()
    assert lib.dca_abi_version() == 21
    buf = (ctypes.c_char * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)           # a non-null host pointer: refused calls never touch it
    # null pointers
    assert lib.dca_frame_hist(None, None, None, 16, 32, 3, None) != 0
    assert lib.dca_frame_hist(p, p, None, 16, 32, 3, None) != 0
    assert lib.dca_frame_lut(None, 512, None, None, None) != 0
    assert lib.dca_frame_lut(p, 512, p, None, None) != 0
    assert lib.dca_frame_apply(None, None, None, None, None, 16, 32, 3, 16, 32, 0, 0, 16, 32, None) != 0
    assert lib.dca_disp_export(None, p, p, 16, 32, 0, 16, 32, 256.0, None) != 0
    assert lib.dca_disp_export(p, None, None, 16, 32, 0, 16, 32, 256.0, None) != 0       # nothing to write
    # channel counts, sizes
    assert lib.dca_frame_hist(p, p, p, 16, 32, 2, None) != 0 and lib.dca_frame_hist(p, p, p, 16, 32, 5, None) != 0
    assert lib.dca_frame_hist(p, p, p, 1 << 16, 1 << 15, 3, None) != 0                     # H W = 2^31
    assert lib.dca_frame_lut(p, 0, p, p, None) != 0
    assert lib.dca_frame_apply(p, p, p, p, p, 16, 32, 1, 16, 32, 0, 0, 16, 32, None) != 0
    # windows that do not fit the source or the frame
    for H, W, Hc, Wc, sy, dy, rows, cols in ((16, 32, 16, 32, 1, 0, 16, 32), (16, 32, 16, 32, 0, 1, 16, 32),
                                             (16, 32, 16, 32, 0, 0, 16, 33), (16, 32, 8, 32, 0, 0, 16, 32),
                                             (16, 32, 16, 16, 0, 0, 16, 32), (16, 32, 16, 32, -1, 0, 4, 4),
                                             (16, 32, 16, 32, 0, -1, 4, 4), (16, 32, 16, 32, 0, 0, -4, 4)):
        assert lib.dca_frame_apply(p, p, p, p, p, H, W, 3, Hc, Wc, sy, dy, rows, cols, None) != 0
    for Hc, Wc, y0, h, w in ((16, 32, 1, 16, 32), (16, 32, 0, 16, 33), (16, 32, -1, 4, 4), (16, 32, 0, 0, 4)):
        assert lib.dca_disp_export(p, p, p, Hc, Wc, y0, h, w, 256.0, None) != 0


def test_frame_ops_refuse_cpu_tensors():
    from dcanet_amd import ops
    img = torch.zeros(16, 32, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.frame_histogram(img, img)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.frame_lut(torch.zeros(2, 3, 256, dtype=torch.int32), 512)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.frame_apply(img, img, torch.zeros(2, 3, 256), (16, 32), 0, 0, 16, 32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.disp_export(torch.zeros(16, 32), 0, 16, 32)


def test_host_path_is_the_default_and_keeps_its_signature():
    import inspect
    from dcanet_amd.inference import KittiInference
    sig = inspect.signature(KittiInference.__init__)
    positional = [k for k, p in sig.parameters.items() if p.kind is p.POSITIONAL_OR_KEYWORD]
    assert positional[1:] == ["model", "crop_height", "crop_width", "graph", "dtype", "device_io"]
    assert [k for k in sig.parameters if k not in positional] == ["rectify"]       # keyword-only, None: no rectification
    assert sig.parameters["rectify"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["rectify"].default is None
    # device_io=None stands for the class's own default, which is the host path here
    assert sig.parameters["device_io"].default is None and KittiInference.device_io is False
    infer = KittiInference(torch.nn.Linear(1, 1))
    assert infer.device_io is False and KittiInference(torch.nn.Linear(1, 1), 384, 1248, True, None, True).device_io is True
    with pytest.raises(RuntimeError, match="device_io=True"):
        next(infer.stream([]))
