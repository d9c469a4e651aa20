"""dcanet_amd.training on the host: the numpy restatements of the reference's training loaders
(dataloader/datasets.py:221-317) pinned to what those loaders actually call -- PIL's enhancers, convert("L"), ImageStat,
`point`, numpy's mean -- and the draw helpers to the order in which the loaders consume the generators."""
import random

import numpy as np
import pytest
import torch
from PIL import Image, ImageEnhance, ImageStat


def _with_ramp(rs, h, w):
    """a small random image with a 256-value ramp appended, so every byte occurs in every channel"""
    img = rs.randint(0, 256, (h * w, 3)).astype(np.uint8)
    ramp = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, 1)
    return np.concatenate([img, ramp]).reshape(1, -1, 3)


def test_tables_equal_pil_enhancers():
    from dcanet_amd import training as T
    rs = np.random.RandomState(2024)
    bad = {"brightness": 0, "luma": 0, "mean": 0, "contrast": 0}
    factors = [(rs.uniform(0.5, 2.0), rs.uniform(0.8, 1.2)) for _ in range(300)] + [(1.0, 1.0), (0.5, 0.8), (2.0, 1.2)]
    for b, c in factors:
        img = _with_ramp(rs, int(rs.randint(3, 12)), int(rs.randint(3, 12)))
        pil = Image.fromarray(img)
        bright = ImageEnhance.Brightness(pil).enhance(b)
        got = T.brightness_table(b)[img]
        bad["brightness"] += int((np.asarray(bright) != got).sum())
        luma = np.asarray(bright.convert("L"))
        bad["luma"] += int((luma != T.luma_plane(img, T.brightness_table(b))).sum())
        mean = int(ImageStat.Stat(bright.convert("L")).mean[0] + 0.5)
        got_mean = T.contrast_mean(T.luma_sum(img, T.brightness_table(b)), luma.size)
        bad["mean"] += int(mean != got_mean)
        contrast = ImageEnhance.Contrast(bright).enhance(c)
        bad["contrast"] += int((np.asarray(contrast) != T.contrast_table(got_mean, c)[got]).sum())
    print(bad)
    assert bad == {"brightness": 0, "luma": 0, "mean": 0, "contrast": 0}


def test_blend_table_outside_unit_interval_and_at_its_ends():
    from dcanet_amd import training as T
    v = np.arange(256)
    assert np.array_equal(T.blend_table(77, 1.0), v) and np.array_equal(T.blend_table(77, 0.0), np.full(256, 77))
    assert np.array_equal(T.blend_table(0, 2.0), np.minimum(2 * v, 255))
    assert np.array_equal(T.blend_table(255, 2.0), np.maximum(2 * v - 255, 0))
    for c, f in ((0, 1.7), (255, 1.15), (128, 1.2), (128, 0.8), (0, 0.5)):
        pil = Image.fromarray(v.astype(np.uint8)[None])
        want = np.asarray(Image.blend(Image.new("L", pil.size, c), pil, f))[0]
        assert np.array_equal(T.blend_table(c, f), want), (c, f)


def test_gamma_table_is_the_stated_formula():
    from dcanet_amd import training as T
    for gamma in (0.8, 1.0, 1.2, 0.9371):
        want = [int((255 + 1 - 1e-3) * 1 * pow(v / 255.0, gamma)) for v in range(256)]
        assert T.gamma_table(gamma).tolist() == want and T.gamma_table(gamma).dtype == np.uint8
    assert T.gamma_table(1.0).tolist() == list(range(256))
    assert T.gamma_table(1.0, gain=2.0).max() == 255


@pytest.mark.parametrize("th,tw,n", [(16, 32, 200), (24, 40, 200), (256, 512, 200), (320, 704, 200)])
def test_patch_bytes_equals_the_reference_expression(th, tw, n):
    from dcanet_amd import training as T
    rs = np.random.RandomState(th + tw)
    bad = 0
    for k in range(n):
        crop = rs.randint(0, 256, (th, tw, 3)).astype(np.uint8)
        if k % 4 == 1:
            crop[:, :, k % 3] = rs.randint(0, 256)                 # a constant plane: the mean is an exact integer
        if k % 4 == 2:
            crop[:] = rs.randint(0, 256, 3).astype(np.uint8)       # all three
        if k % 8 == 3:
            crop = np.sort(crop, axis=0)                           # columns with very different means
        want = np.zeros((1, 1, 3), np.uint8)
        want[0:1, 0:1] = np.mean(np.mean(crop, 0), 0)[np.newaxis, np.newaxis]      # datasets.py:306
        bad += int((T.patch_bytes(crop) != want[0, 0]).any())
    print(f"{th}x{tw}: {bad} of {n} differ")
    assert bad == 0


def _exact_mean_crop(rs, th, tw):
    """a random crop whose three channel sums are multiples of th * tw: the mean is an exact integer"""
    crop = rs.randint(1, 256, (th, tw, 3)).astype(np.uint8)
    n = th * tw
    for ch in range(3):
        r = int(crop[:, :, ch].astype(np.int64).sum() % n)
        plane = crop[:, :, ch].reshape(-1)
        plane[rs.permutation(n)[:r]] -= 1                          # every value is >= 1
        assert crop[:, :, ch].astype(np.int64).sum() % n == 0
    return crop


@pytest.mark.parametrize("th,tw,exact", [(16, 32, True), (256, 512, True), (64, 100, True), (24, 40, False), (31, 45, False)])
def test_patch_bytes_at_exact_integer_means(th, tw, exact):
    """`patch_bytes` and the kernel follow the EXACT mean, floor(sum / (th tw)).  The loader's fp64 mean of column means
    equals it whenever th is a power of two (every column mean k / th is exact, at the reference's 256 x 512 for one);
    at other heights the rounded column means can add up to just below an exact-integer mean, and the loader's
    truncation then gives one less.  That is the only way the two differ."""
    from dcanet_amd import training as T
    rs = np.random.RandomState(th * tw)
    differ = 0
    for _ in range(60 if th * tw > 10000 else 300):
        crop = _exact_mean_crop(rs, th, tw)
        loader = np.zeros(3, np.uint8)
        loader[:] = np.mean(np.mean(crop, 0), 0)
        got = T.patch_bytes(crop)
        assert got.tolist() == (crop.reshape(-1, 3).astype(np.int64).sum(0) // (th * tw)).tolist()
        d = got.astype(np.int64) - loader.astype(np.int64)
        assert ((d == 0) | (d == 1)).all()
        differ += int(d.any())
    print(f"{th}x{tw}: the loader's fp64 mean is one below the exact integer mean in {differ} crops")
    if exact:
        assert differ == 0
    else:
        assert differ > 0                                          # 187 of 300 at 24x40, 214 of 300 at 31x45


def _pil_kitti_sample(left, right, disp_u16, p, th, tw):
    """datasets.py:282-315 written with the PIL calls torchvision's functional transforms make"""
    from dcanet_amd import training as T
    mean = torch.tensor([0.485, 0.456, 0.406], dtype=torch.float32).view(3, 1, 1)
    std = torch.tensor([0.229, 0.224, 0.225], dtype=torch.float32).view(3, 1, 1)
    out = []
    for i, arr in enumerate((left, right)):
        img = Image.fromarray(arr)
        img = ImageEnhance.Brightness(img).enhance(p.brightness[i])
        img = img.point(T.gamma_table(p.gamma[i]).tolist() * 3)
        img = ImageEnhance.Contrast(img).enhance(p.contrast[i])
        img = np.array(img.crop((p.x1, p.y1, p.x1 + tw, p.y1 + th)))
        if i == 1 and p.patch is not None:
            r0, r1, c0, c1 = p.patch
            img[r0:r1, c0:c1] = np.mean(np.mean(img, 0), 0)[np.newaxis, np.newaxis]
        t = torch.from_numpy(img).permute(2, 0, 1).contiguous().float().div(255)       # ToTensor
        out.append(t.sub_(mean).div_(std).numpy())                                     # Normalize
    gt = (np.ascontiguousarray(disp_u16, dtype=np.float32) / 256)[p.y1:p.y1 + th, p.x1:p.x1 + tw]
    return out[0], out[1], gt


@pytest.mark.parametrize("seed", range(6))
def test_host_sample_equals_the_pil_pipeline_bitwise(seed):
    from dcanet_amd import training as T
    rs = np.random.RandomState(100 + seed)
    h, w, th, tw = 61 + seed, 97 + 3 * seed, 32, 48
    left = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
    right = np.clip(left.astype(np.int64) + rs.randint(-9, 10, (h, w, 3)), 0, 255).astype(np.uint8)
    disp = rs.randint(0, 256 * 80, (h, w)).astype(np.uint16)
    disp[rs.rand(h, w) < 0.3] = 0
    patch = None if seed % 2 else (3, 20, 10, 41)
    if seed == 4:
        patch = (0, th, 0, tw)
    p = T.AugParams(x1=int(rs.randint(0, w - tw + 1)), y1=int(rs.randint(0, h - th + 1)),
                    brightness=tuple(rs.uniform(0.5, 2.0, 2)), gamma=tuple(rs.uniform(0.8, 1.2, 2)),
                    contrast=tuple(rs.uniform(0.8, 1.2, 2)), patch=patch)
    gl, gr, gt, mask = T.host_sample(left, right, disp, p, (th, tw), 64, "kitti")
    wl, wr, wgt = _pil_kitti_sample(left, right, disp, p, th, tw)
    assert gl.dtype == gr.dtype == gt.dtype == np.float32 and mask.dtype == np.bool_
    assert gl.tobytes() == wl.tobytes() and gr.tobytes() == wr.tobytes() and gt.tobytes() == wgt.tobytes()
    t = torch.from_numpy(wgt)
    assert np.array_equal(mask, ((t < 64) & (t > 0)).numpy()) and 0 < mask.sum() < mask.size
    # the SceneFlow loader: crop, ToTensor, Normalize; the PFM payload is bottom-up
    pfm = rs.rand(h, w).astype(np.float32) * 90
    sl, sr, sgt, smask = T.host_sample(left, right, pfm, T.AugParams(p.x1, p.y1), (th, tw), 64, "sceneflow", flip_rows=True)
    mean = torch.tensor([0.485, 0.456, 0.406]).view(3, 1, 1)
    std = torch.tensor([0.229, 0.224, 0.225]).view(3, 1, 1)
    for got, arr in ((sl, left), (sr, right)):
        c = torch.from_numpy(arr[p.y1:p.y1 + th, p.x1:p.x1 + tw].copy()).permute(2, 0, 1).contiguous().float().div(255)
        assert got.tobytes() == c.sub_(mean).div_(std).numpy().tobytes()
    assert np.array_equal(sgt, np.flipud(pfm)[p.y1:p.y1 + th, p.x1:p.x1 + tw])
    assert np.array_equal(smask, (sgt > 0) & (sgt < 64))


def test_crop_disparity_special_values():
    from dcanet_amd import training as T
    d = np.array([[0.0, 32.0, -1.0, np.inf, np.nan, 31.999998, 1e-30, -np.inf]], np.float32)
    g, m = T.crop_disparity(d, 0, 0, 1, 8, 32)
    assert g.tobytes() == d.tobytes() and m.tolist() == [[False, False, False, False, False, True, True, False]]
    g, m = T.crop_disparity(d, 0, 0, 1, 8, 32, inf_to_zero=True)
    assert g[0, 3] == 0 and np.isneginf(g[0, 7]) and not m[0, 3]
    u = np.array([[0, 1, 255, 256, 8191, 8192, 65535]], np.uint16)
    g, m = T.crop_disparity(u, 0, 0, 1, 7, 32, scale=1 / 256)
    assert g.tolist() == [[0, 1 / 256, 255 / 256, 1, 8191 / 256, 32, 65535 / 256]]
    assert m.tolist() == [[False, True, True, True, True, False, False]]
    with pytest.raises(ValueError):
        T.crop_disparity(u, 0, 1, 1, 7, 32)


def test_draw_helpers_consume_the_generators_in_the_reference_order():
    from dcanet_amd import training as T
    hits = 0
    for seed in range(40):
        nr, pr = np.random.RandomState(seed), random.Random(seed)
        p = T.draw_kitti(1242, 375, (256, 512), nr, pr)
        nr2, pr2 = np.random.RandomState(seed), random.Random(seed)
        b, g, c = nr2.uniform(0.5, 2.0, 2), nr2.uniform(0.8, 1.2, 2), nr2.uniform(0.8, 1.2, 2)
        x1, y1 = pr2.randint(0, 1242 - 512), pr2.randint(0, 375 - 256)
        patch = None
        if nr2.binomial(1, 0.2):
            sx, sy = int(nr2.uniform(35, 100)), int(nr2.uniform(25, 75))
            cx, cy = int(nr2.uniform(sx, 256 - sx)), int(nr2.uniform(sy, 512 - sy))
            patch = (cx - sx, cx + sx, cy - sy, cy + sy)
            hits += 1
        assert (p.x1, p.y1, p.patch) == (x1, y1, patch)
        assert p.brightness == tuple(b) and p.gamma == tuple(g) and p.contrast == tuple(c)
        assert nr.uniform() == nr2.uniform() and pr.random() == pr2.random()        # nothing more, nothing less was drawn
        assert 0 <= p.x1 <= 1242 - 512 and 0 <= p.y1 <= 375 - 256
        if p.patch is not None:
            r0, r1, c0, c1 = p.patch
            assert 0 <= r0 < r1 <= 256 and 0 <= c0 < c1 <= 512
        pr3 = random.Random(seed)
        s = T.draw_sceneflow(960, 540, (256, 512), pr3)
        pr4 = random.Random(seed)
        assert (s.x1, s.y1) == (pr4.randint(0, 960 - 512), pr4.randint(0, 540 - 256)) and pr3.random() == pr4.random()
        assert s.patch is None and s.brightness == s.gamma == s.contrast == (1.0, 1.0)
    assert 2 <= hits <= 20


def test_train_input_host_path_and_package_export():
    import dcanet_amd
    from dcanet_amd import training as T
    assert dcanet_amd.training is T
    rs = np.random.RandomState(1)
    ti = T.TrainInput(2, crop=(16, 24), maxdisp=32, kind="kitti")
    samples = []
    for b, (h, w) in enumerate(((30, 40), (25, 33))):
        left, right = rs.randint(0, 256, (h, w, 3)).astype(np.uint8), rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
        disp = rs.randint(0, 256 * 40, (h, w)).astype(np.uint16)
        p = T.draw_kitti(w, h, (16, 24), np.random.RandomState(b), random.Random(b))
        samples.append((left, right, disp, p))
    with pytest.raises(RuntimeError, match="not loaded"):
        ti.batch()
    for b, s in enumerate(samples):
        ti.load(b, *s)
    imgL, imgR, gt, mask = ti.batch()
    assert imgL.shape == imgR.shape == (2, 3, 16, 24) and gt.shape == mask.shape == (2, 16, 24) and mask.dtype == torch.bool
    for b, s in enumerate(samples):
        l, r, g, m = T.host_sample(*s, (16, 24), 32, "kitti")
        assert imgL[b].numpy().tobytes() == l.tobytes() and imgR[b].numpy().tobytes() == r.tobytes()
        assert gt[b].numpy().tobytes() == g.tobytes() and np.array_equal(mask[b].numpy(), m)
    with pytest.raises(ValueError):
        ti.load(0, samples[0][0], samples[0][1], samples[0][2], T.AugParams(x1=30, y1=0))


def test_launchers_refuse_bad_geometry_before_any_launch():
    """the window / patch / size checks of the C ABI return hipErrorInvalidValue (1) without touching a device"""
    import ctypes
    from dcanet_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(16)
    assert lib.dca_train_crop_norm(p, p, p, None, None, p, p, 20, 30, 3, 13, 0, 8, 16, 0, 0, 0, 0, None) == 1    # rows
    assert lib.dca_train_crop_norm(p, p, p, None, None, p, p, 20, 30, 3, 0, 15, 8, 16, 0, 0, 0, 0, None) == 1    # columns
    assert lib.dca_train_crop_norm(p, p, p, p, p, p, p, 20, 30, 3, 0, 0, 8, 16, 0, 0, 9, 4, None) == 1           # patch
    assert lib.dca_train_crop_norm(p, p, p, None, None, p, p, 20, 30, 3, 0, 0, 8, 16, 0, 0, 2, 2, None) == 1    # no colour
    assert lib.dca_train_crop_norm(p, p, p, None, None, p, p, 20, 30, 5, 0, 0, 8, 16, 0, 0, 0, 0, None) == 1    # C
    assert lib.dca_train_disp_crop(p, 0, p, p, 20, 30, 0, 15, 8, 16, 0, 1.0, 0, 32.0, None) == 1
    assert lib.dca_train_disp_crop(p, 0, p, p, 20, 30, -1, 0, 8, 16, 0, 1.0, 0, 32.0, None) == 1
    assert lib.dca_train_patch_colour(p, p, p, p, 20, 30, 3, 0, 0, 21, 4, None) == 1
    assert lib.dca_train_luma_sum(p, p, p, p, 0, 30, 3, None) == 1
    assert lib.dca_train_luma_sum(p, p, p, p, 1 << 16, 1 << 15, 3, None) == 1                                 # H W >= 2^31
    assert lib.dca_train_tables(p, 0, p, 1.0, 1.0, p, p, p, None) == 1
    assert lib.dca_train_tables(p, 10, p, float("nan"), 1.0, p, p, p, None) == 1
    assert lib.dca_train_tables(p, 10, p, 1.0, float("inf"), p, p, p, None) == 1          # inf * 0 in the blend would be NaN
    assert lib.dca_train_tables(p, 10, p, float("-inf"), 1.0, p, p, p, None) == 1
