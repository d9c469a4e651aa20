"""Training inputs on the MI355X (csrc/train_io.hip, dcanet_amd.training): every kernel bitwise against its numpy
restatement, TrainInput(device_io=True) against the host path, the kernels of one sample inside a hipGraph, and TrainStep
against the reference's literal training loop."""
import copy
import random

import numpy as np
import pytest
import torch

from oracle import dcanet_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _pair(rs, h, w, c=3):
    return rs.randint(0, 256, (h, w, c)).astype(np.uint8), rs.randint(0, 256, (h, w, c)).astype(np.uint8)


def _bg(rs):
    from dcanet_amd import training as T
    p = T.AugParams(0, 0, tuple(rs.uniform(0.5, 2.0, 2)), tuple(rs.uniform(0.8, 1.2, 2)), tuple(rs.uniform(0.8, 1.2, 2)))
    return T.photometric_tables(p), p


# ---- luma sum --------------------------------------------------------------------------------------------------------------
# 48-byte vector groups: 37*121*3 = 279 groups + 39 bytes; 40x64x4 has only whole groups; 1x7 has none
@pytest.mark.parametrize("h,w,c", [(37, 121, 3), (40, 64, 4), (1, 7, 3), (37, 121, 4), (200, 333, 3)])
def test_luma_sum_equals_numpy(h, w, c):
    from dcanet_amd import ops, training as T
    rs = np.random.RandomState(h + w + c)
    left, right = _pair(rs, h, w, c)
    bg, _ = _bg(rs)
    got = ops.train_luma_sum(_dev(left), _dev(right), _dev(bg))
    assert got.dtype == torch.int64 and got.tolist() == [T.luma_sum(left, bg[0]), T.luma_sum(right, bg[1])]
    assert torch.equal(got, ops.train_luma_sum(_dev(left), _dev(right), _dev(bg)))


def test_luma_sum_unaligned_base_single_value_and_no_32_bit_overflow():
    from dcanet_amd import ops, training as T
    rs = np.random.RandomState(5)
    ident = np.stack([np.arange(256, dtype=np.uint8)] * 2)
    l2, r2 = _pair(rs, 37, 121)
    n = l2.size
    flat = torch.zeros(2 * n + 64, dtype=torch.uint8, device=DEV)
    flat[1:1 + n] = _dev(l2).view(-1)
    flat[n + 7:2 * n + 7] = _dev(r2).view(-1)
    lv, rv = flat[1:1 + n].view(37, 121, 3), flat[n + 7:2 * n + 7].view(37, 121, 3)
    assert lv.data_ptr() % 16 and rv.data_ptr() % 16
    bg, _ = _bg(rs)
    assert ops.train_luma_sum(lv, rv, _dev(bg)).tolist() == [T.luma_sum(l2, bg[0]), T.luma_sum(r2, bg[1])]
    one = np.full((50, 70, 3), 93, np.uint8)
    assert ops.train_luma_sum(_dev(one), _dev(l2[:1, :7].repeat(50, 0).repeat(10, 1)), _dev(bg))[0].item() == \
        50 * 70 * int(T.luma_plane(one[:1, :1], bg[0])[0, 0])
    white = np.full((375, 1242, 3), 255, np.uint8)                      # 375 * 1242 * 255 = 118 766 250 per image ...
    big = np.full((3000, 6000, 3), 255, np.uint8)                       # ... and 4.59e9 > 2^32 here
    white, big, ident = _dev(white), _dev(big), _dev(ident)
    assert ops.train_luma_sum(white, white, ident).tolist() == [375 * 1242 * 255] * 2
    assert ops.train_luma_sum(big, big, ident).tolist() == [3000 * 6000 * 255] * 2


# ---- tables ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", [(0.8, 1.2), (1.0, 0.0), (2.0, 1.0), (0.0, 2.0), (0.93, 1.07), (1.7, 0.31), (-0.5, 3.0)])
@pytest.mark.parametrize("image", ["random", "black", "white"])
def test_tables_equal_numpy_bitwise(f, image):
    from dcanet_amd import ops, training as T
    from dcanet_amd.inference import imagenet_lut
    rs = np.random.RandomState(int(abs(f[0]) * 100) + 7)
    h, w = 23, 31
    left, right = _pair(rs, h, w)
    bg, _ = _bg(rs)
    if image != "random":                                               # a contrast mean of 0 / of 255
        left[:] = right[:] = 0 if image == "black" else 255
        bg = np.stack([np.arange(256, dtype=np.uint8)] * 2)
    norm = imagenet_lut().numpy().copy()
    norm[1] = rs.randn(3, 256).astype(np.float32)                       # the two images' tables are told apart
    S = ops.train_luma_sum(_dev(left), _dev(right), _dev(bg))
    U, Tt = ops.train_tables(S, h * w, _dev(bg), f, _dev(norm))
    means = [T.contrast_mean(T.luma_sum(img, bg[i]), h * w) for i, img in enumerate((left, right))]
    if image != "random":
        assert means == [0 if image == "black" else 255] * 2
    wantU = np.stack([T.contrast_table(means[i], f[i])[bg[i]] for i in range(2)])
    wantT = np.stack([np.stack([norm[i, ch][wantU[i]] for ch in range(3)]) for i in range(2)])
    assert U.dtype == torch.uint8 and np.array_equal(U.cpu().numpy(), wantU)
    assert Tt.cpu().numpy().tobytes() == wantT.tobytes()


# ---- patch colour ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,c,y1,x1,th,tw", [(37, 121, 3, 0, 0, 37, 121), (50, 70, 4, 7, 5, 24, 40), (300, 600, 3, 44, 87, 256, 512),
                                               (20, 30, 3, 19, 29, 1, 1)])
def test_patch_colour_equals_numpy(h, w, c, y1, x1, th, tw):
    from dcanet_amd import ops, training as T
    rs = np.random.RandomState(h + w)
    _, right = _pair(rs, h, w, c)
    U = rs.randint(0, 256, (2, 256)).astype(np.uint8)
    got = ops.train_patch_colour(_dev(right), _dev(U), y1, x1, th, tw)
    assert got.cpu().numpy().tolist() == T.patch_bytes(U[1][right[y1:y1 + th, x1:x1 + tw, :3]]).tolist()
    right[:] = 200                                                      # a constant plane: the mean is an exact integer
    got = ops.train_patch_colour(_dev(right), _dev(U), y1, x1, th, tw)
    assert got.cpu().numpy().tolist() == [int(U[1][200])] * 3


# ---- crop and normalise ----------------------------------------------------------------------------------------------------
# (H, W, C, th, tw, y1, x1, slot, misaligned): B = 3 throughout
CROP_CASES = {
    "origin_tw32_slot0": (37, 61, 3, 16, 32, 0, 0, 0, False),
    "corner_tw32_last_slot": (37, 61, 3, 16, 32, 21, 29, 2, False),
    "odd_x1_tw32_slot1": (37, 61, 3, 16, 32, 5, 13, 1, False),
    "origin_tw30_slot0": (37, 61, 3, 17, 30, 0, 0, 0, False),
    "corner_odd_x1_tw30_last_slot": (37, 61, 3, 17, 30, 20, 31, 2, False),
    "misaligned_view_tw32": (37, 61, 3, 16, 32, 3, 8, 1, True),
    "rgba_tw32": (37, 61, 4, 16, 32, 21, 29, 2, False),
    "two_blocks_per_image": (80, 200, 3, 48, 128, 32, 71, 1, False),
}


@pytest.mark.parametrize("patch", ["none", "two_edges", "whole"])
@pytest.mark.parametrize("case", list(CROP_CASES))
def test_crop_norm_equals_numpy_and_leaves_neighbours(case, patch):
    from dcanet_amd import ops
    H, W, C, th, tw, y1, x1, slot, misaligned = CROP_CASES[case]
    rs = np.random.RandomState(len(case) * 3 + len(patch))
    left, right = _pair(rs, H, W, C)
    Tt, norm = rs.randn(2, 3, 256).astype(np.float32), rs.randn(2, 3, 256).astype(np.float32)
    colour = rs.randint(0, 256, 3).astype(np.uint8)
    rect = {"none": None, "two_edges": (th - 7, th, 0, 11), "whole": (0, th, 0, tw)}[patch]
    B, n = 3, 3 * 3 * th * tw
    flat = [torch.full((n + 8,), -12345.0, device=DEV) for _ in range(2)]
    off = 1 if misaligned else 0
    outL, outR = (f[off:off + n].view(B, 3, th, tw) for f in flat)
    assert (outL.data_ptr() % 16 != 0) == misaligned
    ops.train_crop_norm(_dev(left), _dev(right), _dev(Tt), y1, x1, outL[slot], outR[slot], rect, _dev(norm), _dev(colour))
    want = []
    for i, img in enumerate((left, right)):
        c = img[y1:y1 + th, x1:x1 + tw]
        o = np.stack([Tt[i, ch][c[:, :, ch]] for ch in range(3)])
        if i == 1 and rect is not None:
            o[:, rect[0]:rect[1], rect[2]:rect[3]] = norm[1, np.arange(3), colour][:, None, None]
        want.append(o)
    for out, f, w in ((outL, flat[0], want[0]), (outR, flat[1], want[1])):
        assert out[slot].cpu().numpy().tobytes() == w.tobytes()
        rest = f.cpu().numpy().copy()
        rest[off + slot * 3 * th * tw:off + (slot + 1) * 3 * th * tw] = -12345.0
        assert (rest == -12345.0).all()                                 # neighbouring slots and the guard words


def test_crop_norm_refuses_windows_and_patches_that_do_not_fit():
    from dcanet_amd import ops
    left, right = _pair(np.random.RandomState(1), 20, 30)
    Tt = torch.zeros((2, 3, 256), device=DEV)
    out = torch.zeros((2, 3, 8, 16), device=DEV)
    col = torch.zeros(3, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="does not fit"):
        ops.train_crop_norm(_dev(left), _dev(right), Tt, 13, 0, out[0], out[1])
    with pytest.raises(RuntimeError, match="does not fit"):
        ops.train_crop_norm(_dev(left), _dev(right), Tt, 0, 15, out[0], out[1])
    with pytest.raises(RuntimeError, match="leave the"):
        ops.train_crop_norm(_dev(left), _dev(right), Tt, 0, 0, out[0], out[1], (0, 9, 0, 4), Tt, col)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.train_crop_norm(torch.from_numpy(left), _dev(right), Tt, 0, 0, out[0], out[1])


# ---- disparity crop --------------------------------------------------------------------------------------------------------
SPECIAL = np.array([0.0, 32.0, -1.0, np.inf, np.nan, 31.999998, 1e-30, -np.inf, -0.0, 32.000004, 7.25], np.float32)


@pytest.mark.parametrize("kind", ["f32", "f32_flip", "f32_inf0", "u16", "f32_scaled"])
@pytest.mark.parametrize("h,w,th,tw,y1,x1", [(37, 61, 16, 30, 21, 31), (37, 61, 37, 61, 0, 0), (90, 300, 70, 257, 13, 40)])
def test_disp_crop_equals_numpy_and_torch_mask(kind, h, w, th, tw, y1, x1):
    from dcanet_amd import ops, training as T
    rs = np.random.RandomState(h + th)
    if kind == "u16":
        disp = rs.randint(0, 256 * 40, (h, w)).astype(np.uint16)
        disp.reshape(-1)[rs.permutation(h * w)[:6]] = [0, 1, 8191, 8192, 8193, 65535]     # 8192 / 256 = maxdisp exactly
    else:
        disp = (rs.rand(h, w).astype(np.float32) * 40 - 4)
        k = (h * w * 2 // 5) // SPECIAL.size                             # two pixels in five: every crop window gets each
        disp.reshape(-1)[rs.permutation(h * w)[:k * SPECIAL.size]] = np.tile(SPECIAL, k)
        disp.view(np.uint32)[y1, x1] = 0x7FC12345                       # a NaN with a payload: scale 1 copies the bits
    opts = dict(flip_rows=kind == "f32_flip", inf_to_zero=kind == "f32_inf0",
                scale={"u16": 1 / 256, "f32_scaled": 0.5}.get(kind, 1.0))
    gt = torch.full((3, th, tw), -7.0, device=DEV)
    mask = torch.zeros((3, th, tw), dtype=torch.bool, device=DEV)
    ops.train_disp_crop(_dev(disp), y1, x1, 32, gt[1], mask[1], **opts)
    want, wmask = T.crop_disparity(disp, y1, x1, th, tw, 32, **opts)
    assert gt[1].cpu().numpy().tobytes() == want.tobytes()
    assert (gt[0] == -7.0).all() and (gt[2] == -7.0).all() and not mask[0].any() and not mask[2].any()
    assert torch.equal(mask[1], (gt[1] < 32) & (gt[1] > 0)) and np.array_equal(mask[1].cpu().numpy(), wmask)
    assert mask[1].view(torch.uint8).max().item() <= 1 and 0 < mask[1].sum().item() < th * tw
    if kind.startswith("f32"):                                            # the window really holds the special values
        src = (disp[::-1] if kind == "f32_flip" else disp)[y1:y1 + th, x1:x1 + tw]
        assert np.isposinf(src).any() and np.isnan(src).any() and (src == 32).any() and (src == 0).any() and (src < 0).any()
        assert bool(torch.isposinf(gt[1]).any()) == (kind != "f32_inf0") and torch.isnan(gt[1]).any()


# ---- TrainInput ------------------------------------------------------------------------------------------------------------
def _samples(rs, kind, crop, k, seed):
    from dcanet_amd import training as T
    th, tw = crop
    out = []
    for b, (h, w) in enumerate(((50, 100), (64, 120), (47, 93))):
        left, right = _pair(rs, h, w)
        if kind == "kitti":
            disp = rs.randint(0, 256 * 40, (h, w)).astype(np.uint16)
            p = T.draw_kitti(w, h, crop, np.random.RandomState(seed + 10 * k + b), random.Random(seed + 10 * k + b))
            if (k + b) % 2 == 0:
                p.patch = (3 + b, th - 2, 0, tw // 2 + b)
            out.append(((left, right, disp, p), {}))
        else:
            disp = rs.rand(h, w).astype(np.float32) * 40 - 2
            p = T.draw_sceneflow(w, h, crop, random.Random(seed + 10 * k + b))
            out.append(((left, right, disp, p), {"flip_rows": True}))
    return out


@pytest.mark.parametrize("kind,crop", [("kitti", (32, 64)), ("sceneflow", (32, 64)), ("kitti", (31, 45))])
def test_train_input_device_io_equals_host_path_over_four_batches(kind, crop):
    """Four batches through a ring of depth 2, loaded back to back with no synchronisation in between: the only things
    that keep a pinned buffer from being rewritten before its copy, and a device stage from being overwritten before its
    kernels have read it, are the ring's events.  The outputs are cloned on the stream; everything is compared after ONE
    synchronisation at the end."""
    from dcanet_amd import training as T
    rs = np.random.RandomState(17)
    dev = T.TrainInput(3, crop, 32, kind, device_io=True, depth=2)
    batches = [_samples(rs, kind, crop, k, 40) for k in range(4)]
    kept = []
    for samples in batches:
        for b, (args, kw) in enumerate(samples):
            dev.load(b, *args, **kw)
        got = dev.batch()
        assert all(t.is_cuda for t in got) and got[0].data_ptr() == dev.imgL.data_ptr()      # static outputs
        kept.append([t.clone() for t in got])                           # enqueued behind the kernels
    torch.cuda.synchronize()
    host = T.TrainInput(3, crop, 32, kind)
    for k, samples in enumerate(batches):
        for b, (args, kw) in enumerate(samples):
            host.load(b, *args, **kw)
        for name, g, w in zip(("imgL", "imgR", "gt", "mask"), kept[k], host.batch()):
            assert g.dtype == w.dtype and g.shape == w.shape
            assert g.cpu().numpy().tobytes() == w.numpy().tobytes(), f"batch {k}: {name} differs"
        assert 0 < kept[k][3].sum().item() < kept[k][3].numel()
    assert not torch.equal(kept[0][0], kept[2][0])                      # the ring's stages were reused with other data
    with pytest.raises(RuntimeError, match="not loaded"):
        dev.batch()


# ---- hipGraph ----------------------------------------------------------------------------------------------------------------
def test_kitti_sample_kernels_and_metric_accumulation_replay_from_a_hipgraph():
    from dcanet_amd import ops, training as T
    from dcanet_amd.inference import imagenet_lut
    h, w, th, tw, y1, x1 = 50, 100, 32, 64, 11, 23
    rs = np.random.RandomState(21)
    norm = imagenet_lut().to(DEV)
    L, R = (torch.empty((h, w, 3), dtype=torch.uint8, device=DEV) for _ in range(2))
    D = torch.empty((h, w), dtype=torch.uint16, device=DEV)
    bg = torch.empty((2, 256), dtype=torch.uint8, device=DEV)
    imgL, imgR = torch.empty((1, 3, th, tw), device=DEV), torch.empty((1, 3, th, tw), device=DEV)
    gt, mask = torch.empty((1, th, tw), device=DEV), torch.empty((1, th, tw), dtype=torch.bool, device=DEV)
    state = torch.zeros(4, dtype=torch.float64, device=DEV)
    rect, contrast = (4, 30, 0, 40), (0.87, 1.13)

    def run():
        S = ops.train_luma_sum(L, R, bg)
        U, Tt = ops.train_tables(S, h * w, bg, contrast, norm)
        colour = ops.train_patch_colour(R, U, y1, x1, th, tw)
        ops.train_crop_norm(L, R, Tt, y1, x1, imgL[0], imgR[0], rect, norm, colour)
        ops.train_disp_crop(D, y1, x1, 32, gt[0], mask[0], scale=1 / 256)
        pred = (imgL[:, 0] * 3 + imgR[:, 1]).abs().contiguous()          # stands in for the network
        rec = ops.disp_metrics(pred, gt, 32, mask)
        n = rec[:, 0].sum()
        state.add_(torch.stack([torch.ones_like(n), n * 0.5, rec[:, 2].sum() / n, n]))
        return S, U, Tt, colour, rec

    def fill():
        left, right = _pair(rs, h, w)
        tables, _ = _bg(rs)
        L.copy_(_dev(left)), R.copy_(_dev(right)), bg.copy_(_dev(tables))
        D.view(torch.int16).copy_(_dev(rs.randint(0, 256 * 40, (h, w)).astype(np.int16)))     # < 2^15: the same bits
        return left, right, tables

    fill()
    run()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs_g = run()
    for _ in range(2):
        left, right, tables = fill()
        state.zero_()
        g.replay()
        got = [t.clone() for t in (*outs_g, imgL, imgR, gt, mask, state)]
        state.zero_()
        outs_e = run()
        for a, b in zip(got, (*outs_e, imgL, imgR, gt, mask, state)):
            assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
        assert got[0].tolist() == [T.luma_sum(left, tables[0]), T.luma_sum(right, tables[1])]      # really the new data
        assert state[0].item() == 1 and state[3].item() == mask.sum().item() > 0


# ---- TrainStep -------------------------------------------------------------------------------------------------------------
def load_seeded(module):
    shapes = {k: tuple(v.shape) for k, v in module.state_dict().items()}
    module.load_state_dict(O.seeded_state_dict(shapes), strict=True)
    return module


@pytest.mark.timeout(900)
def test_train_step_equals_the_literal_loop(monkeypatch):
    """main_dca.py:122-141 spelled out (mask, zero_grad, forward, focal_loss + model_loss, boolean-indexed EPE, backward,
    Adam, two .item() calls) against TrainStep on a copy of the model: parameters and the loss sum bit for bit; the EPE
    sum against the masked mean of the fp32 errors taken in fp64 by torch, to 1e-12 relative (the kernel forms e in fp32
    and adds 8192 of them per image in fp64 in a fixed order: n 2^-53 ~ 1e-12)."""
    from dcanet_amd import training as T
    from dcanet_amd.models.gwcnet_dca_g import GwcNet
    from dcanet_amd.models.loss import focal_loss, model_loss
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)      # MIOpen convolutions of the 2D networks
    D, B, H, W = 32, 2, 64, 128
    ref = load_seeded(GwcNet(D, use_concat_volume=False)).to(DEV)
    net = copy.deepcopy(ref)
    opt_ref = torch.optim.Adam(ref.parameters(), lr=1e-3, betas=(0.9, 0.999))
    opt = torch.optim.Adam(net.parameters(), lr=1e-3, betas=(0.9, 0.999))
    ts = T.TrainStep(net, opt, maxdisp=D, focal_coefficient=5.0, sparse=False)
    g = torch.Generator().manual_seed(3)
    sum_loss, sum_epe64, pixels = 0.0, 0.0, 0
    for k in range(3):
        imgL, imgR = torch.randn(B, 3, H, W, generator=g).to(DEV), torch.randn(B, 3, H, W, generator=g).to(DEV)
        gt = (torch.rand(B, H, W, generator=g) * (D + 6) - 3).to(DEV)     # values below 0 and above maxdisp: a real mask
        if k == 2:
            gt = torch.full((B, H, W), float(D + 1), device=DEV)          # all invalid
        # the literal loop
        ref.train()
        disp_true = gt.unsqueeze(1)
        mask = ((disp_true < D) & (disp_true > 0)).byte().bool()
        mask.detach_()
        opt_ref.zero_grad()
        cls_outputs, disp_outputs = ref(imgL, imgR)
        loss = focal_loss(cls_outputs, disp_true, D, 5.0, False) + model_loss(disp_outputs, disp_true, mask)
        e = torch.abs(disp_outputs[-1][mask] - disp_true[mask])
        epe = torch.mean(e)
        loss.backward()
        opt_ref.step()
        sum_loss += loss.item()
        sum_epe64 += e.double().mean().item()
        pixels += mask.sum().item()
        # TrainStep: the mask from the device kernel's rule on even steps, handed in on odd ones
        ts.step(imgL, imgR, gt, None if k % 2 == 0 else mask[:, 0].clone())
        state = ts.state.cpu().numpy()
        print(f"step {k}: loss {loss.item()!r} epe {epe.item()!r}; state {state.tolist()}")
        if k < 2:
            assert 0 < mask.sum().item() < mask.numel() and np.isfinite(loss.item())
            assert state[T.SUM_LOSS] == sum_loss
            assert abs(state[T.SUM_EPE] - sum_epe64) <= 1e-12 * abs(sum_epe64)
            assert state[T.PIXELS] == pixels
            for (name, a), b in zip(ref.named_parameters(), net.parameters()):
                assert torch.equal(a, b), f"step {k}: {name} differs"
            for a, b in zip(ref.buffers(), net.buffers()):
                assert torch.equal(a, b)
            res = ts.result()
            assert res["steps"] == k + 1 and res["loss"] == sum_loss / (k + 1)
        else:
            assert mask.sum().item() == 0 and np.isnan(loss.item()) and np.isnan(epe.item())
            assert np.isnan(state[T.SUM_LOSS]) and np.isnan(state[T.SUM_EPE]) and state[T.STEPS] == 3
            assert np.isnan(ts.last[0].item()) and np.isnan(ts.last[1].item())


class _HotOnly(torch.nn.Module):
    """the model from the 1/4-resolution features on (what dcanet_amd.graph captures elsewhere): fixed features stand in
    for the 2D networks, the images are ignored"""

    def __init__(self, net, fL, fR, guid):
        super().__init__()
        self.net = net
        for name, t in (("fL", fL), ("fR", fR), ("guid", guid)):
            self.register_buffer(name, t)

    def forward(self, imgL, imgR):
        r = self.net.hot_path(self.fL, self.fR)
        pred4 = self.net.prop(self.guid, r["pred4_q"])
        return [r["pred0"], r["pred_dca1"], r["pred_dca2"], r["pred1"], r["pred2"]], [r["pred_dca3"], pred4]


@pytest.mark.timeout(900)
def test_train_step_callables_replay_in_a_graphed_train_step():
    """TrainStep.bind + local_step / optimizer_step handed to GraphedTrainStep (3 eager warm-up steps, then 2 replays)
    against 5 eager TrainStep.step calls on a copy: parameters and the run state bit for bit."""
    from dcanet_amd import training as T
    from dcanet_amd.graph import GraphedTrainStep
    from dcanet_amd.models.gwcnet_dca_g import GwcNet
    from oracle.seeded import seeded_tensor
    D, H, W = 32, 64, 128
    base = load_seeded(GwcNet(D, use_concat_volume=False))
    fL, fR = seeded_tensor("gts.fL", (1, 320, H // 4, W // 4)), seeded_tensor("gts.fR", (1, 320, H // 4, W // 4))
    guid = seeded_tensor("tio.guid", (1, 64, H // 4, W // 4))
    imgL = imgR = torch.zeros((1, 3, H, W), device=DEV)
    gt = (seeded_tensor("gts.gt", (1, H, W)).abs() * 10 + 1).to(DEV)
    gt[0, :4] = 0                                                      # a real mask
    mask = (gt < D) & (gt > 0)

    def build():
        model = _HotOnly(copy.deepcopy(base), fL.clone(), fR.clone(), guid.clone()).to(DEV)
        opt = torch.optim.Adam(model.parameters(), lr=1e-3, betas=(0.9, 0.999), capturable=True)
        return model, T.TrainStep(model, opt, maxdisp=D)

    m_e, ts_e = build()
    for _ in range(5):
        ts_e.step(imgL, imgR, gt, mask)
    m_g, ts_g = build()
    ts_g.bind(imgL, imgR, gt, mask)
    step = GraphedTrainStep(ts_g.local_step, ts_g.optimizer_step)
    step(), step()
    torch.cuda.synchronize()
    for (name, a), b in zip(m_e.named_parameters(), m_g.parameters()):
        assert torch.equal(a, b), name
    se, sg = ts_e.state.cpu().numpy(), ts_g.state.cpu().numpy()
    print(se.tolist(), sg.tolist())
    assert se[T.STEPS] == sg[T.STEPS] == 5 and se[T.PIXELS] == 5 * mask.sum().item()
    assert se.tobytes() == sg.tobytes() and np.isfinite(se).all()
