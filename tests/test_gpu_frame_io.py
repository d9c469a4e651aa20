"""Device frame I/O on the MI355X (csrc/frame_io.hip, dcanet_amd.inference.KittiInference(device_io=True)): each kernel
against its numpy / host-path statement, the wrapper against the same steps called by hand, the frame pipeline against
one-at-a-time calls, and all four kernels inside a hipGraph."""
import numpy as np
import pytest
import torch

from oracle import dcanet_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"


def load_seeded(module):
    shapes = {k: tuple(v.shape) for k, v in module.state_dict().items()}
    module.load_state_dict(O.seeded_state_dict(shapes), strict=True)
    return module


def _ulp_distance(a, b):
    def key(x):
        i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


def _pair(rs, h, w, c=3):
    return rs.randint(0, 256, (h, w, c)).astype(np.uint8), rs.randint(0, 256, (h, w, c)).astype(np.uint8)


def _bincount(left, right):
    return np.stack([[np.bincount(img[:, :, c].ravel(), minlength=256) for c in range(3)] for img in (left, right)])


def _dev(a):
    return torch.from_numpy(a).to(DEV)


# ---- frame_histogram ------------------------------------------------------------------------------------------------------
# 48-byte vector groups: 37*121*3 = 13431 = 279*48 + 39; 1x7 has no whole group; 64x128 has only whole groups; 375x1242 is
# the KITTI size (more groups than one pass of the grid)
@pytest.mark.parametrize("h,w,c", [(37, 121, 3), (1, 7, 3), (64, 128, 3), (375, 1242, 3), (37, 121, 4), (5, 3, 4),
                                   (375, 1242, 4), (50, 100, 3)])
def test_frame_histogram_equals_bincount(h, w, c):
    from dcanet_amd import ops
    left, right = _pair(np.random.RandomState(h + w + c), h, w, c)
    got = ops.frame_histogram(_dev(left), _dev(right))
    assert got.shape == (2, 3, 256) and got.dtype == torch.int32
    assert np.array_equal(got.cpu().numpy().astype(np.int64), _bincount(left, right))
    again = ops.frame_histogram(_dev(left), _dev(right))
    assert torch.equal(got, again)


def test_frame_histogram_single_valued_plane_and_unaligned_base():
    """every pixel on one bin (worst contention), and images that start at an address that is not a multiple of 16"""
    from dcanet_amd import ops
    left, right = _pair(np.random.RandomState(3), 375, 1242)
    left[:, :, 0] = 200
    right[:] = 0
    got = ops.frame_histogram(_dev(left), _dev(right)).cpu().numpy()
    assert np.array_equal(got, _bincount(left, right)) and got[0, 0, 200] == 375 * 1242 and got[1, :, 0].tolist() == [375 * 1242] * 3
    l2, r2 = _pair(np.random.RandomState(4), 37, 121)
    n = l2.size
    flat = torch.zeros(2 * n + 64, dtype=torch.uint8, device=DEV)
    flat[1:1 + n] = _dev(l2).view(-1)
    flat[n + 7:2 * n + 7] = _dev(r2).view(-1)
    lv, rv = flat[1:1 + n].view(37, 121, 3), flat[n + 7:2 * n + 7].view(37, 121, 3)
    assert lv.data_ptr() % 16 and rv.data_ptr() % 16
    assert np.array_equal(ops.frame_histogram(lv, rv).cpu().numpy(), _bincount(l2, r2))


# ---- frame_lut ------------------------------------------------------------------------------------------------------------
def _lut_images():
    rs = np.random.RandomState(9)
    yield _pair(rs, 375, 1242)
    yield _pair(rs, 37, 121)
    yield rs.randint(100, 104, (60, 90, 3)).astype(np.uint8), (rs.rand(60, 90, 3) < 0.03).astype(np.uint8) * 255
    const = rs.randint(0, 256, (20, 30, 3)).astype(np.uint8)
    const[:, :, 2] = 9                                        # std = 0: NaN at the one entry that is looked up
    yield const, rs.randint(0, 256, (20, 30, 3)).astype(np.uint8)


@pytest.mark.parametrize("case", range(4))
def test_frame_lut_equals_numpy_restatement_bitwise(case):
    from dcanet_amd import ops
    from dcanet_amd.inference import lut_from_histogram
    left, right = list(_lut_images())[case]
    n = left.shape[0] * left.shape[1]
    hist = ops.frame_histogram(_dev(left), _dev(right))
    lut, stats = ops.frame_lut(hist, n)
    with np.errstate(all="ignore"):
        want_lut, want_stats = lut_from_histogram(hist.cpu().numpy(), n)
    assert lut.dtype == torch.float32 and stats.dtype == torch.float64
    assert stats.cpu().numpy().tobytes() == want_stats.tobytes()
    assert lut.cpu().numpy().tobytes() == want_lut.tobytes()
    if case == 3:
        assert np.isnan(lut[0, 2, 9].item()) and stats[0, 2].tolist() == [9.0, 0.0]      # 0/0; the other entries are x/0


# ---- frame_apply ----------------------------------------------------------------------------------------------------------
APPLY_CASES = [(50, 100, 64, 128), (64, 128, 64, 128), (64, 100, 64, 128), (50, 128, 64, 128), (1, 7, 64, 128),
               (80, 150, 64, 128), (81, 128, 64, 128), (64, 150, 64, 128), (375, 1242, 384, 1248), (400, 1300, 384, 1248),
               (37, 121, 40, 123), (50, 130, 40, 125)]          # the last two: Wc % 4 != 0 (scalar stores)


@pytest.mark.parametrize("h,w,Hc,Wc,c", [k + (3,) for k in APPLY_CASES] + [k + (4,) for k in APPLY_CASES if k[0] * k[1] < 20000])
def test_frame_apply_equals_host_normalise_and_pad(h, w, Hc, Wc, c):
    from dcanet_amd import ops
    from dcanet_amd.inference import normalize_pair, pad_or_crop, placement
    left, right = _pair(np.random.RandomState(h * 7 + w + c), h, w, c)
    wl, wr, _, _ = pad_or_crop(normalize_pair(left, right), Hc, Wc)
    want = np.concatenate([wl.numpy(), wr.numpy()])
    L, R = _dev(left), _dev(right)
    lut, _ = ops.frame_lut(ops.frame_histogram(L, R), h * w)
    out = torch.full((2, 3, Hc, Wc), -12345.0, device=DEV)          # sentinel: the kernel writes every element
    gl, gr = ops.frame_apply(L, R, lut, (Hc, Wc), *placement(h, w, Hc, Wc), out=out)
    assert gl.shape == (1, 3, Hc, Wc) and gl.data_ptr() == out.data_ptr() and gr.data_ptr() == out[1].data_ptr()
    got = out.cpu().numpy()
    assert not (got == -12345.0).any() and np.isfinite(got).all()
    d = _ulp_distance(got, want)
    print(f"{h}x{w}x{c} -> {Hc}x{Wc}: max ulp distance {d.max()}, {int((d > 0).sum())} elements differ")
    assert d.max() <= 1
    zero = want == 0
    assert np.array_equal(got[zero].view(np.uint32), np.zeros(int(zero.sum()), np.uint32))      # padding: +0.0 exactly
    fresh = ops.frame_apply(L, R, lut, (Hc, Wc), *placement(h, w, Hc, Wc))                        # allocates its own frame
    assert torch.equal(torch.cat(fresh), out)


def test_frame_apply_unaligned_frame_and_bad_window():
    from dcanet_amd import ops
    from dcanet_amd.inference import placement
    left, right = _pair(np.random.RandomState(8), 50, 100)
    L, R = _dev(left), _dev(right)
    lut, _ = ops.frame_lut(ops.frame_histogram(L, R), 5000)
    want = torch.cat(ops.frame_apply(L, R, lut, (64, 128), *placement(50, 100, 64, 128)))
    flat = torch.full((2 * 3 * 64 * 128 + 4,), 7.0, device=DEV)
    out = flat[1:1 + 2 * 3 * 64 * 128].view(2, 3, 64, 128)          # 4-byte aligned only: the scalar path
    assert out.data_ptr() % 16 == 4
    ops.frame_apply(L, R, lut, (64, 128), *placement(50, 100, 64, 128), out=out)
    assert torch.equal(out, want) and flat[0] == 7.0 and flat[-1] == 7.0
    with pytest.raises(RuntimeError, match="does not fit"):
        ops.frame_apply(L, R, lut, (64, 128), 1, 0, 50, 100)
    with pytest.raises(RuntimeError, match="does not fit"):
        ops.frame_apply(L, R, lut, (40, 128), 0, 0, 50, 100)


def test_frame_apply_with_imagenet_table_equals_torch_restatement():
    from dcanet_amd import ops
    from dcanet_amd.inference import imagenet_lut
    left, right = _pair(np.random.RandomState(12), 97, 131)
    mean = torch.tensor([0.485, 0.456, 0.406]).view(3, 1, 1)
    std = torch.tensor([0.229, 0.224, 0.225]).view(3, 1, 1)
    gl, gr = ops.frame_apply(_dev(left), _dev(right), imagenet_lut().to(DEV), (97, 131), 0, 0, 97, 131)
    for got, img in ((gl, left), (gr, right)):
        want = torch.from_numpy(img).permute(2, 0, 1).float().div(255).sub(mean).div(std)
        assert got[0].cpu().numpy().tobytes() == want.numpy().tobytes()


# ---- disp_export ----------------------------------------------------------------------------------------------------------
def _pred(Hc, Wc, seed=0):
    rs = np.random.RandomState(seed)
    pred = (rs.rand(Hc, Wc) * 255.99).astype(np.float32)
    k = rs.randint(0, 65535, 400).astype(np.float32) / np.float32(256)          # exact multiples of 1/256 ...
    edge = np.concatenate([k, np.nextafter(k, np.float32(-1)), np.nextafter(k, np.float32(1e9))]).astype(np.float32)
    edge = edge[(edge >= 0) & (edge * np.float32(256) < 65536)]                  # ... and their two neighbours
    pred.reshape(-1)[:edge.size] = edge
    return rs.permutation(pred.reshape(-1)).reshape(Hc, Wc)


@pytest.mark.parametrize("h,w,Hc,Wc", [(50, 100, 64, 128), (64, 128, 64, 128), (80, 150, 64, 128), (37, 121, 40, 123)])
def test_disp_export_equals_crop_back_and_uint16_cast(h, w, Hc, Wc):
    from dcanet_amd import ops
    from dcanet_amd.inference import crop_back, placement
    pred = _pred(Hc, Wc, h)
    _, y0, rows, cols = placement(h, w, Hc, Wc)
    want = crop_back(pred, h, w, Hc, Wc)
    assert want.shape == (rows, cols)
    P = _dev(pred).view(1, 1, Hc, Wc)
    f, u = ops.disp_export(P, y0, rows, cols, f32=True, u16=True)
    assert f.dtype == torch.float32 and u.dtype == torch.uint16 and f.shape == u.shape == (rows, cols)
    assert f.cpu().numpy().tobytes() == np.ascontiguousarray(want).tobytes()
    assert np.array_equal(u.cpu().numpy(), (want * 256).astype("uint16"))
    # either output alone (the other pointer is null)
    f2, none = ops.disp_export(P, y0, rows, cols)
    assert none is None and torch.equal(f2, f)
    none, u2 = ops.disp_export(P, y0, rows, cols, f32=False, u16=True)
    assert none is None and np.array_equal(u2.cpu().numpy(), u.cpu().numpy())
    with pytest.raises(RuntimeError, match="nothing to export"):
        ops.disp_export(P, y0, rows, cols, f32=False, u16=False)
    with pytest.raises(RuntimeError, match="does not fit"):
        ops.disp_export(P, y0 + 1, rows, cols)


def test_disp_export_saturation_nan_and_bit_copy():
    from dcanet_amd import ops
    special = np.array([0.0, -0.0, -1.0, -1e-3, np.nan, -np.nan, np.inf, -np.inf, 255.99609375, 256.0, 255.998, 1e9, 1e-9,
                        0.00390625, 0.0039062, 1.0, 65535.0 / 256, 3e38], np.float32)
    pred = np.zeros((4, 8), np.float32)
    pred.reshape(-1)[:special.size] = special
    pred.view(np.uint32)[3, 7] = 0x7FC12345                                       # a NaN with a payload
    f, u = ops.disp_export(_dev(pred), 0, 4, 8, f32=True, u16=True)
    assert f.cpu().numpy().tobytes() == pred.tobytes()
    with np.errstate(invalid="ignore", over="ignore"):
        v = pred.astype(np.float32) * np.float32(256)
        want = np.where(np.isnan(v), 0, np.clip(np.trunc(np.nan_to_num(v, nan=0.0, posinf=1e30, neginf=-1e30)), 0, 65535)).astype(np.uint16)
    assert np.array_equal(u.cpu().numpy(), want)
    assert want.reshape(-1)[[4, 6, 8, 9, 11]].tolist() == [0, 65535, 65535, 65535, 65535]
    _, u1 = ops.disp_export(_dev(pred), 0, 4, 8, scale=1.0, f32=False, u16=True)   # another scale
    assert u1.cpu().numpy().reshape(-1)[[8, 9, 15]].tolist() == [255, 256, 1]


# ---- the wrapper -----------------------------------------------------------------------------------------------------------
def _model():
    from dcanet_amd.models.gwcnet_dca_g import GwcNet
    return load_seeded(GwcNet(32)).to(DEV).eval()


@pytest.mark.timeout(900)
def test_kitti_inference_device_io_wiring_and_host_gap(monkeypatch):
    """device_io=True == the ops and forward_frame called by hand (bitwise); uint16 == (float * 256).astype; and the gap to the
    host-I/O wrapper on the same images.  Measured on the MI355X: bitwise-equal frames and max |device-io - host-io| = 0 on
    all three pairs, so equal outputs are asserted (the images are seeded; whether their frames are equal does not depend
    on the box: tests/test_frame_io_cpu.py checks the same table form on the host)."""
    from dcanet_amd import ops
    from dcanet_amd.inference import KittiInference, crop_back, normalize_pair, pad_or_crop, placement
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)      # MIOpen convolutions of the 2D networks; restored
    model = _model()
    dev_io = KittiInference(model, crop_height=64, crop_width=128, device_io=True)
    by_hand = KittiInference(model, crop_height=64, crop_width=128)
    host = KittiInference(model, crop_height=64, crop_width=128)
    rng = np.random.default_rng(11)
    for h, w in ((50, 100), (64, 128), (50, 100)):
        left = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        right = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        disp = dev_io(left, right)
        assert disp.shape == (h, w) and disp.dtype == np.float32 and disp.std() > 0.1
        L, R = _dev(left), _dev(right)
        lut, _ = ops.frame_lut(ops.frame_histogram(L, R), h * w)
        fl, fr = ops.frame_apply(L, R, lut, (64, 128), *placement(h, w, 64, 128))
        want = crop_back(by_hand.forward_frame(fl, fr).squeeze().cpu().numpy(), h, w, 64, 128)
        assert disp.tobytes() == np.ascontiguousarray(want).tobytes()
        u16 = dev_io(left, right, as_uint16=True)
        assert u16.dtype == np.uint16 and np.array_equal(u16, (disp * 256).astype("uint16"))
        # against the host path: the frames first, then the outputs
        hl, hr, _, _ = pad_or_crop(normalize_pair(left, right), 64, 128)
        frames_equal = torch.equal(fl.cpu(), hl) and torch.equal(fr.cpu(), hr)
        d = _ulp_distance(torch.cat([fl, fr]).cpu().numpy(), torch.cat([hl, hr]).numpy()).max()
        assert d <= 1
        ref = host(left, right)
        gap = np.abs(disp - ref).max()
        print(f"{h}x{w}: frames differ by {d} ulp at most (bitwise equal: {frames_equal}); max |device-io - host-io| = {gap:.3e}")
        # equal frames (what the table form gives on every image tried: DESIGN.md section 6c) must give equal outputs
        assert frames_equal, "the frames differ from the host path's: measure the output gap and gate on it (DESIGN.md 6c)"
        assert disp.tobytes() == ref.tobytes()
        assert np.array_equal(host(left, right, as_uint16=True), (ref * 256).astype("uint16"))


@pytest.mark.timeout(900)
@pytest.mark.parametrize("graph", [True, False])
def test_stream_equals_one_at_a_time_calls(graph, monkeypatch):
    from dcanet_amd.inference import KittiInference
    # without it the MIOpen convolutions of the 2D networks differ in the last bits from call to call
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    model = _model()
    infer = KittiInference(model, crop_height=64, crop_width=128, graph=graph, device_io=True)
    rng = np.random.default_rng(5)
    pairs = []
    for i in range(6):
        h, w = ((50, 100), (64, 120))[i % 2] if i != 3 else (50, 100)
        pairs.append((rng.integers(0, 256, (h, w, 3), dtype=np.uint8), rng.integers(0, 256, (h, w, 3), dtype=np.uint8)))
    single = [infer(l, r) for l, r in pairs]
    assert any(not np.array_equal(single[0], s) for s in single[2::2])            # same size, different content
    for depth in (2, 1, 3):
        got = list(infer.stream(iter(pairs), depth=depth))
        assert len(got) == 6
        for i, (g, s) in enumerate(zip(got, single)):
            assert g.shape == s.shape and g.tobytes() == s.tobytes(), f"depth {depth}: frame {i} differs"
    got16 = list(infer.stream(pairs, depth=2, as_uint16=True))
    for g, s in zip(got16, single):
        assert g.dtype == np.uint16 and np.array_equal(g, (s * 256).astype("uint16"))
    assert infer(*pairs[1]).tobytes() == single[1].tobytes()                      # per-call use after a stream
    with pytest.raises(ValueError):
        infer(np.zeros((80, 100, 3), np.uint8), np.zeros((80, 100, 3), np.uint8))  # taller and narrower than the frame


def test_pre_kernels_and_export_replay_from_a_hipgraph():
    from dcanet_amd import ops
    from dcanet_amd.inference import placement
    h, w, Hc, Wc = 50, 100, 64, 128
    rs = np.random.RandomState(21)
    place = placement(h, w, Hc, Wc)
    L, R = torch.empty((h, w, 3), dtype=torch.uint8, device=DEV), torch.empty((h, w, 3), dtype=torch.uint8, device=DEV)
    frames = torch.empty((2, 3, Hc, Wc), device=DEV)
    of, ou = torch.empty((h, w), device=DEV), torch.empty((h, w), dtype=torch.uint16, device=DEV)

    def run():
        lut, stats = ops.frame_lut(ops.frame_histogram(L, R), h * w)
        fl, fr = ops.frame_apply(L, R, lut, (Hc, Wc), *place, out=frames)
        pred = (fl[0, 0] * 3 + fr[0, 1]).abs().contiguous()                    # stands in for the network
        ops.disp_export(pred, place[1], h, w, f32=True, u16=True, out_f32=of, out_u16=ou)
        return lut, stats

    first = _pair(rs, h, w)
    L.copy_(_dev(first[0])), R.copy_(_dev(first[1]))
    run()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        lut_g, stats_g = run()
    for _ in range(2):
        left, right = _pair(rs, h, w)
        L.copy_(_dev(left)), R.copy_(_dev(right))
        g.replay()
        got = [t.clone() for t in (lut_g, stats_g, frames, of, ou)]
        lut_e, stats_e = run()
        for a, b in zip(got, (lut_e, stats_e, frames, of, ou)):
            assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
        assert of.std() > 0.1 and ou.cpu().numpy().max() > 0
