"""The self-supervised loss, the parts that need no GPU: the plain-torch restatement that the GPU
tests compare against (tests/_selfsup_reference.py) differentiates correctly, keeps every pixel of every GPU scene away
from the kinks, has the closed form on a linear image and reproduces the reference's own `loss_disp_smoothness`; the two C
entry points are bound and refuse bad arguments before anything touches a device; the operators refuse CPU tensors."""
import ctypes
import math

import numpy as np
import pytest
import torch

import _selfsup_reference as S


def test_restatement_autograd_matches_central_differences():
    """fp64 autograd of the restatement against central differences at every pixel of a small scene, with valid, all
    terms on.  Step 1e-5, margins >= 1e-3: no kink is crossed.  The loss is about 5 and its largest gradient about 4e-4,
    so the rounding of the two fp64 losses over the step (1e-15 / 2e-5) is about 1e-7 of the largest gradient, and the
    third-derivative term of a central difference stays below that between kinks; the bound is 1e-6."""
    sc = S.scene((2, 7, 37, 2))
    I, R, ds, valid = S.to_torch(sc)
    w = S.WEIGHTS[:2]
    _, _, grads = S.reference_grads(I, R, ds, w, valid)
    h = 1e-5
    for l in range(2):
        base = [d.double() for d in ds]
        fd = torch.zeros_like(base[l])
        flat = fd.view(-1)
        for i in range(flat.numel()):
            vals = []
            for s in (h, -h):
                cur = [b.clone() for b in base]
                cur[l].view(-1)[i] += s
                vals.append(S.selfsup_reference(I, R, cur, w, valid)[0])
            flat[i] = (vals[0] - vals[1]) / (2 * h)
        err = ((fd - grads[l]).abs().max() / grads[l].abs().max()).item()
        print(f"level {l}: |central differences - autograd|max / |grad|max = {err:.2e}")
        assert err < 1e-6


@pytest.mark.parametrize("shape", S.SHAPES + (S.TRAIN_SHAPE,))
def test_scenes_keep_their_distance_from_every_kink(shape):
    sc = S.scene(shape)
    assert set(sc["margins"]) == {"frac", "border", "l1", "ssim", "dd"}
    for k, v in sc["margins"].items():
        assert v >= S.MARGIN, (shape, k, v)
    assert len(sc["disps"]) == shape[3]
    for d, (plain, masked) in zip(sc["disps"], sc["kept"]):
        assert d.dtype == np.float32 and d.shape == shape[:3]
        assert 0.3 <= masked <= plain <= 0.9, (shape, plain, masked)
        xs = np.arange(shape[2])[None, None, :] - d.astype(np.float64)
        assert (xs < 0).any()                                       # the clamp on the left is exercised ...
        if shape[2] >= 8:
            assert (xs > shape[2] - 1).any() and d.max() > shape[2] / 2 - 1     # ... and on the right; disparities reach W/2
    again = S.scene.__wrapped__(shape)
    assert all(np.array_equal(a, b) for a, b in zip(again["disps"], sc["disps"])) and np.array_equal(again["left"], sc["left"])


def test_closed_form_on_a_linear_image():
    """I = a x + b, R(x) = I(x + k), constant d = k + delta, alpha = 0: Y(x) = I(x - delta) wherever the warp is not
    clamped, so photo = |a delta|, smooth = 0, and d loss / d d = w sign(delta) |a| / sum M at in-view interior pixels
    whose sample is not clamped (dY/dd = -a there, d|I - Y|/dY = sign(Y - I) = -sign(a delta))."""
    B, H, W, k, a, b, w = 2, 6, 24, 3, 0.25, -1.0, 1.8
    x = torch.arange(W, dtype=torch.float64)
    for delta in (0.375, -0.375):
        I = (a * x + b).view(1, 1, 1, W).expand(B, 3, H, W).contiguous()
        R = (a * (x + k) + b).view(1, 1, 1, W).expand(B, 3, H, W).contiguous()
        d = torch.full((B, H, W), k + delta, dtype=torch.float64)
        loss, stats, (g,) = S.reference_grads(I, R, [d], (w,), None, alpha=0.0, lam=0.1)
        xs = x - (k + delta)
        inview = (xs >= 0) & (xs <= W - 1)
        sum_m = B * (H - 2) * int(inview[1:-1].sum())
        assert stats[0, 2].item() == sum_m
        assert abs(stats[0, 0].item() - abs(a * delta)) < 1e-12 and stats[0, 1].item() == 0.0
        assert abs(loss.item() - w * abs(a * delta)) < 1e-12
        want = torch.zeros(B, H, W, dtype=torch.float64)
        want[:, 1:-1, 1:-1] = (w * math.copysign(1.0, delta) * abs(a) / sum_m) * inview[1:-1].double()
        assert (g - want).abs().max().item() < 1e-15


def test_smoothness_term_equals_the_reference_fixture(golden):
    """tests/golden/disp_smoothness.npz: inputs, value and autograd gradient of the reference's own loss_disp_smoothness
    (tools/make_selfsup_golden.py)"""
    g = golden("disp_smoothness")
    d = torch.from_numpy(g["disp"]).requires_grad_()
    v = S.smoothness(d[:, 0], torch.from_numpy(g["img"]))
    grad, = torch.autograd.grad(v, d)
    assert abs(v.item() - float(g["value"])) <= 1e-14 * abs(float(g["value"]))
    assert np.abs(grad.numpy() - g["grad"]).max() <= 1e-14 * np.abs(g["grad"]).max()
    # and it is what the whole restatement reports as the level's smooth term
    _, stats = S.selfsup_reference(torch.from_numpy(g["img"]), torch.from_numpy(g["img"]), [d.detach()], (1.0,))
    assert abs(stats[0, 1].item() - float(g["value"])) <= 1e-14 * abs(float(g["value"]))


def test_selfsup_entry_points_are_bound_and_exported():
    from dcanet_amd import _lib, ops
    lib = _lib.load()
    for name in ("dca_selfsup_loss_fwd", "dca_selfsup_loss_bwd"):
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    assert len(_lib.SIGNATURES["dca_selfsup_loss_fwd"][1]) == 18 and len(_lib.SIGNATURES["dca_selfsup_loss_bwd"][1]) == 19
    assert lib.dca_abi_version() == 21 and _lib.ABI_VERSION == 21
    assert ops.SELFSUP_MAX_LEVELS == _lib.CONSTANTS["DCA_SELFSUP_MAX_LEVELS"] == 8
    assert ops.SELFSUP_TILE == (16, 64) and ops.SELFSUP_SUMS == 4 and ops.SELFSUP_OUT == 5


def test_selfsup_launchers_refuse_bad_arguments_before_any_launch():
    """hipErrorInvalidValue (1) without touching a device"""
    from dcanet_amd import _lib
    lib = _lib.load()
    p, q, r, s, t = (ctypes.c_void_p(16 * k) for k in range(1, 6))

    def ptrs(n, base=4096):
        return (ctypes.c_void_p * n)(*[base + 16 * i for i in range(n)])

    def weights(n):
        return (ctypes.c_float * n)(*([1.0] * n))

    def fwd(left=p, right=q, disps=ptrs(2), wts=weights(2), nlev=2, valid=None, u8=0, work=r, out=s, B=1, H=8, W=8,
            alpha=0.85, lam=0.1, c1=1e-4, c2=9e-4, ps=1.0):
        return lib.dca_selfsup_loss_fwd(left, right, disps, wts, nlev, valid, u8, work, out, B, H, W, alpha, lam, c1, c2, ps, None)

    def bwd(left=p, right=q, disps=ptrs(2), gd=ptrs(2, 8192), wts=weights(2), nlev=2, valid=None, u8=0, out=s, gloss=t, B=1,
            H=8, W=8, alpha=0.85, lam=0.1, c1=1e-4, c2=9e-4, ps=1.0):
        return lib.dca_selfsup_loss_bwd(left, right, disps, gd, wts, nlev, valid, u8, out, gloss, B, H, W, alpha, lam, c1, c2,
                                        ps, None)

    for f in (fwd, bwd):
        assert f(left=None) == 1 and f(right=None) == 1 and f(disps=None) == 1 and f(wts=None) == 1 and f(out=None) == 1
        assert f(nlev=0) == 1 and f(nlev=9, disps=ptrs(9), wts=weights(9)) == 1
        assert f(disps=(ctypes.c_void_p * 2)(4096, None)) == 1
        assert f(H=2) == 1 and f(W=2) == 1 and f(B=0) == 1 and f(B=65536) == 1 and f(H=-3) == 1
        assert f(H=30000, W=30000) == 1                            # 3 H W >= 2^31
        assert f(H=3, W=(1 << 24) + 1) == 1
        assert f(u8=2) == 1
        assert f(alpha=-0.1) == 1 and f(alpha=1.5) == 1 and f(alpha=math.nan) == 1
        assert f(c1=0.0) == 1 and f(c2=-1.0) == 1 and f(lam=math.nan) == 1 and f(ps=math.nan) == 1
    assert fwd(work=None) == 1
    assert bwd(gd=None) == 1 and bwd(gloss=None) == 1 and bwd(gd=(ctypes.c_void_p * 2)(8192, None)) == 1
    assert bwd(gd=ptrs(2)) == 1                                   # the gradient must not alias its disparity map


def test_selfsup_operators_refuse_cpu_tensors_and_bad_shapes():
    from dcanet_amd import frame_ops, ops
    from dcanet_amd.models.loss import PhotometricLoss
    from dcanet_amd.utils import loss_disp_smoothness
    I, R, d = torch.zeros(1, 3, 4, 8), torch.zeros(1, 3, 4, 8), torch.zeros(1, 4, 8)
    with pytest.raises(RuntimeError):
        ops.selfsup_loss(I, R, [d], [1.0])
    with pytest.raises(RuntimeError):
        PhotometricLoss()([d, d], I, R)
    with pytest.raises(RuntimeError):
        PhotometricLoss()([d], I, R)                               # two weights, one map
    with pytest.raises(RuntimeError):
        loss_disp_smoothness(d.unsqueeze(1), I)
    # the argument check itself, on stand-ins that claim to be on the device: shapes, dtypes, layout, level count
    from unittest import mock
    with mock.patch.object(torch.Tensor, "is_cuda", new_callable=mock.PropertyMock, return_value=True):
        chk = lambda *a, scalars=(0.85, 0.1, 1e-4, 9e-4): frame_ops._selfsup_check(*a, scalars)
        assert chk(I, R, [d], (1.0,), None) == (1, 4, 8, [1.0], 0)
        assert chk(I, R, [d.unsqueeze(1)], (1.0,), torch.ones(1, 4, 8, dtype=torch.bool))[4] == 1
        bad = [
            (torch.zeros(1, 3, 2, 8), torch.zeros(1, 3, 2, 8), [torch.zeros(1, 2, 8)], (1.0,), None),       # H < 3
            (torch.zeros(1, 3, 4, 2), torch.zeros(1, 3, 4, 2), [torch.zeros(1, 4, 2)], (1.0,), None),       # W < 3
            (I, R.double(), [d], (1.0,), None), (I, R, [d.double()], (1.0,), None),                         # dtypes
            (I, torch.zeros(1, 3, 4, 9), [d], (1.0,), None), (I[:, :1], R[:, :1], [d], (1.0,), None),       # shapes
            (I, R, [torch.zeros(1, 8, 4).transpose(1, 2)], (1.0,), None),                                   # not contiguous
            (I, R, [torch.zeros(1, 4, 7)], (1.0,), None), (I, R, [d] * 9, (1.0,) * 9, None), (I, R, [], (), None),
            (I, R, [d], (1.0, 2.0), None),
            (I, R, [d], (1.0,), torch.ones(1, 4, 8, dtype=torch.float64)), (I, R, [d], (1.0,), torch.ones(1, 4, 7)),
            (I, R, [d], (1.0,), torch.ones(1, 4, 8, requires_grad=True)),
        ]
        for args in bad:
            with pytest.raises(RuntimeError):
                chk(*args)
        for scalars in ((1.5, 0.1, 1e-4, 9e-4), (0.85, math.nan, 1e-4, 9e-4), (0.85, 0.1, 0.0, 9e-4), (0.85, 0.1, 1e-4, -1.0)):
            with pytest.raises(RuntimeError):
                chk(I, R, [d], (1.0,), None, scalars=scalars)
        # beyond the documented 32-bit limit: 3 H W of one sample must stay below 2^31 (a meta tensor: nothing is allocated)
        big = torch.empty(1, 3, 30000, 30000, device="meta")
        with pytest.raises(RuntimeError, match="32-bit"):
            chk(big, big, [torch.empty(1, 30000, 30000, device="meta")], (1.0,), None)


def test_selfsup_step_host_logic():
    from dcanet_amd.training import SelfSupStep, SS_STEPS, SS_LOSS, SS_PHOTO, SS_SMOOTH, SS_KEPT
    from dcanet_amd.models.loss import PhotometricLoss
    net = torch.nn.Linear(1, 1)
    ss = SelfSupStep(net, torch.optim.SGD(net.parameters(), lr=0.1))
    assert isinstance(ss.loss, PhotometricLoss) and ss.loss.weights == (1.8, 2.1) and ss.mask is None and ss.tau == 1.0
    assert (ss.loss.alpha, ss.loss.lam, ss.loss.c1, ss.loss.c2) == (0.85, 0.1, 1e-4, 9e-4)
    assert ss.state.dtype == torch.float64 and ss.state.shape == (5,) and not ss.state.any()
    assert (SS_STEPS, SS_LOSS, SS_PHOTO, SS_SMOOTH, SS_KEPT) == (0, 1, 2, 3, 4)
    assert ss.result() == {"steps": 0, "loss": 0.0, "photo": 0.0, "smooth": 0.0, "kept": 0.0}
    assert SelfSupStep(net, None, mask="lr", tau=2.0).tau == 2.0
    with pytest.raises(ValueError):
        SelfSupStep(net, None, mask="rl")
    with pytest.raises(ValueError):
        ss.bind(torch.zeros(1, 1, 4, 8), torch.zeros(1, 1, 4, 8))
    for name in ("bind", "local_step", "optimizer_step", "step", "result", "reset"):
        assert callable(getattr(ss, name))
