"""GPU tests of the fused self-supervised loss (csrc/selfsup.hip, `ops.selfsup_loss`, `PhotometricLoss`, `SelfSupStep`;
DESIGN.md section 6h) against the plain-torch restatement of tests/_selfsup_reference.py.

Gates.  The truth is the restatement in float64.  The yardstick is the error of the SAME restatement run in float32 on
the same scene and device; the gate is FOUR times that error (the fused kernels order the fp32 operations inside a window
differently).  For gradients, error is the max-norm relative to the map's largest gradient.  One floor is needed for the
gate to be well posed, from the number format alone: the fused results are fp32 numbers, so a yardstick that happens to be
0 (it does on the 3 x 5 scene) cannot be met.  The loss and the per-level terms come out of fp64 sums and are rounded to
fp32 once, after the fp32 weights were applied: floor 2^-23 relative.  A gradient element is a product chain
gloss * w * (1 / sum M) * (window terms) * dY/dd with four roundings of 2^-24 each: floor 2^-22 of the largest gradient.

Measured on one MI355X: MEASURED below, per scene the yardstick (fp32 restatement) and the fused error, worst case over
alpha in {0, 0.85, 1}, lam in {0, 0.1}, with and without valid; the test prints every figure before it asserts.  The
gradient errors of both implementations are the same to two digits: they come from the warped sample Y, which both round to
fp32 (2^-24 relative) before the windows with a small var_I + var_Y + c2 amplify it by up to 1 / c2.  `smoothness` through
`dcanet_amd.utils.loss_disp_smoothness`: value 3.4e-9 against a yardstick of 3.4e-9, gradient 9.4e-8 against 1.1e-7.
Whole-model parameter gradients (test_selfsup_step_parameter_gradients), two runs: max-norm 3.8e-3 and 1.1e-4 against
yardsticks of 3.9e-3 and 1.6e-4, relative L2 3.2e-3 and 1.3e-4 against 3.2e-3 and 1.7e-4 -- the size of the network's own
run-to-run spread, not of the loss."""
import functools

import pytest
import torch

import _selfsup_reference as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
ALPHAS, LAMS = (0.0, 0.85, 1.0), (0.0, 0.1)
FLOOR_SUM, FLOOR_GRAD = 2.0 ** -23, 2.0 ** -22

# scene: (loss yardstick, loss fused, gradient yardstick, gradient fused), worst case over the parameter grid, as printed by
# test_gates_against_fp64 / test_training_size on the MI355X; the gate applied is max(4 x yardstick, floor) per case
MEASURED = {
    (1, 3, 5, 1): (1.5e-7, 2.7e-8, 4.0e-7, 2.0e-7),
    (2, 7, 37, 2): (7.1e-8, 7.3e-8, 7.3e-6, 7.4e-6),
    (1, 19, 70, 2): (8.4e-8, 4.9e-8, 6.0e-5, 5.9e-5),
    (2, 33, 130, 3): (8.1e-8, 5.9e-8, 7.2e-5, 6.9e-5),
    (2, 256, 512, 2): (2.3e-8, 6.4e-8, 5.9e-4, 5.9e-4),
}


@functools.lru_cache(maxsize=None)
def dev_scene(shape):
    return S.to_torch(S.scene(shape), DEV)


@functools.lru_cache(maxsize=None)
def yardstick(shape, with_valid, alpha, lam):
    """(loss64, stats64, grads64, loss32, stats32, grads32) of the restatement on the device; computed once per case"""
    I, R, ds, valid = dev_scene(shape)
    w = S.WEIGHTS[:shape[3]]
    v = valid if with_valid else None
    return S.reference_grads(I, R, ds, w, v, alpha, lam) + S.reference_grads(I, R, ds, w, v, alpha, lam, dtype=torch.float32)


def fused(shape, with_valid, alpha, lam, gloss=None, levels=None, four_dim=False, valid=None, photo_scale=1.0):
    from dcanet_amd import ops
    I, R, ds, v = dev_scene(shape)
    levels = range(shape[3]) if levels is None else levels
    ds = [ds[l].clone().requires_grad_() for l in levels]
    if four_dim:
        ds = [d.detach().unsqueeze(1).requires_grad_() for d in ds]
    valid = valid if valid is not None else (v if with_valid else None)
    loss, stats = ops.selfsup_loss(I, R, ds, [S.WEIGHTS[l] for l in levels], valid, alpha, lam, S.C1, S.C2, photo_scale)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and stats.shape == (len(ds), 3) and not stats.requires_grad
    grads = torch.autograd.grad(loss if gloss is None else loss * gloss, ds)
    assert all(g.shape == d.shape and g.dtype == torch.float32 for g, d in zip(grads, ds))
    return loss.detach(), stats, list(grads)


def rel(a, b):
    return ((a.double() - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()


def check_gates(shape, with_valid, alpha, lam):
    l64, s64, g64, l32, s32, g32 = yardstick(shape, with_valid, alpha, lam)
    loss, stats, grads = fused(shape, with_valid, alpha, lam)
    tag = f"{shape} valid={with_valid} alpha={alpha} lam={lam}"
    y, e = abs(l32.double() - l64).item() / abs(l64.item()), abs(loss.double() - l64).item() / abs(l64.item())
    print(f"{tag}: loss {l64.item():.9g}  yardstick {y:.2e}  fused {e:.2e}")
    failures = []
    if e > max(4 * y, FLOOR_SUM):
        failures.append(f"loss: {e:.3e} > max(4 x {y:.3e}, {FLOOR_SUM:.2e})")
    assert torch.equal(stats[:, 2].double(), s64[:, 2]), "sum M is a count: exact"
    for l in range(shape[3]):
        for j, name in ((0, "photo"), (1, "smooth")):
            ref = s64[l, j].item()
            if ref == 0.0:
                assert stats[l, j].item() == 0.0
                continue
            y, e = abs(s32[l, j].item() - ref) / abs(ref), abs(stats[l, j].item() - ref) / abs(ref)
            print(f"  level {l} {name} {ref:.9g}  yardstick {y:.2e}  fused {e:.2e}")
            if e > max(4 * y, FLOOR_SUM):
                failures.append(f"level {l} {name}: {e:.3e} > max(4 x {y:.3e}, {FLOOR_SUM:.2e})")
        if not g64[l].any():                                       # alpha = 1 on a scene without SSIM gradient cannot happen;
            assert not grads[l].any()                              # lam = 0 and nothing in view could: then exactly 0
            continue
        y, e = rel(g32[l], g64[l]), rel(grads[l], g64[l])
        print(f"  level {l} gradient |max| {g64[l].abs().max().item():.3e}  yardstick {y:.2e}  fused {e:.2e}")
        if e > max(4 * y, FLOOR_GRAD):
            failures.append(f"level {l} gradient: {e:.3e} > max(4 x {y:.3e}, {FLOOR_GRAD:.2e})")
    assert not failures, tag + ": " + "; ".join(failures)


@pytest.mark.parametrize("lam", LAMS)
@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("with_valid", [False, True])
@pytest.mark.parametrize("shape", S.SHAPES)
def test_gates_against_fp64(shape, with_valid, alpha, lam):
    check_gates(shape, with_valid, alpha, lam)


def test_training_size():
    """2 x 256 x 512, two levels: 16 x 8 tiles per sample, the same gate"""
    check_gates(S.TRAIN_SHAPE, True, S.ALPHA, S.LAM)


@pytest.mark.parametrize("shape", [(1, 19, 70, 2), (2, 33, 130, 3)])
def test_two_runs_are_bitwise_identical(shape):
    a, b = fused(shape, True, S.ALPHA, S.LAM), fused(shape, True, S.ALPHA, S.LAM)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert all(torch.equal(x, y) for x, y in zip(a[2], b[2]))


def test_levels_are_independent():
    """each level's gradient and terms in a joint call equal those of the level run alone, bit for bit"""
    shape = (2, 33, 130, 3)
    _, stats, grads = fused(shape, True, S.ALPHA, S.LAM)
    for l in range(3):
        _, s1, g1 = fused(shape, True, S.ALPHA, S.LAM, levels=[l])
        assert torch.equal(g1[0], grads[l]) and torch.equal(s1[0], stats[l]), l


def test_incoming_gradient_scales_the_gradients():
    """the kernel multiplies gloss * w first: against 0.37 x (the gradient for gloss = 1) that is two more roundings"""
    shape = (1, 19, 70, 2)
    _, _, g1 = fused(shape, True, S.ALPHA, S.LAM)
    _, _, g2 = fused(shape, True, S.ALPHA, S.LAM, gloss=0.37)
    for a, b in zip(g1, g2):
        want = a.double() * float(torch.tensor(0.37, dtype=torch.float32))
        assert b.abs().max() > 0 and ((b.double() - want).abs() <= 2.0 ** -22 * want.abs() + 1e-40).all()


def test_four_dimensional_maps_give_the_same_bits():
    shape = (2, 7, 37, 2)
    a, b = fused(shape, True, S.ALPHA, S.LAM), fused(shape, True, S.ALPHA, S.LAM, four_dim=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert all(y.shape == (2, 1, 7, 37) and torch.equal(x, y[:, 0]) for x, y in zip(a[2], b[2]))


def test_bool_valid_gives_the_same_bits():
    shape = (1, 19, 70, 2)
    v = dev_scene(shape)[3]
    a, b = fused(shape, True, S.ALPHA, S.LAM), fused(shape, True, S.ALPHA, S.LAM, valid=v > 0)
    assert torch.equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[2], b[2]))


def test_empty_mask_leaves_the_smoothness_term():
    shape = (2, 33, 130, 3)
    zero = torch.zeros_like(dev_scene(shape)[3])
    loss, stats, grads = fused(shape, True, S.ALPHA, S.LAM, valid=zero)
    assert not stats[:, 0].any() and not stats[:, 2].any() and (stats[:, 1] > 0).all()
    assert all(torch.isfinite(g).all() and g.any() for g in grads)
    l0, s0, g0 = fused(shape, False, S.ALPHA, S.LAM, photo_scale=0.0)
    assert torch.equal(loss, l0) and torch.equal(stats[:, 1], s0[:, 1])
    assert all(torch.equal(a, b) for a, b in zip(grads, g0))


def test_loss_disp_smoothness_mirror(golden):
    """`dcanet_amd.utils.loss_disp_smoothness(disp, img)` against the reference's own value and gradient
    (tests/golden/disp_smoothness.npz), gated by four times the error of the fp32 restatement, floors as above"""
    from dcanet_amd.utils import loss_disp_smoothness
    g = golden("disp_smoothness")
    disp = torch.from_numpy(g["disp"]).float().to(DEV)
    img = torch.from_numpy(g["img"]).float().to(DEV)
    d64 = disp.double().requires_grad_()
    v64 = S.smoothness(d64[:, 0], img.double())                   # truth for the fp32-rounded inputs
    g64, = torch.autograd.grad(v64, d64)
    assert abs(v64.item() - float(g["value"])) < 1e-6 * float(g["value"])      # the inputs were rounded to fp32
    d32 = disp.clone().requires_grad_()
    v32 = S.smoothness(d32[:, 0], img)
    g32, = torch.autograd.grad(v32, d32)
    d = disp.clone().requires_grad_()
    v = loss_disp_smoothness(d, img)
    gd, = torch.autograd.grad(v, d)
    y, e = abs(v32.item() - v64.item()) / v64.item(), abs(v.item() - v64.item()) / v64.item()
    yg, eg = rel(g32, g64), rel(gd, g64)
    print(f"value {v64.item():.9g}: yardstick {y:.2e} fused {e:.2e}; gradient: yardstick {yg:.2e} fused {eg:.2e}")
    assert e <= max(4 * y, FLOOR_SUM) and eg <= max(4 * yg, FLOOR_GRAD)


def test_photometric_loss_is_the_op():
    from dcanet_amd import ops
    from dcanet_amd.models.loss import PhotometricLoss
    shape = (2, 7, 37, 2)
    I, R, ds, v = dev_scene(shape)
    crit = PhotometricLoss()
    a = crit(ds, I, R, v)
    b, stats = ops.selfsup_loss(I, R, ds, (1.8, 2.1), v)
    assert torch.equal(a, b) and torch.equal(crit.last, stats)


def test_forward_and_backward_replay_from_a_graph():
    """no host synchronisation, launches on the current stream: forward + backward captured once, replayed on new values"""
    from dcanet_amd import ops
    shape = (1, 19, 70, 2)
    I, R, ds, v = dev_scene(shape)
    static = [torch.zeros_like(d).requires_grad_() for d in ds]
    w = S.WEIGHTS[:2]

    def run():
        loss, _ = ops.selfsup_loss(I, R, static, w, v)
        return (loss,) + torch.autograd.grad(loss, static)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run()
    with torch.no_grad():
        for s, d in zip(static, ds):
            s.copy_(d)
    graph.replay()
    torch.cuda.synchronize()
    loss, _, grads = fused(shape, True, S.ALPHA, S.LAM)
    assert torch.equal(outs[0], loss) and all(torch.equal(a, b) for a, b in zip(outs[1:], grads))


# ---- SelfSupStep on the whole model ------------------------------------------------------------------------------------------
class RestatedLoss:
    """PhotometricLoss's interface with the restatement inside (float32, or float64 behind a cast of the disparities)"""

    def __init__(self, dtype, weights=(1.8, 2.1)):
        self.dtype, self.weights, self.last = dtype, weights, None

    def __call__(self, disp_ests, left, right, valid=None):
        loss, self.last = S.selfsup_reference(left, right, list(disp_ests), self.weights, valid, dtype=self.dtype)
        return loss


def whole_model():
    from test_gpu_boundary import make_model
    return make_model("g", True)


def whole_images():
    from test_gpu_boundary import images
    return images()


def step_grads(loss):
    from dcanet_amd.training import SelfSupStep
    m = whole_model()
    ss = SelfSupStep(m, torch.optim.SGD(m.parameters(), lr=0.0), loss=loss)
    ss.bind(*whole_images())
    ss.local_step()
    return m, ss, {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in m.named_parameters()}


@functools.lru_cache(maxsize=None)
def three_steps():
    """the same step with the fused loss, the fp32 and the fp64 restatement.  The MIOpen convolutions of the 2D networks are
    held to their deterministic algorithms: left alone they differ from run to run (relative L2 1e-4 over all parameter
    gradients, 3e-3 when an activation of the network flips with them), in ONE of the three steps at a time, which is
    neither the loss's error nor in the yardstick"""
    from dcanet_amd.models.loss import PhotometricLoss
    old = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        return (step_grads(PhotometricLoss()), step_grads(RestatedLoss(torch.float32)),
                step_grads(RestatedLoss(torch.float64)))
    finally:
        torch.backends.cudnn.deterministic = old


HEADS = ("classif0.", "classif1.", "classif2.")


def test_selfsup_step_parameter_gradients():
    """One `local_step` of the whole model at 1 x 3 x 64 x 128 (seeded weights, the size of tests/test_gpu_boundary.py):
    the parameter gradients with the fused loss against the same step with the fp64 restatement as its loss; yardstick:
    the same step with the fp32 restatement; gate: four times the yardstick, derived as above.  The parameter gradients
    are linear in d loss / d disparity, so they inherit its error; the network's own forward and backward are the same
    bits in the three steps (`three_steps`).  Error: max-norm over ALL parameters relative to the
    largest parameter gradient, and the relative L2 norm of the whole gradient.
    Measured on the MI355X: see DESIGN.md section 6h."""
    (_, ss, gf), (_, _, g32), (_, _, g64) = three_steps()
    names = [n for n, g in g64.items() if g is not None and not n.startswith(HEADS)]
    cat = lambda g: torch.cat([g[n].double().reshape(-1) for n in names])
    f, y, t = cat(gf), cat(g32), cat(g64)
    assert torch.isfinite(f).all() and t.abs().max() > 0
    e_max, y_max = ((f - t).abs().max() / t.abs().max()).item(), ((y - t).abs().max() / t.abs().max()).item()
    e_l2, y_l2 = ((f - t).norm() / t.norm()).item(), ((y - t).norm() / t.norm()).item()
    print(f"parameter gradients: max-norm yardstick {y_max:.2e} fused {e_max:.2e}; L2 yardstick {y_l2:.2e} fused {e_l2:.2e}")
    assert e_max <= max(4 * y_max, FLOOR_GRAD) and e_l2 <= max(4 * y_l2, FLOOR_GRAD)
    stats = ss.loss.last
    assert stats.shape == (2, 3) and (stats[:, 2] > 0).all()


def test_selfsup_step_leaves_the_class_heads_alone():
    """only disp_outputs are supervised: the parameters that only the class-volume heads depend on get no gradient"""
    (m, _, gf), _, _ = three_steps()
    head = [n for n in gf if n.startswith(HEADS)]
    assert head and all(gf[n] is None or not gf[n].any() for n in head)
    for n in ("classif3.2.weight", "feature_extraction.firstconv.0.0.weight", "prop.conv.2.weight", "cva3.cost_agg.conv3.0.weight"):
        assert gf[n] is not None and gf[n].any(), n


def test_selfsup_step_state_accumulates():
    from dcanet_amd.training import SelfSupStep
    m = whole_model()
    ss = SelfSupStep(m, torch.optim.SGD(m.parameters(), lr=1e-4))
    L, R = whole_images()
    losses, rows = [], []
    for _ in range(2):
        losses.append(ss.step(L, R).double())
        rows.append(ss.last[1].double())
    w = torch.tensor([1.8, 2.1], dtype=torch.float64, device=DEV) / 3.9
    want = torch.stack([torch.tensor(2.0, dtype=torch.float64, device=DEV), losses[0] + losses[1],
                        sum((w * r[:, 0]).sum() for r in rows), sum((w * r[:, 1]).sum() for r in rows),
                        sum(r[:, 2].mean() / (62 * 126) for r in rows)])
    assert torch.allclose(ss.state, want, rtol=1e-12, atol=0)
    res = ss.result()
    assert res["steps"] == 2 and abs(res["loss"] - (losses[0] + losses[1]).item() / 2) <= 1e-12 * abs(res["loss"])
    assert 0 < res["kept"] <= 1 and res["photo"] > 0 and res["smooth"] > 0
    assert m.training


def test_lr_mask_pass_leaves_batchnorm_statistics_alone():
    """mask="lr": two eval passes under no_grad before the training forward.  AFTER THE MASK PASS -- at the moment the
    training forward begins -- the BatchNorm running statistics and step counters are bit-identical to those of the same
    step with mask=None (same seeded model, same batch), the model is in train mode, and the mask was used.  The
    comparison is taken there and not after the step because the training forward of this network is itself not
    reproducible bit for bit from run to run (measured: two mask=None steps on equal models differ in the last bit of 95
    of the running statistics, from feature_extraction.layer4 on), which has nothing to do with the mask."""
    from dcanet_amd.training import SelfSupStep
    m = whole_model()
    L, R = whole_images()
    before = {k: v.clone() for k, v in m.state_dict().items()}
    valid = m.predict_lr(L, R, 1.0)["valid"]                       # the mask pass on its own, on a model in train mode
    assert m.training and valid.shape == (1, 1, 64, 128)
    assert all(torch.equal(v, before[k]) for k, v in m.state_dict().items())
    stats = []
    for mask in (None, "lr"):
        m = whole_model()
        seen = []

        def at_training_forward(module, args, seen=seen):
            assert module.training
            seen.append({k: v.clone() for k, v in module.state_dict().items() if "running_" in k or "num_batches" in k})

        m.register_forward_pre_hook(at_training_forward)
        ss = SelfSupStep(m, torch.optim.SGD(m.parameters(), lr=0.0), mask=mask, tau=1.0)
        ss.bind(L, R)
        ss.local_step()
        assert m.training and len(seen) == 1                       # predict_lr's two passes do not come through __call__
        assert int(m.dres0[0][1].num_batches_tracked) == 1         # one training forward moved the statistics, once
        stats.append((seen[0], ss.last[1][:, 2].clone()))
    (a, kept_plain), (b, kept_lr) = stats
    assert a.keys() == b.keys() and len(a) > 100
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert (kept_lr <= kept_plain).all() and (kept_lr < kept_plain).any()
