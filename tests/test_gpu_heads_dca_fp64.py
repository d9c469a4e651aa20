"""fp64 gates of the head and DCA kernels on every launch branch: the soft-argmin family (csrc/volume.hip), the fused
up-sampling head (csrc/up_softargmin.hip) and its documented fall-back, context injection and disparity attention
(csrc/context_attention.hip), trilinear interpolation and average pooling (csrc/pointwise.hip) and the stereo focal loss
(csrc/heads2d.hip).  tests/test_gpu_parity.py and tests/test_gpu_heads.py compare these kernels with the fp32 CPU oracle at
fixed tolerances on a handful of tiny unit-magnitude shapes; here every case of tests/_heads_cases.py sits on one branch of a
launcher (second block, tail, grid-stride iteration, the 65535 | 65536 grid limits, NMAX, QPT = 7, the NT switch, ...; the
arithmetic is checked without a GPU in tests/test_heads_cases_cpu.py) and is reached through the public op of ops.py,
forward and all gradients.

Gate.  Truth: the dtype-generic oracle in float64, differentiated by autograd.  Yardstick: the same functions in float32 on
the CPU.  Metric: max |a - ref| / max(1, max |ref|) per output and per gradient (`close()` of the parity tests).  A kernel
passes at max(4 x yardstick, 2^-22): the factor and the form of the floor are those of tests/test_gpu_selfsup.py; the floor
is the fp32 format's, every output here being at least a product and a quotient of three rounded fp32 quantities, and exact
float32 results (K = 1, mode 2 of `regression`, pooling) make the yardstick 0.  A case at the magnitude of its sibling in the
parity tests must meet that sibling's fixed tolerance as well, so nothing gets looser.  k* maps are compared exactly,
constructed ties included, and each family's largest case is run twice and compared bit for bit.  The gradient seeds are
chosen so that no gradient is far below 1, where the metric's max(1, .) would make the gate absolute (`seed_scale`).

Measured on one MI355X: MEASURED below, per case the worst (yardstick, error) over the forward outputs and over the
gradients, as printed by the tests before they assert."""
import pytest
import torch

import _heads_cases as H

pytestmark = pytest.mark.gpu
DEV = "cuda"

# case id: (forward yardstick, forward error, gradient yardstick, gradient error); the gate applied is per output
MEASURED = {
    "softargmin-mode0-1x1x3x5@2": (0.0e+00, 0.0e+00, 0.0e+00, 0.0e+00),
    "softargmin-mode1-1x1x3x5@2": (0.0e+00, 0.0e+00, 0.0e+00, 0.0e+00),
    "softargmin-mode2-1x1x3x5@2": (0.0e+00, 0.0e+00, 0.0e+00, 0.0e+00),
    "softargmin-mode0-3x48x7x37@2": (2.4e-07, 2.4e-07, 3.1e-07, 3.1e-07),
    "softargmin-mode1-3x48x7x37@2": (1.8e-07, 2.7e-07, 4.5e-07, 6.9e-07),
    "softargmin-mode2-3x48x7x37@2": (9.6e-08, 1.6e-07, 3.8e-08, 3.8e-08),
    "softargmin-mode0-3x48x7x37@30": (2.1e-07, 2.1e-07, 6.2e-07, 6.2e-07),
    "softargmin-mode1-3x48x7x37@30": (2.1e-07, 1.5e-07, 9.9e-07, 9.5e-07),
    "softargmin-mode2-3x48x7x37@30": (1.2e-07, 1.3e-07, 3.8e-08, 3.8e-08),
    "softargmin-mode0-3x48x7x37@80": (9.9e-08, 9.9e-08, 2.1e-07, 2.1e-07),
    "softargmin-mode1-3x48x7x37@80": (1.0e-07, 1.1e-07, 1.0e-06, 8.1e-07),
    "softargmin-mode2-3x48x7x37@80": (1.0e-07, 1.2e-07, 3.8e-08, 3.8e-08),
    "softargmin-mode0-1x192x4x6@2": (1.6e-07, 1.6e-07, 9.7e-08, 9.7e-08),
    "softargmin-mode1-1x192x4x6@2": (3.8e-07, 5.1e-07, 1.1e-06, 8.7e-07),
    "softargmin-mode2-1x192x4x6@2": (9.0e-08, 1.4e-07, 3.3e-08, 3.3e-08),
    "softargmin-mode0-1x2x1025x1024@2": (9.3e-08, 9.2e-08, 3.3e-07, 3.3e-07),
    "softargmin-mode1-1x2x1025x1024@2": (9.3e-08, 9.1e-08, 4.2e-07, 2.5e-07),
    "softargmin-mode2-1x2x1025x1024@2": (0.0e+00, 0.0e+00, 0.0e+00, 0.0e+00),
    "up_softargmin-scale4-2x6x5x7@2": (2.2e-07, 2.2e-07, 7.1e-07, 2.6e-07),
    "up_softargmin-scale4-2x6x5x7@30": (2.6e-07, 3.2e-07, 9.5e-07, 1.3e-06),
    "up_softargmin-scale4-1x48x3x5@2": (4.9e-07, 6.7e-07, 6.6e-07, 7.2e-07),
    "up_softargmin-scale4-1x48x3x5@30": (7.2e-07, 4.0e-07, 1.8e-06, 1.3e-06),
    "up_softargmin-scale8-1x64x2x3@2": (8.8e-07, 1.1e-06, 1.6e-06, 1.9e-06),
    "up_softargmin-scale8-1x2x1x1@2": (2.7e-08, 2.7e-08, 7.5e-07, 2.8e-07),
    "up_softargmin-scale8-1x4x2x33@2": (2.8e-07, 2.5e-07, 1.9e-06, 4.4e-07),
    "up_softargmin-scale8-1x24x4x6@30": (7.4e-07, 7.0e-07, 7.6e-07, 9.1e-07),
    "up_softargmin-scale2-2x3x3x129@2": (1.5e-07, 1.3e-07, 2.4e-07, 1.7e-07),
    "up_softargmin-scale2-1x2x1025x1024@2": (1.7e-07, 1.8e-07, 5.9e-07, 3.7e-07),
    "up_softargmin-scale2-1x65x2x3@2": (3.5e-07, 3.5e-07, 5.7e-07, 7.3e-07),
    "up_softargmin-scale8-1x1x3x4@2": (0.0e+00, 6.8e-08, 1.0e-05, 2.0e-06),
    "up_softargmin-scale3-1x4x2x3@2": (1.4e-07, 1.4e-07, 3.3e-07, 3.3e-07),
    "context-buildmargin-2x8x6x28x40@1.5": (6.1e-08, 6.1e-08, 5.0e-07, 3.0e-07),
    "context-buildmargin-1x8x64x5x9@1.5": (4.2e-08, 4.2e-08, 4.8e-08, 4.8e-08),
    "context-buildmargin-1x8x4x257x257@1.5": (7.9e-08, 7.9e-08, 2.1e-06, 5.3e-07),
    "context-buildmargin-1x1x2x1449x1449@1.5": (8.6e-08, 8.6e-08, 2.9e-04, 1.7e-06),
    "context-buildmargin-2x8x6x9x13@1.5": (5.9e-08, 7.0e-08, 9.5e-08, 1.7e-07),
    "context-buildmargin-2x8x6x9x13@40": (7.9e-08, 7.9e-08, 6.0e-07, 4.0e-07),
    "context-buildtie-2x8x6x9x13@1.5": (6.6e-08, 6.6e-08, 1.7e-07, 1.7e-07),
    "context-buildabsent-2x8x6x9x13@1.5": (7.2e-08, 7.0e-08, 1.2e-07, 1.2e-07),
    "attention-1x8x49x2x7@1": (3.1e-07, 3.1e-07, 2.2e-07, 3.7e-07),
    "attention-1x8x56x3x4@1": (3.4e-07, 3.2e-07, 2.9e-07, 4.2e-07),
    "attention-2x16x40x3x6@1": (2.5e-07, 3.0e-07, 4.2e-07, 3.7e-07),
    "attention-1x32x24x5x13@6": (5.1e-06, 4.0e-06, 3.2e-06, 4.1e-06),
    "trilinear-scale4-2x3x2x3x5@1": (1.2e-07, 1.2e-07, 3.6e-07, 1.1e-07),
    "trilinear-scale8-1x1x2x9x229@1": (1.2e-07, 1.4e-07, 3.1e-06, 5.8e-07),
    "trilinear-scale2-1x65535x1x2x2@1": (5.7e-08, 5.7e-08, 4.9e-07, 1.0e-07),
    "trilinear-scale2-1x65536x1x2x3@1": (7.7e-08, 7.2e-08, 3.5e-07, 1.2e-07),
    "trilinear-scale2-1x65537x1x4x8@1": (9.2e-08, 8.7e-08, 3.6e-07, 1.7e-07),
    "avgpool-1x65535x1x2x4@1": (4.2e-08, 4.2e-08, 1.4e-08, 1.7e-08),
    "avgpool-1x65536x1x2x4@1": (4.2e-08, 4.2e-08, 1.5e-08, 1.7e-08),
    "focal-1x64x5x7@1": (6.0e-07, 4.9e-07, 3.2e-07, 3.1e-07),
    "focal-1x65x5x7@1": (2.3e-07, 4.1e-07, 5.9e-07, 2.6e-07),
    "focal-1x256x3x5@1": (3.8e-07, 3.0e-07, 4.2e-07, 4.8e-07),
    "focal-1x64x5x7@20": (5.8e-07, 5.0e-07, 3.5e-07, 3.3e-07),
    "focal-1x65x5x7@20": (2.8e-07, 4.1e-07, 5.7e-07, 2.6e-07),
    "focal-1x256x3x5@20": (4.3e-07, 3.6e-07, 4.4e-07, 5.0e-07),
}


def run(case):
    from dcanet_amd import ops
    return H.evaluate(case, torch.float32, DEV, H.public_op(ops))


def check(case):
    ref, exact = H.truth(case)
    yard = H.yardstick(case)
    got, got_exact = run(case)
    torch.cuda.synchronize()
    sib_mag, sib_tol = H.SIBLING[case.family]
    print(f"{case.id}: {case.branch}")
    failures, worst = [], {"fwd": (0.0, 0.0), "grad": (0.0, 0.0)}
    for name, want in ref.items():
        assert got[name].dtype == torch.float32 and got[name].shape == want.shape, name
        assert torch.isfinite(got[name]).all(), name
        y, e = yard[name], H.error(got[name], want)
        print(f"  {name}: |ref|max {want.abs().max().item():.3e}  yardstick {y:.2e}  error {e:.2e}  gate {H.gate(y):.2e}")
        kind = "fwd" if name == "fwd" else "grad"
        if e >= worst[kind][1]:
            worst[kind] = (y, e)
        if e > H.gate(y):
            failures.append(f"{name}: {e:.3e} > max(4 x {y:.3e}, 2^-22)")
        if case.mag == sib_mag and e > sib_tol[name]:
            failures.append(f"{name}: {e:.3e} > the sibling's {sib_tol[name]:.0e}")
    print(f'  MEASURED "{case.id}": ({worst["fwd"][0]:.1e}, {worst["fwd"][1]:.1e}, {worst["grad"][0]:.1e}, '
          f'{worst["grad"][1]:.1e}),')
    for name, want in exact.items():
        mism = int((got_exact[name].cpu() != want).sum())
        print(f"  {name}: {mism} mismatches of {want.numel()}")
        if mism:
            failures.append(f"{name}: {mism} mismatches")
    assert not failures, f"{case.id} ({case.branch}): " + "; ".join(failures)


def ids(cases):
    return [c.id for c in cases]


@pytest.mark.parametrize("case", H.SOFTARGMIN, ids=ids(H.SOFTARGMIN))
def test_softargmin(case):
    check(case)


@pytest.mark.parametrize("case", H.UP_SOFTARGMIN, ids=ids(H.UP_SOFTARGMIN))
def test_up_softargmin(case):
    check(case)


@pytest.mark.parametrize("case", H.CONTEXT, ids=ids(H.CONTEXT))
def test_context_inject(case):
    check(case)


@pytest.mark.parametrize("case", H.ATTENTION, ids=ids(H.ATTENTION))
def test_disparity_attention(case):
    check(case)


@pytest.mark.parametrize("case", H.TRILINEAR, ids=ids(H.TRILINEAR))
def test_trilinear(case):
    check(case)


@pytest.mark.parametrize("case", H.AVGPOOL, ids=ids(H.AVGPOOL))
def test_avgpool(case):
    check(case)


@pytest.mark.parametrize("case", H.FOCAL, ids=ids(H.FOCAL))
def test_focal_loss(case):
    check(case)


def test_fallback_of_up_softargmin_is_the_unfused_pair():
    """the documented fall-back (n > 64, n < 2, other scales) is `softargmin(trilinear_upsample(.))`, bit for bit"""
    from dcanet_amd import ops
    for case in H.UP_SOFTARGMIN:
        if not case.branch.startswith("fallback"):
            continue
        x = H.inputs(case)[0]["x"].to(DEV)
        want = ops.softargmin(ops.trilinear_upsample(x.unsqueeze(1), case.p["scale"]).squeeze(1))
        assert torch.equal(ops.up_softargmin(x, case.p["scale"]), want), case.id


LARGEST = [max(cases, key=lambda c: H.prod(c.shape)) for cases in H.FAMILIES.values()]


@pytest.mark.parametrize("case", LARGEST, ids=ids(LARGEST))
def test_two_calls_are_bit_identical(case):
    """each family at its largest case (the order-fixed class sums of context injection with 8202 blocks among them)"""
    (a, ea), (b, eb) = run(case), run(case)
    print(f"{case.id}: {case.branch}")
    assert all(torch.equal(a[k], b[k]) for k in a) and all(torch.equal(ea[k], eb[k]) for k in ea)
