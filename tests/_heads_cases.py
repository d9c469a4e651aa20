"""Case tables, input builders, float64 references and yardsticks for the head and DCA kernels: the soft-argmin family
(csrc/volume.hip), the fused up-sampling head (csrc/up_softargmin.hip), context injection and disparity attention
(csrc/context_attention.hip), trilinear interpolation and average pooling (csrc/pointwise.hip) and the stereo focal loss
(csrc/heads2d.hip).  Importable without a GPU: tests/test_heads_cases_cpu.py checks what the tables claim,
tests/test_gpu_heads_dca_fp64.py runs the kernels against them.

A case is one launch branch of one kernel.  Its row names the shape, the magnitude of the inputs, the branch it exists for
(printed when the case runs) and the arithmetic that puts the shape on that branch, written with the launchers' constants
restated below.  The truth is the dtype-generic oracle (oracle/dcanet_oracle.py, ATen for softmax / interpolate / pooling)
evaluated in float64 and differentiated by autograd; the yardstick is the error of the SAME functions in float32 on the CPU.
Errors use the metric of the parity tests' `close()`: max |a - ref| / max(1, max |ref|), per output and per gradient."""
import functools
from dataclasses import dataclass, field
from typing import Callable

import torch
import torch.nn.functional as F

from oracle import dcanet_oracle as O
from oracle.seeded import seeded_tensor

# ---- launcher constants, restated ----------------------------------------------------------------------------------------------
VOL_EW_CAP = 4096 * 256     # csrc/volume.hip:398-401  ew_grid: at most 4096 blocks of 256 threads, then a grid-stride loop
EW_CAP = 8192 * 256         # csrc/context_attention.hip:437-440, csrc/pointwise.hip:971-974 ew_grid; csrc/up_softargmin.hip:188 g2
GRID_YZ = 65535             # csrc/pointwise.hip:1138 (avg-pool forward), :1166 / :1179 / :1185 (x2 trilinear): NC * D as grid.z
UP_NMAX = 64                # csrc/up_softargmin.hip:16  planes in dynamic LDS: n * 256 floats
UP_SCALES = (2, 4, 8)       # csrc/up_softargmin.hip:171; ops.py:310 falls back to the unfused kernels otherwise
BLOCK = 256                 # threads per workgroup of every kernel here except attention backward for n > 32 and focal K > 64
LDS_64K = 64 * 1024
FL_NT_SWITCH = 64           # csrc/heads2d.hip:287, :308  nt = K <= 64 ? 256 : 64
FL_KMAX = 256               # csrc/heads2d.hip:105
ATTN_NMAX = 64              # csrc/context_attention.hip:487

FACTOR, FLOOR = 4.0, 2.0 ** -22
MAX_INPUT_BYTES = 64 << 20
MARGIN = 0.05               # added to the winning logit of every pixel of a context case
MIN_GAP = 1e-4              # smallest float64 top-2 probability gap a context case may have away from its constructed ties


def gate(yardstick):
    """FACTOR x the float32 oracle's own error; the floor is the fp32 format's (three rounded operations, 2^-24 each, and
    exact float32 results make the yardstick 0)"""
    return max(FACTOR * yardstick, FLOOR)


def cdiv(a, b):
    return -(-a // b)


def prod(t):
    r = 1
    for v in t:
        r *= int(v)
    return r


@dataclass(frozen=True, eq=False)
class Case:
    family: str
    shape: tuple
    mag: float
    branch: str                       # what the case exists for; printed when it runs
    arith: Callable[[], bool]         # the launcher arithmetic that puts `shape` on that branch
    p: dict = field(default_factory=dict)

    @property
    def id(self):
        extra = "-".join(f"{k}{v}" for k, v in self.p.items())
        return f"{self.family}{'-' + extra if extra else ''}-{'x'.join(map(str, self.shape))}@{self.mag:g}"


# ---- soft-argmin family: ops.softmax_dim1 / softargmin / regression on (B, K, H, W) --------------------------------------------
def _sa(shape, mag, branch, arith):
    return [Case("softargmin", shape, mag, f"mode {m}: {branch}", arith, {"mode": m}) for m in (0, 1, 2)]


def _sa_threads(s):
    return s[0] * s[2] * s[3]           # one thread per (b, pixel): volume.hip:343, :509


SOFTARGMIN = (
    _sa((1, 1, 3, 5), 2.0, "K = 1, one partial block",
        lambda s=(1, 1, 3, 5): s[1] == 1 and _sa_threads(s) < BLOCK)
    + [c for mag in (2.0, 30.0, 80.0) for c in
       _sa((3, 48, 7, 37), mag, "four blocks, idx >= total tail in the last, K = 48, logits up to ~4 x magnitude",
           lambda s=(3, 48, 7, 37): BLOCK < _sa_threads(s) <= VOL_EW_CAP and _sa_threads(s) % BLOCK != 0)]
    + _sa((1, 192, 4, 6), 2.0, "K = 192", lambda s=(1, 192, 4, 6): s[1] == 192)
    + _sa((1, 2, 1025, 1024), 2.0, "grid-stride iteration: 1,049,600 threads > 4096 * 256",
          lambda s=(1, 2, 1025, 1024): VOL_EW_CAP < _sa_threads(s) < 2 * VOL_EW_CAP)
)


# ---- fused head: ops.up_softargmin on (B, n, hc, wc) ---------------------------------------------------------------------------
def _up(scale, shape, mag, branch, arith):
    return Case("up_softargmin", shape, mag, branch, arith, {"scale": scale})


def _up_fused(scale, s):
    return 2 <= s[1] <= UP_NMAX and scale in UP_SCALES          # ops.py:310, up_softargmin.hip:170-171


UP_SOFTARGMIN = [
    _up(4, (2, 6, 5, 7), 2.0, "S = 4 instantiation, B = 2", lambda: _up_fused(4, (2, 6, 5, 7))),
    _up(4, (2, 6, 5, 7), 30.0, "S = 4 instantiation, B = 2, saturated", lambda: _up_fused(4, (2, 6, 5, 7))),
    _up(4, (1, 48, 3, 5), 2.0, "S = 4, n = 48 (192 bins, the baseline head)", lambda: _up_fused(4, (1, 48, 3, 5))),
    _up(4, (1, 48, 3, 5), 30.0, "S = 4, n = 48, saturated", lambda: _up_fused(4, (1, 48, 3, 5))),
    _up(8, (1, 64, 2, 3), 2.0, "n = NMAX = 64: exactly 64 KiB of dynamic LDS",
        lambda: _up_fused(8, (1, 64, 2, 3)) and 64 * BLOCK * 4 == LDS_64K),            # up_softargmin.hip:173 lds = n * 256 * 4
    _up(8, (1, 2, 1, 1), 2.0, "n = 2 on one coarse cell: every source index clamps", lambda: _up_fused(8, (1, 2, 1, 1))),
    _up(8, (1, 4, 2, 33), 2.0, "W = 264: blockIdx.x = 1 and the x >= W exit",
        lambda: _up_fused(8, (1, 4, 2, 33)) and BLOCK < 8 * 33 < 2 * BLOCK),           # up_softargmin.hip:78-79, :172
    _up(8, (1, 24, 4, 6), 30.0, "S = 8, saturated soft-max (online rescaling)", lambda: _up_fused(8, (1, 24, 4, 6))),
    _up(2, (2, 3, 3, 129), 2.0, "S = 2, W = 258: blockIdx.x = 1 and the x >= W exit",
        lambda: _up_fused(2, (2, 3, 3, 129)) and BLOCK < 2 * 129 < 2 * BLOCK),
    _up(2, (1, 2, 1025, 1024), 2.0, "bwd2 grid-stride iteration: 2,099,200 coarse voxels > 8192 * 256",
        lambda: _up_fused(2, (1, 2, 1025, 1024)) and EW_CAP < prod((1, 2, 1025, 1024)) < 2 * EW_CAP
        and 2 * 1025 <= GRID_YZ),                                                       # up_softargmin.hip:187-188, :171
    _up(2, (1, 65, 2, 3), 2.0, "fallback: n = 65 > NMAX", lambda: not _up_fused(2, (1, 65, 2, 3)) and 65 > UP_NMAX),
    _up(8, (1, 1, 3, 4), 2.0, "fallback: n = 1 < 2", lambda: not _up_fused(8, (1, 1, 3, 4)) and 1 < 2),
    _up(3, (1, 4, 2, 3), 2.0, "fallback: scale 3", lambda: not _up_fused(3, (1, 4, 2, 3)) and 3 not in UP_SCALES),
]


# ---- context injection: ops.context_inject on x (B, C, n, H, W), preds (B, n, H, W) --------------------------------------------
def _ctx(shape, mag, branch, arith, build="margin"):
    return Case("context", shape, mag, branch, arith, {"build": build})


def _ctx_quads(s):
    """pixel quads per plane if ctx_scale_launch takes ctx_scale4_kernel (context_attention.hip:445), else 0"""
    hw = s[3] * s[4]
    return hw // 4 if hw % 4 == 0 and s[1] * s[2] <= GRID_YZ else 0


def _ctx_nblk(s):
    return cdiv(s[3] * s[4], BLOCK)     # context_attention.hip:460, :475


_C9 = (2, 8, 6, 9, 13)
CONTEXT = [
    _ctx((2, 8, 6, 28, 40), 1.5, "ctx_scale4_kernel with HW/4 = 280 > 256 (blockIdx.x = 1, q >= HWq exit), nblk = 5",
         lambda s=(2, 8, 6, 28, 40): BLOCK < _ctx_quads(s) < 2 * BLOCK and _ctx_nblk(s) == 5),
    _ctx((1, 8, 64, 5, 9), 1.5, "n = 64 classes (cva without down-sampling), flat ctx_scale_kernel",
         lambda s=(1, 8, 64, 5, 9): s[2] == 64 and _ctx_quads(s) == 0),
    _ctx((1, 8, 4, 257, 257), 1.5, "flat ctx_scale_kernel grid-stride iteration: 2,113,568 elements > 8192 * 256, nblk = 259",
         lambda s=(1, 8, 4, 257, 257): _ctx_quads(s) == 0 and EW_CAP < prod(s) < 2 * EW_CAP and _ctx_nblk(s) == 259),
    _ctx((1, 1, 2, 1449, 1449), 1.5, "ctx_bwd_preds_kernel grid-stride iteration: 2,099,601 pixels > 8192 * 256",
         lambda s=(1, 1, 2, 1449, 1449): EW_CAP < s[0] * s[3] * s[4] < 2 * EW_CAP and _ctx_quads(s) == 0),   # :479
    _ctx(_C9, 1.5, "B = 2, odd map, unit magnitude", lambda: _ctx_quads(_C9) == 0 and _ctx_nblk(_C9) == 1),
    _ctx(_C9, 40.0, "saturated soft-max over the classes", lambda: _ctx_quads(_C9) == 0),
    _ctx(_C9, 1.5, "exact ties on a checkerboard: the lowest index among the maxima wins (ctx_stats_kernel `p > best`)",
         lambda: _C9[2] >= 3, "tie"),
    _ctx(_C9, 1.5, "a class empty in batch element 0 and present in element 1 (denom = T = 0 for it)",
         lambda: _C9[0] == 2, "absent"),
]
ABSENT_CLASS = 2


# ---- disparity attention: ops.disparity_attention on q, k, v (B, C, n, H, W) ---------------------------------------------------
def _at(shape, mag, branch, arith):
    return Case("attention", shape, mag, branch, arith)


def _qpt(s):
    return (s[2] + 7) // 8              # context_attention.hip:491, :519


def _at_quads(s):
    return (s[3] * s[4]) % 4 == 0       # context_attention.hip:172  16-byte buffer staging, else the scalar loop


ATTENTION = [
    _at((1, 8, 49, 2, 7), 1.0, "QPT = 7 (n = 49), scalar staging, backward PW = 16, forward LDS > 64 KiB",
        lambda s=(1, 8, 49, 2, 7): _qpt(s) == 7 and not _at_quads(s) and s[2] > 32 and 2 * 8 * s[2] * 32 * 4 > LDS_64K),
    _at((1, 8, 56, 3, 4), 1.0, "QPT = 7 (n = 56), HW % 4 == 0 buffer staging, backward PW = 16",
        lambda s=(1, 8, 56, 3, 4): _qpt(s) == 7 and _at_quads(s) and s[2] > 32 and s[2] <= ATTN_NMAX),
    _at((2, 16, 40, 3, 6), 1.0, "B = 2 and two heads with n = 40 (QPT = 5)",
        lambda s=(2, 16, 40, 3, 6): s[0] > 1 and s[1] // 8 == 2 and _qpt(s) == 5),
    _at((1, 32, 24, 5, 13), 6.0, "scores of tens of units: the online soft-max rescales (corr) at almost every key; "
        "three pixel blocks, the last partial", lambda s=(1, 32, 24, 5, 13): _qpt(s) == 3 and cdiv(s[3] * s[4], 32) == 3
        and (s[3] * s[4]) % 32 != 0),
]


# ---- trilinear interpolation and average pooling on (N, C, D, H, W) ------------------------------------------------------------
def _tl(scale, shape, branch, arith):
    return Case("trilinear", shape, 1.0, branch, arith, {"scale": scale})


def _tl_up2(scale, s):
    return scale == 2 and s[3] <= GRID_YZ and s[0] * s[1] * s[2] <= GRID_YZ         # pointwise.hip:1166, :1179, :1185


TRILINEAR = [
    _tl(4, (2, 3, 2, 3, 5), "generic kernels at scale 4", lambda: not _tl_up2(4, (2, 3, 2, 3, 5))),
    _tl(8, (1, 1, 2, 9, 229), "generic forward grid-stride iteration: 2,110,464 outputs > 8192 * 256",
        lambda s=(1, 1, 2, 9, 229): not _tl_up2(8, s) and EW_CAP < prod(s) * 8 ** 3 < 2 * EW_CAP),     # pointwise.hip:1171
    _tl(2, (1, 65535, 1, 2, 2), "NC * Di = 65535: the x2 kernels (up2 forward, tiled backward)",
        lambda s=(1, 65535, 1, 2, 2): _tl_up2(2, s) and s[0] * s[1] * s[2] == GRID_YZ and s[4] % 2 == 0),
    _tl(2, (1, 65536, 1, 2, 3), "NC * Di = 65536: scale 2 on the generic kernels (forward takes a grid-stride iteration)",
        lambda s=(1, 65536, 1, 2, 3): not _tl_up2(2, s) and s[0] * s[1] * s[2] == GRID_YZ + 1 and prod(s) * 8 > EW_CAP),
    _tl(2, (1, 65537, 1, 4, 8), "generic backward grid-stride iteration: 2,097,184 inputs > 8192 * 256",
        lambda s=(1, 65537, 1, 4, 8): not _tl_up2(2, s) and EW_CAP < prod(s) < 2 * EW_CAP),             # pointwise.hip:1190
]


def _ap(shape, branch, arith):
    return Case("avgpool", shape, 1.0, branch, arith)


def _ap_tiled(s):
    return s[4] % 4 == 0 and s[0] * s[1] * ((s[2] + 1) // 2) <= GRID_YZ                # pointwise.hip:1138


AVGPOOL = [
    _ap((1, 65535, 1, 2, 4), "NC * Do = 65535: tiled forward", lambda s=(1, 65535, 1, 2, 4): _ap_tiled(s)
        and s[1] * ((s[2] + 1) // 2) == GRID_YZ),
    _ap((1, 65536, 1, 2, 4), "NC * Do = 65536: direct forward with Wi % 4 == 0",
        lambda s=(1, 65536, 1, 2, 4): not _ap_tiled(s) and s[4] % 4 == 0 and s[1] * ((s[2] + 1) // 2) == GRID_YZ + 1),
]


# ---- focal loss: ops.focal_loss_levels on two estimates (B, K, H, W), ground truth at their resolution -------------------------
FOCAL_WEIGHTS, FOCAL_COEF = (0.5, 0.7), 5.0


def _fl(shape, mag, branch, arith):
    return Case("focal", shape, mag, branch, arith)


FOCAL = [c for mag in (1.0, 20.0) for c in (
    _fl((1, 64, 5, 7), mag, "K = 64: the last K on NT = 256", lambda: 64 <= FL_NT_SWITCH),
    _fl((1, 65, 5, 7), mag, "K = 65: the first K on NT = 64", lambda: FL_NT_SWITCH < 65 <= FL_KMAX),
    _fl((1, 256, 3, 5), mag, "K = 256 = FL_KMAX: 64 KiB of LDS with NT = 64",
        lambda: 256 == FL_KMAX and 256 * 64 * 4 == LDS_64K),                             # heads2d.hip:295 K * 64 * sizeof(float)
)]

FAMILIES = {"softargmin": SOFTARGMIN, "up_softargmin": UP_SOFTARGMIN, "context": CONTEXT, "attention": ATTENTION,
            "trilinear": TRILINEAR, "avgpool": AVGPOOL, "focal": FOCAL}
ALL = [c for cases in FAMILIES.values() for c in cases]
assert len({c.id for c in ALL}) == len(ALL)

# the fixed tolerances of each family's sibling in tests/test_gpu_parity.py / tests/test_gpu_heads.py and the magnitude that
# sibling runs at: a case at that magnitude has to meet them too
SIBLING = {
    "softargmin": (2.0, {"fwd": 2e-6, "d x": 1e-5}),
    "up_softargmin": (2.0, {"fwd": 2e-6, "d x": 2e-5}),
    "context": (1.5, {"fwd": 2e-6, "d x": 2e-6, "d preds": 2e-5}),
    "attention": (1.0, {"fwd": 5e-6, "d q": 1e-5, "d k": 1e-5, "d v": 1e-5}),
    "trilinear": (1.0, {"fwd": 2e-6, "d x": 1e-5}),
    "avgpool": (1.0, {"fwd": 1e-6, "d x": 1e-6}),
    "focal": (1.0, {"fwd": 1e-5, "d est0": 1e-5, "d est1": 1e-5}),
}


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def lowest_argmax(p):
    """k* as the kernel defines it: the LOWEST index among the maxima of p over dim 1 (torch.argmax leaves ties open)"""
    n = p.shape[1]
    idx = torch.arange(n, device=p.device).view(1, n, 1, 1)
    return torch.where(p == p.amax(1, keepdim=True), idx, torch.full_like(idx, n)).amin(1)


def context_preds(case):
    """(preds, tie mask): seeded logits x magnitude with MARGIN added to the winning logit of every pixel, which bounds the
    top-2 probability gap below by about (1 - exp(-MARGIN)) / n whatever the map size.  build = "absent": plane ABSENT_CLASS
    of batch element 0 is pushed below everything first.  build = "tie": on a checkerboard the winning plane is then copied
    bitwise into its upper neighbour (into the lower one where the winner is the last plane), so two maxima are exactly
    equal and the lower index has to win."""
    B, _, n, H, W = case.shape
    preds = seeded_tensor(f"hc.ctx.p{case.shape}", (B, n, H, W)) * case.mag
    build = case.p["build"]
    if build == "absent":
        preds[0, ABSENT_CLASS] = preds.min() - 1.0
    win = preds.argmax(1, keepdim=True)
    preds = preds + MARGIN * torch.zeros_like(preds).scatter_(1, win, 1.0)
    win = preds.argmax(1, keepdim=True)
    tie = torch.zeros(B, H, W, dtype=torch.bool)
    if build == "tie":
        yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
        tie = ((yy + xx) % 2 == 0).expand(B, H, W).clone()
        partner = torch.where(win < n - 1, win + 1, win - 1)
        copied = preds.scatter(1, partner, preds.gather(1, win))
        preds = torch.where(tie.unsqueeze(1), copied, preds)
    return preds, tie


def inputs(case):
    """{name: float32 CPU tensor} of the differentiated inputs, and {name: tensor} of the rest"""
    s, tag = case.shape, f"hc.{case.family}.{case.shape}"
    f = case.family
    if f in ("softargmin", "up_softargmin", "trilinear", "avgpool"):
        return {"x": seeded_tensor(tag + ".x", s) * case.mag}, {}
    if f == "context":
        preds, tie = context_preds(case)
        return {"x": seeded_tensor(tag + ".x", s), "preds": preds}, {"tie": tie}
    if f == "attention":
        return {n: seeded_tensor(f"{tag}.{n}", s) * case.mag for n in "qkv"}, {}
    if f == "focal":
        B, K, H, W = s
        gt = torch.rand(B, 1, H, W, generator=torch.Generator().manual_seed(K)) * (K + 8.0) - 4.0      # [-4, K + 4)
        return {f"est{i}": seeded_tensor(f"{tag}.e{i}", s) * case.mag for i in range(len(FOCAL_WEIGHTS))}, {"gt": gt}
    raise KeyError(f)


def input_bytes(case):
    a, b = inputs(case)
    return sum(t.numel() * t.element_size() for t in list(a.values()) + list(b.values()))


# ---- the operation of a case: as the oracle states it, and as ops.py serves it --------------------------------------------------
def reference(case, t, other):
    """(output, {name: exact integer result}) from the dtype-generic oracle functions on the tensors `t`"""
    f, p = case.family, case.p
    if f == "softargmin":
        K = case.shape[1]
        if p["mode"] == 0:
            return F.softmax(t["x"], 1), {}
        return O.disparity_regression(F.softmax(t["x"], 1) if p["mode"] == 1 else t["x"], K), {}
    if f == "up_softargmin":
        up = F.interpolate(t["x"].unsqueeze(1), scale_factor=(p["scale"],) * 3, mode="trilinear").squeeze(1)
        return O.disparity_regression(F.softmax(up, 1), p["scale"] * case.shape[1]), {}
    if f == "context":
        key, kstar, _ = O.context_inject(t["x"], t["preds"])
        want = lowest_argmax(F.softmax(t["preds"].detach(), 1))
        assert torch.equal(kstar, want), "the oracle's argmax did not return the lowest index among the maxima"
        return key, {"kstar": kstar}
    if f == "attention":
        return O.disparity_attention_core(t["q"], t["k"], t["v"]), {}
    if f == "trilinear":
        return F.interpolate(t["x"], scale_factor=(p["scale"],) * 3, mode="trilinear"), {}
    if f == "avgpool":
        # AvgPool3d(3, 2, 1) with count_include_pad: ATen refuses a dimension below the kernel size even where the padding
        # makes up for it (D = 1 here), so the zero padding is made explicit -- the same sums over the same 27 taps
        return F.avg_pool3d(F.pad(t["x"], (1, 1, 1, 1, 1, 1)), (3, 3, 3), stride=2, padding=0), {}
    if f == "focal":
        gt, K = other["gt"].to(t["est0"].dtype), case.shape[1]
        return sum(w * O.stereo_focal_loss_level(t[f"est{i}"], gt, K, FOCAL_COEF, False)
                   for i, w in enumerate(FOCAL_WEIGHTS)), {}
    raise KeyError(f)


def public_op(ops):
    """the same operations through the public ops of `ops` (the package's ops.py) on device tensors"""
    def call(case, t, other):
        f, p = case.family, case.p
        if f == "softargmin":
            return (ops.softmax_dim1, ops.softargmin, ops.regression)[p["mode"]](t["x"]), {}
        if f == "up_softargmin":
            return ops.up_softargmin(t["x"], p["scale"]), {}
        if f == "context":
            key, kstar = ops.context_inject(t["x"], t["preds"])
            return key, {"kstar": kstar.view(other["tie"].shape).long()}
        if f == "attention":
            return ops.disparity_attention(t["q"], t["k"], t["v"]), {}
        if f == "trilinear":
            return ops.trilinear_upsample(t["x"], p["scale"]), {}
        if f == "avgpool":
            return ops.avg_pool3d_k3s2p1(t["x"]), {}
        if f == "focal":
            return ops.focal_loss_levels([t[f"est{i}"] for i in range(len(FOCAL_WEIGHTS))], other["gt"], FOCAL_WEIGHTS,
                                         FOCAL_COEF), {}
        raise KeyError(f)
    return call


def seed_scale(case):
    """Factor on the gradient seed.  The injection weight of a pixel is a soft-max over the pixels of its class, about n / HW,
    and d preds is proportional to it: 2e-6 on the two-megapixel map with a unit seed, where the metric's max(1, max |ref|)
    would turn the relative gate into an absolute one that an unwritten element passes.  A seed of HW / n brings d preds to
    the order of 1 (and d x to HW / n, which the relative metric does not mind)."""
    if case.family == "context":
        return max(1.0, case.shape[3] * case.shape[4] / case.shape[2])
    return 1.0


def evaluate(case, dtype, device="cpu", call=reference):
    """forward and all gradients of one case: ({"fwd": out, "d <input>": gradient, ...}, {exact results}), detached, on
    `device`.  The gradient seed is a seeded tensor of the output's shape times `seed_scale` (1 for the scalar loss), rounded
    to float32 before it is cast, so every precision gets the same seed."""
    t, other = inputs(case)
    t = {k: v.to(device=device, dtype=dtype).requires_grad_() for k, v in t.items()}
    other = {k: v.to(device) for k, v in other.items()}
    out, exact = call(case, t, other)
    if out.dim() == 0:
        seed = torch.ones((), dtype=out.dtype, device=out.device)
    else:
        seed = (seeded_tensor(f"hc.{case.family}.{case.shape}.g", out.shape) * seed_scale(case)).to(device=out.device,
                                                                                                     dtype=out.dtype)
    grads = torch.autograd.grad((out * seed).sum(), list(t.values()))
    res = {"fwd": out.detach()}
    res.update({f"d {k}": g for k, g in zip(t, grads)})
    return res, {k: v.detach() for k, v in exact.items()}


def error(a, ref):
    """the metric of `close()` in tests/test_gpu_parity.py: max |a - ref| / max(1, max |ref|)"""
    a, ref = a.detach().cpu().double(), ref.detach().cpu().double()
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return (a - ref).abs().max().item() / max(1.0, ref.abs().max().item())


@functools.lru_cache(maxsize=4)
def truth(case):
    """the float64 results of a case on the CPU; computed once, never modified"""
    return evaluate(case, torch.float64)


@functools.lru_cache(maxsize=None)
def yardstick(case):
    """{output or gradient name: error of the float32 CPU oracle against the float64 one}"""
    ref, exact = truth(case)
    got, exact32 = evaluate(case, torch.float32)
    assert all(torch.equal(exact[k], exact32[k]) for k in exact), "float32 and float64 oracle disagree on an exact result"
    return {k: error(got[k], ref[k]) for k in ref}
