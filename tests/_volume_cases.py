"""Case tables, input builders, float64 references and yardsticks for the cost-volume kernels: the separate builders and
their backward kernels (csrc/volume.hip: gwc_fwd_kernel, gwc_bwd_kernel, gwc_bwd_blocked_kernel, concat_fwd_kernel,
concat_bwd_kernel) and the fused builder (csrc/volume_fused.hip: gwc_fused_kernel, concat_fused_kernel).  Importable without a
GPU: tests/test_volume_cases_cpu.py checks what the tables claim, tests/test_gpu_volume_fp64.py runs the kernels against them.

A case is one launch branch.  Its row names the shape, the branch it exists for (printed when the case runs) and the
arithmetic that puts the shape on that branch, written with the launchers' constants and the blocked / plain predicate of
`gwc_bwd_blocked_rows` restated below.  The GPU test asks the library which backward kernel serves a shape
(`dca_gwc_volume_bwd_rows`) and requires the answer to equal the restated one before it compares anything.

The truth is `O.build_gwc_volume` / `O.build_concat_volume` (oracle/dcanet_oracle.py) on float64 leaves, differentiated by
autograd; the yardstick is the error of the SAME functions in float32 on the CPU.  Errors use the metric of the parity tests'
`close()`: max |a - ref| / max(1, max |ref|), per output and per gradient."""
import functools
from dataclasses import dataclass, field
from typing import Callable

import torch

from oracle import dcanet_oracle as O
from oracle.seeded import seeded_tensor

from _heads_cases import FACTOR, FLOOR, MAX_INPUT_BYTES, cdiv, error, gate, prod  # noqa: F401  (one gate for both files)

# ---- launcher constants, restated (csrc/volume.hip unless another file is named) ------------------------------------------------
SEG = 12                      # :31   gwc_fwd_kernel: disparities per work item; items = ceil(W / 4) * ceil(D / SEG), 256 per pass
BLOCK = 256                   # gwc_fwd_kernel, gwc_bwd_kernel, the concat kernels, gwc_fused_kernel
WG_TARGET = 1280              # :425  gwc_bwd_blocked_rows: gx = ceil(1280 / (G * B)), clipped to [1, H]
GV_QUADS = 3072               # :420  D * (W / 4) <= 3072: six 16-byte quads of gv per thread of 512 (KG = 6, :162)
LR_QUADS = 512                # :421  CPG * (W / 4) <= 512: one quad of L and of R per thread (KC = 1, :162)
BLOCKED_LDS_MAX = 80 * 1024   # :421  (D + 2 CPG) * (W + D + 4) * 4 bytes (:414)
LDS_ATTR = 64 * 1024          # :407, :435; volume_fused.hip:164  above it the launcher raises the kernel's dynamic-LDS limit
LDS_REFUSE = 160 * 1024       # :453, :468; volume_fused.hip:163  above it the entry returns hipErrorInvalidValue
VOL_EW_CAP = 4096 * 256       # :398-401  ew_grid of the concat kernels: at most 4096 blocks of 256, then a grid-stride loop
FUSED_EW_CAP = 8192 * 256     # volume_fused.hip:192-194  concat_fused_kernel: one thread per x quad, at most 8192 blocks
OFF31 = 0x7ffffff0            # :421-422  byte offsets of the buffer loads inside one (b, g) plane fit 31 bits
CPGS = (1, 2, 4, 8, 16)       # :470, :482-486  instantiations; anything else is refused


def blocked_lds(cpg, W, D):
    """:414 gwc_bwd_blocked_lds"""
    return (D + 2 * cpg) * (W + D + 4) * 4


def plain_bwd_lds(cpg, W, D):
    """:434 gwc_bwd_kernel"""
    return (D + 2 * cpg) * W * 4


def fwd_lds(cpg, W):
    """:406 gwc_fwd_kernel"""
    return 2 * cpg * W * 4


def fused_lds(cpg, W, D):
    """volume_fused.hip:161-162"""
    return cpg * (2 * W + ((D + 3) & ~3)) * 4


def blocked_terms(B, C, G, H, W, D):
    """:420-422 the shape part of the blocked / plain choice, term by term"""
    cpg = C // G
    return {
        "cpg": cpg <= 8 and cpg % 2 == 0,
        "W%4": W % 4 == 0,
        "W<=256": W <= 256,
        "D%4": D % 4 == 0,
        "D>=6cpg": D >= 6 * cpg,
        "gv quads": D * (W // 4) <= GV_QUADS,
        "lr quads": cpg * (W // 4) <= LR_QUADS,
        "lds": blocked_lds(cpg, W, D) <= BLOCKED_LDS_MAX,
        "off31": D * H * W * 4 < OFF31 and cpg * H * W * 4 < OFF31,
    }


def accepted(B, C, G, H, W, D):
    """:465-471 gwc_bwd_shape_ok"""
    if min(B, C, G, H, W, D) <= 0 or C % G or max(H, G, B) > 65535:
        return False
    return plain_bwd_lds(C // G, W, D) <= LDS_REFUSE and C // G in CPGS


def bwd_rows(B, C, G, H, W, D):
    """dca_gwc_volume_bwd_rows restated: grid.x of gwc_bwd_blocked_kernel (:419-428), 0 = gwc_bwd_kernel, -1 = refused"""
    if not accepted(B, C, G, H, W, D):
        return -1
    if not all(blocked_terms(B, C, G, H, W, D).values()):
        return 0
    return max(1, min(H, cdiv(WG_TARGET, G * B)))


def only_fails(shape, term):
    """the shape is on the plain kernel because of exactly this term of the predicate"""
    t = blocked_terms(*shape)
    return [k for k, v in t.items() if not v] == [term]


def trips(H, gx):
    """rows walked by each workgroup x of the blocked kernel: y = x, x + gx, ... < H"""
    return [cdiv(H - x, gx) for x in range(gx)]


def fwd_items(W, D):
    """gwc_fwd_kernel :32-34  (x quads) x (disparity segments)"""
    return cdiv(W, 4) * cdiv(D, SEG)


def fused_iq_trips(W, D):
    """volume_fused.hip:86-99  trips of the `iq += rows` loop of the thread rows iq0 = 0 .. rows - 1 (WQ <= 256)"""
    WQ, DQ = W // 4, (D + 3) // 4
    rows = max(1, BLOCK // WQ)
    return [cdiv(DQ - r, rows) for r in range(min(rows, DQ))]


# ---- the tables ----------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True, eq=False)
class Case:
    family: str                       # gwc | concat | fused
    shape: tuple                      # gwc / fused: (B, C, G, H, W, D); concat: (B, C, H, W, D)
    branch: str                       # what the case exists for; printed when it runs
    arith: Callable[[], bool]         # the launcher arithmetic that puts `shape` on that branch
    regimes: tuple = ()               # names that tests/test_volume_cases_cpu.py requires to be present
    p: dict = field(default_factory=dict)

    @property
    def id(self):
        extra = "-".join(f"{k}{'+'.join(map(str, v)) if isinstance(v, tuple) else v}" for k, v in self.p.items())
        return f"{self.family}{'-' + extra if extra else ''}-{'x'.join(map(str, self.shape))}"

    @property
    def cpg(self):
        return self.shape[1] // self.shape[2] if self.family != "concat" else 1

    @property
    def rows(self):
        """restated dca_gwc_volume_bwd_rows of the case's backward launch (None for the concat family)"""
        return None if self.family == "concat" else bwd_rows(*self.shape)


def _g(shape, branch, arith, *regimes):
    return Case("gwc", shape, branch, arith, regimes)


def _blk(s, gx, cpg, extra=True):
    return bwd_rows(*s) == gx and s[1] // s[2] == cpg and extra


_S = {  # the blocked rows
    "deep": (2, 320, 40, 40, 16, 48),
    "hot": (1, 320, 40, 35, 240, 48),
    "gx1": (1, 2560, 1280, 3, 8, 12),
    "cpg4-full": (1, 16, 4, 2, 256, 24),
    "cpg2-idle": (1, 8, 4, 2, 256, 12),
    "D>W": (1, 16, 2, 3, 8, 48),
    "edge-quads": (1, 8, 1, 2, 236, 52),
    "edge-lds": (1, 8, 1, 2, 216, 56),
    "cpg4-walk": (2, 256, 64, 12, 32, 24),
    "cpg2-walk": (1, 128, 64, 23, 64, 16),
}

GWC_BLOCKED = [
    _g(_S["deep"], "blocked <8>: gx 16 < H 40, ragged walk 3,3,...,2 trips; 12 blocks of four disparities, 3 per wave",
       lambda s=_S["deep"]: _blk(s, 16, 8) and trips(40, 16) == [3] * 8 + [2] * 8, "blocked-deep-ragged"),
    _g(_S["hot"], "blocked <8>: the training row width W 240, D 48; gx 32 < H 35: two trips for y % 32 < 3, else one",
       lambda s=_S["hot"]: _blk(s, 32, 8) and trips(35, 32) == [2] * 3 + [1] * 29 and blocked_lds(8, 240, 48) == 74752,
       "blocked-hot-two"),
    _g(_S["gx1"], "blocked <2>: G * B >= 1280 so gx 1, one workgroup walks all three rows; D == 6 CPG",
       lambda s=_S["gx1"]: _blk(s, 1, 2) and trips(3, 1) == [3] and s[5] == 6 * 2, "blocked-gx1", "blocked-cpg2-multitrip"),
    _g(_S["cpg4-full"], "blocked <4>: D == 6 CPG (the partial sums fill the whole gv image), W 256 = all 64 lanes active",
       lambda s=_S["cpg4-full"]: _blk(s, 2, 4) and s[5] == 6 * 4 and s[4] // 4 == 64, "blocked-cpg4-D6cpg"),
    _g(_S["cpg2-idle"], "blocked <2>: D == 6 CPG = 12: three blocks of four disparities, wave 3 has none",
       lambda s=_S["cpg2-idle"]: _blk(s, 2, 2) and s[5] == 12 and len(range(4 * 3, s[5], 16)) == 0, "blocked-cpg2-wave3-idle"),
    _g(_S["D>W"], "blocked <8>: D 48 > W 8: two active lanes, most disparities see only the zero pads",
       lambda s=_S["D>W"]: _blk(s, 3, 8) and s[5] > s[4] and s[4] // 4 == 2, "blocked-D>W"),
    _g(_S["edge-quads"], "blocked <8>: D % 16 != 0 (wave 0 gets a fourth block), 3068 quads <= 3072, 79424 B <= 80 KiB",
       lambda s=_S["edge-quads"]: _blk(s, 2, 8) and s[5] % 16 and s[5] * s[4] // 4 == 3068 and blocked_lds(8, 236, 52) == 79424
       and bwd_rows(1, 8, 1, 2, 240, 52) == 0, "blocked-edge-quads"),
    _g(_S["edge-lds"], "blocked <8>: D % 16 != 0, 79488 B of LDS: the last D at this width inside 80 KiB",
       lambda s=_S["edge-lds"]: _blk(s, 2, 8) and s[5] % 16 and blocked_lds(8, 216, 56) == 79488
       and blocked_lds(8, 216, 60) > BLOCKED_LDS_MAX, "blocked-edge-lds"),
    _g(_S["cpg4-walk"], "blocked <4>: gx 10 < H 12: two trips for y % 10 < 2, else one; D == 6 CPG",
       lambda s=_S["cpg4-walk"]: _blk(s, 10, 4) and trips(12, 10) == [2, 2] + [1] * 8, "blocked-cpg4-multitrip"),
    _g(_S["cpg2-walk"], "blocked <2>: gx 20 < H 23: two trips for y % 20 < 3, else one; four blocks, one per wave",
       lambda s=_S["cpg2-walk"]: _blk(s, 20, 2) and trips(23, 20) == [2] * 3 + [1] * 17, "blocked-cpg2-multitrip"),
]

# shapes one step outside the blocked predicate: gwc_bwd_kernel, and the query says 0
GWC_BOUNDARY = [
    _g((1, 8, 1, 2, 240, 52), "plain: 3120 quads of gv > 3072 (80512 B would fit); forward D % 12 != 0 with 300 items > 256",
       lambda s=(1, 8, 1, 2, 240, 52): bwd_rows(*s) == 0 and only_fails(s, "gv quads") and s[5] * s[4] // 4 == 3120
       and s[5] > SEG and s[5] % SEG and fwd_items(s[4], s[5]) == 300, "plain-quads", "fwd-partial-seg-second-pass"),
    _g((1, 8, 1, 2, 192, 64), "plain: 83200 B of blocked LDS > 80 KiB (3072 quads fit)",
       lambda s=(1, 8, 1, 2, 192, 64): bwd_rows(*s) == 0 and only_fails(s, "lds") and blocked_lds(8, 192, 64) == 83200
       and s[5] * s[4] // 4 == GV_QUADS, "plain-lds"),
    _g((1, 8, 1, 2, 16, 44), "plain: D 44 < 6 CPG = 48",
       lambda s=(1, 8, 1, 2, 16, 44): bwd_rows(*s) == 0 and only_fails(s, "D>=6cpg"), "plain-D<6cpg"),
    _g((1, 4, 2, 2, 260, 12), "plain: W 260 > 256",
       lambda s=(1, 4, 2, 2, 260, 12): bwd_rows(*s) == 0 and only_fails(s, "W<=256"), "plain-W>256"),
    _g((1, 32, 2, 2, 16, 96), "plain: CPG 16 (D 96 = 6 CPG)",
       lambda s=(1, 32, 2, 2, 16, 96): bwd_rows(*s) == 0 and only_fails(s, "cpg") and s[1] // s[2] == 16, "plain-cpg16"),
    _g((1, 4, 4, 2, 16, 8), "plain: CPG 1; forward D < 12",
       lambda s=(1, 4, 4, 2, 16, 8): bwd_rows(*s) == 0 and only_fails(s, "cpg") and s[1] // s[2] == 1 and s[5] < SEG,
       "plain-cpg1", "fwd-D<12"),
    _g((1, 8, 1, 2, 16, 50), "plain: D % 4 != 0",
       lambda s=(1, 8, 1, 2, 16, 50): bwd_rows(*s) == 0 and only_fails(s, "D%4"), "plain-D%4"),
]


def _tail(s, r):
    return bwd_rows(*s) == 0 and s[4] % 4 == r and not blocked_terms(*s)["W%4"]


GWC_PLAIN = [
    _g((1, 8, 2, 3, 17, 6), "non-vec kernels: W % 4 == 1 (forward tail of one x), CPG 4",
       lambda s=(1, 8, 2, 3, 17, 6): _tail(s, 1) and s[1] // s[2] == 4, "plain-W%4=1", "fwd-tail"),
    _g((2, 32, 4, 5, 18, 6), "non-vec kernels: W % 4 == 2, B 2, CPG 8",
       lambda s=(2, 32, 4, 5, 18, 6): _tail(s, 2) and s[1] // s[2] == 8, "plain-W%4=2"),
    _g((1, 4, 2, 2, 19, 5), "non-vec kernels: W % 4 == 3, CPG 2, odd D",
       lambda s=(1, 4, 2, 2, 19, 5): _tail(s, 3) and s[1] // s[2] == 2, "plain-W%4=3"),
    _g((1, 16, 1, 2, 40, 12), "plain vec <16>: CPG * W = 640 > 256, three passes of the item loop; forward D == 12",
       lambda s=(1, 16, 1, 2, 40, 12): bwd_rows(*s) == 0 and s[4] % 4 == 0 and cdiv(16 * s[4], BLOCK) == 3 and s[5] == SEG,
       "plain-second-item-pass", "fwd-D=12"),
    _g((1, 4, 2, 2, 6, 9), "plain non-vec: D 9 > W 6 (nl, nr clip at the row ends; forward: disparities without any x)",
       lambda s=(1, 4, 2, 2, 6, 9): bwd_rows(*s) == 0 and s[5] > s[4], "plain-D>W", "fwd-D>W"),
    _g((1, 16, 1, 2, 208, 48), "plain vec <16>: 66560 B of LDS > 64 KiB, the attribute branch of gwc_bwd_launch",
       lambda s=(1, 16, 1, 2, 208, 48): bwd_rows(*s) == 0 and plain_bwd_lds(16, 208, 48) == 66560 > LDS_ATTR, "plain-lds>64K"),
    _g((1, 16, 1, 2, 516, 5), "forward <16>: 66048 B of LDS > 64 KiB, the attribute branch of gwc_fwd_launch",
       lambda s=(1, 16, 1, 2, 516, 5): fwd_lds(16, 516) == 66048 > LDS_ATTR and bwd_rows(*s) == 0
       and LDS_ATTR < plain_bwd_lds(16, 516, 5) <= LDS_REFUSE, "fwd-lds>64K"),
]

GWC = GWC_BLOCKED + GWC_BOUNDARY + GWC_PLAIN


def _c(shape, branch, arith, *regimes):
    return Case("concat", shape, branch, arith, regimes)


def _cat_fwd(s):
    return s[0] * 2 * s[1] * s[4] * s[2] * s[3]


def _cat_bwd(s):
    return s[0] * s[1] * s[2] * s[3]


CONCAT = [
    _c((2, 3, 5, 18, 6), "one partial block each way, B 2",
       lambda s=(2, 3, 5, 18, 6): _cat_fwd(s) < VOL_EW_CAP and _cat_bwd(s) % BLOCK != 0, "concat-small"),
    _c((1, 2, 130, 509, 4), "concat_fwd_kernel grid-stride iteration: 1,058,720 elements > 4096 * 256; D 4, odd W",
       lambda s=(1, 2, 130, 509, 4): VOL_EW_CAP < _cat_fwd(s) < 2 * VOL_EW_CAP and _cat_bwd(s) < VOL_EW_CAP, "concat-fwd-stride"),
    _c((1, 12, 300, 296, 4), "concat_bwd_kernel grid-stride iteration: 1,065,600 pixels > 4096 * 256 (forward: nine sweeps)",
       lambda s=(1, 12, 300, 296, 4): VOL_EW_CAP < _cat_bwd(s) < 2 * VOL_EW_CAP and _cat_fwd(s) > 8 * VOL_EW_CAP,
       "concat-bwd-stride"),
]


def _f(shape, branch, arith, regimes, **p):
    return Case("fused", shape, branch, arith, regimes, p)


_HOT = (1, 320, 40, 2, 240, 48)
_HOT_SEG = (64, 128, 128)
_FCAT = (1, 1, 1, 64, 688, 8)
FUSED = [
    _f(_HOT, "gwc_fused_kernel<8, float, false> at W 240, D 48: rows 4, DQ 12, three `iq` trips; per-row maxima emitted",
       lambda: fused_iq_trips(240, 48) == [3, 3, 3, 3] and bwd_rows(*_HOT) == 2, ("fused-hot-iq3",), seg=_HOT_SEG, Cc=0,
       dtype="fp32"),
    _f(_HOT[:5] + (50,), "gwc_fused_kernel<8, bf16, true>: D 50, DQ 13: four `iq` trips for the first thread row, partial last quad",
       lambda: fused_iq_trips(240, 50) == [4, 3, 3, 3] and 50 % 4 != 0, ("fused-tail-iq",), seg=_HOT_SEG, Cc=0, dtype="bf16"),
    _f(_HOT[:5] + (50,), "gwc_fused_kernel<8, f16, true>: D 50, DQ 13: four `iq` trips for the first thread row, partial last quad",
       lambda: fused_iq_trips(240, 50) == [4, 3, 3, 3] and 50 % 4 != 0, ("fused-tail-iq",), seg=_HOT_SEG, Cc=0, dtype="fp16"),
    _f(_FCAT, "concat_fused_kernel grid-stride iteration: 2,113,536 x quads > 8192 * 256; gwc_fused_kernel<1>",
       lambda s=_FCAT: FUSED_EW_CAP < s[0] * 2 * 12 * s[5] * s[3] * (s[4] // 4) < 2 * FUSED_EW_CAP and s[4] % 4 == 0
       and s[5] % 4 == 0, ("fused-concat-stride",), seg=(1,), Cc=12, dtype="fp32"),
]

FAMILIES = {"gwc": GWC, "concat": CONCAT, "fused": FUSED}
ALL = GWC + CONCAT + FUSED
assert len({c.id for c in ALL}) == len(ALL)

# C-ABI rows with every operand 4 bytes off 16-byte alignment (a contiguous view at element 1 of a larger buffer): `_req` of
# ops.py clones such tensors, so the non-vec branches at W % 4 == 0 are reachable only here.  Same kernel, same order of the
# arithmetic as the aligned run: bitwise equal.
ABI_MISALIGNED = {
    "bwd": _g((2, 32, 2, 3, 24, 8), "dca_gwc_volume_bwd, W % 4 == 0, plain kernel (CPG 16): vec = 0 at misaligned gvol / L / R",
              lambda s=(2, 32, 2, 3, 24, 8): bwd_rows(*s) == 0 and s[4] % 4 == 0, "abi-misaligned-bwd"),
    "fwd": _g((2, 16, 2, 3, 24, 20), "dca_gwc_volume_fwd, W % 4 == 0: vec = 0 at a misaligned vol; two disparity segments",
              lambda s=(2, 16, 2, 3, 24, 20): s[4] % 4 == 0 and cdiv(s[5], SEG) == 2, "abi-misaligned-fwd"),
}
# what the launchers refuse before any launch: hipErrorInvalidValue
REFUSED = _g((1, 16, 1, 1, 1284, 4), "CPG 16, W 1284: 164352 B of forward LDS > 160 KiB",
             lambda s=(1, 16, 1, 1, 1284, 4): fwd_lds(16, 1284) == 164352 > LDS_REFUSE and bwd_rows(*s) == -1, "refused")

# the six shapes of tests/test_gpu_parity.py::test_gwc_volume and the backward route each takes
PARITY_SHAPES = [(2, 32, 4, 5, 18, 6), (1, 320, 40, 3, 10, 12), (1, 320, 40, 6, 64, 16), (2, 64, 8, 7, 40, 48),
                 (1, 80, 10, 2, 240, 48), (1, 32, 8, 3, 256, 20)]
PARITY_ROUTES = [0, 0, 0, 7, 2, 0]

REQUIRED_REGIMES = (
    "blocked-deep-ragged", "blocked-hot-two", "blocked-gx1", "blocked-cpg4-D6cpg", "blocked-cpg2-wave3-idle", "blocked-D>W",
    "blocked-edge-quads", "blocked-edge-lds", "blocked-cpg2-multitrip", "blocked-cpg4-multitrip",
    "plain-quads", "plain-lds", "plain-D<6cpg", "plain-W>256", "plain-cpg16", "plain-cpg1",
    "plain-W%4=1", "plain-W%4=2", "plain-W%4=3", "plain-second-item-pass", "plain-D>W", "plain-lds>64K",
    "fwd-D<12", "fwd-D=12", "fwd-partial-seg-second-pass", "fwd-D>W", "fwd-tail", "fwd-lds>64K",
    "concat-fwd-stride", "concat-bwd-stride", "fused-hot-iq3", "fused-tail-iq", "fused-concat-stride",
    "abi-misaligned-bwd", "abi-misaligned-fwd", "refused",
)

# the fixed tolerances of the sibling parity tests (tests/test_gpu_parity.py::test_gwc_volume, ::test_concat_volume,
# tests/test_gpu_fused_nodes.py::_vol_check); every case here runs at their unit magnitude and has to meet them too
SIBLING = {"fwd": 2e-6, "d L": 1e-5, "d R": 1e-5, "concat": 0.0, "d cl": 1e-6, "d cr": 1e-6}
SIBLING_CONCAT = {"fwd": 0.0, "d L": 1e-6, "d R": 1e-6}
LP = {"bf16": (torch.bfloat16, 2.0 ** -8), "fp16": (torch.float16, 2.0 ** -11)}     # storage type, half an ulp of it


def sibling(case):
    return SIBLING_CONCAT if case.family == "concat" else SIBLING


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def seed_scale(case):
    """Factor on the gradient seed.  d L[c, x] = 1 / CPG sum_i gV[i, x] R[c, x - i]: with unit inputs its spread is
    sqrt(min(D, x + 1)) / CPG, for CPG 16 and a short D below 1 everywhere, where the metric's max(1, max |ref|) would turn
    the relative gate into an absolute one.  A seed of CPG (a power of two: exact) takes the 1 / CPG out."""
    return float(case.cpg)


def has_grads(case):
    return case.p.get("dtype", "fp32") == "fp32"


def inputs(case):
    """{name: float32 CPU tensor} of the differentiated inputs (gwc features as a list of channel segments under "L" / "R"),
    and the gradient seed for the whole output volume"""
    tag = f"vc.{case.id}"
    if case.family == "concat":
        B, C, H, W, D = case.shape
        t = {"L": [seeded_tensor(tag + ".L", (B, C, H, W))], "R": [seeded_tensor(tag + ".R", (B, C, H, W))]}
        return t, seeded_tensor(tag + ".g", (B, 2 * C, D, H, W))
    B, C, G, H, W, D = case.shape
    seg, Cc = case.p.get("seg", (C,)), case.p.get("Cc", 0)
    assert sum(seg) == C
    t = {"L": [seeded_tensor(f"{tag}.L{i}", (B, c, H, W)) for i, c in enumerate(seg)],
         "R": [seeded_tensor(f"{tag}.R{i}", (B, c, H, W)) for i, c in enumerate(seg)]}
    if Cc:
        t["cl"], t["cr"] = [seeded_tensor(tag + ".cl", (B, Cc, H, W))], [seeded_tensor(tag + ".cr", (B, Cc, H, W))]
    return t, seeded_tensor(tag + ".g", (B, G + 2 * Cc, D, H, W)) * seed_scale(case)


def volume_numel(case):
    """elements of the case's output volume"""
    if case.family == "concat":
        B, C, H, W, D = case.shape
        return B * 2 * C * D * H * W
    B, C, G, H, W, D = case.shape
    return B * (G + 2 * case.p.get("Cc", 0)) * D * H * W


def input_sizes(case):
    """bytes of every single input tensor, the gradient seed among them"""
    t, seed = inputs(case)
    return [x.numel() * x.element_size() for v in t.values() for x in v] + [seed.numel() * seed.element_size()]


# ---- the operation of a case: as the oracle states it, and as ops.py serves it --------------------------------------------------
def reference(case, t):
    """the whole output volume from the dtype-generic oracle functions on the tensors `t`"""
    L, R = torch.cat(t["L"], 1) if len(t["L"]) > 1 else t["L"][0], torch.cat(t["R"], 1) if len(t["R"]) > 1 else t["R"][0]
    if case.family == "concat":
        return O.build_concat_volume(L, R, case.shape[4])
    G, D = case.shape[2], case.shape[5]
    vol = O.build_gwc_volume(L, R, D, G)
    if "cl" in t:
        vol = torch.cat((vol, O.build_concat_volume(t["cl"][0], t["cr"][0], D)), 1)
    return vol


def public_op(ops):
    """the same through the public ops of `ops` (the package's ops.py) on device tensors"""
    def call(case, t):
        if case.family == "concat":
            return ops.concat_volume(t["L"][0], t["R"][0], case.shape[4])
        G, D = case.shape[2], case.shape[5]
        if case.family == "gwc":
            return ops.gwc_volume(t["L"][0], t["R"][0], D, G)
        one = len(t["L"]) == 1
        cl, cr = (t["cl"][0], t["cr"][0]) if "cl" in t else (None, None)
        dtype = torch.float32 if has_grads(case) else LP[case.p["dtype"]][0]
        return ops.cost_volume(t["L"][0] if one else tuple(t["L"]), t["R"][0] if one else tuple(t["R"]), D, G, cl, cr,
                               out_dtype=dtype)
    return call


def evaluate(case, dtype, device="cpu", call=reference):
    """forward and all gradients of one case: ({"fwd": gwc part (or the concat family's volume), "concat": concat part of a
    fused volume, "d L", "d R"[, "d cl", "d cr"]}, the raw output), detached, on `device`.  The gradient seed is rounded to
    float32 before it is cast, so every precision gets the same seed; segment gradients are concatenated along the channels."""
    t, seed = inputs(case)
    t = {k: [x.to(device=device, dtype=dtype).requires_grad_(has_grads(case)) for x in v] for k, v in t.items()}
    out = call(case, t)
    G = case.shape[2] if case.family != "concat" else out.shape[1]
    res = {"fwd": out.detach()[:, :G]}
    if out.shape[1] > G:
        res["concat"] = out.detach()[:, G:]
    if has_grads(case):
        leaves = [x for v in t.values() for x in v]
        grads = list(torch.autograd.grad((out * seed.to(device=out.device, dtype=out.dtype)).sum(), leaves))
        for k, v in t.items():
            gs, grads = grads[:len(v)], grads[len(v):]
            res[f"d {k}"] = gs[0] if len(gs) == 1 else torch.cat(gs, 1)
    return res, out


def row_errors(a, ref):
    """the metric per image row y of a (B, C, H, W) gradient: max over (b, c, x) of |a - ref|, over max(1, max |ref|) of the
    whole tensor"""
    a, ref = a.detach().cpu().double(), ref.detach().cpu().double()
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return (a - ref).abs().amax((0, 1, 3)) / max(1.0, ref.abs().max().item())


@functools.lru_cache(maxsize=2)
def truth(case):
    """the float64 results of a case on the CPU; computed once, never modified"""
    return evaluate(case, torch.float64)[0]


@functools.lru_cache(maxsize=None)
def yardstick(case):
    """{output or gradient name: error of the float32 CPU oracle against the float64 one}"""
    ref = truth(case)
    got = evaluate(case, torch.float32)[0]
    return {k: error(got[k], ref[k]) for k in ref}
