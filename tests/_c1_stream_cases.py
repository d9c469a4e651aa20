"""Cases, fp64 references and group arithmetic of tests/test_gpu_c1_stream_fp64.py (no GPU import here; the arithmetic, the
table and the references are checked without a GPU by tests/test_c1_stream_cases_cpu.py).

Three streaming kernels serve the 1x1x1 convolutions and share one walk: `conv1_x3_kernel<NC1, NC2, STATS>` (conv1_x3.hip),
`conv1_lp_kernel<MT, OUT32>` (conv1_lp.hip) and `conv1_mfma_kernel<NG, VEC>` (conv3d_mfma.hip).  A wave owns groups of 128
consecutive voxels of one sample: G = ceil(S / 128) groups per sample, T = N * G in all.  The launcher starts
`grid = min(ceil(T / 4), 2048)` workgroups of four waves -- `c1x_blocks` of conv1_x3.hip, lines 202-204 of
`dca_conv1_lp_forward` in conv1_lp.hip, lines 642-643 of `dca_conv3d_forward` in conv3d_mfma.hip: the cap is the constant
256 * 8, no function of the device -- and wave `u = 4 * blockIdx.x + wv` loops over the groups `u, u + 4 * grid, ... < T`.
Group g is sample n = g / G, first voxel (g % G) * 128 + 4 * (lane & 31); lanes beyond S are predicated (`dca_pred_off`, or
`v < S` in the scalar form).  The decode of a group that is not the wave's first, the per-sample buffer descriptors rebuilt
per group, the statistics shift K taken on the wave's first group and reused, the sums that run across groups and the
single `fs_flush` per workgroup exist only from a wave's second trip through that loop on.  Every row below names the REGIME
of the walk it exists for; the regimes are predicates on `walk(N, S)`, not on shapes.

The references never go through `dcanet_amd`: a matrix product per sample on double copies, in sample chunks."""
from collections import namedtuple

import torch
import torch.nn.functional as F

from _conv_tile_cases import fold_partials, ref_epilogue, ref_stats      # noqa: F401  (re-exported to the tests)
from _wgrad_cases import cdiv

GROUP = 128             # voxels of a group: 32 lanes x 4 voxels, both wave halves on the same voxels
WAVES = 4               # waves of a workgroup
GRID_CAP = 256 * 8      # c1x_blocks: `if (blocks > 256 * 8) blocks = 256 * 8`
DEVICE_BYTES_CAP = 1 << 30   # live device memory of one row: operands, residuals and ONE output (the first goes to the host)


# ---- the walk, restated -------------------------------------------------------------------------------------------------------------
def groups(N, S):
    """(G, T): groups per sample and in all"""
    G = cdiv(S, GROUP)
    return G, N * G


def grid(N, S):
    """workgroups of the launch: min(ceil(T / 4), 2048)"""
    return min(cdiv(groups(N, S)[1], WAVES), GRID_CAP)


def walk(N, S):
    """the groups of every launched wave u = 4 * blockIdx.x + wv, in the order the wave takes them"""
    T = groups(N, S)[1]
    nw = WAVES * grid(N, S)
    return [list(range(u, T, nw)) for u in range(nw)]


def decode(g, S):
    """group -> (n, first voxel of the group in its sample, lanes of a wave half that are in range)"""
    G = cdiv(S, GROUP)
    v0 = (g % G) * GROUP
    return g // G, v0, min(32, cdiv(S - v0, 4))


def group_voxels(g, S):
    """voxels of the group that exist"""
    return min(GROUP, S - decode(g, S)[1])


Walk = namedtuple("Walk", "N S G T grid waves")


def geometry(N, S):
    G, T = groups(N, S)
    return Walk(N, S, G, T, grid(N, S), walk(N, S))


# ---- regimes: predicates on the walk ------------------------------------------------------------------------------------------------
def _lens(g):
    return [len(w) for w in g.waves]


def _pairs(g):
    return ((a, b) for w in g.waves for a, b in zip(w, w[1:]))


def _idle(g):
    return any(not g.waves[u] and any(g.waves[4 * (u // 4) + k] for k in range(WAVES)) for u in range(len(g.waves)))


REGIMES = {
    # the capped grid with waves of one and of two groups, at least 1024 of each
    "mixed": lambda g: g.grid == GRID_CAP and _lens(g).count(1) >= 1024 and _lens(g).count(2) >= 1024,
    # every wave owns at least 3 groups
    "deep": lambda g: min(_lens(g)) >= 3,
    # n changes between consecutive groups of at least one wave
    "samples": lambda g: any(a // g.G != b // g.G for a, b in _pairs(g)),
    # the position in the sample changes between consecutive groups of at least one wave (so a wave meets the ragged last
    # group after a full one): needs 4 * grid % G != 0
    "shift": lambda g: any(a % g.G != b % g.G for a, b in _pairs(g)),
    # a launched wave owns no group while another wave of its workgroup does
    "idle": _idle,
}


# ---- shapes: the smallest that reach the regimes ------------------------------------------------------------------------------------
Shape = namedtuple("Shape", "N dims")
SHAPES = {
    # S = 324, G = 3: two full groups and a ragged one of 68 voxels (17 lanes of each half); T = 9216 = 8192 + 1024
    "M": Shape(3072, (3, 4, 27)),
    # S = 325, S % 4 == 1: not for conv1_x3 / conv1_lp; conv1_mfma_kernel<., false>.  The ragged group ends inside a lane
    "Mu": Shape(3072, (5, 5, 13)),
    # S = 68, G = 1: every group ragged; T = 3 * 8192 + 256: 256 waves with four groups, the others three
    "D": Shape(24832, (1, 4, 17)),
    # S = 576, 5 groups, 2 workgroups: waves 5, 6, 7 are idle beside wave 4
    "I": Shape(1, (2, 4, 72)),
}


def voxels(shape):
    d = SHAPES[shape].dims
    return d[0] * d[1] * d[2]


# ---- cases --------------------------------------------------------------------------------------------------------------------------
# kernel  "x3" (conv1_x3.hip), "mfma" (conv1_mfma_kernel of conv3d_mfma.hip), "lp" (conv1_lp.hip)
# inst    the template instantiation the row launches
# tags    "plain"; "epi" (scale, shift, slope 0.1, res_pre, res_post); "stats" (training forward with fused BatchNorm
#         statistics); "dx" (the kernel as backward-data of the row's operator, through autograd); "two" (two inputs);
#         "c64" (one 64-channel input); "slices" (64 output channels: two launches with co_off 0 and 32); "head" (27 output
#         channels: channels >= Cout of the MFMA block must be dropped); "vec" / "scalar" (conv1_mfma's VEC); "out32"
# lp      None, or "bf16" / "fp16"
Case = namedtuple("Case", "id kernel inst shape C1 C2 Cout regimes tags lp")

_M = ("mixed", "samples", "shift")
_D = ("deep", "samples")


def _c(id, kernel, inst, shape, C1, C2, Cout, regimes, tags, lp=None):
    return Case(id, kernel, inst, shape, C1, C2, Cout, tuple(regimes), tuple(tags), lp)


X3 = [
    _c("x3-M-32-plain", "x3", "<2,0,false>", "M", 32, 0, 32, _M, ("plain",)),
    _c("x3-M-32-epi", "x3", "<2,0,false>", "M", 32, 0, 32, _M, ("epi",)),
    _c("x3-M-64-plain", "x3", "<4,0,false>", "M", 64, 0, 32, _M, ("plain", "c64")),
    _c("x3-M-64-epi", "x3", "<4,0,false>", "M", 64, 0, 32, _M, ("epi", "c64")),
    _c("x3-M-2in-plain", "x3", "<2,2,false>", "M", 32, 32, 32, _M, ("plain", "two")),
    _c("x3-M-2in-epi", "x3", "<2,2,false>", "M", 32, 32, 32, _M, ("epi", "two")),
    _c("x3-M-64to64-plain", "x3", "<4,0,false>", "M", 64, 0, 64, _M, ("plain", "c64", "slices")),
    # the residuals and the affine of the second slice are read at co_off = 32
    _c("x3-M-64to64-epi", "x3", "<4,0,false>", "M", 64, 0, 64, _M, ("epi", "c64", "slices")),
    _c("x3-M-27-plain", "x3", "<2,0,false>", "M", 32, 0, 27, _M, ("plain", "head")),
    _c("x3-M-32-stats", "x3", "<2,0,true>", "M", 32, 0, 32, _M, ("stats",)),                 # LANE_ACC
    _c("x3-M-64-stats", "x3", "<4,0,true>", "M", 64, 0, 32, _M, ("stats", "c64")),           # LDS-atomic sums
    _c("x3-M-2in-stats", "x3", "<2,2,true>", "M", 32, 32, 32, _M, ("stats", "two")),         # LDS-atomic sums
    _c("x3-M-64to64-stats", "x3", "<4,0,true>", "M", 64, 0, 64, _M, ("stats", "c64", "slices")),   # two slices fill one part
    # dx of the row's operator: the kernel over dy with the transposed weight; 64 -> 32 gives A = 32, B = 64 (two slices)
    _c("x3-M-32-dx", "x3", "<2,0,false>", "M", 32, 0, 32, _M, ("dx",)),
    _c("x3-M-64-dx", "x3", "<2,0,false>", "M", 64, 0, 32, _M, ("dx", "slices")),
    _c("x3-M-2in-dx", "x3", "<2,0,false>", "M", 32, 32, 32, _M, ("dx", "two")),              # dx and dx2
    _c("x3-D-32-plain", "x3", "<2,0,false>", "D", 32, 0, 32, _D, ("plain",)),
    _c("x3-D-32-stats", "x3", "<2,0,true>", "D", 32, 0, 32, _D, ("stats",)),
    _c("x3-I-32-stats", "x3", "<2,0,true>", "I", 32, 0, 32, ("idle",), ("stats",)),
]
MFMA = [
    # VEC form: the bf16x3 family switched off
    _c("mfma-M-32-epi", "mfma", "<1,true>", "M", 32, 0, 32, _M, ("epi", "vec")),
    _c("mfma-M-2in-epi", "mfma", "<2,true>", "M", 32, 32, 32, _M, ("epi", "two", "vec")),
    # scalar form: S % 4 == 1 sends the default flags here
    _c("mfma-Mu-32-epi", "mfma", "<1,false>", "Mu", 32, 0, 32, _M, ("epi", "scalar")),
    _c("mfma-Mu-2in-plain", "mfma", "<2,false>", "Mu", 32, 32, 32, _M, ("plain", "two", "scalar")),
    _c("mfma-D-32-plain", "mfma", "<1,true>", "D", 32, 0, 32, _D, ("plain", "vec")),
]
LP = []
for _lp, _mt in (("bf16", "__bf16"), ("fp16", "_Float16")):
    LP += [
        _c(f"lp-M-32-epi-{_lp}", "lp", f"<{_mt},false>", "M", 32, 0, 32, _M, ("epi",), _lp),
        _c(f"lp-M-2in-epi-{_lp}", "lp", f"<{_mt},false>", "M", 32, 32, 32, _M, ("epi", "two"), _lp),
        _c(f"lp-M-27-plain-{_lp}", "lp", f"<{_mt},true>", "M", 32, 0, 27, _M, ("plain", "head", "out32"), _lp),
        _c(f"lp-D-32-plain-{_lp}", "lp", f"<{_mt},false>", "D", 32, 0, 32, _D, ("plain",), _lp),
    ]

ALL = X3 + MFMA + LP

# the instantiations the three launchers can make: every one has a row, and a `mixed` one
INSTANCES = {
    "x3": ["<2,0,false>", "<4,0,false>", "<2,2,false>", "<2,0,true>", "<4,0,true>", "<2,2,true>"],
    "mfma": ["<1,true>", "<2,true>", "<1,false>", "<2,false>"],
    "lp": ["<__bf16,false>", "<__bf16,true>", "<_Float16,false>", "<_Float16,true>"],
}

# (kernel, tag or None = every row of the kernel) -> the regimes that need a row (for "lp": in each 2-byte type)
REQUIRED = {
    ("x3", "plain"): ("mixed", "deep", "samples", "shift"),
    ("x3", "epi"): ("mixed", "samples", "shift"),
    ("x3", "stats"): ("mixed", "deep", "samples", "shift", "idle"),
    ("x3", "dx"): ("mixed", "samples", "shift"),
    ("x3", "two"): ("mixed",), ("x3", "c64"): ("mixed",), ("x3", "slices"): ("mixed",), ("x3", "head"): ("mixed",),
    ("mfma", "vec"): ("mixed", "deep", "samples", "shift"),
    ("mfma", "scalar"): ("mixed", "samples", "shift"),
    ("mfma", "two"): ("mixed",), ("mfma", "epi"): ("mixed",), ("mfma", "plain"): ("mixed", "deep"),
    ("lp", None): ("mixed", "deep", "samples", "shift"),
    ("lp", "epi"): ("mixed",), ("lp", "two"): ("mixed",), ("lp", "head"): ("mixed",), ("lp", "out32"): ("mixed",),
    ("lp", "plain"): ("mixed", "deep"),
}


def shape_of(case):
    """(N, S, dims) of the row"""
    s = SHAPES[case.shape]
    return s.N, voxels(case.shape), s.dims


def x3_eligible(case):
    """what `_c1x3_eligible` of ops.py must say about the row's FORWARD operands: channel layout, S % 4 and the 31-bit
    per-sample offset limit (alignment is the allocator's business)"""
    S = voxels(case.shape)
    return (case.C1, case.C2) in ((32, 0), (64, 0), (32, 32)) and S % 4 == 0 and 64 * S * 4 < 0x7ffffff0


def device_bytes(case):
    """live device memory of the row's tensors: operands, residuals and one output (the first launch's output is on the host
    before the second launch allocates its own)"""
    N, S, _ = shape_of(case)
    esz = 2 if case.lp else 4
    osz = 4 if (not case.lp or "out32" in case.tags) else 2
    cin, cout = case.C1 + case.C2, case.Cout
    if "dx" in case.tags:       # x [, x2] (leaves), y, gy, and dx [, dx2]
        return N * S * 4 * (2 * cin + 2 * cout)
    n = N * S * (cin * esz + cout * osz)
    if "epi" in case.tags:
        n += 2 * N * S * cout * osz
    return n


# ---- data ---------------------------------------------------------------------------------------------------------------------------
def data_key(case):
    """rows with equal keys have equal inputs and so one reference"""
    return (case.shape, case.C1, case.C2, case.Cout, case.lp)


def tensor(case, name, seeded_tensor):
    """one fp32 tensor of a row on the CPU, the same for every row of one key: "x", "x2", "w" (Cout, C1 + C2, 1, 1, 1), "gy",
    "res_pre", "res_post" (the output's shape), "scale", "shift" """
    N, S, dims = shape_of(case)
    cin = case.C1 + case.C2
    tag = f"c1s{data_key(case)[:4]}.{name}"
    if name == "x":
        return seeded_tensor(f"c1s.{case.shape}.{case.C1}.x", (N, case.C1) + dims)
    if name == "x2":
        return seeded_tensor(f"c1s.{case.shape}.{case.C2}.x2", (N, case.C2) + dims)
    if name == "w":
        return seeded_tensor(tag, (case.Cout, cin, 1, 1, 1)) * (1.0 / cin) ** 0.5
    if name == "scale":
        return 1.0 + 0.25 * seeded_tensor(tag, (case.Cout,))
    if name == "shift":
        return 0.1 * seeded_tensor(tag, (case.Cout,))
    assert name in ("gy", "res_pre", "res_post"), name
    return seeded_tensor(f"c1s.{case.shape}.{case.Cout}.{name}", (N, case.Cout) + dims)


# ---- references ---------------------------------------------------------------------------------------------------------------------
CHUNK = 512     # samples per fp64 chunk: the host holds one chunk of the operands in double, never the whole tensor


def ref_forward(x, x2, w, chunk=CHUNK):
    """fp64 y (N, Cout, *dims) of the 1x1x1 convolution of cat([x, x2], 1) with w (Cout, C1 + C2 [, 1, 1, 1]): one matrix
    product per sample, in chunks of `chunk` samples.  Operands of a 2-byte type are taken at their rounded values"""
    N, dims = x.shape[0], tuple(x.shape[2:])
    wd = w.detach().cpu().double().reshape(w.shape[0], -1)
    C1 = x.shape[1]
    assert wd.shape[1] == C1 + (0 if x2 is None else x2.shape[1])
    out = torch.empty((N, wd.shape[0]) + dims, dtype=torch.float64)
    o3 = out.view(N, wd.shape[0], -1)
    for n0 in range(0, N, chunk):
        sl = slice(n0, min(N, n0 + chunk))
        y = torch.matmul(wd[:, :C1], x[sl].detach().cpu().double().flatten(2))
        if x2 is not None:
            y += torch.matmul(wd[:, C1:], x2[sl].detach().cpu().double().flatten(2))
        o3[sl] = y
    return out


def ref_backward_data(w, gy, c0, c1, chunk=CHUNK):
    """fp64 gradient of the input channels [c0, c1) of the same operator: dx[n, c] = sum_o w[o, c] gy[n, o] (the operator is
    linear: its value is not needed)"""
    wd = w.detach().cpu().double().reshape(w.shape[0], -1)[:, c0:c1].t().contiguous()
    return ref_forward(gy, None, wd, chunk)


# ---- per-group comparison -----------------------------------------------------------------------------------------------------------
def group_max(v, N, S):
    """v (N, C, *dims) >= 0 -> its maximum per group, flat in group order; NaN counts as infinity"""
    G, T = groups(N, S)
    v = torch.nan_to_num(v, nan=float("inf")).reshape(N, -1, S).amax(1)
    v = F.pad(v, (0, G * GROUP - S))
    return v.view(N, G, GROUP).amax(2).reshape(T)


def worst_group(err, N, S):
    """text that names the group with the largest value of err (error over its gate): index, sample, position in the
    sample, the wave that owns it, which trip of that wave's loop it is, and how many groups exceed the gate"""
    per = group_max(err, N, S)
    g = int(per.argmax())
    n, v0, lanes = decode(g, S)
    nw = WAVES * grid(N, S)
    u, trip = g % nw, g // nw
    own = len(range(u, groups(N, S)[1], nw))
    bad = int((per > 1).sum())
    return (f"worst group {g} = (n {n}, voxels {v0}..{v0 + group_voxels(g, S) - 1}, {lanes} lanes) at {per[g].item():.3e} x "
            f"the gate: wave {u} = workgroup {u // WAVES} wave {u % WAVES}, trip {trip + 1} of its {own}; {bad} of {per.numel()} "
            f"groups over the gate")
