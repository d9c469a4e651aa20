"""Cases, fp64 references and tile arithmetic of tests/test_gpu_conv_tiles_fp64.py (no GPU import here; the arithmetic, the
table and the references are checked without a GPU by tests/test_conv_tile_cases_cpu.py).

Seven forward / backward-data kernels share the persistent tile walk of csrc/dca_tiles.h: `grid = min(tiles, CUs / share)`
workgroups per channel block, each looping over `begin, begin + step, ... < end` inside its XCD's chunk of the tile space.
Everything delicate in them -- the load / MFMA pipeline that runs across tile boundaries, `dca_tile_advance`, the `on` mask
behind the last chunk of the LAST tile, the running BatchNorm sums and the per-channel maxima that are flushed once --
exists only when a workgroup owns two or more tiles.  Every row below names the REGIME of that walk it exists for; the
regimes are predicates on `split_walk(tiles, grid)`, not on shapes, and the GPU test asserts them on the device's own CU
count (and the kernel's own size query where it has one) before it compares anything.

The references never go through `dcanet_amd`: `F.conv3d` / `F.conv_transpose3d` and autograd on double copies."""
from collections import namedtuple

import torch
import torch.nn.functional as F

from _wgrad_cases import cdiv, split_walk

AMAX_CSLOTS = 1024      # DCA_AMAX_CSLOTS of include/dca_hip.h: conv3d_f16x2.hip caps its grid there (x2_geometry)


# ---- tile arithmetic: the *_geometry functions of the seven kernels restated -----------------------------------------------------
# each returns (tile, dims the tile grid covers, share): `share` = the channel blocks of the launch, what the launcher
# passes to dca_persistent_grid.  N, A, B, dims = the LAUNCH: A contraction channels, B output channels, dims of its input.
def tiles_s1(N, A, B, dims):
    """conv3d_f16x2.hip x2_geometry (TD, TH, TW = 4, 8, 16; cblks = (Cout + 31) / 32), conv3d_bf16x3.hip x3_geometry and
    conv3d_lp.hip dca_conv3d_lp_forward (the same two lines): output dims = input dims"""
    return (4, 8, 16), tuple(dims), cdiv(B, 32)


def tiles_s2x2(N, A, B, dims):
    """conv3d_s2_f16x2.hip s2x2_geometry: TD, TH, TW = 2, 4, 32 on the OUTPUT dims (d + 1) / 2; cblks = (Cout + 63) / 64"""
    return (2, 4, 32), tuple((d + 1) // 2 for d in dims), cdiv(B, 64)


def tiles_coarse_in(N, A, B, dims):
    """deconv3d_x3.hip dx_geometry and deconv3d_lp.hip dca_deconv3d_lp_forward: TD, TH, TW = 2, 8, 16 on the coarse INPUT
    dims, one grid row (all <= 32 output channels in one workgroup): dca_persistent_grid(tiles, 1)"""
    return (2, 8, 16), tuple(dims), 1


def tiles_s2lp(N, A, B, dims):
    """conv3d_s2_lp.hip dca_conv3d_s2_lp_forward: TD, TH, TW = 2, 8, 16 on the OUTPUT dims (d + 1) / 2, one grid row
    (all <= 64 output channels in one workgroup)"""
    return (2, 8, 16), tuple((d + 1) // 2 for d in dims), 1


# kernel -> (tile function, stride, transposed, factor from a tile to the voxels of the launch's OUTPUT it covers)
KERNELS = {
    "x2": (tiles_s1, 1, False, 1),          # conv3d_f16x2.hip
    "x3": (tiles_s1, 1, False, 1),          # conv3d_bf16x3.hip
    "s2x2": (tiles_s2x2, 2, False, 1),      # conv3d_s2_f16x2.hip
    "dx3": (tiles_coarse_in, 2, True, 2),   # deconv3d_x3.hip: a coarse tile writes 2 x 2 x 2 as many fine voxels
    "lp": (tiles_s1, 1, False, 1),          # conv3d_lp.hip
    "s2lp": (tiles_s2lp, 2, False, 1),      # conv3d_s2_lp.hip
    "dlp": (tiles_coarse_in, 2, True, 2),   # deconv3d_lp.hip
}
# the `family` ops._conv_family names for the fp32-grade kernels
FAMILY = {"x2": "x2", "x3": "x3", "s2x2": "s2x2", "dx3": "dx3"}


def persistent_grid(kernel, tiles, share, ncu):
    """dca_persistent_grid of csrc/dca_common.h: g = ncu > share ? ncu / share : 1; min(tiles, g).  conv3d_f16x2.hip caps it
    at DCA_AMAX_CSLOTS (a workgroup index is also a slot of the per-channel output maxima)"""
    g = ncu // share if ncu > share else 1
    g = min(tiles, g)
    return min(g, AMAX_CSLOTS) if kernel == "x2" else g


Geometry = namedtuple("Geometry", "tiles share grid N nT tile out_tile walk")


def geometry_of(kernel, N, A, B, dims, ncu=256):
    """the launch geometry of `kernel` over an input (N, A, *dims) with B output channels on a device with ncu CUs"""
    fn, _, _, up = KERNELS[kernel]
    tile, tdims, share = fn(N, A, B, dims)
    nT = tuple(cdiv(d, t) for d, t in zip(tdims, tile))       # dca_tile_grid of csrc/dca_tiles.h
    tiles = N * nT[0] * nT[1] * nT[2]
    grid = persistent_grid(kernel, tiles, share, ncu)
    return Geometry(tiles, share, grid, N, nT, tile, tuple(t * up for t in tile), split_walk(tiles, grid))


def decode(tile, N, nT):
    """dca_tile_decode of csrc/dca_tiles.h: tile index -> (n, td, th, tw), w fastest"""
    tw = tile % nT[2]; tile //= nT[2]
    th = tile % nT[1]; tile //= nT[1]
    return tile // nT[0], tile % nT[0], th, tw


# ---- regimes: predicates on the walk -----------------------------------------------------------------------------------------------
def _lens(g):
    return [len(w) for w in g.walk]


def _crosses_samples(g):
    per = g.nT[0] * g.nT[1] * g.nT[2]
    return any(a // per != b // per for w in g.walk for a, b in zip(w, w[1:]))


REGIMES = {
    # workgroups with one and with two tiles in the same launch
    "mixed": lambda g: g.grid < g.tiles <= 2 * g.grid and {1, 2} <= set(_lens(g)),
    # every workgroup has at least 3 tiles
    "deep": lambda g: min(_lens(g)) >= 3,
    # XCD chunks of unequal length and unequal workgroup count
    "ragged": lambda g: g.grid >= 8 and g.tiles % 8 != 0 and g.grid % 8 != 0,
    # n changes inside the pipeline of at least one workgroup
    "samples": lambda g: g.N >= 2 and _crosses_samples(g),
    # at least one workgroup has no tile while others have some
    "idle": lambda g: min(_lens(g)) == 0 and max(_lens(g)) >= 1,
}


# ---- references ---------------------------------------------------------------------------------------------------------------------
def ref_forward(x, w, stride, transposed):
    """fp64 y of Conv3d(k = 3, padding 1, stride) / ConvTranspose3d(k = 3, stride 2, padding 1, output_padding 1)"""
    xd, wd = x.detach().cpu().double(), w.detach().cpu().double()
    if transposed:
        return F.conv_transpose3d(xd, wd, None, 2, 1, 1)
    return F.conv3d(xd, wd, None, stride, 1)


def ref_backward_data(xshape, w, gy, stride, transposed):
    """fp64 dx of the same operator through autograd on double copies (the operator is linear in x: its value is not needed)"""
    xd = torch.zeros(tuple(xshape), dtype=torch.float64, requires_grad=True)
    y = ref_forward_graph(xd, w.detach().cpu().double(), stride, transposed)
    assert y.shape == gy.shape, (y.shape, gy.shape)
    (gx,) = torch.autograd.grad(y, [xd], gy.detach().cpu().double())
    return gx


def ref_forward_graph(xd, wd, stride, transposed):
    return F.conv_transpose3d(xd, wd, None, 2, 1, 1) if transposed else F.conv3d(xd, wd, None, stride, 1)


def ref_epilogue(y, scale=None, shift=None, slope=1.0, res_pre=None, res_post=None):
    """act(y * scale + shift + res_pre) + res_post in fp64, act = leaky ReLU with `slope`"""
    d = lambda t: t.detach().cpu().double()
    v = d(y)
    if scale is not None:
        v = v * d(scale).view(1, -1, 1, 1, 1) + d(shift).view(1, -1, 1, 1, 1)
    if res_pre is not None:
        v = v + d(res_pre)
    v = torch.where(v > 0, v, v * slope)
    if res_post is not None:
        v = v + d(res_post)
    return v


def ref_stats(y):
    """(mean, biased variance) per channel of the fp64 output"""
    yd = y.detach().cpu().double()
    return yd.mean(dim=(0, 2, 3, 4)), yd.var(dim=(0, 2, 3, 4), unbiased=False)


def ref_cmax(y):
    """per-channel max |y| of the fp64 output"""
    return y.detach().cpu().double().abs().amax((0, 2, 3, 4))


def fold_partials(part, C):
    """(count, mean, biased variance) per channel from the self-centred partials {K, n, sum (y - K), sum (y - K)^2} per
    (channel, workgroup) of csrc/bn_fused_stats.h, folded in fp64 the way dca_bn_finalize_centered does: onto the first
    workgroup's shift.  A workgroup without tiles contributes n = 0"""
    p = part.detach().cpu().double().view(C, -1, 4)
    K, n, s, q = p[..., 0], p[..., 1], p[..., 2], p[..., 3]
    dk = K - K[:, :1]
    cnt = n.sum(1)
    S = (s + n * dk).sum(1)
    Q = (q + 2 * dk * s + n * dk * dk).sum(1)
    return cnt, K[:, 0] + S / cnt, Q / cnt - (S / cnt) ** 2


# ---- per-tile comparison ------------------------------------------------------------------------------------------------------------
def tile_max(v, g):
    """v (N, C, Do, Ho, Wo) >= 0 on the launch's output -> its maximum per tile, flat in tile-index order (n, td, th, tw);
    NaN counts as infinity"""
    v = torch.nan_to_num(v, nan=float("inf")).amax(1)
    N = v.shape[0]
    pad = [t * n - d for t, n, d in zip(g.out_tile, g.nT, v.shape[1:])]
    assert N == g.N and all(0 <= p < t for p, t in zip(pad, g.out_tile)), (v.shape, g.nT, g.out_tile)
    v = F.pad(v, (0, pad[2], 0, pad[1], 0, pad[0]))
    v = v.view(N, g.nT[0], g.out_tile[0], g.nT[1], g.out_tile[1], g.nT[2], g.out_tile[2])
    return v.amax((2, 4, 6)).reshape(-1)


def tile_owner(g, tile):
    """(workgroup, position in that workgroup's walk, tiles of that workgroup) of a tile"""
    for wg, w in enumerate(g.walk):
        if tile in w:
            return wg, w.index(tile), len(w)
    raise AssertionError(f"tile {tile} is in nobody's walk")


def worst_tile(v, g):
    """text that names the tile with the largest value of v: index, coordinates, owner and the branch it sits on"""
    per = tile_max(v, g)
    t = int(per.argmax())
    n, td, th, tw = decode(t, g.N, g.nT)
    wg, pos, cnt = tile_owner(g, t)
    bad = int((per > 1).sum())
    return (f"worst tile {t} = (n {n}, d0 {td * g.out_tile[0]}, h0 {th * g.out_tile[1]}, w0 {tw * g.out_tile[2]}) at "
            f"{per[t].item():.3e} x the gate: workgroup {wg}, tile {pos + 1} of its {cnt}; {bad} of {g.tiles} tiles over the gate")


# ---- cases --------------------------------------------------------------------------------------------------------------------------
# N, Cin, Cout, dims describe the OPERATOR of the row (dims = its input's); tags name the variant:
#   staging   "quad" (fp32 input, W % 4 == 0), "single" (W % 4 != 0), "px2" (packed input, f16x2 only)
#   epilogue  "plain", "epi" (inference epilogue: scale, shift, slope 0.1, residuals; on f16x2 also the y_cmax slots), "stats"
#             (forward with fused BatchNorm statistics), "dx" (the kernel as backward-data of the row's own operator, through
#             autograd), "bwd" (deconv3d_x3 as backward-data of the row's stride-2 convolution)
#   "stream"  8+ channel chunks: the weight-fragment stream is long relative to a tile
# lp: None, or "bf16" / "fp16" for the reduced-precision kernels
Case = namedtuple("Case", "id kernel N Cin Cout dims regimes tags lp")


def launch_of(case):
    """(N, A, B, input dims) of the launch under test"""
    if "dx" in case.tags:        # _Conv3d.backward: the stride-1 kernel over dy with the channel roles exchanged
        return case.N, case.Cout, case.Cin, case.dims
    if "bwd" in case.tags:       # _Conv3d.backward of the stride-2 convolution: the transposed kernel over the coarse dy
        return case.N, case.Cout, case.Cin, tuple((d + 1) // 2 for d in case.dims)
    return case.N, case.Cin, case.Cout, case.dims


def geometry(case, ncu=256):
    return geometry_of(case.kernel, *launch_of(case), ncu=ncu)


def _c(id, kernel, N, Cin, Cout, dims, regimes, tags, lp=None):
    return Case(id, kernel, N, Cin, Cout, tuple(dims), tuple(regimes), tuple(tags), lp)


# partial tiles open a new tile per extra voxel: (5, 9, 20) is 2 x 2 x 2 = 8 stride-1 tiles for 900 voxels
Q8, S8 = (5, 9, 20), (5, 9, 17)         # W % 4 == 0 / != 0, 8 tiles each
S12 = (5, 9, 33)                        # W % 4 != 0, 12 tiles
Q9 = (9, 17, 12)                        # 3 x 3 x 1 = 9 tiles: on a grid of 9, XCD 0 has two workgroups and one tile

# stride-1 split kernels.  share 1 (32 output channels, what the model launches): grid 256, mixed = 264 tiles, deep = 768;
# 96 output channels: share 3, grid 85 (85 % 8 = 5), 276 tiles in XCD chunks of 34 / 35 over 11 / 10 workgroups
_S1_ROWS = [
    # name, N, Cin, Cout, dims, regimes, tags
    ("m1q-plain", 33, 32, 32, Q8, ("mixed", "samples"), ("quad", "plain")),
    ("m1q-epi", 33, 32, 32, Q8, ("mixed", "samples"), ("quad", "epi")),
    ("m1q-stats", 33, 32, 32, Q8, ("mixed", "samples"), ("quad", "stats")),
    ("d1q-plain", 96, 32, 32, Q8, ("deep", "samples"), ("quad", "plain")),
    ("d1q-epi", 96, 32, 32, Q8, ("deep", "samples"), ("quad", "epi")),
    ("d1q-stats", 96, 32, 32, Q8, ("deep", "samples"), ("quad", "stats")),
    ("m1s-plain", 33, 32, 32, S8, ("mixed", "samples"), ("single", "plain")),
    ("m1s-stats", 33, 32, 32, S8, ("mixed", "samples"), ("single", "stats")),
    ("d3s-plain", 23, 32, 96, S12, ("deep", "ragged", "samples"), ("single", "plain")),
    ("d3s-epi", 23, 32, 96, S12, ("deep", "ragged", "samples"), ("single", "epi")),
    ("d3s-stats", 23, 32, 96, S12, ("deep", "ragged", "samples"), ("single", "stats")),
    ("idle-epi", 1, 32, 32, Q9, ("idle",), ("quad", "epi")),
    ("idle-stats", 1, 32, 32, Q9, ("idle",), ("quad", "stats")),
    ("stream-m", 17, 64, 64, Q8, ("mixed", "samples"), ("quad", "plain", "stream")),     # share 2: grid 128, 136 tiles
    # backward-data with Cin = 40: dx has a partial second 32-channel block, share 2, grid 128
    ("dx-m", 17, 40, 32, Q8, ("mixed", "samples"), ("quad", "dx")),                      # 136 tiles
    ("dx-d", 48, 40, 32, Q8, ("deep", "samples"), ("quad", "dx")),                       # 384 tiles
]
_PX2_ROWS = [
    ("m1q-px2", 33, 32, 32, Q8, ("mixed", "samples"), ("px2", "plain")),
    ("m1q-px2-stats", 33, 32, 32, Q8, ("mixed", "samples"), ("px2", "stats")),
    ("d1q-px2", 96, 32, 32, Q8, ("deep", "samples"), ("px2", "plain")),
    ("d1q-px2-stats", 96, 32, 32, Q8, ("deep", "samples"), ("px2", "stats")),
]
X2 = [_c(f"x2-{r[0]}", "x2", *r[1:]) for r in _S1_ROWS + _PX2_ROWS]
X3 = [_c(f"x3-{r[0]}", "x3", *r[1:]) for r in _S1_ROWS]

# conv3d_s2_f16x2: tile 2 x 4 x 32 on the output dims.  (6, 10, 68) -> output (3, 5, 34): 2 x 2 x 2 = 8 tiles
F8 = (6, 10, 68)
S2X2 = [
    _c("s2x2-m-plain", "s2x2", 33, 32, 64, F8, ("mixed", "samples"), ("plain",)),
    _c("s2x2-m-epi", "s2x2", 33, 32, 64, F8, ("mixed", "samples"), ("epi",)),
    _c("s2x2-d-plain", "s2x2", 96, 32, 64, F8, ("deep", "samples"), ("plain",)),
    _c("s2x2-d-epi", "s2x2", 96, 32, 64, F8, ("deep", "samples"), ("epi",)),
    _c("s2x2-m30-plain", "s2x2", 33, 30, 64, F8, ("mixed", "samples"), ("plain",)),      # Cin % 8 != 0: a partial chunk of 4
    # 160 output channels: share 3, grid 85; (5, 10, 132) -> output (3, 5, 66): 2 x 2 x 3 = 12 tiles, 276 in all
    _c("s2x2-r-epi", "s2x2", 23, 32, 160, (5, 10, 132), ("deep", "ragged", "samples"), ("epi",)),
]

# deconv3d_x3: tile 2 x 8 x 16 on the coarse input dims; its cursor counts (chunk, kd) steps, 3 NCH per tile.
# (3, 9, 20) coarse = 2 x 2 x 2 = 8 tiles
C8 = (3, 9, 20)
C9 = (5, 17, 16)                        # 3 x 3 x 1 = 9 tiles
FINE8 = (6, 18, 40)                     # the stride-2 convolution whose coarse gradient has dims C8
DX3 = [
    _c("dx3-m-plain", "dx3", 33, 64, 32, C8, ("mixed", "samples"), ("plain",)),
    _c("dx3-m-epi", "dx3", 33, 64, 32, C8, ("mixed", "samples"), ("epi",)),
    _c("dx3-m-stats", "dx3", 33, 64, 32, C8, ("mixed", "samples"), ("stats",)),
    _c("dx3-d-plain", "dx3", 96, 64, 32, C8, ("deep", "samples"), ("plain",)),
    _c("dx3-d-epi", "dx3", 96, 64, 32, C8, ("deep", "samples"), ("epi",)),
    _c("dx3-d-stats", "dx3", 96, 64, 32, C8, ("deep", "samples"), ("stats",)),
    _c("dx3-m40-plain", "dx3", 33, 40, 27, C8, ("mixed", "samples"), ("plain",)),       # partial chunk and block
    _c("dx3-d40-stats", "dx3", 96, 40, 27, C8, ("deep", "samples"), ("stats",)),
    _c("dx3-idle-stats", "dx3", 1, 64, 32, C9, ("idle",), ("stats",)),
    # backward-data of Conv3d(32 -> 64, stride 2) over fine dims FINE8: the transposed kernel reads the coarse dy (64 channels)
    _c("dx3-m-bwd", "dx3", 33, 32, 64, FINE8, ("mixed", "samples"), ("bwd",)),
    _c("dx3-d-bwd", "dx3", 96, 32, 64, FINE8, ("deep", "samples"), ("bwd",)),
]

# reduced precision.  conv3d_lp: 8 chunks of 16 channels (Cin 128) = streaming-weights mode
LP = []
for _lp in ("bf16", "fp16"):
    LP += [
        _c(f"lp-m-{_lp}", "lp", 33, 32, 32, Q8, ("mixed", "samples"), ("quad",), _lp),
        _c(f"lp-d-{_lp}", "lp", 96, 32, 32, Q8, ("deep", "samples"), ("quad",), _lp),
        _c(f"lp-m-single-{_lp}", "lp", 33, 32, 32, S8, ("mixed", "samples"), ("single",), _lp),
        _c(f"lp-m-stream-{_lp}", "lp", 17, 128, 64, Q8, ("mixed", "samples"), ("quad", "stream"), _lp),
        _c(f"s2lp-m-{_lp}", "s2lp", 33, 16, 64, FINE8, ("mixed", "samples"), (), _lp),
        _c(f"s2lp-d-{_lp}", "s2lp", 96, 16, 64, FINE8, ("deep", "samples"), (), _lp),
        _c(f"dlp-m-{_lp}", "dlp", 33, 32, 32, C8, ("mixed", "samples"), (), _lp),
        _c(f"dlp-d-{_lp}", "dlp", 96, 32, 32, C8, ("deep", "samples"), (), _lp),
    ]

ALL = X2 + X3 + S2X2 + DX3 + LP

# (kernel, tag or None = every row of the kernel, lp) -> the regimes that need a row
_MD = ("mixed", "deep")
REQUIRED = {
    ("x2", "quad"): _MD, ("x2", "single"): _MD, ("x2", "px2"): _MD,
    ("x2", "plain"): _MD + ("ragged", "samples"), ("x2", "epi"): _MD + ("ragged", "samples", "idle"),
    ("x2", "stats"): _MD + ("ragged", "samples", "idle"), ("x2", "dx"): _MD, ("x2", "stream"): ("mixed",),
    ("x3", "quad"): _MD, ("x3", "single"): _MD,
    ("x3", "plain"): _MD + ("ragged", "samples"), ("x3", "epi"): _MD + ("ragged", "samples"),
    ("x3", "stats"): _MD + ("ragged", "samples", "idle"), ("x3", "dx"): _MD, ("x3", "stream"): ("mixed",),
    ("s2x2", "plain"): _MD, ("s2x2", "epi"): _MD + ("ragged", "samples"),
    ("dx3", "plain"): _MD, ("dx3", "epi"): _MD, ("dx3", "stats"): _MD + ("samples", "idle"), ("dx3", "bwd"): _MD,
    ("lp", None): _MD, ("s2lp", None): _MD, ("dlp", None): _MD,
}
# share == 1 is what the model's 32-channel layers launch
SHARE1 = {"x2": _MD, "x3": _MD}


# ---- data ---------------------------------------------------------------------------------------------------------------------------
def op_of(case):
    """(stride, transposed) of the row's operator"""
    if "bwd" in case.tags:
        return 2, False
    return KERNELS[case.kernel][1], KERNELS[case.kernel][2]


def out_dims(case):
    stride, transposed = op_of(case)
    if stride == 1:
        return case.dims
    return tuple(2 * d for d in case.dims) if transposed else tuple((d + 1) // 2 for d in case.dims)


def data_key(case):
    """rows with equal keys have equal inputs and so one reference"""
    return (case.N, case.Cin, case.Cout, case.dims) + op_of(case) + (case.lp,)


def tensor(case, name, seeded_tensor):
    """one fp32 tensor of a row on the CPU, the same for every row of one key: "x", "w" (PyTorch layout of the operator), "gy"
    (gradient of the output), "scale", "shift", "res_pre", "res_post" (the output's shape)"""
    stride, transposed = op_of(case)
    tag = f"ctc{data_key(case)[:6]}.{name}"
    N, Cin, Cout = case.N, case.Cin, case.Cout
    oshape = (N, Cout) + out_dims(case)
    if name == "x":
        return seeded_tensor(tag, (N, Cin) + case.dims)
    if name == "w":
        fan = Cin * 27 / (8 if transposed else 1)
        return seeded_tensor(tag, ((Cin, Cout) if transposed else (Cout, Cin)) + (3, 3, 3)) * (1.0 / fan) ** 0.5
    if name == "scale":
        return 1.0 + 0.25 * seeded_tensor(tag, (Cout,))
    if name == "shift":
        return 0.1 * seeded_tensor(tag, (Cout,))
    assert name in ("gy", "res_pre", "res_post"), name
    return seeded_tensor(tag, oshape)
