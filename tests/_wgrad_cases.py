"""Cases, fp64 reference and tile arithmetic of tests/test_gpu_wgrad_fp64.py (no GPU import here; the arithmetic and the
table are checked without a GPU by tests/test_wgrad_cases_cpu.py).

The weight-gradient kernels are persistent: `nblk` workgroups per channel-tile pair walk `ntiles` spatial tiles, fetch the
next tile while they multiply the current one, write one slab each, and `wgrad_reduce_kernel` adds the `nblk` slabs.  Every
row below names the REGIME of that control flow it exists for; the GPU test reads `nblk` back from the kernel's own size
query and asserts the regime before it compares anything, so a row that drifts off its branch fails instead of passing on
other grounds.

The reference never goes through `dcanet_amd`: `reference` is `torch.nn.grad.conv3d_weight` on double copies."""
from collections import namedtuple

import torch


def cdiv(a, b):
    return (a + b - 1) // b


# ---- reference ----------------------------------------------------------------------------------------------------------------
def reference(x, dy, ksize, stride):
    """fp64 dW[cy][cx][k] (Cy, Cx, ksize^3) of a convolution with padding ksize // 2: x (N, Cx, D, H, W) its input, dy
    (N, Cy, Do, Ho, Wo) the gradient of its output"""
    Cx, Cy = x.shape[1], dy.shape[1]
    w = torch.nn.grad.conv3d_weight(x.detach().cpu().double(), (Cy, Cx, ksize, ksize, ksize), dy.detach().cpu().double(),
                                    stride=stride, padding=ksize // 2)
    return w.reshape(Cy, Cx, ksize ** 3)


def scatter_index(Cy, Cx, K, s_cy, s_cx, offset):
    """flat destination index of dW[cy][cx][k] in the layout of dca_hip.h: offset + cy * s_cy + cx * s_cx + k"""
    cy = torch.arange(Cy).view(Cy, 1, 1)
    cx = torch.arange(Cx).view(1, Cx, 1)
    k = torch.arange(K).view(1, 1, K)
    return offset + cy * s_cy + cx * s_cx + k


def scatter(ref, dest, s_cy, s_cx, offset):
    """writes ref (Cy, Cx, K) into the flat tensor dest at dest[offset + cy*s_cy + cx*s_cx + k] and returns the boolean mask
    of the elements written; every other element of dest is left alone"""
    idx = scatter_index(*ref.shape, s_cy, s_cx, offset).reshape(-1)
    assert dest.dim() == 1 and int(idx.min()) >= 0 and int(idx.max()) < dest.numel()
    assert idx.unique().numel() == idx.numel(), "the layout maps two elements onto one"
    dest[idx] = ref.reshape(-1).to(dest.dtype)
    mask = torch.zeros(dest.numel(), dtype=torch.bool)
    mask[idx] = True
    return mask


# ---- tile arithmetic: the *_geometry functions of csrc/conv3d_wgrad*.hip restated ------------------------------------------------
# each returns (ntiles, nCT, share): spatial tiles, 32 x 32 channel tiles (slabs per workgroup set), grid rows dividing the CUs
def tiles_split_s1(N, Cx, Cy, dims):
    """conv3d_wgrad_f16x2.hip / conv3d_wgrad_bf16x3.hip: tile 2 x 4 x 16"""
    D, H, W = dims
    nCT = cdiv(Cx, 32) * cdiv(Cy, 32)
    return N * cdiv(D, 2) * cdiv(H, 4) * cdiv(W, 16), nCT, nCT


def tiles_s2x2(N, Cx, Cy, dims):
    """conv3d_wgrad_s2_f16x2.hip: tile 1 x 4 x 16 on the coarse dims, one workgroup row per (32 x, 64 dy) channel block pair"""
    Do, Ho, Wo = ((d + 1) // 2 for d in dims)
    return N * Do * cdiv(Ho, 4) * cdiv(Wo, 16), cdiv(Cx, 32) * cdiv(Cy, 32), cdiv(Cx, 32) * cdiv(Cy, 64)


def generic_tile_w(W):
    """wg_tile_w of the generic 3x3x3 stride-1 kernel: 16 where that pads the row less than 32 does"""
    return 16 if cdiv(W, 16) * 16 < cdiv(W, 32) * 32 else 32


def tiles_generic_s1(N, Cx, Cy, dims):
    """wgrad3_kernel<1, 32>: tile 2 x 4 x 32; wgrad3_kernel<1, 16>: 2 x 8 x 16"""
    D, H, W = dims
    TW = generic_tile_w(W)
    nCT = cdiv(Cx, 32) * cdiv(Cy, 32)
    return N * cdiv(D, 2) * cdiv(H, 4 if TW == 32 else 8) * cdiv(W, TW), nCT, nCT


def tiles_generic_s2(N, Cx, Cy, dims):
    """wgrad3_kernel<2, 32>: tile 1 x 2 x 32 on the coarse dims"""
    Do, Ho, Wo = ((d + 1) // 2 for d in dims)
    nCT = cdiv(Cx, 32) * cdiv(Cy, 32)
    return N * Do * cdiv(Ho, 2) * cdiv(Wo, 32), nCT, nCT


def tiles_k1(N, Cx, Cy, dims):
    """wgrad1_kernel: 256 voxels per tile"""
    D, H, W = dims
    nCT = cdiv(Cx, 32) * cdiv(Cy, 32)
    return N * cdiv(D * H * W, 256), nCT, nCT


# family -> (tile function, ksize, stride, does the grid rule ask the device for its CU count)
FAMILIES = {
    "x2": (tiles_split_s1, 3, 1, True),       # conv3d_wgrad_f16x2.hip
    "x3": (tiles_split_s1, 3, 1, True),       # conv3d_wgrad_bf16x3.hip
    "s2x2": (tiles_s2x2, 3, 2, True),         # conv3d_wgrad_s2_f16x2.hip
    "g3s1": (tiles_generic_s1, 3, 1, False),  # wgrad3_kernel<1, 32> / <1, 16>
    "g3s2": (tiles_generic_s2, 3, 2, False),  # wgrad3_kernel<2, 32>
    "g1": (tiles_k1, 1, 1, False),            # wgrad1_kernel<false>
    "head": (tiles_k1, 1, 1, False),          # wgrad1_kernel<true>: the 27 taps are the dy "channels"
}


def workgroups(family, ntiles, nCT, share, ncu):
    """nblk of the launch: dca_persistent_grid for the split kernels, wg_workers (the constant 256) for the generic ones"""
    if FAMILIES[family][3]:
        return min(ntiles, max(1, ncu // share))
    return min(ntiles, max(1, 256 * (2 if FAMILIES[family][1] == 1 else 1) // nCT))


def split_walk(ntiles, nblk):
    """tiles each workgroup of a split kernel visits: dca_tile_walk_of of csrc/dca_tiles.h restated on its own (eight XCD
    chunks of T * xcd / 8, each shared by the `cnt` workgroups dealt to that XCD; one chunk when the grid has fewer than eight
    workgroups); tests/test_wgrad_cases_cpu.py compares it with the library's dca_tile_walk"""
    nx = 8 if nblk >= 8 else 1
    out = []
    for b in range(nblk):
        xcd = b % nx
        cnt = (nblk - xcd + nx - 1) // nx
        out.append(list(range(ntiles * xcd // nx + b // nx, ntiles * (xcd + 1) // nx, cnt)))
    return out


def generic_walk(ntiles, nblk):
    """tiles each workgroup of a generic kernel visits: tile = blockIdx.x; tile += gridDim.x"""
    return [list(range(b, ntiles, nblk)) for b in range(nblk)]


def reduce_iters(nblk):
    """(unrolled 8-way iterations, tail iterations) of each of the 16 thread groups of wgrad_reduce_kernel"""
    out = []
    for g in range(16):
        b, u, t = g, 0, 0
        while b + 7 * 16 < nblk:
            b += 8 * 16
            u += 1
        while b < nblk:
            b += 16
            t += 1
        out.append((u, t))
    return out


# ---- cases --------------------------------------------------------------------------------------------------------------------
# pack: which operands of the f16x2 kernel are packed px2 images ("ff" = none, "pf" = x, "fp" = dy, "pp" = both)
# mag: factors on x and dy; pow2: every channel times its own power of two; misalign: operand that starts 4 bytes past a
# 16-byte boundary; N for the head family counts batch elements of a (N, C, D, H, W) input with one output channel (Cy = 27 taps)
Case = namedtuple("Case", "id family N Cx Cy dims regimes pack mag pow2 misalign")


def _c(id, family, N, Cx, Cy, dims, regimes, pack="ff", mag=(1.0, 1.0), pow2=False, misalign=None):
    return Case(id, family, N, Cx, Cy, tuple(dims), tuple(regimes), pack, mag, pow2, misalign)


def geometry(case, ncu=256):
    """(ntiles, nCT, share, nblk) of a case by the arithmetic above"""
    ntiles, nCT, share = FAMILIES[case.family][0](case.N, case.Cx, case.Cy, case.dims)
    return ntiles, nCT, share, workgroups(case.family, ntiles, nCT, share, ncu)


def out_dims(case):
    stride = FAMILIES[case.family][2]
    return tuple((d + stride - 1) // stride for d in case.dims)


def _walk(case, ntiles, nblk):
    return (split_walk if FAMILIES[case.family][3] else generic_walk)(ntiles, nblk)


def _vec_flags(case):
    """(vecx, vecy) as the generic launcher sets them"""
    ok_x, ok_y = case.misalign != "x", case.misalign != "dy"
    if FAMILIES[case.family][1] == 1:
        D, H, W = case.dims
        v = (D * H * W) % 4 == 0 and ok_x and ok_y
        return v, v
    return case.dims[2] % 4 == 0 and ok_x, out_dims(case)[2] % 4 == 0 and ok_y


def _partial(case):
    """partial channel blocks and a partial tile in every spatial dimension"""
    fam = case.family
    od = out_dims(case)
    if fam in ("x2", "x3"):
        t = (2, 4, 16)
    elif fam == "s2x2":
        t = (1, 4, 16)
    elif fam == "g3s1":
        t = (2, 4, 32) if generic_tile_w(case.dims[2]) == 32 else (2, 8, 16)
    elif fam == "g3s2":
        t = (1, 2, 32)
    else:
        return case.Cx % 32 != 0 and case.Cy % 32 != 0 and (od[0] * od[1] * od[2]) % 256 != 0
    spatial = all(d % td != 0 for d, td in zip(od, t) if td > 1)
    return case.Cx % 32 != 0 and case.Cy % 32 != 0 and spatial


# regime name -> predicate(case, ntiles, nCT, nblk); nblk comes from the device's size query on the GPU
REGIMES = {
    # tile loop and cross-tile prefetch
    "every workgroup has 3+ tiles": lambda c, T, nCT, nb: min(len(w) for w in _walk(c, T, nb)) >= 3,
    "every workgroup has 2+ tiles": lambda c, T, nCT, nb: min(len(w) for w in _walk(c, T, nb)) >= 2,
    "some workgroups have 2+ tiles": lambda c, T, nCT, nb: max(len(w) for w in _walk(c, T, nb)) >= 2,
    "uneven cnt between XCDs": lambda c, T, nCT, nb: nb >= 8 and nb % 8 != 0,
    "nx = 1, 2 tiles on some workgroups and 1 on others":
        lambda c, T, nCT, nb: nb < 8 and {len(w) for w in _walk(c, T, nb)} == {1, 2},
    "partial channel blocks and partial tiles": lambda c, T, nCT, nb: _partial(c),
    "odd fine D and H": lambda c, T, nCT, nb: c.dims[0] % 2 == 1 and c.dims[1] % 2 == 1,
    "blk_on false in the last coarse pair": lambda c, T, nCT, nb: 0 < c.Cy % 64 <= 32 and c.Cy > 64,
    "packed x": lambda c, T, nCT, nb: c.pack[0] == "p" and c.Cx % 8 == 0,
    "packed dy": lambda c, T, nCT, nb: c.pack[1] == "p" and c.Cy % 8 == 0,
    "both packed, two LDS image sets": lambda c, T, nCT, nb: c.pack == "pp" and max(len(w) for w in _walk(c, T, nb)) >= 2,
    "W % 4 != 0": lambda c, T, nCT, nb: c.dims[2] % 4 != 0,
    "scaled operands": lambda c, T, nCT, nb: c.mag == (1e3, 1e-9),
    # generic kernels: template and staging path
    "tile width 32": lambda c, T, nCT, nb: c.family == "g3s1" and generic_tile_w(c.dims[2]) == 32,
    "tile width 16": lambda c, T, nCT, nb: c.family == "g3s1" and generic_tile_w(c.dims[2]) == 16,
    "pipelined": lambda c, T, nCT, nb: _vec_flags(c) == (True, True),
    "not pipelined": lambda c, T, nCT, nb: _vec_flags(c) != (True, True) and c.misalign is None,
    "vecx on, vecy off": lambda c, T, nCT, nb: _vec_flags(c) == (True, False),
    "vecx off, vecy off": lambda c, T, nCT, nb: _vec_flags(c) == (False, False),
    "misaligned base at an aligned width":
        lambda c, T, nCT, nb: c.misalign is not None and c.dims[2] % 4 == 0 and out_dims(c)[2] % 4 == 0,
    "voxel count % 4 != 0": lambda c, T, nCT, nb: (c.dims[0] * c.dims[1] * c.dims[2]) % 4 != 0,
    "256 workgroups": lambda c, T, nCT, nb: nb == 256,
    # wgrad_reduce_kernel
    "nCT = 1": lambda c, T, nCT, nb: nCT == 1,
    "nCT = 3": lambda c, T, nCT, nb: nCT == 3,
    "one slab": lambda c, T, nCT, nb: nb == 1,
    "tail loop only, fewer slabs than thread groups": lambda c, T, nCT, nb: 1 < nb < 16,
    "tail loop only": lambda c, T, nCT, nb: 16 <= nb <= 112,
    "unrolled loop in part of the groups": lambda c, T, nCT, nb: len({u for u, _ in reduce_iters(nb)}) == 2 and nb < 128,
    "unrolled loop, then the tail": lambda c, T, nCT, nb: all(u == 1 and t >= 1 for u, t in reduce_iters(nb)),
    "capped grid, unrolled loop twice": lambda c, T, nCT, nb: T > nb and all(u == 2 and t == 0 for u, t in reduce_iters(nb)),
}

MANY3, MANY2, SOME2 = "every workgroup has 3+ tiles", "every workgroup has 2+ tiles", "some workgroups have 2+ tiles"

# stride-1 split kernels: each row on x3, and on x2 in every operand combination its channel counts allow
_SPLIT_ROWS = [
    ("uneven", 2, 96, 96, (7, 14, 44), (MANY3, "uneven cnt between XCDs")),
    ("nx1", 1, 192, 192, (4, 8, 40), ("nx = 1, 2 tiles on some workgroups and 1 on others",)),
    ("partial", 1, 33, 40, (9, 17, 36), (SOME2, "partial channel blocks and partial tiles")),
]
_PACK_REGIME = {"ff": (), "pf": ("packed x",), "fp": ("packed dy",), "pp": ("packed x", "packed dy")}
X3 = [_c(f"x3-{n}", "x3", N, cx, cy, d, r, pow2=(n == "uneven")) for n, N, cx, cy, d, r in _SPLIT_ROWS]
X2 = [_c(f"x2-{n}-{p}", "x2", N, cx, cy, d, r + _PACK_REGIME[p] + (("both packed, two LDS image sets",) if p == "pp" else ()),
         pack=p, pow2=(n == "uneven"))
      for n, N, cx, cy, d, r in _SPLIT_ROWS for p in ("ff", "pf", "fp", "pp")
      if (p[0] == "f" or cx % 8 == 0) and (p[1] == "f" or cy % 8 == 0)]
X2.append(_c("x2-w42-pp", "x2", 2, 96, 96, (7, 14, 42),
             (MANY3, "uneven cnt between XCDs", "both packed, two LDS image sets", "W % 4 != 0"), pack="pp"))

_S2_ROWS = [
    ("blkoff", 2, 96, 160, (10, 26, 72), (MANY3, "uneven cnt between XCDs", "blk_on false in the last coarse pair")),
    # 18 batch elements: 15 tiles each, so that the 256 workgroups of the single channel block pair get 1 or 2
    ("odd", 18, 20, 33, (9, 17, 24), (SOME2, "odd fine D and H", "partial channel blocks and partial tiles")),
]
S2X2 = [_c(f"s2x2-{n}{'-scaled' if m != (1.0, 1.0) else ''}", "s2x2", N, cx, cy, d,
           r + (("scaled operands",) if m != (1.0, 1.0) else ()), mag=m, pow2=(n == "blkoff" and m == (1.0, 1.0)))
        for n, N, cx, cy, d, r in _S2_ROWS for m in ((1.0, 1.0), (1e3, 1e-9))]

GENERIC = [
    _c("g32-pipelined", "g3s1", 3, 96, 96, (7, 14, 60), (MANY3, "tile width 32", "pipelined"), pow2=True),
    _c("g32-plain", "g3s1", 3, 96, 96, (7, 14, 58), (MANY3, "tile width 32", "not pipelined")),
    _c("g16-pipelined", "g3s1", 4, 96, 96, (7, 14, 44), (MANY3, "tile width 16", "pipelined")),
    _c("g16-plain", "g3s1", 4, 96, 96, (7, 14, 42), (MANY3, "tile width 16", "not pipelined")),
    _c("gs2-vec", "g3s2", 2, 96, 96, (10, 20, 72), (MANY3, "pipelined")),
    _c("gs2-vecx", "g3s2", 4, 96, 96, (10, 20, 20), (MANY3, "vecx on, vecy off")),      # N = 4: one 32-wide tile per row
    _c("gs2-scalar", "g3s2", 2, 96, 96, (10, 20, 70), (MANY3, "vecx off, vecy off")),
    _c("g32-misaligned-x", "g3s1", 3, 96, 96, (7, 14, 60), (MANY3, "tile width 32", "misaligned base at an aligned width"),
       misalign="x"),
    _c("gs2-misaligned-dy", "g3s2", 2, 96, 96, (10, 20, 72), (MANY3, "misaligned base at an aligned width"), misalign="dy"),
    _c("g1-vec", "g1", 6, 96, 96, (9, 17, 40), (MANY2, "pipelined"), pow2=True),           # 56 workgroups, 144 tiles
    _c("g1-scalar", "g1", 6, 96, 96, (9, 17, 41), (MANY2, "voxel count % 4 != 0", "not pipelined")),
]

# the logit heads through ops._Conv3dC1 (Cx = C input channels, one output channel: Cy = 27 taps)
HEAD = [
    _c("head-c64", "head", 5, 64, 27, (17, 30, 60), (MANY2, "256 workgroups"), pow2=True),     # 600 tiles
    _c("head-c32-small", "head", 2, 32, 27, (5, 9, 20), ()),                                    # also on the expand route
]

# wgrad_reduce_kernel: 32 -> 32 channels on both stride-1 split kernels, so nblk = the tile count up to the device's cap
_REDUCE_ROWS = [
    (1, 1, (2, 4, 16), ("nCT = 1", "one slab")),
    (12, 1, (4, 8, 48), ("nCT = 1", "tail loop only, fewer slabs than thread groups")),
    (75, 1, (10, 20, 48), ("nCT = 1", "tail loop only")),
    (120, 1, (10, 16, 96), ("nCT = 1", "unrolled loop in part of the groups")),
    (150, 2, (10, 20, 48), ("nCT = 1", "unrolled loop, then the tail")),
    (288, 1, (17, 30, 60), ("nCT = 1", "capped grid, unrolled loop twice")),
]
REDUCE = [_c(f"reduce-{fam}-{t}", fam, N, 32, 32, d, r) for t, N, d, r in _REDUCE_ROWS for fam in ("x2", "x3")]
REDUCE.append(_c("reduce-g1-170x3", "g1", 8, 96, 32, (9, 17, 40), ("nCT = 3", "unrolled loop, then the tail")))   # 192 tiles

ALL = X2 + X3 + S2X2 + GENERIC + HEAD + REDUCE

# every regime the gate exists for: tests/test_wgrad_cases_cpu.py requires a row for each
REQUIRED = {
    "x2": [MANY3, "uneven cnt between XCDs", "nx = 1, 2 tiles on some workgroups and 1 on others",
           "partial channel blocks and partial tiles", "packed x", "packed dy", "both packed, two LDS image sets", "W % 4 != 0",
           "one slab", "tail loop only", "unrolled loop in part of the groups", "unrolled loop, then the tail",
           "capped grid, unrolled loop twice"],
    "x3": [MANY3, "uneven cnt between XCDs", "nx = 1, 2 tiles on some workgroups and 1 on others",
           "partial channel blocks and partial tiles", "one slab", "tail loop only", "unrolled loop in part of the groups",
           "unrolled loop, then the tail", "capped grid, unrolled loop twice"],
    "s2x2": [MANY3, "uneven cnt between XCDs", "blk_on false in the last coarse pair", "odd fine D and H",
             "partial channel blocks and partial tiles", "scaled operands"],
    "g3s1": ["tile width 32", "tile width 16", "pipelined", "not pipelined", "misaligned base at an aligned width", MANY3],
    "g3s2": ["pipelined", "vecx on, vecy off", "vecx off, vecy off", MANY3],
    "g1": [MANY2, "pipelined", "voxel count % 4 != 0", "nCT = 3"],
    "head": [MANY2, "256 workgroups"],
}


# the strided destination.  (1) the second input (40 channels, behind C1 = 32) of a two-input 1x1x1 convolution with 64
# outputs, as _Conv3d.backward writes it: s_cy = Cin = 72, s_cx = 1, offset C1.  (2) the transposed convolution 64 -> 32 from
# coarse 5 x 13 x 36: the fine output gradient is x, the coarse input dy, dW[cin][cout][k]
STRIDED_C1 = _c("strided-c1-second-input", "g1", 12, 40, 64, (9, 17, 40), (MANY2,))
STRIDED_C1_FIRST = 32
STRIDED_T = _c("strided-transposed", "s2x2", 6, 32, 64, (10, 26, 72), (SOME2, "256 workgroups"))
EVERY = ALL + [STRIDED_C1, STRIDED_T]


def inputs(case, seeded_tensor):
    """(x, dy) of a case on the CPU in fp32; the same tensors for every case of one shape and scaling"""
    tag = f"{case.N},{case.Cx},{case.Cy},{case.dims},{FAMILIES[case.family][1:3]}"
    Cy = 1 if case.family == "head" else case.Cy
    x = seeded_tensor(f"wgc.x{tag}", (case.N, case.Cx) + case.dims) * case.mag[0]
    dy = seeded_tensor(f"wgc.g{tag}", (case.N, Cy) + out_dims(case)) * case.mag[1]
    if case.pow2:
        x = x * torch.exp2(torch.arange(case.Cx).float() % 7).view(1, -1, 1, 1, 1)
        dy = dy * torch.exp2(-(torch.arange(Cy).float() % 5)).view(1, -1, 1, 1, 1)
    return x, dy


def data_key(case):
    """cases with equal keys have equal inputs and so one reference"""
    return (case.N, case.Cx, case.Cy, case.dims, FAMILIES[case.family][1:3], case.mag, case.pow2, case.family == "head")
