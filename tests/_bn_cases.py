"""Cases, chunk arithmetic, data and fp64 reference of tests/test_gpu_bn_chunks_fp64.py (no GPU and no library here; the
table, the arithmetic, the plants and the reference are checked without a GPU by tests/test_bn_cases_cpu.py).

Every kernel of the BatchNorm family in csrc/pointwise.hip splits a channel's S = D*H*W voxels into chunks (`chunking`): a
workgroup takes chunk `ch` = [ch * chunk_len, min(S, (ch + 1) * chunk_len)) of one channel (fp32 kernels, `chunking(S, C)`) or
of one group of eight channels (the kernels that write the packed px2 format, `chunking(S, C / 8)`), writes one partial sum
and one per-channel maximum into slot `ch`, and a finalize kernel of one wave per channel reads `nchunk` partials / slots in
trips of 64.  A chunk is never shorter than 1024 voxels, so everything that depends on `ch > 0` -- the chunk's start, the
clipped last chunk, the second trip of the finalize loops, the slot count handed from the writer to the reader, which differs
between the two chunkings -- exists only above S = 1024.  Every row below names the regimes it exists for; the regimes are
predicates on the chunk arithmetic, and a row that drifts off one of them fails.

The reference never goes through `dcanet_amd`: `F.batch_norm` + residual + `F.leaky_relu` on CPU copies, differentiated by
autograd, in double (the truth) or in float (PyTorch's own fp32 result, the yardstick of the gates)."""
import math
import struct
from collections import namedtuple

import torch
import torch.nn.functional as F

BN_MAX_CHUNKS = 256     # the cap `chunking` puts on its chunk count (<= DCA_AMAX_CSLOTS, the stride of the slot table)
EPS = 1e-5
MOMENTUM = 0.1


# ---- chunk arithmetic: `chunking` of csrc/pointwise.hip restated ----------------------------------------------------------
def chunking(S, C):
    """(nchunk, chunk_len) of `chunking(S, C)`"""
    want = min(256, (2048 + C - 1) // C)
    length = (S + want - 1) // want
    length = (length + 1023) // 1024 * 1024
    return (S + length - 1) // length, length


def plain_chunks(C, S):
    """dca_bn_num_chunks: the fp32 kernels (one channel per workgroup)"""
    return chunking(S, C)


def pack_chunks(C, S):
    """dca_bn_pack_chunks: the kernels that write the packed px2 format (eight channels per workgroup)"""
    return chunking(S, (C + 7) // 8)


def x2_scale_exp(v):
    """x2_scale_exp of csrc/dca_common.h on the fp32 number v >= 0: 141 - biased exponent, clamped to [-100, 126]; 0 for a
    zero exponent field (zero and the denormals)"""
    bits = struct.unpack("<I", struct.pack("<f", float(v)))[0]
    e = (bits >> 23) & 255
    ex = 0 if e == 0 else 141 - e
    return max(-100, min(126, ex))


# ---- the table -------------------------------------------------------------------------------------------------------------
Geometry = namedtuple("Geometry", "N C S plain plain_len pack pack_len packable")


def geometry(case):
    S = case.dims[0] * case.dims[1] * case.dims[2]
    (pn, pl), (kn, kl) = plain_chunks(case.C, S), pack_chunks(case.C, S)
    return Geometry(case.N, case.C, S, pn, pl, kn, kl, case.C % 8 == 0)


REGIMES = {
    "many": lambda g: g.plain > 1 and g.pack > 1,
    "vector": lambda g: g.S % 4 == 0,                               # the 16-byte forms, bn_apply_pack4 with residuals
    "scalar": lambda g: g.S % 4 != 0,                               # the scalar forms, the single-voxel pack kernel
    "odd": lambda g: g.S % 2 == 1,
    "clipped": lambda g: g.S % g.plain_len != 0 and g.S % g.pack_len != 0,     # s1 = S inside the last chunk
    "samples": lambda g: g.N > 1,
    "unpackable": lambda g: not g.packable,                         # C % 8 != 0: the packed forms must fall back to fp32
    "packable": lambda g: g.packable,
    "counts-differ": lambda g: g.packable and g.plain != g.pack,    # writer and reader must agree on WHICH count
    "pack-second-trip": lambda g: g.packable and g.pack > 64,       # `i += 64` runs twice over the pack kernels' slots
    "plain-second-trip": lambda g: g.plain > 64,                    # ... over the fp32 kernels' partials and slots
    "plain-one-trip": lambda g: g.plain <= 64,
    "full-table": lambda g: g.plain == BN_MAX_CHUNKS and g.pack == BN_MAX_CHUNKS,
}

Case = namedtuple("Case", "id N C dims S plain pack regimes")
CASES = [
    Case("few", 2, 32, (6, 20, 36), 4320, 5, 5, ("many", "vector", "clipped", "samples", "packable", "plain-one-trip")),
    Case("few-scalar", 2, 32, (5, 21, 38), 3990, 4, 4, ("many", "scalar", "clipped", "samples", "packable")),
    Case("c12", 2, 12, (6, 20, 36), 4320, 5, None, ("many", "vector", "clipped", "samples", "unpackable")),
    Case("over64-pack", 1, 32, (12, 60, 96), 69120, 34, 68,
         ("many", "vector", "clipped", "counts-differ", "pack-second-trip", "plain-one-trip")),
    Case("over64-pack-odd", 1, 32, (11, 61, 103), 69113, 34, 68,
         ("many", "scalar", "odd", "clipped", "counts-differ", "pack-second-trip", "plain-one-trip")),
    Case("over64-plain", 1, 8, (12, 60, 96), 69120, 68, 68, ("many", "vector", "clipped", "packable", "plain-second-trip")),
    Case("full256", 1, 8, (17, 124, 124), 261392, 256, 256,
         ("many", "vector", "clipped", "packable", "plain-second-trip", "pack-second-trip", "full-table")),
]
BY_ID = {c.id: c for c in CASES}

# (slope, res_pre, res_post): the combinations of test_bn_act -- every slope, every residual form
COMBOS = [(0.0, False, False), (0.1, False, False), (1.0, False, True), (0.0, True, True), (1.0, True, False)]
EVAL_COMBO = (0.1, True, False)


# ---- plants ----------------------------------------------------------------------------------------------------------------
# One voxel per channel and quantity that holds the channel's extreme value.  Channels cycle over three positions: the first
# chunk, the last (clipped) chunk, and a chunk with index >= 64 in whichever chunking has that many (else the middle
# chunk); the quantities are shifted against each other, so a channel's four plants sit in different chunks.
QUANTITIES = ("y", "dz", "rp", "rq")
KINDS = ("first", "last", "high")
Plant = namedtuple("Plant", "n c voxel kind plain_chunk pack_chunk")
MARGIN = 2.0 ** -10        # no pre-activation lies closer to the kink of the activation than this (see `data`)
Y_PLANT, DZ_PLANT, U_AT_DZ = 9.0, 8.0, 3.0


def _fine(g):
    """(chunk length, chunk count) of the finer of the two chunkings: both lengths are multiples of 1024 and the row's
    regimes keep the coarser a multiple of the finer, so a chunk of the coarser is a union of chunks of the finer"""
    fine_len = min(g.plain_len, g.pack_len)
    return fine_len, (g.S + fine_len - 1) // fine_len


def high_chunk(g):
    """the `high` position in the finer chunking: past the first trip of the 64-lane loops where there is one (65 of 68,
    128 of 256), else the middle chunk"""
    _, n = _fine(g)
    return 64 + (n - 64) // 3 if n > 65 else n // 2


def claimed_chunks(case, kind):
    """(plain chunk, pack chunk) a plant of `kind` must lie in"""
    g = geometry(case)
    if kind == "first":
        return 0, 0
    if kind == "last":
        return g.plain - 1, g.pack - 1
    fine_len, _ = _fine(g)
    start = high_chunk(g) * fine_len
    return start // g.plain_len, start // g.pack_len


def plants(case, quantity):
    """the plant of every channel for `quantity`: a voxel inside one chunk of the finer chunking (the claim about both
    chunkings is checked, not assumed: tests/test_bn_cases_cpu.py recomputes both chunk indices from the voxel)"""
    g = geometry(case)
    k = QUANTITIES.index(quantity)
    fine_len, fine_n = _fine(g)
    out = []
    for c in range(case.C):
        kind = KINDS[(c + k) % 3]
        start = {"first": 0, "last": fine_n - 1, "high": high_chunk(g)}[kind] * fine_len
        extent = min(g.S, start + fine_len) - start
        voxel = start + (37 * c + 101 * k + 5) % extent
        out.append(Plant(c % case.N, c, voxel, kind, voxel // g.plain_len, voxel // g.pack_len))
    return out


def residual_bound(case, gamma, beta):
    """the bound of bn_bound_exp without residuals, per channel: |gamma| sqrt(N S) + |beta|"""
    g = geometry(case)
    return gamma.double().abs() * math.sqrt(g.N * g.S) + beta.double().abs()


# ---- data ------------------------------------------------------------------------------------------------------------------
_DATA = {}


def _put(t, ps, values):
    for p, v in zip(ps, values):
        t[p.n, p.c].view(-1)[p.voxel] = float(v)


def _unkink(t, u, step):
    """moves the elements of t whose pre-activation u (fp64) lies within MARGIN of 0 away from it by `step` per unit of u"""
    near = u.abs() < MARGIN
    sign = torch.where(u >= 0, 1.0, -1.0)
    return torch.where(near, t.double() + sign * 2 * MARGIN * step, t.double()).float()


def _affine(y, gamma, beta, mean, var):
    v = (1, -1, 1, 1, 1)
    return (y.double() - mean.view(v)) / torch.sqrt(var.view(v) + EPS) * gamma.double().view(v) + beta.double().view(v)


def data(case, seeded_tensor):
    """the row's tensors (fp32, CPU), built once and shared:
      y (1.7 * randn + 0.3), gamma in [0.5, 1.5], beta (0.2 * randn), running mean / variance, dz (randn * 2^-(c % 9)),
      rp / rq (randn): the residuals of the fp32-against-fp64 comparison; rp_eval: the res_pre of the eval-mode run;
      rp_big / rq_big: rp / rq with the residual plants, each >= 2^8 times the bound of bn_bound_exp;
      dz_corr: a gradient correlated with xhat, 2^-(c % 9) (0.5 xhat + 0.05 randn), and against it at the y plant
      (-sign(xhat) 2^-(c % 9)): dgamma / count is then 0.5 2^-(c % 9), and the term max |xhat| |dgamma / count| of the dy
      bound of bn_bwd_finalize_kernel is two thirds of the bound -- the exponent of dy depends on whether the reader of
      the max |y - mean| slots reaches the chunk of the y plant (with dz it is 1e-3 of the bound).
    Plants: y -> mean + 1.7 * 9 (alternating sign), a Gaussian's maximum over 5e5 samples being 5 sigma; dz -> 8 * 2^-(c % 9)
    at a voxel whose pre-activation is made positive (y = mean + 1.7 * 3, rp = 0.25 there), so that it is max |g| at every
    slope.  The activation's kink: fp32 and fp64 disagree about the SIGN of a pre-activation u closer to 0 than its
    rounding error, and one flipped sign is a gradient error of |dz|; over 2e6 elements some u lands there.  The data, not
    the gate, avoids it: y is moved so that |BN(y)| >= MARGIN, then rp (rp_big, rp_eval) so that |BN(y) + rp| >= MARGIN,
    in training and, for rp_eval, with the running statistics."""
    if case.id in _DATA:
        return _DATA[case.id]
    N, C = case.N, case.C
    shape = (N, C) + case.dims
    v = (1, C, 1, 1, 1)
    gen = lambda seed: torch.rand(C, generator=torch.Generator().manual_seed(seed))     # noqa: E731
    gamma, beta = gen(1) + 0.5, seeded_tensor("bnc.b", (C,)) * 0.2
    rm, rv = seeded_tensor("bnc.rm", (C,)) * 0.1, gen(2) + 0.5
    y = seeded_tensor("bnc.y." + case.id, shape) * 1.7 + 0.3
    sign = [1.0 if c % 2 == 0 else -1.0 for c in range(C)]
    _put(y, plants(case, "y"), [0.3 + s * 1.7 * Y_PLANT for s in sign])
    _put(y, plants(case, "dz"), [0.3 + 1.7 * U_AT_DZ] * C)
    for _ in range(2):      # the move changes the batch statistics by ~1e-6 of MARGIN: the second pass finds nothing
        yd = y.double()
        y = _unkink(y, _affine(y, gamma, beta, yd.mean((0, 2, 3, 4)), yd.var((0, 2, 3, 4), unbiased=False)),
                    (torch.sqrt(yd.var((0, 2, 3, 4), unbiased=False)) / gamma.double()).view(v))
    yd = y.double()
    u_train = _affine(y, gamma, beta, yd.mean((0, 2, 3, 4)), yd.var((0, 2, 3, 4), unbiased=False))
    u_eval = _affine(y, gamma, beta, rm.double(), rv.double())
    dz = seeded_tensor("bnc.dz." + case.id, shape) * torch.exp2(-(torch.arange(C) % 9).float()).view(v)
    _put(dz, plants(case, "dz"), [s * DZ_PLANT * 2.0 ** -(c % 9) for c, s in enumerate(sign)])
    big = residual_bound(case, gamma, beta) * 2.0 ** 8 * 1.5
    rp = seeded_tensor("bnc.rp." + case.id, shape)
    _put(rp, plants(case, "dz"), [0.25] * C)
    rp_eval = _unkink(rp, u_eval + rp.double(), 1.0)
    rp_big = rp.clone()
    _put(rp_big, plants(case, "rp"), [-s * b for s, b in zip(sign, big.tolist())])
    rp, rp_big = _unkink(rp, u_train + rp.double(), 1.0), _unkink(rp_big, u_train + rp_big.double(), 1.0)
    rq = seeded_tensor("bnc.rq." + case.id, shape)
    rq_big = rq.clone()
    _put(rq_big, plants(case, "rq"), [s * b for s, b in zip(sign, big.tolist())])
    cscale = torch.exp2(-(torch.arange(C) % 9).double()).view(v)
    xhat = (yd - yd.mean((0, 2, 3, 4)).view(v)) / torch.sqrt(yd.var((0, 2, 3, 4), unbiased=False).view(v) + EPS)
    dz_corr = (cscale * (0.5 * xhat + 0.05 * seeded_tensor("bnc.dzc." + case.id, shape).double())).float()
    _put(dz_corr, plants(case, "y"), [-s * 2.0 ** -(c % 9) for c, s in enumerate(sign)])
    _DATA[case.id] = dict(y=y, gamma=gamma, beta=beta, rm=rm, rv=rv, dz=dz, rp=rp, rq=rq, rp_eval=rp_eval, rp_big=rp_big,
                          rq_big=rq_big, dz_corr=dz_corr)
    return _DATA[case.id]


# ---- reference -------------------------------------------------------------------------------------------------------------
def bn_ref(y, gamma, beta, rm, rv, training, slope, res_pre, res_post):
    z = F.batch_norm(y, rm, rv, gamma, beta, training, MOMENTUM, EPS)
    if res_pre is not None:
        z = z + res_pre
    z = F.leaky_relu(z, slope) if slope != 1.0 else z
    if res_post is not None:
        z = z + res_post
    return z


NAMES = ("z", "dy", "dgamma", "dbeta", "dres_pre", "dres_post", "running_mean", "running_var")


def reference(case, seeded_tensor, training, slope, pre, post, dtype=torch.float64, rp="rp", rq="rq", dz="dz"):
    """{name: tensor} of z = act(BN(y) + res_pre) + res_post and the gradients of sum(z * dz), on CPU in `dtype` (every
    configuration has one reader, so nothing is kept)"""
    d = data(case, seeded_tensor)
    leaf = lambda t: t.detach().to(dtype).clone().requires_grad_()      # noqa: E731
    yc, gc, bc = leaf(d["y"]), leaf(d["gamma"]), leaf(d["beta"])
    rpc, rqc = (leaf(d[rp]) if pre else None), (leaf(d[rq]) if post else None)
    rmc, rvc = d["rm"].to(dtype).clone(), d["rv"].to(dtype).clone()
    z = bn_ref(yc, gc, bc, rmc, rvc, training, slope, rpc, rqc)
    wrt = [yc, gc, bc] + ([rpc] if pre else []) + ([rqc] if post else [])
    gr = list(torch.autograd.grad((z * d[dz].to(dtype)).sum(), wrt))
    out = {"z": z.detach(), "dy": gr[0], "dgamma": gr[1], "dbeta": gr[2], "running_mean": rmc, "running_var": rvc}
    if pre:
        out["dres_pre"] = gr[3]
    if post:
        out["dres_post"] = gr[-1]
    return out


def preactivation(case, seeded_tensor, training, pre, rp="rp"):
    """u = BN(y) + res_pre in double: what the activation's kink and the gradient mask g = dz (u > 0 ? 1 : slope) depend on"""
    d = data(case, seeded_tensor)
    u = F.batch_norm(d["y"].double(), d["rm"].double().clone(), d["rv"].double().clone(), d["gamma"].double(),
                     d["beta"].double(), training, MOMENTUM, EPS)
    return u + d[rp].double() if pre else u


# ---- the exponent bounds of the packed forms ---------------------------------------------------------------------------------
EXP_GUARD = 1e-4       # a bound this close (relatively) to a power of two may round into either binade in fp32: not judged


def expected_exps(bound):
    """(exps, sure): x2_scale_exp of the fp64 per-channel bound (C,), and whether the bound is far enough from a power of
    two for the kernel's fp32 evaluation of the same formula to land in the same binade"""
    m, e = torch.frexp(bound.double())
    exps = (15 - e).clamp(-100, 126)
    sure = (m > 0.5 * (1 + EXP_GUARD)) & (m < 1 - EXP_GUARD) & (bound > 0)
    return exps.to(torch.int32), sure


def z_bound(case, seeded_tensor, rp=None, rq=None):
    """the bound of bn_bound_exp in double: (|gamma| sqrt(N S) + |beta| + max |res_pre| + max |res_post|) 1.0001"""
    d = data(case, seeded_tensor)
    b = residual_bound(case, d["gamma"], d["beta"])
    for name in (rp, rq):
        if name is not None:
            b = b + d[name].double().abs().amax((0, 2, 3, 4))
    return b * 1.0001


def dy_bound(case, seeded_tensor, slope, dz="dz", without_plant_of=None):
    """the bound of bn_bwd_finalize_kernel in double, training, no res_pre:
    |scale| (max |g| + |dbeta / count| + max |xhat| |dgamma / count|) 1.0001 with max |xhat| = invstd max |y - mean|.
    without_plant_of: a set of plant kinds whose y plant the maximum of |y - mean| is taken WITHOUT -- what a reader finds
    that misses the slots of those chunks (tests/test_bn_cases_cpu.py: the exponent must depend on it)"""
    d = data(case, seeded_tensor)
    C = case.C
    v = (1, C, 1, 1, 1)
    yd = d["y"].double()
    mean, var = yd.mean((0, 2, 3, 4)), yd.var((0, 2, 3, 4), unbiased=False)
    invstd = 1.0 / torch.sqrt(var + EPS)
    xhat = (yd - mean.view(v)) * invstd.view(v)
    u = xhat * d["gamma"].double().view(v) + d["beta"].double().view(v)
    g = d[dz].double() * torch.where(u > 0, 1.0, slope)
    count = case.N * case.S
    k1, k2 = g.sum((0, 2, 3, 4)).abs() / count, (g * xhat).sum((0, 2, 3, 4)).abs() / count
    ax = xhat.abs().clone()
    if without_plant_of:
        for p in plants(case, "y"):
            if p.kind in without_plant_of:
                ax[p.n, p.c].view(-1)[p.voxel] = 0.0
    return (d["gamma"].double() * invstd).abs() * (g.abs().amax((0, 2, 3, 4)) + k1 + ax.amax((0, 2, 3, 4)) * k2) * 1.0001


# the gates of test_bn_act (tests/test_gpu_parity.py `close`): max-abs <= tol * max(1, max |ref|)
GATES = {"z": 1e-5, "dy": 2e-5, "dgamma": 2e-5, "dbeta": 2e-5, "dres_pre": 2e-5, "dres_post": 2e-5, "running_mean": 1e-6,
         "running_var": 1e-6}


def gate_ratio(got, ref, tol):
    """max |got - ref| over the gate tol * max(1, max |ref|); NaN counts as infinite"""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = torch.nan_to_num((got - ref).abs(), nan=float("inf"))
    return err.max().item() / (tol * max(1.0, ref.abs().max().item()))


def worst_chunk(got, ref, chunk_len):
    """names the chunk (of length chunk_len along S) that holds the largest |got - ref| of an (N, C, D, H, W) pair"""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    N, C = ref.shape[0], ref.shape[1]
    S = ref[0, 0].numel()
    err = torch.nan_to_num((got - ref).abs(), nan=float("inf")).reshape(N, C, S)
    nchunk = (S + chunk_len - 1) // chunk_len
    pad = F.pad(err, (0, nchunk * chunk_len - S)).view(N, C, nchunk, chunk_len)
    per = pad.amax(3)
    n, c, ch = [int(i) for i in (per == per.max()).nonzero()[0]]
    s0, s1 = ch * chunk_len, min(S, (ch + 1) * chunk_len)
    bad = int((per > 0.5 * per.max()).sum()) if per.max() > 0 else 0
    return (f"worst chunk {ch} of {nchunk} (voxels [{s0}, {s1}){', the clipped last chunk' if s1 - s0 < chunk_len else ''}) "
            f"of sample {n}, channel {c}: max err {per.max().item():.3e}; {bad} (sample, channel, chunk) within 2x of it")
