"""The BatchNorm kernels of csrc/pointwise.hip against fp64 beyond one chunk per channel.

bn_stats / bn_finalize / bn_apply / bn_apply_pack / bn_apply_pack4, bn_bwd_reduce / bn_bwd_finalize / bn_bwd_apply /
bn_bwd_apply_pack and cmax / cmax_exps split a channel's S = D*H*W voxels with `chunking`; a chunk is never shorter than 1024
voxels and the op-level BatchNorm tests stay at one chunk (test_bn_act, test_bn_pack_kernels_*, the tag tests) or two (the
packed training chains, S = 1440, through whole-chain relative-L2 gates).  What exists only from the second chunk on -- the
chunk's start `ch * chunk_len`, the clipped last chunk, the second trip of the 64-lane loops over partials and slots, the
last of 256 slots, and the slot COUNT that travels from the kernel that wrote per-channel maxima to the kernel that reads
them, which differs between the fp32 kernels (`dca_bn_num_chunks`) and the pack kernels (`dca_bn_pack_chunks`) -- is gated
here.  Every row of tests/_bn_cases.py names its regimes (`many`, `vector` / `scalar` / `odd`, `clipped`, `samples`,
`counts-differ`, `plain-second-trip`, `pack-second-trip`, `full-table`, `unpackable`) and fails, not skips, off them; the
table, the plants and the references are checked without a GPU by tests/test_bn_cases_cpu.py.  Every run goes through
`ops.bn_act` into memory that held NaN (outputs) or NaN bit patterns (slot tables).

  1. the library's chunk counts are the table's (test_chunk_counts);
  2. the fp32 route in training, the five (slope, res_pre, res_post) combinations of test_bn_act, and one eval-mode run with
     gradients, against fp64 at test_bn_act's gates, errors named per chunk (test_fp32_route_training / _eval);
  3. exact slot maxima: the tag of z and of the dy its producer receives has the writer's chunk count, and the maximum over
     exactly those slots is max |.| bit for bit; the same for untagged tensors through `ops._slots_of`, slot by slot, with
     `ops._exps_of` equal to the x2_scale_exp mirror (test_slot_maxima_and_exponents);
  4. the packed routes (`pack_out=True`, `"both"`, `pack_dy=True`; residuals with maxima planted in the first, the last and
     a high chunk; bn_apply_pack4 on the aligned rows, the single-voxel kernel on the others) against the fp32 kernels on the
     same inputs: unpacked z and dy within 2^-21 of the channel's maximum, every f16 term finite and below 2^15, dgamma /
     dbeta / residual gradients / running statistics bit-equal, the fp32 copy of `"both"` bit-equal with exact slot maxima
     (test_packed_routes_match_fp32_route), and the exponents equal to x2_scale_exp of the kernels' bounds restated in fp64
     (`_exps_are`; channels whose bound is within 1e-4 of a power of two are not judged);
  5. the two places where only an exponent shows a miscount: the dy bound's max |xhat| term, made two thirds of the bound by
     a gradient correlated with xhat (test_packed_gradient_exponent_follows_max_xhat), and a residual whose maxima sit in the
     pack chunking's slots because a `"both"` BatchNorm wrote it (test_residual_written_by_a_packed_batchnorm);
  6. `ops.pack_x2` round-trips; two identical calls give identical bits (outputs, gradients, exponents, written slots);
     row `c12` (C % 8 != 0): the packed requests return the fp32 kernels' bits without a `_dca_px2` tag or a twin.

Gates: those of test_bn_act unchanged -- max-abs <= tol max(1, max |ref|) with tol 1e-5 (z), 2e-5 (gradients), 1e-6 (running
statistics) -- and 2^-21 of the channel's maximum for a packed tensor against its fp32 twin.  No gate was widened: the sums
over 69 k .. 261 k voxels stay as far inside them as the sums over 288.  The activation's kink is kept out of the DATA
(tests/_bn_cases.py `data`): no pre-activation lies within 2^-10 of zero, so fp32 and fp64 agree on every gradient mask.

Not covered: `stats_part` / bn_finalize_centered (tests/test_gpu_conv_tiles_fp64.py gates it); `lazy_dy` /
dca_bn_backward_reduce (tests/test_gpu_c1_bwd_fused.py); tensors above 2 GiB; `pack_dy` in eval mode; the VALUE of max |xhat|
beyond its effect on the exponent.

MEASURED on one MI355X, max error / gate over the seven rows (every test prints its lines), beside PyTorch's own fp32 CPU
BatchNorm on the same data (tests/test_bn_cases_cpu.py):

  quantity       training          eval              PyTorch fp32 CPU
  z              0.004 .. 0.011    0.006 .. 0.007    0.007 .. 0.013
  dy             0.002 .. 0.012    0.001 .. 0.002    0.004 .. 0.007
  dgamma         0.001 .. 0.011    0.003 .. 0.012    0.020 .. 0.264
  dbeta          0.001 .. 0.094    0.002 .. 0.008    0.033 .. 0.310
  running_mean   0.009 .. 0.017    unchanged         0.006 .. 0.017
  running_var    0.047 .. 0.075    unchanged         0.049 .. 0.075
  residual gradients: exact.  Packed against fp32, / 2^-21: z 0.13 .. 0.25, dy 0.01 .. 0.34.  118 tests, 5 s.

One defect found, by item 4 on every packable row: without a res_post the pack kernels added +0 to the activation, so for
ReLU the fp32 copy of `"both"` held +0 where bn_apply_kernel writes -0 (v * 0 for v < 0).  Equal numbers, different bits;
the absent residual is now the neutral -0 in both pack kernels.  The benchmark does not see it (92.70 ms per step against
92.66 with the parent's kernels, means of three alternating runs that spread over 92.5 .. 92.9 either way).

That the gates bite (libraries / ops.py changed in a scratch copy, never committed; each run once).  (1) bn_apply_kernel and
bn_bwd_apply_kernel return at once in their last chunk when there is more than one: 98 of the 118 tests fail (the chunk reads
NaN; the tests that reach neither kernel pass); of the existing tests test_bn_act, test_bn_pack_kernels_* and
test_bn_act_tags_each_output_form pass, the six test_packed_training_chain_* cases (S = 1440: two chunks) fail.  (2) the
partial-sum and slot loops of bn_finalize, bn_bwd_finalize, bn_bound_exp and cmax_exps stop at 64: 38 tests fail -- every test
of `over64-plain` and `full256` that passes a finalize kernel, and on `over64-pack` / `over64-pack-odd` (34 fp32 chunks, 68
pack chunks) the two tests of item 5 (an f16 term overflows; dy exponents one too high); all 34 existing BatchNorm tests pass.
(3) `_BnAct.forward` records dca_bn_num_chunks where the pack kernel wrote dca_bn_pack_chunks slots: 12 tests fail, all on
`over64-pack` / `over64-pack-odd` -- the three `"both"` configurations of item 4 (tag count), both forms of the gradient
exponent test (the packed-only form has no tag: only the exponent shows it) and the packed residual test; all 34 existing
BatchNorm tests pass."""
import pytest
import torch

import _bn_cases as B
from oracle.seeded import seeded_tensor
from test_gpu_parity import _GradProbe, _chan_err, _family, _unpack_px2, close

pytestmark = pytest.mark.gpu

DEV = "cuda"
IDS = [c.id for c in B.CASES]
PACKABLE = [c.id for c in B.CASES if c.pack is not None]
PACK_GATE = 2.0 ** -21        # the gate of test_bn_pack_kernels_match_fp32_kernels, per channel, of the channel's maximum
NAN_BITS = 0x7FC00000


def _setup(monkeypatch):
    import dcanet_amd  # noqa: F401
    from dcanet_amd import ops
    _family(monkeypatch, ops, "f16x2")
    for flag in ("PACK", "AMAX_EMIT"):
        monkeypatch.setattr(ops, flag, True)
    return ops


def _poison(case, ops):
    """fills blocks of the sizes the launch under test allocates -- an output, its twin, a second gradient; slot tables -- with
    NaN and frees them, so that the caching allocator hands the launch memory in which a chunk that is never written stays
    NaN and a slot that is never written is larger than every maximum"""
    big = [torch.full((case.N, case.C) + case.dims, float("nan"), device=DEV) for _ in range(3)]
    small = [torch.full((case.C * ops.CSLOTS,), NAN_BITS, device=DEV, dtype=torch.int32) for _ in range(4)]
    del big, small


def _module(case, d, training):
    bn = torch.nn.BatchNorm3d(case.C).to(DEV)
    with torch.no_grad():
        bn.weight.copy_(d["gamma"]); bn.bias.copy_(d["beta"]); bn.running_mean.copy_(d["rm"]); bn.running_var.copy_(d["rv"])
    return bn.train(training)


def _run(ops, case, training, slope, rp=None, rq=None, pack_out=False, pack_dy=False, dz="dz"):
    """one forward and backward through ops.bn_act into poisoned memory.  rp / rq: names of the row's residual tensors.
    Returns z, the gradient OBJECT the producer of y would receive (g) and {name: tensor} of everything comparable"""
    d = B.data(case, seeded_tensor)
    bn = _module(case, d, training)
    leaf = lambda name: d[name].to(DEV).requires_grad_()      # noqa: E731
    yg, rpg, rqg = leaf("y"), (leaf(rp) if rp else None), (leaf(rq) if rq else None)
    dz = d[dz].to(DEV)
    _poison(case, ops)
    z = ops.bn_act(_GradProbe.apply(yg), bn, slope, rpg, rqg, pack_out=pack_out, pack_dy=pack_dy)
    wrt = [yg, bn.weight, bn.bias] + ([rpg] if rp else []) + ([rqg] if rq else [])
    _poison(case, ops)
    gg = torch.autograd.grad(z, wrt, dz)
    g = _GradProbe.seen.pop("g")
    torch.cuda.synchronize()
    out = {"z": z.detach(), "dy": gg[0], "dgamma": gg[1], "dbeta": gg[2], "running_mean": bn.running_mean.detach().clone(),
           "running_var": bn.running_var.detach().clone()}
    if rp:
        out["dres_pre"] = gg[3]
    if rq:
        out["dres_post"] = gg[-1]
    assert int(bn.num_batches_tracked) == (1 if training else 0)
    return z, g, out


def _report(capsys, case, config, name, ratio):
    with capsys.disabled():
        print(f"\nbn-chunks | {case.id:15s} | {config:44s} | {name:13s} | err / gate {ratio:.4f} |", end="")


def _gate_fp64(capsys, case, config, out, ref):
    """every quantity against fp64 at the gate of test_bn_act; a failure names the worst chunk"""
    g = B.geometry(case)
    assert set(out) == set(ref), (set(out), set(ref))
    for name in B.NAMES:
        if name not in ref:
            continue
        ratio = B.gate_ratio(out[name], ref[name], B.GATES[name])
        _report(capsys, case, config, name, ratio)
        where = B.worst_chunk(out[name], ref[name], g.plain_len) if ref[name].dim() == 5 else ""
        assert ratio <= 1.0, f"{case.id} {config} {name}: max err / gate = {ratio:.3f}; {where}"
        close(out[name], ref[name], B.GATES[name], name)


def _slot_maxima(ops, case, t, want_slots, what):
    """the valid _dca_cmax tag of the fp32 tensor t: as many slots as the kernel that wrote them has chunks, and their
    maximum is max |t| of every channel bit for bit.  Returns the written slots."""
    tag = ops._tag_ok(t, "_dca_cmax")
    assert tag is not None, f"{case.id} {what}: no valid _dca_cmax"
    slots, nslots, _ = tag
    assert nslots == want_slots, f"{case.id} {what}: tagged with {nslots} slots, its kernel wrote {want_slots}"
    s = slots.view(torch.float32).view(case.C, ops.CSLOTS)[:, :nslots]
    assert bool(torch.isfinite(s).all()) and bool((s >= 0).all()), f"{case.id} {what}: a slot below {nslots} was not written"
    want = t.detach().abs().amax((0, 2, 3, 4))
    bad = (s.amax(1) != want).nonzero().flatten().tolist()
    assert not bad, (f"{case.id} {what}: the slots' maximum is not max |.| in channels {bad[:8]}: "
                     f"{s.amax(1)[bad[:4]].tolist()} against {want[bad[:4]].tolist()}")
    return s.clone()


def _f16_terms_in_range(case, what, tp):
    raw = tp.detach().cpu().view(torch.int16).view(torch.float16)
    assert bool(torch.isfinite(raw).all()), (f"{case.id} {what}: an f16 term overflowed (its exponent missed the channel's "
                                             f"maximum)")
    assert raw.abs().max() < 2.0 ** 15, (case.id, what, raw.abs().max().item())


def _packed_close(capsys, case, config, name, tp, ref32):
    """a packed px2 tensor against the fp32 kernel's result: every raw f16 term finite and below 2^15, the unpacked value
    within 2^-21 of the channel's maximum"""
    g = B.geometry(case)
    tag = getattr(tp, "_dca_px2", None)
    assert tag is not None, f"{case.id} {config} {name}: packed px2 tensor expected"
    _f16_terms_in_range(case, f"{config} {name}", tp)
    back = _unpack_px2(tp, tag[0])
    e = _chan_err(back, ref32)
    _report(capsys, case, config, name + " (px2)", e.max().item() / PACK_GATE)
    assert e.max() <= PACK_GATE, (f"{case.id} {config} {name}: {e.max().item():.3e} of the channel's maximum in channel "
                                  f"{int(e.argmax())} (exponents {tag[0].tolist()}); "
                                  + B.worst_chunk(back, ref32, g.pack_len))


def _exps_are(case, what, tp, bound):
    """the exponents of a packed px2 tensor are x2_scale_exp of its bound (fp64 restatement; channels whose bound lies within
    1e-4 of a power of two are not judged): an exponent above it means a slot that holds the channel's maximum was not
    read, one below it that a slot was read that nobody wrote"""
    want, sure = B.expected_exps(bound)
    got = tp._dca_px2[0].cpu()
    bad = ((got != want) & sure).nonzero().flatten().tolist()
    assert int(sure.sum()) >= case.C // 2, (case.id, what, "too few channels can be judged")
    assert not bad, (f"{case.id} {what}: exponents of channels {bad[:8]} are {got[bad[:8]].tolist()}, the bound gives "
                     f"{want[bad[:8]].tolist()}")


@pytest.mark.parametrize("cid", IDS)
def test_chunk_counts(cid, monkeypatch):
    """the table's chunk counts are the library's (the mirror arithmetic is checked in tests/test_bn_cases_cpu.py)"""
    ops = _setup(monkeypatch)
    case, lib = B.BY_ID[cid], ops._L()
    g = B.geometry(case)
    assert lib.dca_bn_num_chunks(case.C, case.S) == case.plain == g.plain
    assert lib.dca_bn_pack_chunks(case.C, case.S) == g.pack
    if case.pack is not None:
        assert lib.dca_bn_pack_chunks(case.C, case.S) == case.pack
    assert B.BN_MAX_CHUNKS <= ops.CSLOTS
    for r in case.regimes:
        assert B.REGIMES[r](g) is True, (cid, r)


@pytest.mark.parametrize("combo", B.COMBOS, ids=lambda c: f"slope{c[0]}-pre{int(c[1])}-post{int(c[2])}")
@pytest.mark.parametrize("cid", IDS)
def test_fp32_route_training(cid, combo, monkeypatch, capsys):
    """dca_bn_stats / finalize / apply and dca_bn_backward in training, every combination of test_bn_act, against fp64 at
    test_bn_act's gates; the maxima the apply kernels emit for z and dy are exact and tagged with the plain chunk count"""
    ops = _setup(monkeypatch)
    case = B.BY_ID[cid]
    slope, pre, post = combo
    z, g, out = _run(ops, case, True, slope, "rp" if pre else None, "rq" if post else None)
    assert not ops._is_packed(z) and not ops._is_packed(g) and ops._twin_of(z) is None
    _slot_maxima(ops, case, z, case.plain, "z")
    _slot_maxima(ops, case, g, case.plain, "dy")
    assert torch.equal(g, out["dy"])
    ref = B.reference(case, seeded_tensor, True, slope, pre, post)
    _gate_fp64(capsys, case, f"train slope {slope} pre {int(pre)} post {int(post)}", out, ref)


@pytest.mark.parametrize("cid", IDS)
def test_fp32_route_eval(cid, monkeypatch, capsys):
    """eval mode with gradients (running statistics; backward without the batch terms), slope 0.1 with res_pre"""
    ops = _setup(monkeypatch)
    case = B.BY_ID[cid]
    slope, pre, post = B.EVAL_COMBO
    z, g, out = _run(ops, case, False, slope, "rp_eval", None, pack_out=True, pack_dy=True)    # packing is for training only
    assert not ops._is_packed(z) and not ops._is_packed(g) and ops._twin_of(z) is None
    _slot_maxima(ops, case, z, case.plain, "z")
    _slot_maxima(ops, case, g, case.plain, "dy")
    ref = B.reference(case, seeded_tensor, False, slope, pre, post, rp="rp_eval")
    _gate_fp64(capsys, case, "eval slope 0.1 pre 1 post 0", out, ref)


@pytest.mark.parametrize("cid", IDS)
def test_slot_maxima_and_exponents(cid, monkeypatch):
    """dca_cmax_f32 / dca_cmax_exps on untagged tensors whose maxima sit in the first, the last and a high chunk, and the
    tags of an fp32 BatchNorm whose residuals carry the plants: exact maxima over exactly the written slots, exponents equal
    to the x2_scale_exp mirror of those maxima"""
    ops = _setup(monkeypatch)
    case = B.BY_ID[cid]
    d = B.data(case, seeded_tensor)
    for name in ("y", "dz", "rp_big", "rq_big"):
        t = d[name].to(DEV)
        assert ops._tag_ok(t, "_dca_cmax") is None
        _poison(case, ops)
        slots, nslots = ops._slots_of(t)
        assert nslots == case.plain
        s = _slot_maxima(ops, case, t, case.plain, name)
        ex = ops._exps_of(t)
        want = [B.x2_scale_exp(m) for m in s.amax(1).tolist()]
        assert ex.tolist() == want, (cid, name, ex.tolist(), want)
        # the per-chunk slots themselves: slot ch is the maximum over chunk ch
        g = B.geometry(case)
        a = torch.nn.functional.pad(t.abs().reshape(case.N, case.C, -1), (0, g.plain * g.plain_len - g.S))
        assert torch.equal(s, a.view(case.N, case.C, g.plain, g.plain_len).amax(3).amax(0)), (cid, name)
    z, g_, _ = _run(ops, case, True, 0.1, "rp_big", "rq_big")
    _slot_maxima(ops, case, z, case.plain, "z with planted residuals")
    _slot_maxima(ops, case, g_, case.plain, "dy with planted residuals")


# (pack_out, slope, res_pre, res_post): every one with pack_dy=True; with res_pre the gradient stays fp32 (_BnAct)
PACK_CONFIGS = [(True, 0.1, None, None), ("both", 0.0, None, None), ("both", 0.1, None, "rq_big"),
                ("both", 0.0, "rp_big", "rq_big"), (True, 1.0, None, "rq")]


@pytest.mark.parametrize("config", PACK_CONFIGS, ids=lambda c: f"{c[0]}-slope{c[1]}-{c[2]}-{c[3]}")
@pytest.mark.parametrize("cid", PACKABLE)
def test_packed_routes_match_fp32_route(cid, config, monkeypatch, capsys):
    """dca_bn_apply_pack (one and four voxels per lane) and dca_bn_backward_pack against dca_bn_apply / dca_bn_backward on
    the same inputs.  The residual plants sit in chunks the finalize kernel reaches only when it reads every slot the
    residual's producer wrote: a missed slot puts the exponent 2^8 too high and an f16 term overflows."""
    ops = _setup(monkeypatch)
    case = B.BY_ID[cid]
    pack_out, slope, rp, rq = config
    name = f"pack {pack_out} slope {slope} {rp} {rq}"
    z32, g32, o32 = _run(ops, case, True, slope, rp, rq)
    z, g, out = _run(ops, case, True, slope, rp, rq, pack_out=pack_out, pack_dy=True)
    if pack_out == "both":
        assert not ops._is_packed(z)
        assert torch.equal(z.detach().view(torch.int32), z32.detach().view(torch.int32)), \
            f"{cid} {name}: the fp32 copy is not the fp32 kernel's z"
        _slot_maxima(ops, case, z, case.pack, "fp32 copy of z")
        tw = ops._twin_of(z)
        assert tw is not None and ops._is_packed(tw)
        _packed_close(capsys, case, name, "z twin", tw, z32)
    else:
        assert ops._is_packed(z) and not hasattr(z, "_dca_cmax")
        _packed_close(capsys, case, name, "z", z, z32)
    _exps_are(case, name + " z", z if pack_out is True else ops._twin_of(z), B.z_bound(case, seeded_tensor, rp, rq))
    if rp is None:
        _packed_close(capsys, case, name, "dy", g, o32["dy"])
        _exps_are(case, name + " dy", g, B.dy_bound(case, seeded_tensor, slope))
    else:
        assert not ops._is_packed(g)
        assert torch.equal(g, o32["dy"])
        _slot_maxima(ops, case, g, case.plain, "dy")
    for k in ("dgamma", "dbeta", "dres_pre", "dres_post", "running_mean", "running_var"):
        if k in o32:
            assert torch.equal(out[k], o32[k]), f"{cid} {name}: {k} differs from the fp32 route's"


@pytest.mark.parametrize("pack_out", [True, "both"], ids=["packed-only", "fp32+twin"])
@pytest.mark.parametrize("cid", PACKABLE)
def test_packed_gradient_exponent_follows_max_xhat(cid, pack_out, monkeypatch, capsys):
    """dca_bn_backward_pack bounds |dy| with max |xhat| from the max |y - mean| slots the FORWARD apply kernel wrote -- as
    many as that kernel has chunks, a count _BnAct carries from forward to backward.  With the row's dz that term is 1e-3
    of the bound; with dz_corr it is two thirds, and the y plants in the last and the high chunk decide the exponent
    (tests/test_bn_cases_cpu.py::test_exponent_bounds_depend_on_the_planted_slots)."""
    ops = _setup(monkeypatch)
    case = B.BY_ID[cid]
    name = f"pack {pack_out} slope 1.0 dz_corr"
    _, _, o32 = _run(ops, case, True, 1.0, dz="dz_corr")
    z, g, out = _run(ops, case, True, 1.0, pack_out=pack_out, pack_dy=True, dz="dz_corr")
    _packed_close(capsys, case, name, "dy", g, o32["dy"])
    _exps_are(case, name + " dy", g, B.dy_bound(case, seeded_tensor, 1.0, "dz_corr"))
    for k in ("dgamma", "dbeta"):
        assert torch.equal(out[k], o32[k]), f"{cid} {name}: {k} differs from the fp32 route's"
    ref = B.reference(case, seeded_tensor, True, 1.0, False, False, dz="dz_corr")
    for k in ("dy", "dgamma", "dbeta"):
        ratio = B.gate_ratio(o32[k], ref[k], B.GATES[k])
        _report(capsys, case, "train slope 1.0 dz_corr", k, ratio)
        assert ratio <= 1.0, (cid, k, ratio)


@pytest.mark.parametrize("cid", PACKABLE)
def test_residual_written_by_a_packed_batchnorm(cid, monkeypatch, capsys):
    """a residual whose per-channel maxima sit in the slots of the PACK chunking: the fp32 copy of a pack_out="both"
    BatchNorm (the block input that is also the block's skip, as in the network).  Its tag says how many slots were
    written; dca_cmax_exps and the bound of the next BatchNorm's packed result (bn_bound_exp) must read exactly those."""
    ops = _setup(monkeypatch)
    case = B.BY_ID[cid]
    d = B.data(case, seeded_tensor)
    _poison(case, ops)
    skip = ops.bn_act(d["y"].to(DEV).requires_grad_(), _module(case, d, True), 1.0, None, d["rq_big"].to(DEV), pack_out="both")
    smax = _slot_maxima(ops, case, skip, case.pack, "skip").amax(1)
    assert ops._exps_of(skip).tolist() == [B.x2_scale_exp(m) for m in smax.tolist()]
    for p in B.plants(case, "rq"):      # the maxima are the residual plants, in the chunks they claim
        assert skip.detach()[p.n, p.c].view(-1)[p.voxel].abs() == smax[p.c], (cid, p)
    bound = B.z_bound(case, seeded_tensor) + smax.cpu().double() * 1.0001
    for pack_out, slope, as_pre in ((True, 0.1, False), ("both", 0.0, True), ("both", 1.0, False)):
        name = f"pack {pack_out} slope {slope} skip as {'res_pre' if as_pre else 'res_post'}"
        res = {}
        for pack in (False, pack_out):
            _poison(case, ops)
            res[pack] = ops.bn_act(d["y"].to(DEV).requires_grad_(), _module(case, d, True), slope, skip if as_pre else None,
                                   None if as_pre else skip, pack_out=pack)
        z32, z = res[False], res[pack_out]
        tp = z if pack_out is True else ops._twin_of(z)
        assert tp is not None
        _packed_close(capsys, case, name, "z", tp, z32)
        _exps_are(case, name, tp, bound)
        if pack_out == "both":
            assert torch.equal(z.detach().view(torch.int32), z32.detach().view(torch.int32))
            _slot_maxima(ops, case, z, case.pack, "z")


@pytest.mark.parametrize("cid", PACKABLE)
def test_pack_x2_roundtrip(cid, monkeypatch):
    """ops.pack_x2 (the identity form of dca_bn_apply_pack, exponents from dca_cmax_f32 / dca_cmax_exps): unpacking gives the
    tensor back to 2^-22 of each element plus 2^-39 of the channel's maximum, the bound of
    test_px2_pack_roundtrip_and_packed_operands_are_bitwise"""
    ops = _setup(monkeypatch)
    case = B.BY_ID[cid]
    d = B.data(case, seeded_tensor)
    for name in ("y", "dz"):
        x = d[name].to(DEV)
        _poison(case, ops)
        xp = ops.pack_x2(x)
        _f16_terms_in_range(case, "pack_x2 " + name, xp)
        ex = xp._dca_px2[0]
        assert ex.tolist() == [B.x2_scale_exp(m) for m in x.abs().amax((0, 2, 3, 4)).tolist()]
        back, xd = _unpack_px2(xp, ex), d[name].double()
        bound = xd.abs().amax((0, 2, 3, 4)).view(1, case.C, 1, 1, 1)
        ok = (back - xd).abs() <= 2.0 ** -22 * xd.abs() + 2.0 ** -39 * bound
        assert bool(ok.all()), f"{cid} pack_x2 {name}: " + B.worst_chunk(back, xd, B.geometry(case).pack_len)


def _bits_of(ops, case, z, g, out):
    """everything a run leaves behind, as comparable bits: outputs, gradients, exponents, the written slots"""
    items = {k: v.view(torch.int32) if v.dtype == torch.float32 else v for k, v in out.items()}
    for name, t in (("z", z), ("g", g), ("twin", ops._twin_of(z))):
        if t is None:
            continue
        items[name + ".bits"] = t.detach().view(torch.int32)
        if ops._is_packed(t):
            items[name + ".exps"] = t._dca_px2[0]
        tag = ops._tag_ok(t, "_dca_cmax")
        if tag is not None:
            items[name + ".slots"] = tag[0].view(case.C, ops.CSLOTS)[:, :tag[1]]
    return items


@pytest.mark.parametrize("cid", IDS)
def test_two_identical_calls_give_identical_bits(cid, monkeypatch):
    ops = _setup(monkeypatch)
    case = B.BY_ID[cid]
    configs = [dict(slope=0.1, rp="rp", rq="rq")]
    if case.pack is not None:
        configs += [dict(slope=0.1, rq="rq_big", pack_out="both", pack_dy=True), dict(slope=0.0, pack_out=True, pack_dy=True)]
    for kw in configs:
        a, b = (_bits_of(ops, case, *_run(ops, case, True, **kw)) for _ in range(2))
        assert set(a) == set(b)
        for k in a:
            assert torch.equal(a[k], b[k]), f"{cid} {kw}: {k} is not bitwise reproducible"


def test_unpackable_channels_fall_back_to_fp32(monkeypatch):
    """row c12 (C % 8 != 0): pack_out / pack_dy leave the fp32 kernels' result, bit for bit, and say so by their tags"""
    ops = _setup(monkeypatch)
    case = B.BY_ID["c12"]
    z32, g32, o32 = _run(ops, case, True, 0.1, None, "rq")
    for pack_out in (True, "both"):
        z, g, out = _run(ops, case, True, 0.1, None, "rq", pack_out=pack_out, pack_dy=True)
        for t in (z, g):
            assert getattr(t, "_dca_px2", None) is None and not ops._is_packed(t)
        assert ops._twin_of(z) is None
        _slot_maxima(ops, case, z, case.plain, "z")
        _slot_maxima(ops, case, g, case.plain, "dy")
        assert set(out) == set(o32)
        for k in out:
            assert torch.equal(out[k], o32[k]), k
