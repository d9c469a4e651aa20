"""GPU checks of the evaluation step (csrc/eval_metrics.hip, dcanet_amd.evaluation):
  1. the three kernels against tests/golden/eval_step.npz -- results of the REFERENCE's own `mytest` /
     `SegmentationMetric` on the CPU (tools/make_eval_golden.py); inputs re-made from the recorded seeds;
  2. against an fp64 torch restatement on the same GPU tensors over shapes, pads, class counts, masks;
  3. accumulation over batches, `result()`, `reset()`;  4. bitwise reproducibility;
  5. the whole boundary (`EvalStep.step`, `mytest`) at a small shape, fp32 and fp16;
  6. hipGraph: `EvalStep(graph=True)` and a direct capture of the three kernels.

Tolerances: counts and confusion matrices are integers and must be EQUAL.  Sums: ours are fp64 sums of fp32 terms; the
fixture's loss / epe are fp32 cascade sums of ~1e6 terms (error up to ~log2(n) 2^-24 = 1.2e-6) -> 5e-6 relative; the
fp64 restatement differs by three fp32 roundings per term (3 x 2^-24) -> 1e-6 relative.  Labels: a cell whose fp64 pooled
value lies within 1e-4 of an integer may floor either way in fp32; such cells are matched against both candidates, and
there may be at most 0.5 % of them."""
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import dcanet_oracle as O
from oracle.seeded import seeded_tensor

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_spec = importlib.util.spec_from_file_location("make_eval_golden", os.path.join(ROOT, "tools", "make_eval_golden.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)


def dev_batch(seed, B, H, W, C=24, invalid=False):
    gt, pred, vols = G.synthetic_batch(seed, B, H, W, C, 8 * C, invalid)
    return torch.from_numpy(gt).to(DEV), torch.from_numpy(pred).to(DEV), [torch.from_numpy(v).to(DEV) for v in vols]


def rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


# ---- fp64 restatement on the device ---------------------------------------------------------------------------------------
def restate_records(pred, gt, maxdisp, mask=None):
    """(B,8) float64.  Counts use e = |pred - gt| in fp32 (what torch, and so the reference, evaluates); the two sums
    are computed entirely in fp64."""
    B, H, W = gt.shape
    p = pred.reshape(B, pred.shape[-2], pred.shape[-1])[:, pred.shape[-2] - H:, :W]
    m = ((gt > 0) & (gt < maxdisp)) if mask is None else mask
    e32 = (p - gt).abs()
    e64 = (p.double() - gt.double()).abs()
    sl1 = torch.where(e64 < 1, 0.5 * e64 * e64, e64 - 0.5)
    d1 = (e32 > 3) & (e32 / gt.abs() > 0.05)
    cols = [m, gt > 0, e64 * m, sl1 * m, (e32 > 1) & m, (e32 > 2) & m, (e32 > 3) & m, d1 & m]
    return torch.stack([c.double().sum(dim=(1, 2)) for c in cols], dim=1).cpu().numpy()


def check_confusion(cm, vols, gt):
    """cm (nvol,C,C) from the kernel == the matrices of the fp64 labels, cells near an integer matched either way"""
    B, H, W = gt.shape
    C, hp = vols[0].shape[1], vols[0].shape[2]
    h, w = H // 8, W // 8
    pooled = F.adaptive_avg_pool2d(gt.double() / 8, (h, w))
    near = (pooled - pooled.round()).abs() < 1e-4
    assert near.sum().item() <= 0.005 * near.numel(), f"{near.sum().item()} of {near.numel()} cells are ambiguous"
    lab = pooled.floor().long()
    cm = cm.cpu().numpy()
    for k, v in enumerate(vols):
        arg = v.argmax(1)[:, hp - h:, :w]
        ok = ~near & (lab >= 0) & (lab < C)
        want = torch.bincount(C * lab[ok] + arg[ok], minlength=C * C).reshape(C, C).cpu().numpy()
        rest = cm[k] - want
        for n, a in zip(pooled[near].round().long().tolist(), arg[near].tolist()):
            cand = [c for c in (n - 1, n)]
            hit = [c for c in cand if 0 <= c < C and rest[c, a] > 0]
            if hit:
                rest[hit[0], a] -= 1
            else:
                assert any(not 0 <= c < C for c in cand), f"head {k}: an ambiguous cell is missing from the matrix"
        assert (rest == 0).all(), f"head {k}: {np.abs(rest).sum()} counts differ from the fp64 restatement"
    return int(near.sum().item())


def host_accumulate(state, rec, cm, npix):
    """numpy restatement of dca_eval_accumulate (state layout: include/dca_hip.h)"""
    from dcanet_amd import evaluation as E
    vals = E.batch_values(rec, cm)
    state[E.BATCHES] += 1
    for i, k in enumerate(E.KEYS):
        state[E.SUMS + i] += vals[k]
    for r in rec:
        state[E.IMG_SEEN] += 1
        if r[0] > 0 and not (np.float32(r[0]) / np.float32(npix)) / (np.float32(r[1]) / np.float32(npix)) < np.float32(0.1):
            state[E.IMG_KEPT] += 1
            state[E.IMG_EPE] += r[2] / r[0]
            state[E.IMG_D1] += r[7] / r[0]
            state[E.IMG_THRES:E.IMG_THRES + 3] += r[4:7] / r[0]
    state[E.PIXELS] += rec[:, 0].sum()
    state[E.STATE_HEAD:] += np.asarray(cm, dtype=np.float64).reshape(-1)
    return state


def assert_state_close(got, want, tol=1e-12):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    err = np.abs(got - want) / np.maximum(np.abs(want), 1e-300)
    err[want == got] = 0
    assert err.max() <= tol, f"state entry {int(err.argmax())}: {got[err.argmax()]!r} vs {want[err.argmax()]!r}"


# ---- 1. the fixture ----------------------------------------------------------------------------------------------------------
def test_kernels_match_reference_fixture(golden):
    from dcanet_amd import ops
    from dcanet_amd import evaluation as E
    fx = golden("eval_step")
    maxdisp = int(fx["maxdisp"])
    for i, (seed, B, H, W, inv) in enumerate(fx["cases"].tolist()):
        gt, pred, vols = dev_batch(seed, B, H, W, 24, bool(inv))
        rec = ops.disp_metrics(pred, gt, maxdisp)
        cm = ops.region_confusion(vols, gt)
        state = ops.eval_accumulate(ops.eval_state(24, DEV), rec, cm, gt.shape)
        rec, cm, state = rec.cpu().numpy(), cm.cpu().numpy(), state.cpu().numpy()
        want_rec, want_vals = fx[f"records{i}"], fx[f"values{i}"]
        print(f"case {i}: values {state[E.SUMS:E.SUMS + 10]} want {want_vals}")
        assert (rec[:, [0, 1, 4, 5, 6, 7]] == want_rec[:, [0, 1, 4, 5, 6, 7]]).all(), (rec, want_rec)
        assert all(rel(a, b) <= 1e-9 for a, b in zip(rec[:, 2:4].ravel(), want_rec[:, 2:4].ravel()) if b)
        if inv:
            assert (cm == 0).all()                                # every label is negative: nothing is scored
            assert (state[E.SUMS:E.SUMS + 10] == 0).all() and state[E.BATCHES] == 1     # the empty-mask rule
            continue
        assert (cm == fx[f"confusion{i}"]).all(), np.abs(cm - fx[f"confusion{i}"]).sum(axis=(1, 2))
        got = state[E.SUMS:E.SUMS + 10]
        for j, k in enumerate(E.KEYS):
            tol = 5e-6 if k in ("loss", "epe") else 1e-6
            assert rel(got[j], want_vals[j]) <= tol, f"{k}: {got[j]!r} vs reference {want_vals[j]!r}"
        assert (state[E.STATE_HEAD:].reshape(3, 24, 24) == fx[f"confusion{i}"]).all()


# ---- 2. fp64 restatement over shapes --------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,C,variant", [
    (1, 250, 470, 24, "plain"), (3, 250, 470, 8, "mask"), (3, 256, 512, 48, "one_empty"), (1, 256, 512, 24, "plain"),
    (3, 250, 470, 48, "one_empty"), (1, 540, 960, 24, "mask")])
def test_kernels_match_fp64_restatement(B, H, W, C, variant):
    from dcanet_amd import ops
    from dcanet_amd import evaluation as E
    gt, pred, vols = dev_batch(100 + H + C + B, B, H, W, C)
    maxdisp, mask = 8 * C, None
    if variant == "mask":
        mask = (gt > 0.25 * maxdisp) & (torch.from_numpy(np.random.RandomState(5).rand(B, H, W) < 0.7).to(DEV))
    if variant == "one_empty":
        gt[1] = -gt[1].abs() - 1.0
    assert gt.min().item() < 0 and gt.max().item() > maxdisp, "degenerate test data"
    rec = ops.disp_metrics(pred, gt, maxdisp, mask)
    want = restate_records(pred, gt, maxdisp, mask)
    got = rec.cpu().numpy()
    print(f"records {got} want {want}")
    assert (got[:, [0, 1, 4, 5, 6, 7]] == want[:, [0, 1, 4, 5, 6, 7]]).all(), (got, want)
    for a, b in zip(got[:, 2:4].ravel(), want[:, 2:4].ravel()):
        assert a == b or rel(a, b) <= 1e-6, (a, b)
    if variant == "one_empty":
        assert got[1, 0] == 0 and got[0, 0] > 0
    for nvol in (3, 1):
        cm = ops.region_confusion(vols[:nvol], gt)
        assert cm.shape == (nvol, C, C) and cm.dtype == torch.int64
        check_confusion(cm, vols[:nvol], gt)
    assert (cm.sum() > 0) and cm.diagonal(dim1=1, dim2=2).sum() < cm.sum(), "degenerate test data"
    cm3 = ops.region_confusion(vols, gt)
    state = ops.eval_accumulate(ops.eval_state(C, DEV), rec, cm3, gt.shape).cpu().numpy()
    assert_state_close(state, host_accumulate(np.zeros_like(state), got, cm3.cpu().numpy(), H * W))
    assert state[E.IMG_SEEN] == B and state[E.IMG_KEPT] == B - (variant == "one_empty")


# ---- 3. / 4. accumulation, result, reset, reproducibility ----------------------------------------------------------------------
def test_accumulation_result_reset_and_reproducibility():
    from dcanet_amd import ops
    from dcanet_amd import evaluation as E
    C, H, W = 24, 250, 470
    batches = [dev_batch(7, 2, H, W, C), dev_batch(8, 2, H, W, C, invalid=True), dev_batch(9, 2, H, W, C)]

    def run():
        state, singles = ops.eval_state(C, DEV), []
        for gt, pred, vols in batches:
            rec, cm = ops.disp_metrics(pred, gt, 8 * C), ops.region_confusion(vols, gt)
            ops.eval_accumulate(state, rec, cm, gt.shape)
            singles.append(ops.eval_accumulate(ops.eval_state(C, DEV), rec, cm, gt.shape))
        return state, singles

    state, singles = run()
    state2, _ = run()
    assert torch.equal(state, state2), "two runs over the same batches differ bitwise"
    total = np.zeros(state.numel())
    for s in singles:
        total += s.cpu().numpy()
    assert_state_close(state.cpu().numpy(), total)
    res = E.state_result(state.cpu().numpy())
    per_batch = [s.cpu().numpy()[E.SUMS:E.SUMS + 10] for s in singles]
    assert (per_batch[1] == 0).all(), "an empty mask makes all ten values 0"
    for i, k in enumerate(E.KEYS):                      # what the reference loop prints: sum of the batch values / #batches
        assert rel(res[k], sum(p[i] for p in per_batch) / 3) <= 1e-12, k
    assert res["batches"] == 3 and res["images"] == 6 and res["images_kept"] == 4
    assert 0 < res["head_mIoU"][2] < res["head_mIoU"][0] < 1 and 0 < res["image_d1"] < res["image_thres3"] < 1
    # the quirk: head 1 is scored on CM0 + CM1; the per-head matrices of the state are NOT accumulated
    cms = singles[0].cpu().numpy()[E.STATE_HEAD:].reshape(3, C, C)
    m = E.SegmentationMetric(C)
    m.addMatrix(cms[0] + cms[1])
    assert rel(per_batch[0][5], m.meanPixelAccuracy()) <= 1e-12
    state.zero_()
    assert state.abs().sum().item() == 0


# ---- 5. the whole boundary --------------------------------------------------------------------------------------------------
@pytest.fixture
def deterministic_2d():
    """The 2D networks are PyTorch-ROCm (MIOpen) convolutions; by default MIOpen may pick solvers whose results differ
    in the last bits from call to call (seen here in the extractor's 128-channel layers at batch 2), which would hide what
    the tests compare: the step against the same pipeline by hand, eager against replayed HIP launches."""
    old = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = old


def seeded_model(maxdisp=64):
    from dcanet_amd.models.gwcnet_dca_g import GwcNet
    m = GwcNet(maxdisp, use_concat_volume=False)
    m.load_state_dict(O.seeded_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}), strict=True)
    return m.to(DEV).eval()


def frames(tag, B=2, H=60, W=120, maxdisp=64, seed=3):
    gt = torch.from_numpy(G.synthetic_batch(seed, B, H, W, maxdisp // 8, maxdisp)[0]).to(DEV)
    return seeded_tensor(tag + ".L", (B, 3, H, W)).to(DEV), seeded_tensor(tag + ".R", (B, 3, H, W)).to(DEV), gt


@pytest.mark.parametrize("dtype", [None, torch.float16])
def test_eval_step_and_mytest_equal_host_restatement(dtype, deterministic_2d):
    import contextlib
    from dcanet_amd import ops
    from dcanet_amd import evaluation as E
    m = seeded_model()
    L, R, gt = frames("eval")
    with torch.no_grad():
        keys = set(m.hot_path(*[m.feature_extraction(x)["gwc_segments"] for x in E.pad16(L, R)[:2]]))
    assert keys == {"pred4_q", "prob_volume2"}, "hot_path() without the keyword must return what it returned before"
    ev = E.EvalStep(torch.nn.DataParallel(m, device_ids=[0]), maxdisp=64, dtype=dtype)
    ev.step(L, R, gt)
    # the same pipeline by hand
    Lp, Rp, top, right = E.pad16(L, R)
    assert (top, right) == (4, 8) and ev.last["top_pad"] == 4 and ev.last["right_pad"] == 8
    with torch.no_grad():
        fl, fr = m.feature_extraction(Lp)["gwc_segments"], m.feature_extraction(Rp)["gwc_segments"]
        with ops.reduced_precision(dtype) if dtype is not None else contextlib.nullcontext():
            r = m.hot_path(fl, fr, aux_volumes=True)
        pred = m.prop(m.guidance(Lp)["g"], r["pred4_q"])
    vols = [r[f"prob_volume{k}"].squeeze(1) for k in (1, 2, 3)]
    assert all(v.dtype == torch.float32 and v.shape == (2, 8, 8, 16) for v in vols)
    assert torch.equal(pred, ev.last["pred"]) and all(torch.equal(a.squeeze(1), b) for a, b in zip(ev.last["volumes"], vols))
    want_rec = restate_records(pred, gt, 64)
    got_rec = ev.last["rec"].cpu().numpy()
    assert (got_rec[:, [0, 1, 4, 5, 6, 7]] == want_rec[:, [0, 1, 4, 5, 6, 7]]).all(), (got_rec, want_rec)
    assert all(rel(a, b) <= 1e-6 for a, b in zip(got_rec[:, 2:4].ravel(), want_rec[:, 2:4].ravel()))
    check_confusion(ev.last["cm"], vols, gt)
    state = ev.state.cpu().numpy()
    assert_state_close(state, host_accumulate(np.zeros_like(state), got_rec, ev.last["cm"].cpu().numpy(), 60 * 120))
    res = ev.result()
    if dtype is None:
        loss, metrics, mpa, miou = E.mytest(m, L.cpu(), R.cpu(), gt.cpu(), maxdisp=64)
        assert torch.is_tensor(loss) and loss.dim() == 0 and loss.is_cuda and loss.dtype == torch.float32
        assert rel(loss.item(), res["loss"]) <= 1e-6
        assert set(metrics) == {"epe", "1px", "3px"} and all(isinstance(v, float) for v in metrics.values())
        assert all(metrics[k] == res[k] for k in metrics)
        assert all(mpa[k] == res[k] for k in ("mpa0", "mpa1", "mpa2")) and isinstance(mpa["mpa0"], np.floating)
        assert all(miou[k] == res[k] for k in ("mIoU0", "mIoU1", "mIoU2"))
        empty = E.mytest(m, L, R, -gt.abs() - 1, maxdisp=64)
        assert empty == (0, {"epe": 0, "1px": 0, "3px": 0}, {"mpa0": 0, "mpa1": 0, "mpa2": 0},
                         {"mIoU0": 0, "mIoU1": 0, "mIoU2": 0})
    ev.reset()
    assert ev.result()["batches"] == 0


# ---- 6. hipGraph ---------------------------------------------------------------------------------------------------------------
def test_eval_step_graph_replay_equals_eager(deterministic_2d):
    from dcanet_amd import evaluation as E
    m = seeded_model()
    eager, graphed = E.EvalStep(m, maxdisp=64), E.EvalStep(m, maxdisp=64, graph=True)
    for i in range(3):
        L, R, gt = frames(f"graph{i}", seed=20 + i)
        eager.step(L, R, gt)
        graphed.step(L, R, gt)
    assert len(graphed._graphed) == 1, "one graph per (frame shape, ground-truth shape)"
    assert eager.result()["batches"] == 3 and eager.result()["pixels"] > 0
    assert torch.equal(eager.state, graphed.state), (eager.state[:20], graphed.state[:20])


def test_metric_kernels_capture_into_one_graph():
    """capture fails if a launcher synchronises or allocates outside torch's allocator"""
    from dcanet_amd import ops
    C = 24
    gt, pred, vols = dev_batch(11, 2, 250, 470, C)
    gt2, pred2, vols2 = dev_batch(12, 2, 250, 470, C)

    def tail(state):
        return ops.eval_accumulate(state, ops.disp_metrics(pred, gt, 8 * C), ops.region_confusion(vols, gt), gt.shape)

    want = tail(ops.eval_state(C, DEV)).clone()
    for a, b in zip([gt, pred] + vols, [gt2, pred2] + vols2):         # other contents while capturing
        a_saved = a.clone()
        a.copy_(b)
        b.copy_(a_saved)
    state = ops.eval_state(C, DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        tail(state)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        tail(state)
    for a, b in zip([gt, pred] + vols, [gt2, pred2] + vols2):         # the first batch back into the static tensors
        a.copy_(b)
    state.zero_()
    graph.replay()
    assert torch.equal(state, want), "replayed state differs from the eager one"
    graph.replay()
    assert torch.equal(state[1:11], 2 * want[1:11]) and state[0].item() == 2
