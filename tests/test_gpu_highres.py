"""High-resolution pairs on the MI355X (csrc/highres.hip): the two area downscales and the guided upsampler bit for bit against
the numpy restatements of dcanet_amd/highres.py, under hipGraph replay, through inference.HighResInference and
training.TrainInput(downscale=), and the refusals of the three wrappers.

Why bitwise, without any tolerance: the uint8 downscale is integer arithmetic; the float32 one is a sum in a fixed order and
two IEEE divisions; the upsampler multiplies and adds in float32 in the order the header fixes, one operation at a time (the
file is compiled without contraction into fused multiply-adds), looks both weights up in tables the host made, and divides
once -- numpy's float32 arithmetic is the same IEEE arithmetic."""
import numpy as np
import pytest
import torch

from _inference_cases import model as _model
from dcanet_amd.highres import (area_downscale_disp_host, area_downscale_pair_host, device_tables, guided_upsample_host,
                                jbu_tables)

pytestmark = pytest.mark.gpu
DEV = "cuda"


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)         # (a copy: the cases are read-only)


def same_bits(got, want, name):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
    bits = np.uint32 if got.dtype == np.float32 else got.dtype
    bad = np.nonzero(got.view(bits) != want.view(bits))
    assert len(bad[0]) == 0, f"{name}: {len(bad[0])} elements differ, first at {[int(i[0]) for i in bad]}: " \
                             f"{got[bad][0]} != {want[bad][0]}"


# ---- the downscales ---------------------------------------------------------------------------------------------------------
def _pair(shape, C, seed):
    """random bytes with an all-255 corner and blocks of [0,1,0,1] / [1,0,1,0]-like rounding ties"""
    rng = np.random.default_rng(seed)
    a, b = (rng.integers(0, 256, shape + (C,), dtype=np.uint8) for _ in range(2))
    a[:4, :4] = 255
    b[-4:, -5:] = 255
    a[:, 4:10] = (np.arange(6) % 2).astype(np.uint8)[None, :, None] * 3 + 7          # sums that are odd multiples of cnt / 2
    b[4:, 0:4] = (np.arange(shape[0] - 4) % 2).astype(np.uint8)[:, None, None]
    return a, b


@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("shape", [(7, 13), (37, 131)])
@pytest.mark.parametrize("s", [2, 3, 4])
def test_area_downscale_pair_is_the_restatement_bit_for_bit(s, shape, C):
    from dcanet_amd import ops
    a, b = _pair(shape, C, 100 * s + C)
    want = area_downscale_pair_host(a, b, s)
    same_bits(ops.area_downscale_pair(dev(a), dev(b), s), want, f"pair s={s} {shape} C={C}")
    out = torch.full(want.shape, 77, device=DEV, dtype=torch.uint8)
    assert ops.area_downscale_pair(dev(a), dev(b), s, out=out) is out
    same_bits(out, want, "out=")


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("shape", [(7, 13), (37, 131)])
@pytest.mark.parametrize("s", [2, 3, 4])
def test_area_downscale_disp_is_the_restatement_bit_for_bit(s, shape, flip):
    from dcanet_amd import ops
    rng = np.random.default_rng(10 * s + flip)
    d = rng.uniform(0, 300, shape).astype(np.float32)
    d[rng.uniform(size=shape) < 0.1] = 0
    d[1, 2], d[3, 5], d[-1, -1], d[2, -1], d[5, 0] = np.inf, np.nan, np.inf, -0.0, -np.inf
    for inf in (True, False):
        want = area_downscale_disp_host(d, s, inf, flip)
        assert np.isfinite(want).all() == inf
        same_bits(ops.area_downscale_disp(dev(d), s, inf, flip), want, f"disp s={s} {shape} inf={inf} flip={flip}")
    want = area_downscale_disp_host(d, s, True, flip)
    out = torch.full(want.shape, 7.0, device=DEV)
    assert ops.area_downscale_disp(dev(d), s, flip_rows=flip, out=out) is out
    same_bits(out, want, "out=")


# ---- the upsampler ----------------------------------------------------------------------------------------------------------
class Up:
    """One case: a (Hc,Wc) frame whose window (y0, rows, cols) is the image; everything outside it is poison.  Inside, a
    rectangle of 2r + 3 pixels each way holds no tap at all (NaN, inf, 0, negative values), so the output pixels over its
    centre are invalid; with `masked`, a second such rectangle is cut out by the mask.  The full-resolution guide is the
    low-resolution one repeated, plus noise, so that colour differences spread over the table."""

    def __init__(self, name, s, r, frame, window, H, W, C=3, masked=False, seed=0):
        self.name, self.s, self.r, self.window, self.C = name, s, r, window, C
        rng = np.random.default_rng(seed)
        y0, rows, cols = window
        assert -(-H // s) == rows and -(-W // s) == cols
        d = np.full(frame, 1e9, np.float32)                              # poison: a finite, positive value
        d[:y0] = rng.choice(np.array([1e9, np.inf, 5e8], np.float32), (y0, frame[1]))
        win = (rng.uniform(1, 60, (rows, cols)) + np.linspace(0, 20, cols)[None, :]).astype(np.float32)
        k = 2 * r + 3
        c0 = 8 if cols >= 8 + k else 0
        hole = win[5:5 + k, c0:c0 + k]
        hole[...] = rng.choice(np.array([np.nan, np.inf, 0.0, -3.0, -0.0, -np.inf], np.float32), hole.shape)
        win[rng.uniform(size=win.shape) < 0.03] = np.nan
        d[y0:y0 + rows, :cols] = win
        self.disp = d
        self.mask = None
        if masked:
            m = rng.uniform(0.5, 1, frame).astype(np.float32)
            m[y0 + rows - k - 1:y0 + rows - 1, 1:1 + k] = rng.uniform(0, 0.49, (k, min(k, frame[1] - 1))).astype(np.float32)
            m[rng.uniform(size=frame) < 0.05] = 0.25
            self.mask = m
        self.guide_lo = rng.integers(0, 256, (rows, cols, C), dtype=np.uint8)
        hi = np.repeat(np.repeat(self.guide_lo, s, 0), s, 1)[:H, :W].astype(np.int64)
        hi += rng.integers(-20, 21, hi.shape) * (rng.uniform(size=hi.shape[:2]) < 0.7)[..., None]
        self.guide_hi = np.clip(hi, 0, 255).astype(np.uint8)
        self.tables = jbu_tables(s, r)
        for a in (self.disp, self.mask, self.guide_lo, self.guide_hi) + self.tables:
            if a is not None:
                a.setflags(write=False)
        self._ref = None

    def ref(self):
        """the restatement, computed once for the module and never modified"""
        if self._ref is None:
            self._ref = guided_upsample_host(self.disp, self.guide_lo, self.guide_hi, self.s, self.tables, self.window,
                                             self.mask, 0.5, counts=True)
            for a in self._ref.values():
                a.setflags(write=False)
        return self._ref

    def run(self, ops, **kw):
        return ops.guided_upsample(dev(self.disp), dev(self.guide_lo), dev(self.guide_hi), self.s,
                                   device_tables(self.tables, DEV), self.window, dev(self.mask), 0.5, **kw)


def _up_cases():
    cases = []
    for s in (2, 3, 4):
        for r in (1, 2, 3):
            # the last blocks are partial in both directions; three tiles down and two or three across, the last ones ragged
            cases.append(Up(f"s{s}_r{r}", s, r, (24, 48), (3, 21, 37), 21 * s - 1, 37 * s - (s - 1), masked=(s + r) % 2 == 0,
                            C=4 if (s, r) == (3, 2) else 3, seed=10 * s + r))
        # a window narrower than the halo
        cases.append(Up(f"s{s}_r3_narrow", s, 3, (14, 8), (1, 12, 2), 12 * s - (s - 1), 2 * s, masked=s == 3, seed=40 + s))
        # rows that start on 16 bytes: the wide loads and stores
        cases.append(Up(f"s{s}_r2_aligned", s, 2, (21, 40), (0, 21, 40), 21 * s, 40 * s, C=3 + s % 2, masked=s == 4, seed=50 + s))
    return cases


UP_CASES = _up_cases()


@pytest.mark.parametrize("case", UP_CASES, ids=lambda c: c.name)
def test_guided_upsample_is_the_restatement_bit_for_bit(case):
    from dcanet_amd import ops
    ref = case.ref()
    full = (2 * case.r + 1) ** 2
    n = ref["valid"].size
    print(f"{case.name}: {ref['valid'].shape} valid {int(ref['valid'].sum())} of {n}, "
          f"valid with fewer than {full} taps {int(((ref['taps'] < full) & (ref['valid'] == 1)).sum())}")
    # the inputs make the comparison mean something
    assert ref["valid"].sum() >= n / 2 and (ref["valid"] == 0).any()
    assert ((ref["taps"] < full) & (ref["valid"] == 1)).any()
    assert (ref["disp"][ref["valid"] == 0] == 0).all() and float(ref["disp"].max()) <= 80 * case.s
    got = case.run(ops)
    assert set(got) == {"disp", "valid"}
    same_bits(got["valid"], ref["valid"], f"{case.name} valid")
    same_bits(got["disp"], ref["disp"], f"{case.name} disp")
    again = case.run(ops)
    assert torch.equal(again["valid"], got["valid"]) and torch.equal(again["disp"].view(torch.int32), got["disp"].view(torch.int32))


def test_guided_upsample_outputs_valid_only_writes_only_that():
    from dcanet_amd import ops
    case = UP_CASES[1]
    ref = case.ref()
    disp = torch.full(ref["disp"].shape, 123.0, device=DEV)
    valid = torch.full(ref["disp"].shape, 9.0, device=DEV)
    got = case.run(ops, outputs=("valid",), out={"disp": disp, "valid": valid})
    assert set(got) == {"valid"} and got["valid"] is valid
    same_bits(valid, ref["valid"], "valid only")
    assert (disp == 123.0).all()
    part = case.run(ops, outputs=("disp",))
    assert set(part) == {"disp"}
    same_bits(part["disp"], ref["disp"], "disp only")
    four = ops.guided_upsample(dev(case.disp)[None, None], dev(case.guide_lo), dev(case.guide_hi), case.s,
                               device_tables(case.tables, DEV), case.window, dev(case.mask)[None, None] if case.mask is not None
                               else None)
    same_bits(four["disp"], ref["disp"], "(1,1,Hc,Wc) in")


def test_highres_ops_under_graph_replay():
    """with `out=` nothing is allocated: the three launches are captured and replayed on a second input"""
    from dcanet_amd import ops
    s, r = 2, 2
    H, W, y0 = 41, 73, 3
    rows, cols = 21, 37
    rng = np.random.default_rng(77)
    tables = jbu_tables(s, r)
    tdev = device_tables(tables, DEV)
    inputs = []
    for _ in range(2):
        left, right = (rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(2))
        gt = rng.uniform(0, 100, (H, W)).astype(np.float32)
        gt[3, 4] = np.inf
        frame = np.full((24, 48), 1e9, np.float32)
        frame[y0:y0 + rows, :cols] = rng.uniform(-5, 60, (rows, cols)).astype(np.float32)
        inputs.append((left, right, gt, frame))
    sl, sr = (torch.empty((H, W, 3), device=DEV, dtype=torch.uint8) for _ in range(2))
    sg, sf = torch.empty((H, W), device=DEV), torch.empty((24, 48), device=DEV)
    small = torch.empty((2, rows, cols, 3), device=DEV, dtype=torch.uint8)
    small_gt = torch.empty((rows, cols), device=DEV)
    out = {"disp": torch.empty((H, W), device=DEV), "valid": torch.empty((H, W), device=DEV)}

    def launches():
        ops.area_downscale_pair(sl, sr, s, out=small)
        ops.area_downscale_disp(sg, s, out=small_gt)
        return ops.guided_upsample(sf, small[0], sl, s, tdev, (y0, rows, cols), out=out)

    for static, a in zip((sl, sr, sg, sf), inputs[1]):
        static.copy_(dev(a))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launches()                                                       # warm-up, outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = launches()
    assert all(res[k] is out[k] for k in out)
    for left, right, gt, frame in inputs + inputs[:1]:
        for static, a in zip((sl, sr, sg, sf), (left, right, gt, frame)):
            static.copy_(dev(a))
        graph.replay()
        torch.cuda.synchronize()
        want_small = area_downscale_pair_host(left, right, s)
        same_bits(small, want_small, "replay pair")
        same_bits(small_gt, area_downscale_disp_host(gt, s), "replay disp")
        ref = guided_upsample_host(frame, want_small[0], left, s, tables, (y0, rows, cols))
        for k in ("valid", "disp"):
            same_bits(out[k], ref[k], f"replay {k}")


# ---- argument refusals ------------------------------------------------------------------------------------------------------
class LibraryTouched(BaseException):
    pass


class NoLibrary:
    def __getattr__(self, name):
        raise LibraryTouched(name)


def _base(op):
    """the keyword arguments of one small accepted call"""
    s = 2
    if op == "area_downscale_pair":
        return dict(left_u8=torch.zeros((6, 10, 3), device=DEV, dtype=torch.uint8),
                    right_u8=torch.zeros((6, 10, 3), device=DEV, dtype=torch.uint8), scale=s)
    if op == "area_downscale_disp":
        return dict(disp=torch.zeros((6, 10), device=DEV), scale=s)
    return dict(disp_lo=torch.ones((8, 12), device=DEV), guide_lo=torch.zeros((5, 7, 3), device=DEV, dtype=torch.uint8),
                guide_hi=torch.zeros((10, 13, 3), device=DEV, dtype=torch.uint8), scale=s, tables=device_tables(jbu_tables(s, 2), DEV),
                window=(1, 5, 7))


def _wide(t):
    """same shape and dtype, every second element of a buffer twice as wide"""
    return torch.zeros(t.shape[:-1] + (2 * t.shape[-1],), device=t.device, dtype=t.dtype)[..., ::2]


def _tables_like(ws=None, wr=None, **kw):
    base = device_tables(jbu_tables(2, 2), DEV)
    return (base[0] if ws is None else ws(base[0]), base[1] if wr is None else wr(base[1]))


def _aliased():
    """a frame as large as the output, handed in as the output too"""
    t = torch.ones((10, 13), device=DEV)
    return dict(disp_lo=t, window=(0, 5, 7), out={"valid": t})


REFUSALS = [
    ("area_downscale_pair", "a CPU tensor", lambda kw: dict(left_u8=kw["left_u8"].cpu())),
    ("area_downscale_pair", "the wrong dtype", lambda kw: dict(right_u8=kw["right_u8"].float())),
    ("area_downscale_pair", "not contiguous", lambda kw: dict(left_u8=_wide(kw["left_u8"]))),
    ("area_downscale_pair", "two shapes", lambda kw: dict(right_u8=kw["right_u8"][:5].contiguous())),
    ("area_downscale_pair", "scale 1", lambda kw: dict(scale=1)),
    ("area_downscale_pair", "scale 5", lambda kw: dict(scale=5)),
    ("area_downscale_pair", "a fractional scale", lambda kw: dict(scale=2.0)),
    ("area_downscale_pair", "out of the wrong shape", lambda kw: dict(out=torch.zeros((2, 3, 5, 4), device=DEV, dtype=torch.uint8))),
    ("area_downscale_pair", "out aliasing an input", lambda kw: dict(out=kw["left_u8"].view(-1)[:90].view(2, 3, 5, 3))),
    ("area_downscale_disp", "a CPU tensor", lambda kw: dict(disp=kw["disp"].cpu())),
    ("area_downscale_disp", "the wrong dtype", lambda kw: dict(disp=kw["disp"].double())),
    ("area_downscale_disp", "not contiguous", lambda kw: dict(disp=_wide(kw["disp"]))),
    ("area_downscale_disp", "a batch", lambda kw: dict(disp=kw["disp"][None])),
    ("area_downscale_disp", "requires_grad", lambda kw: dict(disp=kw["disp"].requires_grad_())),
    ("area_downscale_disp", "scale 5", lambda kw: dict(scale=5)),
    ("area_downscale_disp", "out aliasing the input", lambda kw: dict(out=kw["disp"].view(-1)[:15].view(3, 5))),
    ("guided_upsample", "a CPU tensor", lambda kw: dict(disp_lo=kw["disp_lo"].cpu())),
    ("guided_upsample", "a CPU guide", lambda kw: dict(guide_hi=kw["guide_hi"].cpu())),
    ("guided_upsample", "the wrong dtype", lambda kw: dict(disp_lo=kw["disp_lo"].double())),
    ("guided_upsample", "a float guide", lambda kw: dict(guide_lo=kw["guide_lo"].float())),
    ("guided_upsample", "not contiguous", lambda kw: dict(disp_lo=_wide(kw["disp_lo"]))),
    ("guided_upsample", "a guide that is not contiguous", lambda kw: dict(guide_hi=kw["guide_hi"].transpose(0, 1).contiguous().transpose(0, 1))),
    ("guided_upsample", "requires_grad", lambda kw: dict(disp_lo=kw["disp_lo"].requires_grad_())),
    ("guided_upsample", "guide_hi too tall for rows * s", lambda kw: dict(guide_hi=torch.zeros((11, 13, 3), device=DEV, dtype=torch.uint8))),
    ("guided_upsample", "guide_hi too narrow for cols * s", lambda kw: dict(guide_hi=torch.zeros((10, 12, 3), device=DEV, dtype=torch.uint8))),
    ("guided_upsample", "guide_lo not the window's size", lambda kw: dict(guide_lo=torch.zeros((5, 6, 3), device=DEV, dtype=torch.uint8))),
    ("guided_upsample", "guides of two channel counts", lambda kw: dict(guide_lo=torch.zeros((5, 7, 4), device=DEV, dtype=torch.uint8))),
    ("guided_upsample", "a window outside the frame", lambda kw: dict(window=(4, 5, 7))),
    ("guided_upsample", "a range table of the wrong length", lambda kw: dict(tables=_tables_like(wr=lambda t: t[:765].contiguous()))),
    ("guided_upsample", "a spatial table for another scale", lambda kw: dict(tables=device_tables(jbu_tables(3, 2), DEV))),
    ("guided_upsample", "radius 4", lambda kw: dict(tables=_tables_like(ws=lambda t: torch.ones((2, 9), device=DEV)))),
    ("guided_upsample", "tables on the host", lambda kw: dict(tables=tuple(torch.from_numpy(t) for t in jbu_tables(2, 2)))),
    ("guided_upsample", "float64 tables", lambda kw: dict(tables=_tables_like(ws=lambda t: t.double()))),
    ("guided_upsample", "a mask of another shape", lambda kw: dict(mask=torch.ones((5, 7), device=DEV))),
    ("guided_upsample", "a NaN mask_min", lambda kw: dict(mask=torch.ones((8, 12), device=DEV), mask_min=float("nan"))),
    ("guided_upsample", "an unknown output", lambda kw: dict(outputs=("depth",))),
    ("guided_upsample", "no output", lambda kw: dict(outputs=())),
    ("guided_upsample", "out of the wrong shape", lambda kw: dict(out={"disp": torch.zeros((10, 12), device=DEV)})),
    ("guided_upsample", "out aliasing the disparity", lambda kw: _aliased()),
    ("guided_upsample", "two outputs in one buffer", lambda kw: dict(out=dict.fromkeys(("disp", "valid"), torch.zeros((10, 13), device=DEV)))),
    ("guided_upsample", "scale 5", lambda kw: dict(scale=5)),
]


@pytest.mark.parametrize("op,what,change", REFUSALS, ids=[f"{op}-{what.replace(' ', '_')}" for op, what, _ in REFUSALS])
def test_wrappers_refuse_by_name_before_the_library(op, what, change, monkeypatch):
    from dcanet_amd import highres, ops
    kw = _base(op)
    getattr(ops, op)(**kw)                                               # the base call itself is accepted
    monkeypatch.setattr(highres, "_L", lambda: NoLibrary())
    kw.update(change(kw))
    with pytest.raises(RuntimeError, match="^" + op):
        getattr(ops, op)(**kw)


# ---- through the wrappers ---------------------------------------------------------------------------------------------------
WRAP = dict(crop_height=32, crop_width=64, graph=True, device_io=True)


@pytest.mark.parametrize("mode", [None, "confidence", "lr"])
def test_highres_inference_is_the_ops_around_kitti_inference(mode, monkeypatch):
    """a 57 x 111 pair (odd both ways) and a 64 x 128 one through the 32 x 64 frame at scale 2: (disp, valid) are
    ops.guided_upsample of what the existing class of that mode hands out for the downscaled pair; stream() gives the bytes"""
    from dcanet_amd import ops
    from dcanet_amd.inference import HighResInference, KittiInference, KittiInferenceLR, KittiInferenceWithConfidence
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    model = _model()
    rng = np.random.default_rng(41)
    pairs = [(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
             for h, w in ((57, 111), (64, 128))]
    own = (KittiInferenceWithConfidence if mode == "confidence" else KittiInference)(model, **WRAP)
    tables = jbu_tables(2, 2, 1.0, 24.0)
    smalls = [ops.area_downscale_pair(dev(l), dev(r), 2) for l, r in pairs]
    lows = [own(sm[0].cpu().numpy(), sm[1].cpu().numpy()) for sm in smalls]
    tau = 1e6                                        # "lr": every pixel that is in view passes, the others do not
    if mode == "lr":                                 # the UNFILLED disparity, the check's validity
        lr = KittiInferenceLR(model, tau=tau, **WRAP)
        lows = [(low, lr(sm[0].cpu().numpy(), sm[1].cpu().numpy())[1]) for low, sm in zip(lows, smalls)]
        assert 0 < lows[0][1].sum() < lows[0][1].size
    mask_min = 0.5 if mode != "confidence" else float(np.median(lows[0][1]))
    infer = HighResInference(model, scale=2, mask=mode, mask_min=mask_min, tau=tau, **WRAP)
    single = []
    for i, ((l, r), sm, low) in enumerate(zip(pairs, smalls, lows)):
        disp_lo, conf = low if mode else (low, None)
        assert disp_lo.shape == sm.shape[1:3]
        want = ops.guided_upsample(dev(disp_lo), sm[0], dev(l), 2, device_tables(tables, DEV), mask=dev(conf), mask_min=mask_min)
        got_d, got_v = infer(l, r)
        single.append((got_d, got_v))
        print(f"mode={mode} image {l.shape[:2]}: valid {int(got_v.sum())} of {got_v.size}, max disparity {got_d.max():.2f}")
        assert got_d.shape == got_v.shape == l.shape[:2] and got_d.dtype == got_v.dtype == np.float32
        assert got_v.tobytes() == want["valid"].cpu().numpy().tobytes(), f"image {i}: valid"
        assert got_d.tobytes() == want["disp"].cpu().numpy().tobytes(), f"image {i}: disp"
        assert got_v.sum() > 0
    streamed = list(infer.stream(iter(pairs + pairs[:1]), depth=2))
    assert len(streamed) == 3
    for (gd, gv), (sd, sv) in zip(streamed, single + single[:1]):
        assert gd.tobytes() == sd.tobytes() and gv.tobytes() == sv.tobytes()


def test_highres_inference_refuses_by_name():
    from dcanet_amd.inference import HighResInference
    model = _model()
    for bad in (dict(scale=1), dict(scale=5), dict(scale=2.0)):
        with pytest.raises(ValueError, match="HighResInference"):
            HighResInference(model, **{**WRAP, **bad})
    with pytest.raises(ValueError, match="HighResInference"):
        HighResInference(model, **{**WRAP, "device_io": False})
    with pytest.raises(ValueError):
        HighResInference(model, mask="nope", **WRAP)
    with pytest.raises(ValueError):
        HighResInference(model, radius=4, **WRAP)
    big = np.zeros((66, 128, 3), np.uint8)                               # 33 x 64 at 1/2: one row more than the frame
    with pytest.raises(ValueError, match="does not fit"):
        HighResInference(model, **WRAP)(big, big)


@pytest.mark.parametrize("kind,inf", [("kitti", False), ("sceneflow", True)])
def test_train_input_downscale_is_host_sample_bit_for_bit(kind, inf):
    from dcanet_amd.training import AugParams, TrainInput, host_sample
    rng = np.random.default_rng(13)
    left, right = (rng.integers(0, 256, (37, 51, 3), dtype=np.uint8) for _ in range(2))
    if kind == "kitti":
        disp = rng.integers(0, 90 * 256, (37, 51)).astype(np.uint16)      # the PNG payload, scale 1 / 256
    else:
        disp = rng.uniform(0, 90, (37, 51)).astype(np.float32)            # a bottom-up PFM payload with infinities
        disp[5, 7] = disp[20, 30] = disp[36, 50] = np.inf
    p = AugParams(3, 2, (1.2, 0.8), (0.9, 1.1), (1.1, 0.9), (1, 5, 2, 9))
    want = host_sample(left, right, disp, p, crop=(16, 20), maxdisp=40, kind=kind, flip_rows=inf, inf_to_zero=inf, downscale=2)
    ti = TrainInput(1, crop=(16, 20), maxdisp=40, kind=kind, device_io=True, downscale=2)
    ti.load(0, left, right, disp, p, flip_rows=inf, inf_to_zero=inf)
    got = ti.batch()
    torch.cuda.synchronize()
    assert want[3].any() and not want[3].all() and np.isfinite(want[2]).all()
    for g, w, name in zip(got, want, ("imgL", "imgR", "gt", "mask")):
        same_bits(g[0], w, f"{kind} {name}")
    host = TrainInput(1, crop=(16, 20), maxdisp=40, kind=kind, device_io=False, downscale=2)
    host.load(0, left, right, disp, p, flip_rows=inf, inf_to_zero=inf)
    for g, w in zip(host.batch(), want):
        assert g[0].numpy().tobytes() == w.tobytes()
    with pytest.raises(ValueError, match="TrainInput"):
        TrainInput(1, downscale=5)
