"""CPU checks of the ground-plane operators: the numpy restatement of dcanet_amd/ground.py against the TRUTH of synthetic
scenes (tests/_ground_cases.py) and against closed forms, the operators' refusals, the library's symbols, and the host check
of csrc/ground_math.h under sanitizers.  The kernels are compared with the restatement, bit for bit, in test_gpu_ground.py."""
import ctypes
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import _ground_cases as C
from dcanet_amd import ground as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name,s,nb", C.plane_only_scenes(), ids=lambda v: v if isinstance(v, str) else "")
def test_plane_only_scene_is_found_to_half_a_quantisation_step(name, s, nb):
    """noise-free plane: the fitted p within 1/32 px -- half the step of q, the disparity in sixteenths -- of the true plane at
    EVERY pixel, fit rows or not, sky or not.  A fit worse than the quantisation it sees is wrong."""
    r = G.ground_plane_host(s.d, nb)
    rec = r["plane"]
    p = G.plane_disp(rec, *s.d.shape).astype(np.float64)
    err = float(np.abs(p - s.p).max())
    print(f"{name}: a {rec[0]:.6f} b {rec[1]:.6f} c {rec[2]:.5f} (true {s.a}, {s.b:.6f}, {s.c:.5f}), inliers {int(rec[3])}, "
          f"rms {rec[4]:.4f}, line ({int(rec[6])}, {int(rec[7])}) vote {int(rec[8])}, max |p - p_true| = {err:.5f} px")
    assert rec[5] == 0 and rec[15] == 2 and err <= 1 / 32
    rows = s.d.shape[0]
    nfit = int(((s.d > 0)[rows // 2:]).sum())
    assert rec[3] == nfit, "every road pixel of the fit rows is an inlier of the last round"
    assert r["vdisp"].dtype == np.int32 and int(r["vdisp"].sum()) == int((s.d > 0).sum())
    assert (int(rec[6]) > 0) == ("above" in name or s.p[0, s.d.shape[1] // 2] > 1), "the horizon's side"


@pytest.mark.parametrize("name,s,nb,calib", C.wall_scenes(), ids=lambda v: v if isinstance(v, str) else "")
def test_road_wall_sky_scene_is_labelled_without_exception(name, s, nb, calib):
    """noise-free road, wall, sky and roll: every true road pixel outside the wall is ground; every pixel more than 2 h_ground
    above the road whose disparity exceeds the true plane's by more than tol_d + 1/8 px is an obstacle.  No exceptions."""
    rec = G.ground_plane_host(s.d, nb, calib)["plane"]
    seg = G.ground_segment_host(s.d, rec, calib, nb)
    p = G.plane_disp(rec, *s.d.shape).astype(np.float64)
    with np.errstate(all="ignore"):
        h_true = rec[9] * (s.d - s.p) / (s.d.astype(np.float64) + calib.doffs)
    must = (s.d > 0) & (h_true > 2 * G.GROUND_H_GROUND) & (s.d - s.p > G.GROUND_TOL_D + 1 / 8)
    print(f"{name}: max |p - p_true| on the road = {np.abs(p - s.p)[s.road].max():.4f} px, camera height {rec[9]:.4f} m, "
          f"{int(s.road.sum())} road pixels, {int(must.sum())} certain obstacle pixels of {int(s.wall.sum())} wall pixels; labels "
          f"{np.bincount(seg['label'].ravel(), minlength=5).tolist()}")
    assert rec[5] == 0 and s.road.sum() > 1000 and must.sum() > 50
    assert (seg["label"][s.road] == 1).all()
    assert (seg["label"][must] == 2).all()
    assert (seg["label"][s.d == 0] == 0).all() and (seg["height"][s.d == 0] == 0).all()
    # the free-space walk: below a wall the column's base row is the wall's lowest obstacle pixel
    lab = seg["label"]
    for c in range(s.d.shape[1]):
        run, want = 0, -1
        for r in range(s.d.shape[0] - 1, -1, -1):
            run = run + 1 if lab[r, c] == 2 else 0
            if run == G.GROUND_MIN_RUN:
                want = r + G.GROUND_MIN_RUN - 1
                break
        assert seg["free_row"][c] == want and seg["free_disp"][c] == (s.d[want, c] if want >= 0 else 0)
    assert (seg["free_row"] >= 0).sum() >= 15
    # the grid counts every ground and obstacle pixel inside it once
    assert seg["bev"].dtype == np.int32 and seg["bev"][0].sum() <= (lab == 1).sum() and 0 < seg["bev"][1].sum() <= (lab == 2).sum()


def test_restatement_details_on_the_gpu_cases():
    """what the cases are there for: the statuses, the boundary d_top = -NB, the tie, runs of min_run - 1 and min_run, all five
    labels, pixels outside the grid and cells with many pixels"""
    by = {c.name: c for c in C.cases()}
    out = {}
    for name, c in by.items():
        r = G.ground_plane_host(c.d, **C.plane_kwargs(c))
        out[name] = (r, G.ground_segment_host(c.d, r["plane"], c.calib, **C.segment_kwargs(c)))
    plane = lambda name: out[name][0]["plane"].reshape(-1, G.PLANE_LEN)
    assert plane("no valid pixel | all wall (status 1)")[:, 5].tolist() == [1, 1]
    assert (out["no valid pixel | all wall (status 1)"][1]["label"] == 0).all()
    assert plane("no valid pixel | all wall (status 1)")[0, 6:9].tolist() == [-32, 1, 0], "no vote: the first candidate in order"
    st2 = plane("10 road pixels | one column (status 2)")
    assert st2[:, 5].tolist() == [2, 2] and (st2[:, 0] == 0).all() and (st2[:, 3] == 0).all(), "the Hough line stays"
    sums = out["10 road pixels | one column (status 2)"][0]["sums"]
    assert sums[0, 0, 0] == 10 and sums[1, 0, 0] == 20 and (sums[:, 1:] == 0).all(), "fewer than min_inliers | singular"
    assert plane("d_top = -NB, 40x70")[0, 6:9].tolist() == [-32, 30, 1400]
    assert plane("same, refine 0")[0, [0, 3, 15]].tolist() == [0, 0, 0] and plane("same, refine 0")[0, 5] == 0
    assert plane("window 53x131 of 64x140, mask, roll-, horizon inside")[0, 15] == 4
    # the tie
    c = by["two rows: an exact tie"]
    votes = G.hough_votes(out[c.name][0]["vdisp"], 20, 40, G.GROUND_MIN_RISE)
    best = np.argwhere(votes == votes.max())
    assert len(best) > 1 and votes.max() == 140
    assert plane(c.name)[0, 6:8].tolist() == [best[0][1] - 32, best[0][0] + 1], "the smallest d_bot, then the smallest d_top"
    assert (best[:, 0] >= best[0][0]).all() and (best[best[:, 0] == best[0][0], 1] >= best[0][1]).all()
    # labels, runs, grid
    seg = out["window 53x131 of 64x140, mask, roll-, horizon inside"][1]
    assert all((seg["label"] == k).sum() > 20 for k in range(5)), np.bincount(seg["label"].ravel())
    assert seg["bev"].max() > 50 and seg["bev"].sum() < ((seg["label"] == 1) | (seg["label"] == 2)).sum()
    seg = out["road+wall 48x75 roll+"][1]
    lab = seg["label"]
    assert (lab[40:42, 10] == 2).all() and lab[39, 10] != 2 and lab[42, 10] != 2, "a run of min_run - 1 is passed over"
    assert seg["free_row"][10] == 32 and seg["free_row"][12] == 40 and seg["free_row"][14] == -1
    assert out["same, fit rows 20:45, min_run 1, tol 0.75"][1]["free_row"][14] == 45


@pytest.mark.parametrize("height,pitch,roll,doffs,v0", [(1.65, 2.0, 0.0, 0.0, 0), (1.2, -1.5, 3.0, 0.0, 0),
                                                        (0.8, 5.0, -4.0, 12.5, 120), (2.4, 0.3, -0.2, 0.0, 7)])
def test_plane_pose_inverts_an_analytic_plane(height, pitch, roll, doffs, v0):
    """a plane generated from a chosen height, pitch and roll through a StereoCalib, nothing fitted: plane_pose is a closed form in
    float64, only rounding separates the values"""
    from dcanet_amd.geometry import StereoCalib
    calib = StereoCalib(721.5, 0.54, 609.6, 172.9, doffs)
    rec = G.plane_from_pose(height, pitch, roll, calib, 375, 1242, v0)
    got = G.plane_pose(rec, calib, v0)
    rel = lambda a, b: abs(a - b) / max(abs(b), 1e-300)
    print(got, rec[:3])
    assert rel(got["height"], height) <= 1e-9 and rel(got["pitch"], pitch) <= 1e-9
    assert (roll == 0.0 and abs(got["roll"]) <= 1e-12) or rel(got["roll"], roll) <= 1e-9
    # the horizon: the image row at the principal column where the plane's disparity + doffs vanishes
    pt, rl = math.radians(pitch), math.radians(roll)
    assert rel(got["horizon"], calib.cy - calib.f * math.tan(pt) / math.cos(rl)) <= 1e-9
    assert rel(rec[9], height) <= 1e-12 and abs(math.hypot(*rec[10:13]) - 1) <= 1e-12
    # in the window's own coordinates the plane gives the road's disparity: f B / Z on the ray of a pixel
    r, c = 300, 400
    n = got["normal"]
    ray = np.array([(c - calib.cx) / calib.f, (v0 + r - calib.cy) / calib.f, 1.0])
    Z = height / float(np.dot(n, ray))
    d = calib.f * calib.baseline / Z - doffs
    assert rel(rec[0] * (c - 1242 // 2) + rec[1] * (r - 375 // 2) + rec[2], d) <= 1e-9
    with pytest.raises(ValueError):
        G.plane_pose(np.zeros(G.PLANE_LEN), StereoCalib(721.5, 0.54, 609.6, 172.9))       # a = b = 0 and no offset: no normal
    with pytest.raises(ValueError):
        G.plane_pose(rec[:5], calib)


def _plane_call(lib, **kw):
    p = [ctypes.c_void_p(64 * k) for k in range(1, 6)]
    a = dict(d=p[0], mask=None, plane=p[1], vdisp=p[2], ws=p[3], B=1, Hc=48, Wc=80, y0=0, rows=48, cols=75, max_disp=32, r_lo=24,
             r_hi=48, min_rise=2, min_votes=24, refine=2, min_inliers=16, min_disp=0.0625, tol=1.5, mask_min=0.5, calibrated=0,
             f=0.0, baseline=0.0, cx=0.0, cy=0.0, doffs=0.0, v0=0.0)
    a.update(kw)
    return lib.dca_ground_plane(*a.values(), None)


def _segment_call(lib, **kw):
    p = [ctypes.c_void_p(64 * k) for k in range(1, 9)]
    a = dict(d=p[0], mask=None, plane=p[1], label=p[2], height=p[3], free_row=p[4], free_disp=p[5], bev=p[6], B=1, Hc=48, Wc=80,
             y0=0, rows=48, cols=75, max_disp=32, min_disp=0.0625, mask_min=0.5, tol_d=1.0, h_ground=0.15, h_max=3.0, min_run=3,
             f=60.0, fb=30.0, cx=37.0, doffs=0.0, x_min=-3.0, inv_cell=2.0, max_depth=12.0, NX=12, NZ=24)
    a.update(kw)
    return lib.dca_ground_segment(*a.values(), None)


PLANE_REFUSALS = [dict(d=None), dict(plane=None), dict(vdisp=None), dict(ws=None), dict(B=0), dict(B=65536), dict(y0=1), dict(cols=81),
                  dict(Hc=1 << 16, Wc=1 << 15), dict(rows=1, r_lo=0, r_hi=1), dict(Hc=32769, rows=32769), dict(Wc=32769, cols=32769),
                  dict(max_disp=7), dict(max_disp=1025), dict(r_lo=-1), dict(r_lo=48), dict(r_hi=49), dict(r_lo=30, r_hi=30),
                  dict(min_rise=0), dict(min_rise=33), dict(min_votes=0), dict(refine=-1), dict(refine=5), dict(min_inliers=2),
                  dict(min_disp=-0.5), dict(min_disp=math.inf), dict(min_disp=math.nan), dict(tol=-1.0), dict(tol=math.nan),
                  dict(tol=math.inf), dict(mask=ctypes.c_void_p(4096), mask_min=math.nan), dict(calibrated=2),
                  dict(calibrated=1), dict(calibrated=1, f=60.0), dict(calibrated=1, f=60.0, baseline=0.5, cx=math.nan),
                  dict(calibrated=1, f=math.inf, baseline=0.5), dict(calibrated=1, f=60.0, baseline=0.5, v0=math.inf),
                  dict(calibrated=1, f=60.0, baseline=0.5, doffs=math.nan), dict(calibrated=1, f=60.0, baseline=0.5, cy=-math.inf)]
SEGMENT_REFUSALS = [dict(d=None), dict(plane=None), dict(label=None, height=None, free_row=None, free_disp=None, bev=None),
                    dict(free_row=None), dict(free_disp=None), dict(B=0), dict(B=65536), dict(y0=1), dict(cols=81),
                    dict(Hc=32769, rows=32769), dict(max_disp=7), dict(max_disp=1025), dict(min_disp=-1.0), dict(min_disp=math.nan),
                    dict(tol_d=-1.0), dict(tol_d=math.inf), dict(h_ground=-0.1), dict(h_ground=math.nan), dict(h_max=math.inf),
                    dict(h_max=math.nan), dict(min_run=0), dict(mask=ctypes.c_void_p(4096), mask_min=math.nan), dict(f=0.0),
                    dict(f=math.inf), dict(fb=0.0), dict(fb=math.nan), dict(cx=math.inf), dict(doffs=math.nan), dict(x_min=math.inf),
                    dict(inv_cell=0.0), dict(inv_cell=math.inf), dict(max_depth=0.0), dict(max_depth=math.nan), dict(NX=0),
                    dict(NZ=0), dict(NX=1 << 15, NZ=1 << 15)]


def test_ground_library_abi_symbols_and_refusals():
    """the library loads with ABI 21 -- entry points were added, none changed -- exports the new symbols with the types of the
    header, and its launchers refuse everything the header lists with hipErrorInvalidValue (1), without touching a device"""
    from ctypes import c_double as d, c_float as f, c_int as i, c_void_p as p
    from dcanet_amd import _lib, ops
    lib = _lib.load()
    assert _lib.ABI_VERSION == 21 and lib.dca_abi_version() == 21
    S = _lib.SIGNATURES
    assert S["dca_ground_plane"] == (i, [p] * 5 + [i] * 13 + [f] * 3 + [i] + [d] * 6 + [p])
    assert S["dca_ground_segment"] == (i, [p] * 8 + [i] * 7 + [f] * 5 + [i] + [f] * 7 + [i, i, p])
    assert all(getattr(lib, name) is not None for name in ("dca_ground_plane", "dca_ground_segment"))
    assert (ops.GROUND_PLANE_LEN, ops.GROUND_WS_LEN) == (G.PLANE_LEN, G.WS_LEN) == (16, 48) == (len(G.PLANE_FIELDS), 48)
    assert ops.GROUND_SUMS_AT + 10 * G.MAX_REFINE <= G.WS_LEN and ops.GROUND_OUTPUTS == G.SEGMENT_OUTPUTS
    for bad in PLANE_REFUSALS:
        assert _plane_call(lib, **bad) == 1, bad
    for bad in SEGMENT_REFUSALS:
        assert _segment_call(lib, **bad) == 1, bad


def test_ground_operators_refuse_with_their_name():
    """every refusal of the header, raised where the operators validate once -- `ground.plane_scalars`, `calib_scalars` and
    `segment_scalars`, which they call with RuntimeError and the restatements with ValueError -- and named; the frame checks
    are frame_ops.py's own helpers"""
    from dcanet_amd import ops
    from dcanet_amd.geometry import StereoCalib
    a = torch.zeros(48, 75)
    for call in (lambda t, **kw: ops.ground_plane(t, 32, **kw), lambda t, **kw: ops.ground_segment(t, torch.zeros(16).double(), None, **kw)):
        with pytest.raises(RuntimeError, match=r"ground_(plane|segment): .*no CPU fallback"):
            call(a)
        with pytest.raises(RuntimeError, match="inference only"):
            call(a.clone().requires_grad_())
    good = dict(rows=48, cols=75, max_disp=32, rows_range=None, min_rise=2, min_votes=None, refine=2, min_inliers=16, min_disp=0.0625,
                tol=1.5)
    assert G.plane_scalars("ground_plane", RuntimeError, **good) == (32, 24, 48, 2, 24, 2, 16, 0.0625, 1.5)
    for bad in (dict(rows=1), dict(rows=32769), dict(cols=32769), dict(max_disp=7), dict(max_disp=1025), dict(max_disp=32.5),
                dict(max_disp="x"), dict(rows_range=(-1, 48)), dict(rows_range=(48, 48)), dict(rows_range=(24, 49)),
                dict(rows_range=(30, 30)), dict(rows_range=3), dict(min_rise=0), dict(min_rise=33), dict(min_rise=1.5),
                dict(min_votes=0), dict(refine=-1), dict(refine=5), dict(refine=1.5), dict(min_inliers=2), dict(min_disp=-0.5),
                dict(min_disp=math.inf), dict(min_disp=math.nan), dict(tol=-1.0), dict(tol=math.nan), dict(tol=math.inf),
                dict(tol=None)):
        for err, name in ((RuntimeError, "ground_plane"), (ValueError, "ground_plane_host")):
            with pytest.raises(err, match=name + ":"):
                G.plane_scalars(name, err, **{**good, **bad})
    cal = StereoCalib(60.0, 0.5, 37.0, -7.0)
    assert G.calib_scalars("ground_plane", RuntimeError, cal, 3) == (60.0, 0.5, 37.0, -7.0, 0.0, 3.0)
    half = type("C", (), dict(f=60.0, baseline=0.0, cx=1.0, cy=1.0, doffs=0.0))()
    for bad in ((None, 0), (cal, math.nan), (cal, math.inf), (cal, "x"), (half, 0), (type("C", (), dict(f=60.0))(), 0)):
        with pytest.raises(RuntimeError, match="ground_plane:"):
            G.calib_scalars("ground_plane", RuntimeError, *bad)
    good = dict(max_disp=32, min_disp=0.0625, tol_d=1.0, h_ground=0.15, h_max=3.0, min_run=3, grid=(0.5, 3.0, 12.0))
    assert G.segment_scalars("ground_segment", RuntimeError, **good) == (32, 0.0625, 1.0, 0.15, 3.0, 3, (-3.0, 2.0, 12.0, 12, 24))
    for bad in (dict(max_disp=7), dict(max_disp=1025), dict(max_disp=8.5), dict(min_disp=-1.0), dict(min_disp=math.nan),
                dict(tol_d=-1.0), dict(tol_d=math.inf), dict(h_ground=-0.1), dict(h_ground=math.nan), dict(h_max=math.inf),
                dict(h_max=math.nan), dict(min_run=0), dict(min_run=2.5), dict(grid=(0.0, 3.0, 12.0)), dict(grid=(0.5, 3.0)),
                dict(grid=(0.5, math.inf, 12.0)), dict(grid=(0.5, 3.0, -1.0)), dict(grid=(1e-4, 3.0, 12.0)), dict(grid=None)):
        for err, name in ((RuntimeError, "ground_segment"), (ValueError, "ground_segment_host")):
            with pytest.raises(err, match=name + ":"):
                G.segment_scalars(name, err, **{**good, **bad})
    with pytest.raises(RuntimeError, match="ground_workspace"):
        ops.ground_workspace(1, 75, 32, "cpu")
    with pytest.raises(RuntimeError, match="ground_workspace"):
        ops.ground_workspace(48, 75, 2048, "cpu")
    assert ops.ground_workspace(48, 75, 32, "cpu", batch=3).shape == (3, G.WS_LEN)
    # the restatement's own frame checks
    z = np.zeros((48, 75), np.float32)
    for bad in (dict(disp=z.astype(np.float64)), dict(window=(0, 49, 75)), dict(window=(1, 48, 75)), dict(window=(0, 48, 76)),
                dict(window=(0, 1, 75)), dict(mask=z[:10]), dict(mask=z, mask_min=math.nan), dict(disp=z[None, None, None])):
        with pytest.raises(ValueError, match="ground_plane_host:"):
            G.ground_plane_host(**{**dict(disp=z, max_disp=32), **bad})
    rec = np.zeros(G.PLANE_LEN)
    for bad in (dict(outputs=("nope",)), dict(plane=rec[:8]), dict(plane=np.zeros((2, G.PLANE_LEN))), dict(calib=None)):
        with pytest.raises(ValueError, match="ground_segment_host:"):
            G.ground_segment_host(**{**dict(disp=z, plane=rec, calib=cal, max_disp=32), **bad})
    assert set(G.ground_segment_host(z, rec, cal, 32, outputs=("label", "bev"))) == {"label", "bev"}


def test_ground_inference_wrapper_host_logic():
    """KittiInferenceGround takes KittiInference's arguments plus the stage's, asks for device I/O and a calibration"""
    from dcanet_amd.geometry import StereoCalib
    from dcanet_amd.inference import FrameGround, KittiInference, KittiInferenceGround
    net = torch.nn.Linear(1, 1)
    net.maxdisp = 192
    calib = StereoCalib(721.5, 0.54, 609.6, 172.9)
    g = KittiInferenceGround(net, calib, 64, 128, graph=False)
    assert isinstance(g, KittiInference) and g.device_io and (g.crop_height, g.crop_width) == (64, 128) and g.max_disp == 192
    assert g.mask_mode is None and g.speckle is None and g.median == 0 and g.grid == G.GROUND_GRID and g.Frame is FrameGround
    assert FrameGround._fields == ("disp", "label", "free_row", "free_disp", "bev", "plane")
    fields = dict((n, (dt, sh)) for n, dt, sh in g._fields(30, 100, False))
    assert set(fields) == set(FrameGround._fields) and fields["bev"][1] == (2, 300, 200) and fields["plane"] == (torch.float64, (16,))
    off = 0
    for n, dt, sh in g._fields(31, 99, False):       # back to back from byte 0, every field at a multiple of its element size
        assert off % dt.itemsize == 0, n
        off += math.prod(sh) * dt.itemsize
    assert fields["label"] == (torch.uint8, (30, 100)) and fields["free_row"] == (torch.int32, (100,))
    h = KittiInferenceGround(net, calib, mask="lr", tau=2.0, speckle=(100, 1.0), median=3, max_disp=64, grid=(0.5, 10.0, 30.0),
                             plane=dict(refine=1), segment=dict(min_run=2))
    assert h.mask_mode == "lr" and h.tau == 2.0 and h.speckle == (100, 1.0) and h.median == 3 and h.max_disp == 64
    for bad in (dict(calib=None), dict(device_io=False), dict(mask="nope"), dict(median=4), dict(speckle=(1,)), dict(max_disp=4),
                dict(grid=(0.0, 1.0, 1.0)), dict(plane=dict(refine=7)), dict(segment=dict(min_run=0)), dict(plane=dict(nope=1))):
        with pytest.raises((ValueError, RuntimeError, TypeError)):
            KittiInferenceGround(net, **{**dict(calib=calib), **bad})
    with pytest.raises(TypeError):
        g(np.zeros((8, 8, 3), np.uint8), np.zeros((8, 8, 3), np.uint8), as_uint16=True)


def test_ground_math_host_check_under_sanitizers(tmp_path):
    """tools/ground_math_check.cpp: the floor division, the line's bin, the key and the solve of csrc/ground_math.h, compiled for
    the host with AddressSanitizer and UBSan as a stand-alone program, exits 0"""
    cxx = next((c for c in (shutil.which("clang++"), "/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++",
                            shutil.which("g++")) if c and os.path.exists(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "ground_check")
    csrc = os.path.join(ROOT, "cost-volume-aggregation-in-stereo-matching-revisited_amd", "csrc")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc,
           os.path.join(ROOT, "tools", "ground_math_check.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok"), run.stdout[-2000:] + run.stderr[-2000:]
