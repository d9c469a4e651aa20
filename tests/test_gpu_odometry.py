"""Stereo visual odometry on the MI355X (csrc/odometry.hip): `ops.grey_pyramid`, `ops.disp_pyramid` and `ops.ego_motion` bit for
bit against the numpy restatements of dcanet_amd/odometry.py on the sequences of tests/_odometry_cases.py, and
`ops.disp_reproject` with the matrix on the device against its by-value route.

Why bitwise, without any tolerance: the per-pixel part is a chain of single float32 operations (+ - x / floor rint), each
correctly rounded on the device (contraction off, IEEE division) and in numpy alike, ending in integers; the 29 sums are int64
and integer addition commutes, so the atomics' order of arrival does not matter; the solve is a fixed sequence of float64
+ - x / without any library function."""
import numpy as np
import pytest
import torch

import _odometry_cases as K
import _temporal_cases as C
from dcanet_amd import geometry as GEO
from dcanet_amd import odometry as OD
from dcanet_amd import temporal as T

pytestmark = pytest.mark.gpu
DEV = "cuda"
f32 = np.float32
NAN, INF = float("nan"), float("inf")


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)         # (a copy: the cases are read-only)


def same_bits(got, want, name):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
    bits = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize] if got.dtype.kind == "f" else got.dtype
    bad = np.nonzero(got.view(bits) != want.view(bits))
    assert len(bad[0]) == 0, f"{name}: {len(bad[0])} elements differ, first at {[int(i[0]) for i in bad]}: " \
                             f"{got[bad][0]!r} != {want[bad][0]!r}"


def garbage(levels, iters):
    """output buffers and a workspace that start as garbage: the init launch writes what the others read"""
    out = {"rec": torch.full((OD.REC_LEN,), NAN, device=DEV, dtype=torch.float64), "g": torch.full((24,), INF, device=DEV),
           "sums": torch.full((levels * iters, OD.SUMS), -7, device=DEV, dtype=torch.int64)}
    return out, torch.full((OD.SUMS,), 1 << 61, device=DEV, dtype=torch.int64)


def check_ego(scene, fr, name, levels=K.LEVELS, iters=K.ITERS, init=None, init_dev=None, **kw):
    """`ops.ego_motion` into garbage against the restatement: the record, G and the sums of every iteration; then a second call
    with fresh buffers, the same bits"""
    from dcanet_amd import ops
    kw = {"max_disp": K.MAX_DISP, **kw}
    want = OD.ego_motion_host(fr["prev"], fr["cur"], fr["dpyr"], scene.hw, scene.calib, levels, iters, init=init, **kw)
    out, ws = garbage(levels, iters)
    args = (dev(fr["prev"]), dev(fr["cur"]), dev(fr["dpyr"]), scene.hw, scene.calib, levels, iters)
    start = init if init_dev is None else init_dev
    got = ops.ego_motion(*args, init=start, outputs=OD.EGO_OUTPUTS, out=out, workspace=ws, **kw)
    assert got["rec"] is out["rec"] and got["sums"] is out["sums"] and got["G"].data_ptr() == out["g"].data_ptr()
    same_bits(got["sums"], want["sums"], f"{name}: the sums")
    same_bits(got["rec"], want["rec"], f"{name}: the record")
    same_bits(got["G"], want["G"], f"{name}: G")
    assert not ws.cpu().numpy().any(), "the solve leaves the sums cleared"
    again = ops.ego_motion(*args, init=start, **kw)
    assert set(again) == {"rec", "G"}
    same_bits(again["rec"], want["rec"], f"{name}: the record, second call")
    same_bits(again["G"], want["G"], f"{name}: G, second call")
    return want, got


# ---- the pyramids ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", K.SCENES + K.SMALL, ids=lambda s: s.name)
def test_pyramids_are_the_restatement_bit_for_bit(scene):
    """levels 1 to 5 of random RGB and RGBA images and of a disparity map with 0, NaN, inf and negative values, into garbage"""
    from dcanet_amd import ops
    rng = np.random.default_rng(11)
    H, W = scene.hw
    rgba = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    d = K.frame(scene, "identity", 0.3)["disp"].copy()
    bad = rng.uniform(size=d.shape)
    d[bad < 0.1], d[(bad > 0.1) & (bad < 0.15)], d[(bad > 0.15) & (bad < 0.2)], d[(bad > 0.2) & (bad < 0.25)] = 0.0, NAN, INF, -3.0
    for levels in range(1, 6):
        n = OD.pyramid_len(H, W, levels)
        for img in (rgba, np.ascontiguousarray(rgba[..., :3])):
            out = torch.full((n,), 201, device=DEV, dtype=torch.uint8)
            assert ops.grey_pyramid(dev(img), levels, out=out) is out
            same_bits(out, OD.grey_pyramid_host(img, levels), f"grey, {levels} levels, {img.shape[2]} channels")
        out = torch.full((n,), NAN, device=DEV)
        assert ops.disp_pyramid(dev(d), levels, 0.0625, out=out) is out
        same_bits(out, OD.disp_pyramid_host(d, levels, 0.0625), f"disparity, {levels} levels")
    same_bits(ops.disp_pyramid(dev(d), 3, min_disp=1.5), OD.disp_pyramid_host(d, 3, 1.5), "another min_disp")


# ---- the estimate ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", K.cases(), ids=lambda c: c[0])
def test_ego_motion_is_the_restatement_bit_for_bit(case):
    """every scene under every pose, without and with disparity noise: the pose doubles, G, count, residual, status and the
    int64 sums of all 18 iterations"""
    name, scene, pose, noise = case
    want, _ = check_ego(scene, K.frame(scene, pose, noise), name)
    assert want["rec"][OD.REC_STATUS] == 0 and want["rec"][OD.REC_ITERS] == K.LEVELS * K.ITERS and want["rec"][OD.REC_COUNT] > 1500


@pytest.mark.parametrize("levels", [1, 2, 3, 4])
@pytest.mark.parametrize("iters", [1, 6])
def test_schedules(levels, iters):
    """levels 1 to 4 (the fourth of 53 x 131 is 6 x 16: few pixels, still an estimate) and 1 or 6 iterations each"""
    scene = K.SCENES[1]
    check_ego(scene, K.frame(scene, "mixed", 0.3, levels), f"{levels} x {iters}", levels, iters)


@pytest.mark.parametrize("kw", [dict(grad_min=0), dict(grad_min=120), dict(huber=0.5), dict(huber=200.0), dict(min_ratio=0.9),
                                dict(min_pixels=6), dict(max_disp=20.0), dict(min_disp=0.5)], ids=str)
def test_parameters(kw):
    """no gradient threshold and a large one, a Huber radius so small that most weights are fractional and one so large that
    none is, a depth-ratio limit that bites, another disparity range"""
    scene = K.SCENES[2]
    want, _ = check_ego(scene, K.frame(scene, "forward1m", 0.3), str(kw), **kw)
    assert want["sums"][0, 28] > 0


@pytest.mark.parametrize("scene", K.SMALL, ids=lambda s: s.name)
def test_small_images(scene):
    """one workgroup, odd sizes; with three levels the coarsest has fewer than min_pixels pixels and the estimate fails at
    once, with two it runs"""
    for levels, status in ((1, 0), (2, 0), (3, 1)):
        want, got = check_ego(scene, K.frame(scene, "forward0.2m", 0.3, levels), f"{scene.name}, {levels} levels", levels, 3)
        assert want["rec"][OD.REC_STATUS] == status
        if status:
            assert np.isnan(got["G"].cpu().numpy()).all() and want["rec"][OD.REC_ITERS] == 1 and not want["sums"][1:].any()


def test_invalid_disparities_and_doffs():
    """NaN, inf, 0, negative and >= max_disp disparities take no part; a calibration with doffs > 0"""
    scene = K.SCENES[1]
    fr = dict(K.frame(scene, "yaw2deg", 0.3))
    rng = np.random.default_rng(23)
    d = fr["disp"].copy()
    bad = rng.uniform(size=d.shape)
    for lo, v in ((0.0, 0.0), (0.05, NAN), (0.1, INF), (0.15, -INF), (0.2, -2.0), (0.25, K.MAX_DISP), (0.3, 1e30)):
        d[(bad >= lo) & (bad < lo + 0.05)] = v
    fr["dpyr"] = OD.disp_pyramid_host(d, K.LEVELS)
    want, _ = check_ego(scene, fr, "invalid disparities")
    clean = OD.ego_motion_host(fr["prev"], fr["cur"], K.frame(scene, "yaw2deg", 0.3)["dpyr"], scene.hw, scene.calib, K.LEVELS, K.ITERS,
                               max_disp=K.MAX_DISP)
    assert 0 < want["sums"][-1, 28] < 0.75 * clean["sums"][-1, 28]
    c = scene.calib
    shifted = C.Scene(scene.name, scene.hw, GEO.StereoCalib(c.f, c.baseline, c.cx, c.cy, 3.25), scene.box, scene.backdrop)
    frd = dict(fr)
    frd["dpyr"] = OD.disp_pyramid_host(np.where(fr["disp"] > 3.5, fr["disp"] - f32(3.25), f32(0)).astype(f32), K.LEVELS)
    check_ego(shifted, frd, "doffs 3.25")


def test_five_metres_forward():
    """footprints leave the image and near points fall below min_ratio: fewer pixels, the same bits"""
    scene = K.SCENES[2]
    want, _ = check_ego(scene, K.frame(scene, K.FAR[0], 0.3), "5 m forward", init=np.linalg.inv(K.FAR[1]))
    near = OD.ego_motion_host(*(K.frame(scene, "forward0.2m", 0.3)[k] for k in ("prev", "cur", "dpyr")), scene.hw, scene.calib,
                              K.LEVELS, K.ITERS, max_disp=K.MAX_DISP)
    assert want["sums"][-1, 28] < 0.8 * near["sums"][-1, 28]


def test_start_poses():
    """init= from a host pose (4,4) and (3,4), from the device record of an earlier call -- also in place -- and from a failed one"""
    from dcanet_amd import ops
    scene = K.SCENES[0]
    fr = K.frame(scene, "mixed", 0.3)
    guess = C.translation(z=-0.4) @ C.yaw(-0.8)
    check_ego(scene, fr, "host (4,4)", 3, 2, init=guess)
    check_ego(scene, fr, "host (3,4)", 3, 2, init=guess[:3])
    first = OD.ego_motion_host(fr["prev"], fr["cur"], fr["dpyr"], scene.hw, scene.calib, 3, 2, max_disp=K.MAX_DISP)
    check_ego(scene, fr, "device record", 3, 2, init=first["rec"], init_dev=dev(first["rec"]))
    rec = dev(first["rec"])
    second = OD.ego_motion_host(fr["prev"], fr["cur"], fr["dpyr"], scene.hw, scene.calib, 3, 2, max_disp=K.MAX_DISP, init=first["rec"])
    got = ops.ego_motion(dev(fr["prev"]), dev(fr["cur"]), dev(fr["dpyr"]), scene.hw, scene.calib, 3, 2, max_disp=K.MAX_DISP, init=rec,
                         out={"rec": rec})
    same_bits(got["rec"], second["rec"], "in place")
    failed = first["rec"].copy()
    failed[OD.REC_STATUS] = 1.0
    want, _ = check_ego(scene, fr, "failed record", 3, 2, init=failed, init_dev=dev(failed))
    same_bits(want["rec"], first["rec"], "a failed record starts from the identity")


def test_failed_estimates():
    """a textureless previous image: no pixel, status 1, G all NaN, the start pose kept, later launches return at once"""
    scene = K.SCENES[0]
    fr = dict(K.frame(scene, "forward0.2m"))
    fr["prev"] = np.full_like(fr["prev"], 77)
    guess = C.translation(z=-C.BASELINE)                     # tau = -1 exactly: the record returns the pose to the bit
    want, got = check_ego(scene, fr, "textureless", init=guess)
    assert want["rec"][OD.REC_STATUS] == 1 and np.isnan(got["G"].cpu().numpy()).all() and not want["sums"].any()
    assert np.array_equal(want["rec"][:12].reshape(3, 4), guess[:3])


def test_operator_refusals():
    from dcanet_amd import ops
    scene = K.SCENES[0]
    fr = K.frame(scene, "identity")
    p, c, d = dev(fr["prev"]), dev(fr["cur"]), dev(fr["dpyr"])
    ok = dict(prev=p, cur=c, disp=d, hw=scene.hw, calib=scene.calib, levels=3)
    for bad in (dict(prev=p[:-1]), dict(cur=c.to(torch.int32)), dict(disp=d.double()), dict(disp=d.cpu()), dict(hw=(48, 76)), dict(levels=9),
                dict(iters=0), dict(huber=0.0), dict(max_disp=0.01), dict(init=np.eye(3)), dict(init=torch.zeros(5, device=DEV)),
                dict(outputs=("nope",)), dict(out={"rec": torch.zeros(24, device=DEV)}), dict(out={"x": p}),
                dict(workspace=torch.zeros(5, device=DEV, dtype=torch.int64))):
        kw = {**ok, **bad}
        with pytest.raises(RuntimeError, match="ego_motion"):
            ops.ego_motion(kw.pop("prev"), kw.pop("cur"), kw.pop("disp"), kw.pop("hw"), kw.pop("calib"), **kw)
    with pytest.raises(RuntimeError, match="grey_pyramid"):
        ops.grey_pyramid(dev(fr["rgb_prev"]), 7)
    with pytest.raises(RuntimeError, match="disp_pyramid"):
        ops.disp_pyramid(dev(fr["disp"]), 3, out=torch.zeros(3, device=DEV))


# ---- the reprojection with the matrix on the device -------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.cases(), ids=lambda c: c[0])
def test_reproject_with_a_device_matrix_is_the_by_value_route(case):
    """every scene and pose of _temporal_cases.py: every output and the workspace, bit for bit"""
    from dcanet_amd import ops
    name, scene, pose, Tw = case
    rng = np.random.default_rng(5)
    st = C.state(scene, rng, noise=0.3)
    st["age"] = np.where(st["disp"] > 0, rng.integers(0, 6, scene.hw), 0).astype(np.uint8)
    G = T.reproject_matrix(scene.calib, GEO.relative_pose(np.eye(4), Tw))
    H, W = scene.hw
    state = {k: dev(st[k]) for k in T.STATE_KEYS}
    ws_a, ws_b = (torch.full((H * W,), -1, device=DEV, dtype=torch.int64) for _ in range(2))
    by_value = ops.disp_reproject(state, G, calib=scene.calib, max_disp=C.MAX_DISP, workspace=ws_a)
    by_pointer = ops.disp_reproject(state, dev(G), calib=scene.calib, max_disp=C.MAX_DISP, workspace=ws_b)
    for k in T.REPROJECT_OUTPUTS:
        same_bits(by_pointer[k], by_value[k].cpu().numpy(), f"{name}: {k}")
    same_bits(ws_b, ws_a.cpu().numpy(), f"{name}: the keys")
    assert by_value["count"][0].item() > 1500


def test_a_nan_matrix_on_the_device_leaves_an_empty_prediction():
    """what a failed estimate hands on: nothing kept, count = (0, 0), and the fusion starts every pixel again; the estimate's own
    G goes from `ops.ego_motion` to `ops.disp_reproject` without the host seeing it and equals the host chain"""
    from dcanet_amd import ops
    scene = K.SCENES[1]
    st = C.state(scene)
    state = {k: dev(st[k]) for k in T.STATE_KEYS}
    for G in (np.full((3, 4), NAN, f32), np.where(np.eye(3, 4) > 0, NAN, 0).astype(f32)):     # (the second: a NaN in every row)
        got = ops.disp_reproject(state, dev(G), calib=scene.calib, max_disp=C.MAX_DISP)
        want = T.disp_reproject_host(st, np.full((3, 4), NAN, f32), calib=scene.calib, max_disp=C.MAX_DISP)
        for k in T.REPROJECT_OUTPUTS:
            same_bits(got[k], want[k], k)
        assert got["count"].tolist() == [0, 0] and not got["pred"].any() and not got["age"].any()
        fused = ops.temporal_fuse(got, state["disp"])
        assert not fused["age"].any() and torch.equal(fused["disp"], torch.where(state["disp"] >= T.TEMPORAL_MIN_DISP, state["disp"], 0))
    with pytest.raises(RuntimeError, match="disp_reproject"):
        ops.disp_reproject(state, np.full((3, 4), NAN, f32), calib=scene.calib)          # by value: still refused
    with pytest.raises(RuntimeError, match="disp_reproject"):
        ops.disp_reproject(state, torch.eye(4, device=DEV), calib=scene.calib)
    fr = K.frame(scene, "forward1m", 0.3)
    est = ops.ego_motion(dev(fr["prev"]), dev(fr["cur"]), dev(fr["dpyr"]), scene.hw, scene.calib, K.LEVELS, K.ITERS, max_disp=K.MAX_DISP)
    got = ops.disp_reproject(state, est["G"], calib=scene.calib, max_disp=C.MAX_DISP)
    host = OD.ego_motion_host(fr["prev"], fr["cur"], fr["dpyr"], scene.hw, scene.calib, K.LEVELS, K.ITERS, max_disp=K.MAX_DISP)
    want = T.disp_reproject_host(st, host["G"], calib=scene.calib, max_disp=C.MAX_DISP)
    for k in T.REPROJECT_OUTPUTS:
        same_bits(got[k], want[k], f"the chain: {k}")
    assert want["count"][0] > 1500


def test_a_megapixel_drives_the_sums_to_two_to_the_58_through_the_kernels_reduction():
    """1024 x 1024, the largest image the launcher takes, |gx| = |gy| = 255 at every pixel and one disparity just below max_disp:
    every workgroup's registers, cross-lane reduction, LDS and atomics at that magnitude; the first sum is 64 (255 * 254)^2
    (H - 2)(W - 2) = 2^57.96 (Python integers), and every sum equals the restatement's"""
    from dcanet_amd import ops
    H = W = 1024
    P = np.array([0, 0, 255, 255], np.uint8)
    I = np.ascontiguousarray(P[(np.arange(H)[:, None] + np.arange(W)[None, :]) % 4]).reshape(-1)
    D = np.full(H * W, 63.5, f32)
    calib = GEO.StereoCalib(700.0, 0.5, 511.5, 511.5)
    kw = dict(levels=1, iters=1, max_disp=64.0, huber=8.0)
    want = OD.ego_motion_host(I, I, D, (H, W), calib, **kw)
    got = ops.ego_motion(dev(I), dev(I), dev(D), (H, W), calib, outputs=OD.EGO_OUTPUTS, **kw)
    same_bits(got["sums"], want["sums"], "the sums")
    same_bits(got["rec"], want["rec"], "the record")
    n, q0 = (H - 2) * (W - 2), 255 * 254
    S = [int(v) for v in got["sums"][0].cpu().numpy()]
    assert S[28] == n and S[0] == S[1] == S[6] == 64 * q0 * q0 * n and S[0] > 1 << 57 and not any(S[21:28])
    assert max(abs(v) for v in S) < 1 << 62 and S[20] > 1 << 55                    # (S[20]: w q_5 q_5, both gradients)


# ---- the wrapper -------------------------------------------------------------------------------------------------------------------
WRAP = dict(crop_height=32, crop_width=64, graph=False)
EGO = dict(levels=2, iters=2, min_pixels=32)


def _sequence(seed, sizes):
    from _inference_cases import pairs
    return pairs(np.random.default_rng(seed), sizes)


def test_kitti_inference_odometry(monkeypatch):
    """five frames of 28 x 50 in the 32 x 64 frame, then two of 32 x 64: every frame against the operators run by hand AND
    against the host restatements fed with the network's measurement, bit for bit; the first frame of a size is
    KittiInferenceTemporal's first frame; one read-back of the documented size; the chained world pose is the product of the
    motions' inverses in the written order; reset() starts again; stream() gives the same bytes"""
    from _inference_cases import model as _model
    from dcanet_amd import ops
    from dcanet_amd.inference import FrameOdometry, KittiInference, KittiInferenceOdometry, KittiInferenceTemporal
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    model = _model()
    calib = GEO.StereoCalib(40.0, 0.5, 24.5, 13.5)
    sizes = [(28, 50)] * 5 + [(32, 64)] * 2
    pairs = _sequence(43, sizes)
    rk = dict(q=0.01, hint_min_age=1, max_disp=float(model.maxdisp), min_disp=0.0)
    fk = dict(meas_var=1.0, gate=4.0, min_disp=0.0)
    ek = dict(max_disp=float(model.maxdisp), min_disp=0.0, **EGO)
    plain = KittiInference(model, device_io=True, **WRAP)
    parent = KittiInferenceTemporal(model, calib, **rk, meas_var=1.0, gate=4.0, **WRAP)
    infer = KittiInferenceOdometry(model, calib, **rk, meas_var=1.0, gate=4.0, **EGO, **WRAP)
    copies = []
    readback = infer._readback
    monkeypatch.setattr(infer, "_readback", lambda s, copy: (copies.append(s.out_bytes), readback(s, copy))[1])
    single, state, last_hw, prev_pyr, dpyr, rec, world = [], None, None, None, None, None, None
    host_world, ok_frames = None, 0
    for i, (l, r) in enumerate(pairs):
        h, w = l.shape[:2]
        fresh = last_hw != (h, w)
        cur_pyr = ops.grey_pyramid(dev(l), EGO["levels"])
        same_bits(cur_pyr, OD.grey_pyramid_host(l, EGO["levels"]), f"frame {i}: the grey pyramid")
        pred = est = host_pred = host_est = None
        if fresh:
            world = torch.zeros(12, device=DEV, dtype=torch.float64)
        else:
            host_in = (prev_pyr.cpu().numpy(), cur_pyr.cpu().numpy(), dpyr.cpu().numpy(), (h, w), calib)
            host_est = OD.ego_motion_host(*host_in, init=None if rec is None else rec.cpu().numpy(), **ek)
            est = ops.ego_motion(prev_pyr, cur_pyr, dpyr, (h, w), calib, init=rec, **ek)
            same_bits(est["rec"], host_est["rec"], f"frame {i}: the record")
            same_bits(est["G"], host_est["G"], f"frame {i}: G")
            pred = ops.disp_reproject(state, est["G"], calib, **rk)
            host_pred = T.disp_reproject_host({k: v.cpu().numpy() for k, v in state.items()}, host_est["G"], calib, **rk)
        meas = plain(l, r)
        host_state = T.temporal_fuse_host(host_pred, meas, **fk)
        state = ops.temporal_fuse(pred, dev(meas), **fk)
        dpyr = ops.disp_pyramid(state["disp"], EGO["levels"], 0.0)
        same_bits(dpyr, OD.disp_pyramid_host(host_state["disp"], EGO["levels"], 0.0), f"frame {i}: the disparity pyramid")
        host_world, host_odo = OD.pose_chain_host(None if fresh else host_est["rec"], host_world)
        odo = ops.pose_chain(None if fresh else est["rec"], world)
        same_bits(odo, host_odo, f"frame {i}: the frame's doubles")
        before = len(copies)
        got = infer(l, r)
        assert len(copies) == before + 1 and copies[-1] == 8 * OD.FRAME_LEN + 9 * h * w, "one read-back of exactly the record's bytes"
        assert isinstance(got, FrameOdometry) and got.pose.shape == got.motion.shape == (4, 4) and got.pose.dtype == np.float64
        for k in T.STATE_KEYS:
            assert getattr(got, k).tobytes() == state[k].cpu().numpy().tobytes() == host_state[k].tobytes(), f"frame {i}: {k}"
        assert got.pose.tobytes() == host_odo[:16].tobytes() and got.motion.tobytes() == host_odo[16:32].tobytes(), f"frame {i}: pose"
        assert (got.count, got.residual, got.status) == (int(host_odo[32]), float(host_odo[33]), int(host_odo[34]))
        if fresh:
            first = parent(l, r, np.eye(4))
            parent.reset()
            assert all(getattr(got, k).tobytes() == getattr(first, k).tobytes() for k in T.STATE_KEYS), "a first frame is the parent's"
            assert np.array_equal(got.pose, np.eye(4)) and np.array_equal(got.motion, np.eye(4)) and got.count == 0 and not got.age.any()
        else:
            print(f"frame {i}: status {got.status}, count {got.count}, residual {got.residual:.1f}, |t| {np.linalg.norm(got.motion[:3, 3]):.3f}")
            assert got.count > 0
            ok_frames += got.status == 0
        single.append(got)
        rec = None if fresh else est["rec"]
        prev_pyr, last_hw = cur_pyr, (h, w)
    assert ok_frames >= 2, "the sequence holds estimates that succeeded"
    # the world pose: the product of the motions' inverses since the sequence started
    W = np.eye(4)
    for i, f in enumerate(single):
        W = np.eye(4) if i in (0, 5) else W @ np.linalg.inv(f.motion)
        assert np.abs(f.pose - W).max() < 1e-9 * max(1.0, np.abs(W).max()), f"frame {i}: the chained pose"
    infer.reset()
    again = infer(*pairs[0])
    assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(again, single[0])), "reset() starts the sequence again"
    infer.reset()
    streamed = list(infer.stream(pairs, depth=2))
    assert len(streamed) == len(single)
    for i, (a, b) in enumerate(zip(streamed, single)):
        assert all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b)), f"stream(), frame {i}"
    identity = KittiInferenceOdometry(model, calib, **rk, meas_var=1.0, gate=4.0, init="identity", **EGO, **WRAP)
    frames = [identity(l, r) for l, r in pairs[:3]]
    assert frames[1].motion.tobytes() == single[1].motion.tobytes(), "the second frame has no motion before it to start from"
    host_in = (OD.grey_pyramid_host(pairs[1][0], 2), OD.grey_pyramid_host(pairs[2][0], 2),
               OD.disp_pyramid_host(frames[1].disp, 2, 0.0), (28, 50), calib)
    assert frames[2].motion[:3].tobytes() == OD.ego_motion_host(*host_in, **ek)["rec"][:12].tobytes(), "init='identity'"


def test_kitti_inference_odometry_with_given_poses():
    """pose= overrides the estimate: disp, var and age are KittiInferenceTemporal's bit for bit for the same calls, the frame
    hands the given pose out, and an estimated frame behind it chains on from that pose"""
    from _inference_cases import model as _model
    from dcanet_amd.inference import KittiInferenceOdometry, KittiInferenceTemporal
    model = _model()
    calib = GEO.StereoCalib(40.0, 0.5, 24.5, 13.5)
    pairs = _sequence(47, [(28, 50)] * 4)
    poses = [C.translation(x=1.0, z=0.02 * i) @ C.yaw(0.3 * i) for i in range(3)]
    rk = dict(q=0.01, max_disp=float(model.maxdisp), min_disp=0.0, meas_var=1.0, gate=4.0)
    parent = KittiInferenceTemporal(model, calib, **rk, **WRAP)
    infer = KittiInferenceOdometry(model, calib, **rk, **EGO, **WRAP)
    for i, ((l, r), pose) in enumerate(zip(pairs, poses)):
        want, got = parent(l, r, pose), infer(l, r, pose=pose)
        assert all(getattr(got, k).tobytes() == getattr(want, k).tobytes() for k in T.STATE_KEYS), f"frame {i}"
        assert np.array_equal(got.pose, pose) and got.status == 0 and got.count == 0
        assert np.array_equal(got.motion, np.eye(4) if i == 0 else GEO.relative_pose(poses[i - 1], pose))
    assert (got.age > 0).sum() > 100, "the given poses carry a state"
    nxt = infer(*pairs[3])
    assert nxt.count > 0
    if nxt.status == 0:
        assert np.abs(nxt.pose - poses[2] @ np.linalg.inv(nxt.motion)).max() < 1e-9
    else:
        assert np.array_equal(nxt.pose, poses[2])
    streamed = list(KittiInferenceOdometry(model, calib, **rk, **EGO, **WRAP).stream(
        [(l, r, p) for (l, r), p in zip(pairs, poses)] + [pairs[3]]))
    assert all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(streamed[3], nxt)), "stream() with a third item"


def test_kitti_inference_odometry_refusals():
    from _inference_cases import model as _model
    from dcanet_amd.inference import KittiInferenceOdometry
    model, calib = _model(), GEO.StereoCalib(40.0, 0.5, 24.5, 13.5)
    for bad in (dict(calib=None), dict(device_io=False), dict(init="first"), dict(levels=0), dict(levels=9), dict(iters=0), dict(huber=0.0),
                dict(grad_min=600), dict(min_pixels=2), dict(min_ratio=0.0)):
        with pytest.raises((ValueError, RuntimeError, TypeError)):
            KittiInferenceOdometry(model, **{**dict(calib=calib), **WRAP, **bad})
    infer = KittiInferenceOdometry(model, calib, levels=6, **WRAP)
    l = np.zeros((28, 50, 3), np.uint8)
    with pytest.raises(ValueError, match="coarsest"):
        infer(l, l)                                          # 28 >> 5 = 0
    with pytest.raises(ValueError):
        infer(l, l, pose=np.eye(3))
