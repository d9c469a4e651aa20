"""CPU checks of temporal stereo: the numpy restatements of dcanet_amd/temporal.py against an independent per-pixel Python loop
(bit for bit, the tie rule included), against the TRUTH of synthetic scenes re-rendered at the new pose (tests/_temporal_cases.py)
and against closed forms; the matrix of the ego-motion, the pose readers, the operators' refusals, and the host check of
csrc/temporal_math.h under sanitizers.  The kernels are compared with the restatement, bit for bit, in test_gpu_temporal.py."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import _temporal_cases as C
from dcanet_amd import geometry as GEO
from dcanet_amd import temporal as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _G(scene, T_world_cur, T_world_prev=None):
    return T.reproject_matrix(scene.calib, GEO.relative_pose(np.eye(4) if T_world_prev is None else T_world_prev, T_world_cur))


# ---- the independent loop: one pixel at a time, numpy float32 scalars, one operation at a time ---------------------------------
def reproject_loop(state, G, doffs, max_disp, min_disp, min_ratio, occl, q, hint_min_age, mask=None, mask_min=0.5):
    d, var, age = state["disp"], state["var"], state["age"]
    H, W = d.shape
    g = [f32(x) for x in np.asarray(G, f32).reshape(-1)]
    doffs, max_disp, min_disp, min_ratio, q = f32(doffs), f32(max_disp), f32(min_disp), f32(min_ratio), f32(q)
    rx, ry, occl_px = occl[0], occl[1], f32(occl[2])

    def ratio(u, v, den):
        return ((g[8] * f32(u) + g[9] * f32(v)) + g[10]) + g[11] * den

    best = {}                                              # target -> (den', source index): nearest, then the smallest index
    kept = 0
    with np.errstate(all="ignore"):
        for v in range(H):
            for u in range(W):
                dd = d[v, u]
                if not (np.isfinite(dd) and dd >= min_disp) or (mask is not None and not mask[v, u] >= f32(mask_min)):
                    continue
                den = dd + doffs
                x = ((g[0] * f32(u) + g[1] * f32(v)) + g[2]) + g[3] * den
                y = ((g[4] * f32(u) + g[5] * f32(v)) + g[6]) + g[7] * den
                z = ratio(u, v, den)
                uf, vf = np.floor(x / z + f32(0.5)), np.floor(y / z + f32(0.5))
                dn = den / z
                dp = dn - doffs
                if not (z >= min_ratio and 0 <= uf < W and 0 <= vf < H and dp >= min_disp and dp < max_disp):
                    continue
                kept += 1
                tgt, src = int(vf) * W + int(uf), v * W + u
                if tgt not in best or dn > best[tgt][0] or (dn == best[tgt][0] and src < best[tgt][1]):
                    best[tgt] = (dn, src)
        pred, pvar = np.zeros((H, W), f32), np.zeros((H, W), f32)
        page, hints = np.zeros((H, W), np.uint8), np.zeros((H, W), f32)
        visible = 0
        for tgt, (dn, src) in best.items():
            r, c = divmod(tgt, W)
            denmax = max(best.get(rr * W + cc, (f32(0), 0))[0] for rr in range(max(r - ry, 0), min(r + ry, H - 1) + 1)
                         for cc in range(max(c - rx, 0), min(c + rx, W - 1) + 1))
            if not dn + occl_px >= denmax:
                continue
            visible += 1
            sv, su = divmod(src, W)
            z = ratio(su, sv, d[sv, su] + doffs)
            pred[r, c] = dn - doffs
            pvar[r, c] = var[sv, su] / (z * z) + q
            page[r, c] = min(int(age[sv, su]) + 1, 255)
            hints[r, c] = pred[r, c] if page[r, c] >= hint_min_age else f32(0)
    return {"pred": pred, "var": pvar, "age": page, "hints": hints, "count": np.array([visible, kept], np.int64)}


def fuse_loop(pred, meas, vm, y0, rows, cols, mask, mask_min, min_disp, gate2, var_max):
    out = {k: np.zeros((rows, cols), np.uint8 if k == "age" else f32) for k in T.FUSE_OUTPUTS}
    gate2, var_max = f32(gate2), f32(var_max)
    with np.errstate(all="ignore"):
        for r in range(rows):
            for c in range(cols):
                m = meas[y0 + r, c]
                v = vm[y0 + r, c] if isinstance(vm, np.ndarray) else f32(vm)
                m_ok = bool(np.isfinite(m) and m >= f32(min_disp) and (mask is None or mask[y0 + r, c] >= f32(mask_min))
                            and v > 0 and v < np.inf)
                p_ok = pred is not None and bool(pred["pred"][r, c] > 0 and pred["var"][r, c] >= 0 and pred["var"][r, c] <= var_max)
                if m_ok and p_ok:
                    p, pv = pred["pred"][r, c], pred["var"][r, c]
                    e, s = m - p, pv + v
                    out["innov"][r, c] = abs(e)
                    if e * e <= gate2 * s:
                        k = pv / s
                        res = (p + k * e, pv - k * pv, pred["age"][r, c])
                    else:
                        res = (m, v, 0)
                elif m_ok:
                    res = (m, v, 0)
                elif p_ok:
                    res = (pred["pred"][r, c], pred["var"][r, c], pred["age"][r, c])
                else:
                    continue
                out["disp"][r, c], out["var"][r, c], out["age"][r, c] = res
    return out


def same_bits(got, want, name):
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
    bits = np.uint32 if got.dtype.kind == "f" else got.dtype
    bad = np.nonzero(got.view(bits) != want.view(bits))
    assert len(bad[0]) == 0, f"{name}: {len(bad[0])} elements differ, first at {[int(i[0]) for i in bad]}: " \
                             f"{got[bad][0]!r} != {want[bad][0]!r}"


KW = dict(max_disp=C.MAX_DISP, min_disp=T.TEMPORAL_MIN_DISP, min_ratio=T.TEMPORAL_MIN_RATIO, q=0.01, hint_min_age=3)


@pytest.mark.parametrize("pose", [n for n, _ in C.POSES])
def test_reproject_restatement_is_the_per_pixel_loop_bit_for_bit(pose):
    """the smallest scene under every pose, ages 0 .. 5 so that hint_min_age = 3 splits the hints, a mask, q > 0"""
    s = C.SCENES[0]
    rng = np.random.default_rng(5)
    st = C.state(s, rng, noise=0.3)
    st["age"] = np.where(st["disp"] > 0, rng.integers(0, 6, s.hw), 0).astype(np.uint8)
    st["var"] = (st["var"] * rng.uniform(0.5, 2.0, s.hw)).astype(f32)
    mask = rng.uniform(0, 1, s.hw).astype(f32)
    G = _G(s, dict(C.POSES)[pose])
    for occl, m in (((1, 1, 1.0), None), ((0, 0, 0.0), None), ((2, 1, 0.5), mask)):
        got = T.disp_reproject_host(st, G, calib=s.calib, occl=occl, mask=m, mask_min=0.2, **KW)
        want = reproject_loop(st, G, s.calib.doffs, occl=occl, mask=m, mask_min=0.2, **KW)
        for k in T.REPROJECT_OUTPUTS:
            same_bits(got[k], want[k], f"{pose} occl {occl} {k}")
        assert got["count"][0] == (got["pred"] > 0).sum() > 500


def test_reproject_tie_goes_to_the_smallest_source_index():
    """a wall of ONE disparity under minification (G halves the coordinates, z = 1): four sources per target with the same den';
    the winner is the smallest source index, in the restatement and in the loop, and its payload shows which one it was"""
    H, W = 12, 20
    st = {"disp": np.full((H, W), 7.0, f32), "var": np.arange(H * W, dtype=f32).reshape(H, W) + 1,
          "age": (np.arange(H * W) % 200).astype(np.uint8).reshape(H, W)}
    G = np.array([[0.5, 0, 0, 0], [0, 0.5, 0, 0], [0, 0, 1, 0]], f32)
    got = T.disp_reproject_host(st, G, doffs=0.0, occl=(0, 0, 0.0), **{**KW, "q": 0.0})
    want = reproject_loop(st, G, 0.0, occl=(0, 0, 0.0), **{**KW, "q": 0.0})
    for k in T.REPROJECT_OUTPUTS:
        same_bits(got[k], want[k], k)
    # floor(u / 2 + 0.5): target column c collects the source columns 2c - 1 and 2c, target row r the rows 2r - 1 and 2r
    for r in range(H // 2 + 1):
        for c in range(W // 2 + 1):
            src = max(2 * r - 1, 0) * W + max(2 * c - 1, 0)
            if max(2 * r - 1, 0) < H and max(2 * c - 1, 0) < W:
                assert got["var"][r, c] == f32(src + 1), (r, c)
    assert got["count"].tolist() == [(H // 2 + 1) * (W // 2 + 1), H * W]


def test_fuse_restatement_is_the_per_pixel_loop_bit_for_bit():
    """every row of the table in one map: random validity of either side, innovations on both sides of the gate, a variance
    map with zeros and infinities, a mask, var_max, a window at row 5 of a padded frame"""
    rng = np.random.default_rng(11)
    rows, cols, Hc, Wc, y0 = 37, 50, 48, 64, 5
    p = rng.uniform(1, 40, (rows, cols)).astype(f32)
    pred = {"pred": np.where(rng.uniform(size=p.shape) < 0.8, p, 0).astype(f32),
            "var": rng.uniform(0.01, 2.0, p.shape).astype(f32), "age": rng.integers(0, 256, p.shape).astype(np.uint8)}
    meas = np.full((Hc, Wc), np.nan, f32)
    meas[y0:y0 + rows, :cols] = p + rng.normal(0, 1.5, p.shape)
    bad = rng.uniform(size=meas.shape)
    meas[bad < 0.05], meas[(bad > 0.05) & (bad < 0.1)], meas[(bad > 0.1) & (bad < 0.15)] = np.nan, 0.0, np.inf
    vmap = rng.uniform(0.05, 1.0, meas.shape).astype(f32)
    vmap[rng.uniform(size=meas.shape) < 0.05], vmap[rng.uniform(size=meas.shape) < 0.03] = 0.0, np.inf
    mask = rng.uniform(size=meas.shape).astype(f32)
    for vm, m, gate, var_max in ((0.25, None, 3.0, math.inf), (vmap, mask, 1.0, 1.0), (0.5, mask, math.inf, 0.5), (vmap, None, 0.0, math.inf)):
        got = T.temporal_fuse_host(pred, meas, vm, window=(y0, rows, cols), mask=m, mask_min=0.3, gate=gate, var_max=var_max,
                                   outputs=T.FUSE_OUTPUTS)
        want = fuse_loop(pred, meas, vm, y0, rows, cols, m, 0.3, T.TEMPORAL_MIN_DISP, f32(gate * gate), var_max)
        for k in T.FUSE_OUTPUTS:
            same_bits(got[k], want[k], f"gate {gate} {k}")
    first = T.temporal_fuse_host(None, meas, 0.25, window=(y0, rows, cols), outputs=T.FUSE_OUTPUTS)
    want = fuse_loop(None, meas, 0.25, y0, rows, cols, None, 0.5, T.TEMPORAL_MIN_DISP, 9.0, math.inf)
    for k in T.FUSE_OUTPUTS:
        same_bits(first[k], want[k], f"no prediction {k}")
    assert not first["age"].any() and not first["innov"].any()


def test_fuse_gate_at_equality_and_scalar_against_map():
    """e e == gate2 s exactly passes; a constant variance map gives the scalar's bits"""
    pred = {"pred": np.array([[4.0, 4.0]], f32), "var": np.array([[0.5, 0.5]], f32), "age": np.array([[7, 7]], np.uint8)}
    meas = np.array([[7.0, np.nextafter(f32(7.0), f32(8.0))]], f32)
    r = T.temporal_fuse_host(pred, meas, 0.5, gate=3.0, outputs=T.FUSE_OUTPUTS)
    assert r["disp"].tolist() == [[5.5, float(meas[0, 1])]] and r["var"].tolist() == [[0.25, 0.5]] and r["age"].tolist() == [[7, 0]]
    rm = T.temporal_fuse_host(pred, meas, np.full((1, 2), 0.5, f32), gate=3.0, outputs=T.FUSE_OUTPUTS)
    assert all(r[k].tobytes() == rm[k].tobytes() for k in T.FUSE_OUTPUTS)


# ---- the matrix and the poses ------------------------------------------------------------------------------------------------
def test_reproject_matrix_identity_is_exact_and_moves_agree_with_backprojection():
    for s in C.SCENES:
        assert T.reproject_matrix(s.calib, np.eye(4)).tobytes() == np.eye(3, 4, dtype=f32).tobytes()
    rng = np.random.default_rng(3)
    calib = GEO.StereoCalib(721.5377, 0.5372, 609.5593, 172.854, 3.25)
    Tm = C.yaw(3.0) @ C.pitch(-2.0) @ C.translation(0.2, -0.05, -1.3)
    # G itself in float64, before its one rounding: the restated formula, then back-project -> transform -> project
    K = np.array([[calib.f, 0, calib.cx], [0, calib.f, calib.cy], [0, 0, 1]])
    A = np.array([[1, 0, -calib.cx], [0, 1, -calib.cy], [0, 0, calib.f]])
    G64 = np.hstack([K @ Tm[:3, :3] @ A, (K @ Tm[:3, 3:] / calib.baseline)]) / calib.f
    G32 = T.reproject_matrix(calib, Tm)
    assert np.abs(G32 - G64).max() <= np.abs(G64).max() * 2.0 ** -24
    for _ in range(200):
        u, v, d = rng.uniform(0, 1242), rng.uniform(0, 375), rng.uniform(1, 100)
        Z = calib.f * calib.baseline / (d + calib.doffs)
        P = Tm @ np.array([(u - calib.cx) * Z / calib.f, (v - calib.cy) * Z / calib.f, Z, 1.0])
        want = (calib.f * P[0] / P[2] + calib.cx, calib.f * P[1] / P[2] + calib.cy, calib.f * calib.baseline / P[2], P[2] / Z)
        x, y, z = G64 @ np.array([u, v, 1.0, d + calib.doffs])
        got = (x / z, y / z, (d + calib.doffs) / z, z)
        assert np.allclose(got, want, rtol=0, atol=1e-9), (got, want)
    for bad in (np.eye(3), np.full((4, 4), np.nan), "x"):
        with pytest.raises((ValueError, TypeError)):
            T.reproject_matrix(calib, bad)
    with pytest.raises(ValueError):
        T.reproject_matrix(object(), np.eye(4))


def test_relative_pose_and_kitti_poses_round_trip(tmp_path):
    A, B = C.yaw(10.0) @ C.translation(1, 2, 3), C.pitch(-4.0) @ C.translation(-2, 0.5, 7) @ C.yaw(33.0)
    rel = GEO.relative_pose(A, B)
    assert np.allclose(B @ rel, A, atol=1e-12) and np.allclose(GEO.relative_pose(A, A), np.eye(4), atol=1e-15)
    assert np.allclose(GEO.relative_pose(A[:3], B[:3]), rel, atol=0)
    poses = np.stack([np.eye(4), A, B])
    path = tmp_path / "00.txt"
    path.write_text("\n".join(" ".join(repr(float(x)) for x in P[:3].reshape(-1)) for P in poses) + "\n")
    got = GEO.read_kitti_poses(str(path))
    assert got.shape == (3, 4, 4) and got.tobytes() == poses.tobytes()
    assert GEO.read_kitti_poses(path.read_text()).tobytes() == poses.tobytes()
    # the colour camera lies 0.06 m to the right of cam0: P2[0,3] = -f * 0.06
    calib = "P0: 700 0 600 0 0 700 180 0 0 0 1 0\nP2: 700 0 600 -42 0 700 180 0 0 0 1 0\nP3: 700 0 600 -420 0 700 180 0 0 0 1 0\n"
    moved = GEO.read_kitti_poses(str(path), calib)
    S = C.translation(x=-0.06)
    assert np.allclose(moved, S @ poses @ np.linalg.inv(S), atol=1e-12) and np.array_equal(moved[0], np.eye(4))
    # a point seen by cam2 at time 1, carried to time 2: through cam0's poses and the offset, or through the moved poses
    p2 = np.array([0.3, -0.2, 9.0, 1.0])
    via0 = S @ GEO.relative_pose(poses[1], poses[2]) @ np.linalg.inv(S) @ p2
    assert np.allclose(GEO.relative_pose(moved[1], moved[2]) @ p2, via0, atol=1e-12)
    for bad in ("1 2 3\n", "a b c d e f g h i j k l\n", ""):
        with pytest.raises(ValueError):
            GEO.read_kitti_poses(bad + "\n")


def test_oxts_poses_of_a_straight_level_drive():
    """heading east along the equator-side parallel of the first latitude, level: the IMU moves along its own x axis by the
    Mercator easting, scale * r * dlon; with the camera looking along the IMU's x (KITTI's axes: camera z = IMU x, camera
    x = -IMU y, camera y = -IMU z) the camera moves along +z by that distance -- to 1e-6 m -- and does not turn"""
    lat0, n, step = 49.0, 6, 1.25                                            # metres per frame
    r = GEO.EARTH_RADIUS
    dlon = np.degrees(step / r)                                              # easting = scale * r * dlon_rad with scale = cos(lat0)
    rows = np.array([[lat0, 8.4 + i * dlon / math.cos(math.radians(lat0)), 112.0, 0.0, 0.0, 0.0] for i in range(n)])
    imu_to_velo = C.translation(-0.81, 0.32, -0.8)
    velo_to_cam = np.array([[0.0, -1, 0, 0.05], [0, 0, -1, -0.07], [1, 0, 0, -0.27], [0, 0, 0, 1]])
    poses = GEO.oxts_poses(rows, imu_to_velo, velo_to_cam, np.eye(3))
    assert poses.shape == (n, 4, 4) and np.abs(poses[0] - np.eye(4)).max() < 1e-12
    for i in range(n):
        assert np.abs(poses[i][:3, :3] - np.eye(3)).max() < 1e-12
        assert np.abs(poses[i][:3, 3] - np.array([0.0, 0.0, i * step])).max() < 1e-6, poses[i][:3, 3]
    # a yaw of 90 degrees (heading north) turns the camera about its y axis; the lever arm moves the camera's origin
    turned = GEO.oxts_poses(np.array([rows[0], [*rows[0][:5], math.pi / 2]]), imu_to_velo, velo_to_cam, np.eye(3))[1]
    assert np.allclose(turned[:3, :3], C.yaw(-90.0)[:3, :3], atol=1e-12)
    for bad in (rows[:, :5], np.zeros((0, 6)), np.full((2, 6), np.nan)):
        with pytest.raises(ValueError):
            GEO.oxts_poses(bad, imu_to_velo, velo_to_cam, np.eye(3))


# ---- the restatement against the truth -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", C.SCENES[1:], ids=lambda s: s.name)
def test_forward_one_metre_against_the_rerendered_scene(scene):
    """1 m forward with the default occlusion window (1, 1, 1.0): at least 0.7 of the target pixels are filled, and at most
    0.5 % of the filled ones are more than 1 px from the scene re-rendered at the new pose.  Measured: 53x131 0.774 filled,
    0.24 % off; 40x160 0.807 filled, 0.21 % off (window off: 0.41 % and 0.23 %)."""
    Tw = dict(C.POSES)["forward1m"]
    truth = C.render(scene, Tw)
    st = C.state(scene)
    shares = {}
    for occl in ((1, 1, 1.0), (0, 0, 1.0)):
        r = T.disp_reproject_host(st, _G(scene, Tw), calib=scene.calib, max_disp=C.MAX_DISP, occl=occl)
        filled = r["pred"] > 0
        shares[occl[:2]] = (filled.mean(), (np.abs(r["pred"] - truth)[filled] > 1.0).mean())
        print(f"{scene.name} forward 1 m, occl {occl}: filled {shares[occl[:2]][0]:.4f}, more than 1 px off {100 * shares[occl[:2]][1]:.3f} %")
        assert (r["age"][filled] == 2).all() and not r["age"][~filled].any() and not r["var"][~filled].any()
    assert shares[(1, 1)][0] >= 0.7 and shares[(1, 1)][1] <= 0.005
    assert shares[(1, 1)][1] <= shares[(0, 0)][1], "the window removes wrong pixels, it adds none"


def test_eight_noisy_frames_average_the_noise_down():
    """eight frames 0.5 m apart, 0.5 px Gaussian noise on every measurement, gate 3 sigma: at the pixels of age >= 3 the fused
    map's rms error against the truth is at most 0.65 of the single frame's there (four equal measurements: 0.5 in theory;
    the margin covers occlusion edges)"""
    scene, sigma = C.SCENES[2], 0.5
    rng = np.random.default_rng(2024)
    state, prev, ratios = None, None, []
    for i in range(8):
        Tw = C.translation(z=0.5 * i)
        truth = C.render(scene, Tw)
        meas = np.where(truth > 0, truth + rng.normal(0, sigma, truth.shape), 0).astype(f32)
        pred = None
        if state is not None:
            pred = T.disp_reproject_host(state, _G(scene, Tw, prev), calib=scene.calib, max_disp=C.MAX_DISP)
        state = T.temporal_fuse_host(pred, meas, sigma * sigma, gate=3.0)
        prev = Tw
        old = state["age"] >= 3
        if old.sum() > 500:
            fused = math.sqrt(np.mean((state["disp"][old] - truth[old]) ** 2))
            single = math.sqrt(np.mean((meas[old] - truth[old]) ** 2))
            ratios.append(fused / single)
            print(f"frame {i}: {int(old.sum())} pixels of age >= 3, fused rms {fused:.4f} px, single frame {single:.4f} px, ratio "
                  f"{fused / single:.3f}, mean variance {state['var'][old].mean():.4f}")
    assert len(ratios) >= 4 and max(ratios) <= 0.65


def test_static_scene_variance_is_vm_over_n():
    """identity pose, gate off, q = 0, no occlusion window: after n frames every pixel's variance is vm / n to 1e-5 relative and
    its age n - 1, and the disparity is the mean of the measurements"""
    scene, vm = C.SCENES[0], 0.37
    rng = np.random.default_rng(8)
    truth = C.render(scene)
    G = T.reproject_matrix(scene.calib, np.eye(4))
    state, total = None, np.zeros(truth.shape)
    for n in range(1, 9):
        meas = (truth + rng.normal(0, 0.2, truth.shape)).astype(f32)       # (the backdrop is 1.3 px: every pixel stays valid)
        total += meas
        pred = None if state is None else T.disp_reproject_host(state, G, calib=scene.calib, max_disp=C.MAX_DISP, occl=(0, 0, 0.0))
        state = T.temporal_fuse_host(pred, meas, vm, gate=math.inf)
        assert np.abs(state["var"] / f32(vm / n) - 1).max() <= 1e-5, n
        assert (state["age"] == n - 1).all()
        assert np.abs(state["disp"] - total / n).max() <= 1e-4


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_validators_refuse_what_the_header_refuses():
    nan, inf = float("nan"), float("inf")
    ok = dict(H=10, W=12, G=np.eye(3, 4), doffs=0.0, min_disp=0.0625, max_disp=64.0, min_ratio=0.125, occl=(1, 1, 1.0), q=0.0,
              hint_min_age=1)
    assert T.reproject_scalars("x", ValueError, **ok)[0] == [float(v) for v in np.eye(3, 4).reshape(-1)]
    bad_g = np.eye(3, 4)
    bad_g[1, 2] = inf
    for bad in (dict(G=bad_g), dict(G=np.eye(4)), dict(G=np.eye(3, 4) * 1e300), dict(occl=(9, 0, 1.0)), dict(occl=(0, -1, 1.0)),
                dict(occl=(1.5, 1, 1.0)), dict(occl=(1, 1)), dict(occl=(1, 1, -0.5)), dict(occl=(1, 1, nan)), dict(occl=(1, 1, inf)),
                dict(q=-1.0), dict(q=inf), dict(q=nan), dict(min_ratio=-0.1), dict(min_ratio=nan), dict(min_ratio=inf),
                dict(max_disp=0.01), dict(max_disp=inf), dict(min_disp=-1.0), dict(min_disp=nan), dict(doffs=-1.0), dict(doffs=nan),
                dict(H=1 << 16, W=1 << 15), dict(H=0), dict(hint_min_age=256), dict(hint_min_age=-1), dict(hint_min_age=1.5)):
        with pytest.raises(ValueError, match="^x:"):
            T.reproject_scalars("x", ValueError, **{**ok, **bad})
    assert T.fuse_scalars("y", ValueError, 0.25, 0.0625, 3.0, inf) == (0.25, 0.0625, 9.0, inf)
    assert T.fuse_scalars("y", ValueError, None, 0.0, inf, 2.0) == (None, 0.0, inf, 2.0)
    for bad in ((0.0, 0.0625, 3.0, inf), (-1.0, 0.0625, 3.0, inf), (inf, 0.0625, 3.0, inf), (nan, 0.0625, 3.0, inf),
                (0.25, -1.0, 3.0, inf), (0.25, nan, 3.0, inf), (0.25, 0.0625, -1.0, inf), (0.25, 0.0625, nan, inf),
                (0.25, 0.0625, 3.0, -1.0), (0.25, 0.0625, 3.0, nan)):
        with pytest.raises(ValueError, match="^y:"):
            T.fuse_scalars("y", ValueError, *bad)
    st = C.state(C.SCENES[0])
    G = np.eye(3, 4, dtype=f32)
    for bad in (dict(state={"disp": st["disp"]}), dict(state={**st, "age": st["age"].astype(np.int32)}),
                dict(state={**st, "var": st["var"][:-1]}), dict(outputs=("nope",)), dict(outputs=()), dict(mask=st["disp"][:-1]),
                dict(mask=st["disp"], mask_min=nan), dict(calib=None), dict(doffs=0.0)):
        kw = {**dict(state=st, calib=C.SCENES[0].calib), **bad}
        with pytest.raises(ValueError, match="disp_reproject_host"):
            T.disp_reproject_host(kw.pop("state"), G, **kw)
    meas = st["disp"]
    pred = T.disp_reproject_host(st, G, calib=C.SCENES[0].calib)
    for bad in (dict(meas=meas.astype(np.float64)), dict(meas=np.stack([meas, meas])), dict(window=(0, 49, 75)), dict(window=(1, 48, 75)),
                dict(meas_var=meas[:-1]), dict(mask=meas[:-1]), dict(outputs=("pred",)), dict(pred={"pred": meas}),
                dict(window=(0, 40, 75))):
        kw = {**dict(pred=pred, meas=meas), **bad}
        with pytest.raises(ValueError, match="temporal_fuse_host"):
            T.temporal_fuse_host(kw.pop("pred"), kw.pop("meas"), **kw)


def test_operators_refuse_cpu_tensors_and_the_library_exports_the_entry_points():
    import torch
    from dcanet_amd import _lib, ops
    for fn in ("dca_disp_reproject", "dca_temporal_fuse"):
        assert fn in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["dca_disp_reproject"][1]) == 35 and len(_lib.SIGNATURES["dca_temporal_fuse"][1]) == 21
    assert _lib.CONSTANTS["DCA_TEMPORAL_MAX_RADIUS"] == T.MAX_RADIUS and _lib.ABI_VERSION == 21
    st = {k: torch.from_numpy(v) for k, v in C.state(C.SCENES[0]).items()}
    with pytest.raises(RuntimeError, match="disp_reproject.*ROCm"):
        ops.disp_reproject(st, np.eye(3, 4), doffs=0.0)
    with pytest.raises(RuntimeError, match="temporal_fuse.*ROCm"):
        ops.temporal_fuse(None, st["disp"], 0.25)
    assert ops.disp_reproject is T.disp_reproject and ops.temporal_fuse is T.temporal_fuse and ops.temporal_workspace is T.temporal_workspace


def test_temporal_math_host_check_under_sanitizers(tmp_path):
    """tools/temporal_math_check.cpp: the projection, the keep test, the key and the fusion of csrc/temporal_math.h, compiled for
    the host with AddressSanitizer and UBSan as a stand-alone program, exits 0"""
    cxx = next((c for c in (shutil.which("clang++"), "/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++",
                            shutil.which("g++")) if c and os.path.exists(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "temporal_check")
    csrc = os.path.join(ROOT, "cost-volume-aggregation-in-stereo-matching-revisited_amd", "csrc")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc,
           os.path.join(ROOT, "tools", "temporal_math_check.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok"), run.stdout[-2000:] + run.stderr[-2000:]
