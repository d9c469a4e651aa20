"""Temporal stereo on the MI355X (csrc/temporal.hip): `ops.disp_reproject` and `ops.temporal_fuse` bit for bit against the numpy
restatements of dcanet_amd/temporal.py on the scenes and poses of tests/_temporal_cases.py, a sequence of both, selective
outputs, the operators' refusals, and the way through inference.KittiInferenceTemporal.

Why bitwise, without any tolerance: every float32 formula is a chain of single operations (+ - x / floor), each correctly
rounded on the device (contraction off, IEEE division) and in numpy alike; the scatter is a 64-bit INTEGER maximum over keys
that are unique per source pixel, so the winner does not depend on the order of arrival; the counts are integer sums."""
import numpy as np
import pytest
import torch

import _temporal_cases as C
from _inference_cases import model as _model, pairs as _pairs
from dcanet_amd import geometry as GEO
from dcanet_amd import temporal as T

pytestmark = pytest.mark.gpu
DEV = "cuda"
f32 = np.float32
NAN, INF = float("nan"), float("inf")


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)         # (a copy: the cases are read-only)


def dev_state(st):
    return {k: dev(st[k]) for k in T.STATE_KEYS}


def same_bits(got, want, name):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
    bits = np.uint32 if got.dtype.kind == "f" else got.dtype
    bad = np.nonzero(got.view(bits) != want.view(bits))
    assert len(bad[0]) == 0, f"{name}: {len(bad[0])} elements differ, first at {[int(i[0]) for i in bad]}: " \
                             f"{got[bad][0]!r} != {want[bad][0]!r}"


def _G(scene, T_world_cur, T_world_prev=None):
    return T.reproject_matrix(scene.calib, GEO.relative_pose(np.eye(4) if T_world_prev is None else T_world_prev, T_world_cur))


def garbage(H, W):
    """a workspace and output buffers that start as garbage: the operator clears what it accumulates in and writes every pixel"""
    out = {"pred": torch.full((H, W), NAN, device=DEV), "var": torch.full((H, W), -3.0, device=DEV),
           "age": torch.full((H, W), 201, device=DEV, dtype=torch.uint8), "hints": torch.full((H, W), INF, device=DEV),
           "count": torch.full((2,), -5, device=DEV, dtype=torch.int64)}
    ws = torch.full((H * W,), -1, device=DEV, dtype=torch.int64)                # all ones: above every key
    return out, ws


def check_reproject(st, G, name, mask=None, **kw):
    """`ops.disp_reproject` into garbage against the restatement, every output and the workspace; a second call, the same bits"""
    from dcanet_amd import ops
    want = T.disp_reproject_host(st, G, mask=mask, **kw)
    H, W = st["disp"].shape
    out, ws = garbage(H, W)
    got = ops.disp_reproject(dev_state(st), G, mask=dev(mask), out=out, workspace=ws, **kw)
    assert set(got) == set(T.REPROJECT_OUTPUTS) and all(got[k] is out[k] for k in got)
    for k in T.REPROJECT_OUTPUTS:
        same_bits(got[k], want[k], f"{name}: {k}")
    same_bits(ws.cpu().numpy().view(np.uint64).reshape(H, W), want["keys"], f"{name}: the keys")
    again = ops.disp_reproject(dev_state(st), G, mask=dev(mask), **kw)
    for k in T.REPROJECT_OUTPUTS:
        same_bits(again[k], want[k], f"{name}: {k}, second call")
    return want


def rich_state(scene, seed, T_world_cam=None):
    """noisy disparity, a variance and an age per pixel"""
    rng = np.random.default_rng(seed)
    st = C.state(scene, rng, noise=0.3, T_world_cam=T_world_cam)
    st["age"] = np.where(st["disp"] > 0, rng.integers(0, 6, scene.hw), 0).astype(np.uint8)
    st["var"] = (st["var"] * rng.uniform(0.5, 2.0, scene.hw)).astype(f32)
    return st


@pytest.mark.parametrize("case", C.cases(), ids=lambda c: c[0])
def test_reproject_is_the_restatement_bit_for_bit(case):
    """every scene under every pose, defaults (occlusion window (1, 1, 1.0)); the count is exact"""
    name, scene, pose, Tw = case
    want = check_reproject(rich_state(scene, 5), _G(scene, Tw), name, calib=scene.calib, max_disp=C.MAX_DISP)
    print(f"{name}: {want['count'][1]} sources kept, {want['count'][0]} targets visible of {scene.hw[0] * scene.hw[1]}")
    assert want["count"][0] == (want["pred"] > 0).sum() > 1500 and want["count"][1] >= want["count"][0]


def test_reproject_identity_without_window_returns_the_state():
    from dcanet_amd import ops
    scene = C.SCENES[1]
    st = rich_state(scene, 9)
    got = ops.disp_reproject(dev_state(st), T.reproject_matrix(scene.calib, np.eye(4)), scene.calib, max_disp=C.MAX_DISP,
                             occl=(0, 0, 0.0), hint_min_age=0)
    valid = st["disp"] >= f32(T.TEMPORAL_MIN_DISP)
    assert valid.sum() > 6000
    for k, src in (("pred", "disp"), ("var", "var"), ("hints", "disp")):
        same_bits(np.where(valid, got[k].cpu().numpy(), 0), np.where(valid, st[src], 0).astype(f32), k)
    same_bits(got["age"].cpu().numpy(), np.where(valid, st["age"] + 1, 0).astype(np.uint8), "age")
    assert got["count"].tolist() == [int(valid.sum())] * 2 and not got["pred"].cpu().numpy()[~valid].any()


def test_reproject_tie_goes_to_the_smallest_source_index():
    """a wall of ONE disparity under minification: four sources per target with the same den', the smallest index wins"""
    H, W = 12, 70
    st = {"disp": np.full((H, W), 7.0, f32), "var": np.arange(H * W, dtype=f32).reshape(H, W) + 1,
          "age": (np.arange(H * W) % 200).astype(np.uint8).reshape(H, W)}
    G = np.array([[0.5, 0, 0, 0], [0, 0.5, 0, 0], [0, 0, 1, 0]], f32)
    want = check_reproject(st, G, "tie", doffs=0.0, occl=(0, 0, 0.0), max_disp=C.MAX_DISP)
    assert want["var"][3, 4] == 5 * W + 7 + 1 and want["count"].tolist() == [(H // 2 + 1) * (W // 2 + 1), H * W]


VARIANTS = {
    "occl_off": dict(occl=(0, 0, 1.0)), "occl_3x5": dict(occl=(3, 5, 0.5)), "occl_largest": dict(occl=(8, 8, 2.0)),
    "occl_columns_only": dict(occl=(2, 0, 0.0)), "q": dict(q=0.03), "hints_age0": dict(hint_min_age=0),
    "hints_age3": dict(hint_min_age=3), "hints_age255": dict(hint_min_age=255), "min_ratio0": dict(min_ratio=0.0),
    "min_ratio1": dict(min_ratio=1.0), "narrow_range": dict(min_disp=2.0, max_disp=6.0), "doffs": dict(doffs=3.25),
}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_reproject_variants(variant):
    scene, kw = C.SCENES[0], dict(max_disp=C.MAX_DISP)
    kw.update(VARIANTS[variant])
    if "doffs" not in kw:
        kw["calib"] = scene.calib
    for pose in ("forward1m", "back1m", "yaw2deg"):
        want = check_reproject(rich_state(scene, 21), _G(scene, dict(C.POSES)[pose]), f"{variant}/{pose}", **kw)
        print(f"{variant}/{pose}: kept {want['count'][1]}, visible {want['count'][0]}")
        if variant == "min_ratio1":
            assert (want["count"][0] == 0) == (pose == "forward1m"), "moving forward every ratio is below 1"
        else:
            assert want["count"][0] > 200
    if variant == "hints_age3":
        assert 0 < (want["hints"] > 0).sum() < (want["pred"] > 0).sum()


def test_reproject_bad_pixels_masks_saturation_and_points_behind_the_camera():
    """NaN, +-inf, 0, negative and >= max_disp disparities; a mask; ages up to 255; 5 m forward, which carries the near road
    behind the camera (z <= 0), below min_ratio, or out of the image"""
    scene = C.SCENES[0]
    rng = np.random.default_rng(33)
    st = rich_state(scene, 34)
    pick = rng.integers(0, 12, scene.hw)
    for k, v in enumerate((NAN, INF, -INF, 0.0, -0.0, -2.5, C.MAX_DISP, 1e30, 0.06)):
        st["disp"][pick == k] = v
    st["age"] = rng.integers(250, 256, scene.hw).astype(np.uint8)
    st["var"][rng.uniform(size=scene.hw) < 0.05] = INF
    mask = rng.uniform(size=scene.hw).astype(f32)
    mask[rng.uniform(size=scene.hw) < 0.05] = NAN
    for pose, Tw in (("identity", np.eye(4)), ("forward1m", dict(C.POSES)["forward1m"]), ("forward5m", C.translation(z=5.0)),
                     ("forward12m", C.translation(z=12.0))):
        G = _G(scene, Tw)
        with np.errstate(all="ignore"):
            z = T.project_host(st["disp"], G.reshape(-1), 0.0, T.TEMPORAL_MIN_DISP, C.MAX_DISP, T.TEMPORAL_MIN_RATIO)[3]
        good = np.isfinite(st["disp"]) & (st["disp"] > 0)
        want = check_reproject(st, G, f"bad/{pose}", mask=mask, mask_min=0.3, calib=scene.calib, max_disp=C.MAX_DISP, q=0.01)
        print(f"{pose}: {int((z[good] <= 0).sum())} sources behind the camera, {int(((z[good] > 0) & (z[good] < 0.125)).sum())} below "
              f"min_ratio, kept {want['count'][1]}, visible {want['count'][0]}")
        if pose == "forward12m":
            assert (z[good] <= 0).sum() > 500 and ((z[good] > 0) & (z[good] < 0.125)).sum() > 0
        if pose == "identity":
            assert (want["age"] == 255).sum() > 100 and want["count"][0] > 500
        check_reproject(st, G, f"bad/{pose}/min_ratio0", mask=mask, mask_min=0.3, calib=scene.calib, max_disp=C.MAX_DISP, min_ratio=0.0)


def test_reproject_outputs_leave_the_other_buffers_alone():
    from dcanet_amd import ops
    scene = C.SCENES[2]
    st, G = rich_state(scene, 40), _G(scene, dict(C.POSES)["side0.3m"])
    want = T.disp_reproject_host(st, G, calib=scene.calib, max_disp=C.MAX_DISP)
    for names in (("pred",), ("hints", "count"), ("age",), ("count",), ("var", "age")):
        out, ws = garbage(*scene.hw)
        before = {k: v.clone() for k, v in out.items()}
        got = ops.disp_reproject(dev_state(st), G, scene.calib, max_disp=C.MAX_DISP, outputs=names, out=out, workspace=ws)
        assert set(got) == set(names)
        for k in T.REPROJECT_OUTPUTS:
            if k in names:
                same_bits(out[k], want[k], f"{names}: {k}")
            else:
                assert out[k].cpu().numpy().tobytes() == before[k].cpu().numpy().tobytes(), f"{names}: {k} was touched"
    got = ops.disp_reproject(dev_state(st), G, scene.calib, max_disp=C.MAX_DISP, outputs=("hints",))
    assert set(got) == {"hints"}
    same_bits(got["hints"], want["hints"], "hints alone, allocated")


# ---- the fusion ----------------------------------------------------------------------------------------------------------------
def fuse_inputs():
    rng = np.random.default_rng(11)
    rows, cols, Hc, Wc, y0 = 37, 50, 48, 64, 5
    p = rng.uniform(1, 40, (rows, cols)).astype(f32)
    pred = {"pred": np.where(rng.uniform(size=p.shape) < 0.8, p, 0).astype(f32),
            "var": rng.uniform(0.01, 2.0, p.shape).astype(f32), "age": rng.integers(0, 256, p.shape).astype(np.uint8)}
    pred["var"][rng.uniform(size=p.shape) < 0.03] = NAN
    pred["pred"][rng.uniform(size=p.shape) < 0.03] = NAN
    meas = np.full((Hc, Wc), NAN, f32)
    meas[y0:y0 + rows, :cols] = p + rng.normal(0, 1.5, p.shape)
    bad = rng.uniform(size=meas.shape)
    meas[bad < 0.05], meas[(bad > 0.05) & (bad < 0.1)], meas[(bad > 0.1) & (bad < 0.15)] = NAN, 0.0, INF
    vmap = rng.uniform(0.05, 1.0, meas.shape).astype(f32)
    vmap[rng.uniform(size=meas.shape) < 0.05], vmap[rng.uniform(size=meas.shape) < 0.03] = 0.0, INF
    mask = rng.uniform(size=meas.shape).astype(f32)
    return pred, meas, vmap, mask, (y0, rows, cols)


FUSE = {"defaults": dict(), "gate1_map_mask_varmax": dict(meas_var="map", mask=True, gate=1.0, var_max=1.0),
        "gate_off": dict(meas_var=0.5, mask=True, gate=INF, var_max=0.5), "gate0_map": dict(meas_var="map", gate=0.0),
        "mask_min0": dict(mask=True, mask_min=0.0), "min_disp": dict(min_disp=10.0)}


@pytest.mark.parametrize("variant", list(FUSE))
def test_fuse_is_the_restatement_bit_for_bit(variant):
    """all five rows of the table in one map, a window at row 5 of a padded frame, poisoned outputs; with and without a
    prediction; written over the prediction's own buffers, the same bits"""
    from dcanet_amd import ops
    pred, meas, vmap, mask, window = fuse_inputs()
    kw = dict(FUSE[variant])
    vm = kw.pop("meas_var", 0.25)
    m = mask if kw.pop("mask", False) else None
    kw.setdefault("mask_min", 0.3)
    for p in (pred, None):
        want = T.temporal_fuse_host(p, meas, vmap if vm == "map" else vm, window=window, mask=m, outputs=T.FUSE_OUTPUTS, **kw)
        if p is not None:
            both = want["innov"] > 0
            rows_hit = [int(((want["disp"] == 0) & (want["var"] == 0)).sum()), int((~both & (want["age"] == 0) & (want["disp"] > 0)).sum()),
                        int((~both & (want["disp"] > 0) & (want["disp"] == np.nan_to_num(pred["pred"]))).sum()),
                        int((both & (want["disp"] != meas[5:42, :50])).sum()), int((both & (want["disp"] == meas[5:42, :50])).sum())]
            print(f"{variant}: neither {rows_hit[0]}, only m {rows_hit[1]}, coast {rows_hit[2]}, fused {rows_hit[3]}, new surface {rows_hit[4]}")
            if variant == "defaults":
                assert min(rows_hit) > 10, "every row of the table is exercised"
        dp = None if p is None else {k: dev(v) for k, v in p.items()}
        out = {k: torch.full(window[1:], 77, device=DEV, dtype=torch.uint8 if k == "age" else torch.float32) for k in T.FUSE_OUTPUTS}
        got = ops.temporal_fuse(dp, dev(meas), dev(vmap) if vm == "map" else vm, window=window, mask=dev(m), outputs=T.FUSE_OUTPUTS,
                                out=out, **kw)
        for k in T.FUSE_OUTPUTS:
            same_bits(got[k], want[k], f"{variant}: {k}")
        if p is not None:
            inplace = ops.temporal_fuse(dp, dev(meas), dev(vmap) if vm == "map" else vm, window=window, mask=dev(m),
                                        out={"disp": dp["pred"], "var": dp["var"], "age": dp["age"]}, **kw)
            assert set(inplace) == set(T.STATE_KEYS) and inplace["disp"] is dp["pred"]
            for k in T.STATE_KEYS:
                same_bits(inplace[k], want[k], f"{variant}: {k} written over the prediction")
    only = ops.temporal_fuse(None, dev(meas), 0.25, window=window, outputs=("innov",))
    assert set(only) == {"innov"} and not only["innov"].any()


def test_fuse_gate_at_equality_and_scalar_against_map():
    from dcanet_amd import ops
    pred = {"pred": np.array([[4.0, 4.0]], f32), "var": np.array([[0.5, 0.5]], f32), "age": np.array([[7, 7]], np.uint8)}
    meas = np.array([[7.0, np.nextafter(f32(7.0), f32(8.0))]], f32)                # e e = 9 = gate2 s exactly, and one ulp above
    dp = {k: dev(v) for k, v in pred.items()}
    r = ops.temporal_fuse(dp, dev(meas), 0.5, gate=3.0, outputs=T.FUSE_OUTPUTS)
    assert r["disp"].cpu().tolist() == [[5.5, float(meas[0, 1])]] and r["var"].cpu().tolist() == [[0.25, 0.5]]
    assert r["age"].cpu().tolist() == [[7, 0]]
    rm = ops.temporal_fuse(dp, dev(meas), dev(np.full((1, 2), 0.5, f32)), gate=3.0, outputs=T.FUSE_OUTPUTS)
    assert all(r[k].cpu().numpy().tobytes() == rm[k].cpu().numpy().tobytes() for k in T.FUSE_OUTPUTS)


def test_six_frames_of_both_operators_against_the_host_loop():
    """six frames 0.5 m apart with a yaw, noisy measurements, q > 0: the state is written in place on the device; every frame's
    state equals the host loop's bit for bit"""
    from dcanet_amd import ops
    scene, sigma = C.SCENES[2], 0.5
    rng = np.random.default_rng(77)
    H, W = scene.hw
    kw = dict(calib=scene.calib, max_disp=C.MAX_DISP, q=0.002, hint_min_age=2)
    host, prev = None, None
    state = {"disp": torch.full((H, W), NAN, device=DEV), "var": torch.full((H, W), NAN, device=DEV),
             "age": torch.full((H, W), 9, device=DEV, dtype=torch.uint8)}
    out, ws = garbage(H, W)
    for i in range(6):
        Tw = C.translation(z=0.5 * i) @ C.yaw(0.4 * i)
        truth = C.render(scene, Tw)
        meas = np.where(truth > 0, truth + rng.normal(0, sigma, truth.shape), 0).astype(f32)
        hp = None if host is None else T.disp_reproject_host(host, _G(scene, Tw, prev), **kw)
        host = T.temporal_fuse_host(hp, meas, sigma * sigma)
        dp = None if i == 0 else ops.disp_reproject(state, _G(scene, Tw, prev), out=out, workspace=ws, **kw)
        ops.temporal_fuse(dp, dev(meas), sigma * sigma, out=state)
        prev = Tw
        if hp is not None:
            for k in T.REPROJECT_OUTPUTS:
                same_bits(dp[k], hp[k], f"frame {i}: predicted {k}")
        for k in T.STATE_KEYS:
            same_bits(state[k], host[k], f"frame {i}: {k}")
    assert host["age"].max() == 5 and (host["age"] >= 3).sum() > 1000


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_operators_refuse_what_they_cannot_do_and_launch_nothing():
    from dcanet_amd import ops
    from dcanet_amd._call import _L, _ptr
    scene = C.SCENES[0]
    H, W = scene.hw
    st = dev_state(C.state(scene))
    G = np.eye(3, 4, dtype=f32)
    out, ws = garbage(H, W)
    before = {k: v.clone() for k, v in out.items()}
    bad_g = G.copy()
    bad_g[2, 3] = NAN
    for bad in (dict(G=bad_g), dict(G=np.eye(4)), dict(occl=(9, 1, 1.0)), dict(occl=(1, -1, 1.0)), dict(occl=(1, 1, -1.0)),
                dict(occl=(1, 1, INF)), dict(q=-0.1), dict(q=NAN), dict(min_ratio=-1.0), dict(min_ratio=INF), dict(max_disp=0.01),
                dict(min_disp=-1.0), dict(hint_min_age=256), dict(hint_min_age=0.5), dict(doffs=1.0), dict(calib=None),
                dict(outputs=()), dict(outputs=("nope",)), dict(mask=st["disp"][:-1]), dict(mask=st["disp"], mask_min=NAN),
                dict(state={"disp": st["disp"]}), dict(state={**st, "age": st["age"].int()}), dict(state={**st, "var": st["var"][:-1]}),
                dict(state={k: v.cpu() for k, v in st.items()}), dict(state={**st, "disp": st["disp"][:, ::2]}),
                dict(workspace=ws[:-1]), dict(workspace=ws.int()), dict(out={"pred": st["disp"]}), dict(out={"age": out["pred"]}),
                dict(out={"count": out["count"][:1]})):
        kw = {**dict(state=st, G=G, calib=scene.calib, out=out, workspace=ws), **bad}
        with pytest.raises(RuntimeError, match="disp_reproject"):
            ops.disp_reproject(kw.pop("state"), kw.pop("G"), **kw)
    meas = st["disp"]
    pred = {k: out[k] for k in ("pred", "var", "age")}
    fout = {k: out[k] for k in ("var", "age")}
    for bad in (dict(meas=meas.double()), dict(meas=torch.stack([meas, meas])), dict(meas=meas.cpu()), dict(window=(0, H + 1, W)),
                dict(window=(1, H, W)), dict(window=(0, H - 1, W)), dict(meas_var=0.0), dict(meas_var=-1.0), dict(meas_var=INF),
                dict(meas_var=meas[:-1]), dict(mask=meas[:-1]), dict(mask=meas, mask_min=NAN), dict(gate=-1.0), dict(gate=NAN),
                dict(var_max=-1.0), dict(var_max=NAN), dict(min_disp=-1.0), dict(outputs=()), dict(outputs=("pred",)),
                dict(pred={"pred": meas}), dict(out={"disp": meas}), dict(out={"var": out["age"]})):
        kw = {**dict(pred=pred, meas=meas, out=fout), **bad}
        with pytest.raises(RuntimeError, match="temporal_fuse"):
            ops.temporal_fuse(kw.pop("pred"), kw.pop("meas"), **kw)
    with pytest.raises(RuntimeError, match="inference only"):
        ops.temporal_fuse(None, meas.clone().requires_grad_(), 0.25)
    # the library's own refusals: hipErrorInvalidValue before anything is launched
    lib, p = _L(), lambda t: _ptr(t)
    g = [float(v) for v in G.reshape(-1)]
    ok = dict(mask_min=0.5, g=g, H=H, W=W, doffs=0.0, min_disp=0.0625, max_disp=64.0, min_ratio=0.125, rx=1, ry=1, occl=1.0, q=0.0,
              age=1, outs=[p(out[k]) for k in T.REPROJECT_OUTPUTS], ws=p(ws))

    def reproject(**bad):
        a = {**ok, **bad}
        return lib.dca_disp_reproject(p(st["disp"]), p(st["var"]), p(st["age"]), None, a["mask_min"], *a["g"], a["H"], a["W"],
                                      a["doffs"], a["min_disp"], a["max_disp"], a["min_ratio"], a["rx"], a["ry"], a["occl"], a["q"],
                                      a["age"], *a["outs"], a["ws"], None)
    for bad in (dict(g=g[:5] + [INF] + g[6:]), dict(g=[NAN] + g[1:]), dict(rx=9), dict(ry=-1), dict(occl=-1.0), dict(occl=NAN),
                dict(q=-1.0), dict(q=INF), dict(min_ratio=-0.5), dict(min_ratio=NAN), dict(max_disp=0.01), dict(H=1 << 16, W=1 << 15),
                dict(H=0), dict(ws=None), dict(outs=[None] * 5), dict(age=256), dict(doffs=-1.0)):
        assert reproject(**bad) == 1, bad
    fuse_ok = [None, None, None, p(meas), None, None, 0.25, p(out["pred"]), p(out["var"]), p(out["age"]), None, H, W, 0, H, W,
               0.0625, 0.5, 9.0, INF, None]
    for at, v in ((3, None), (6, 0.0), (6, NAN), (13, 1), (14, H + 1), (15, W + 1), (16, -1.0), (18, -1.0), (18, NAN), (19, NAN),
                  (0, p(out["pred"]))):
        args = list(fuse_ok)
        args[at] = v
        assert lib.dca_temporal_fuse(*args) == 1, (at, v)
    args = list(fuse_ok)
    args[7:11] = [None] * 4
    assert lib.dca_temporal_fuse(*args) == 1, "no output"
    torch.cuda.synchronize()
    for k in out:
        assert out[k].cpu().numpy().tobytes() == before[k].cpu().numpy().tobytes(), f"{k}: a refused call has written"
    assert bool((ws == -1).all())


# ---- through the wrapper ----------------------------------------------------------------------------------------------------
WRAP = dict(crop_height=32, crop_width=64, graph=False)


def _poses(n):
    return [C.translation(z=0.02 * i) @ C.yaw(0.3 * i) for i in range(n)]


@pytest.mark.parametrize("mode,guide", [(None, None), (None, (10.0, 1.0)), ("confidence", None)])
def test_kitti_inference_temporal(mode, guide, monkeypatch):
    """four frames of 28 x 50 in the 32 x 64 frame, then the pose withheld, then a 32 x 64 image: the FIRST frame's disparity is
    KittiInference's bit for bit (guided or not: zero hints are the unguided network), every later frame is ops.disp_reproject,
    [ops.hints_to_quarter, the guided network,] ops.temporal_fuse run by hand, in ONE read-back of exactly the record's bytes;
    pose=None and another size start again; stream() gives the same bytes"""
    from dcanet_amd import ops
    from dcanet_amd.geometry import StereoCalib
    from dcanet_amd.inference import (FrameTemporal, KittiInference, KittiInferenceGuided, KittiInferenceTemporal,
                                      KittiInferenceWithConfidence)
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    model = _model()
    calib = StereoCalib(40.0, 0.5, 24.5, 13.5)
    sizes = [(28, 50)] * 5 + [(32, 64)] * 2
    pairs = _pairs(np.random.default_rng(41), sizes)
    poses = _poses(len(pairs))
    poses[4] = None                                          # frame 4 starts again, and frame 5 has no pose before it
    # min_disp = 0: every pixel the network gives is a measurement, so that a first frame is KittiInference's whole map
    rk = dict(q=0.01, hint_min_age=1, max_disp=float(model.maxdisp), min_disp=0.0)
    fk = dict(meas_var=1.0, gate=4.0, min_disp=0.0)
    if mode == "confidence":
        own = KittiInferenceWithConfidence(model, device_io=True, **WRAP)
    elif guide is not None:
        own = KittiInferenceGuided(model, guide=guide, **WRAP)
    else:
        own = KittiInference(model, device_io=True, **WRAP)
    plain = KittiInference(model, device_io=True, **WRAP)
    infer = KittiInferenceTemporal(model, calib, mask=mode, mask_min=0.4, guide=guide, **rk, meas_var=1.0, gate=4.0, **WRAP)
    copies = []
    readback = infer._readback
    monkeypatch.setattr(infer, "_readback", lambda s, copy: (copies.append(s.out_bytes), readback(s, copy))[1])
    single, state, last = [], None, None
    for i, ((l, r), pose) in enumerate(zip(pairs, poses)):
        h, w = l.shape[:2]
        fresh = pose is None or last is None or last[1] != (h, w)
        pred, hints = None, np.zeros((h, w), f32)
        if not fresh:
            pred = ops.disp_reproject(state, T.reproject_matrix(calib, GEO.relative_pose(last[0], pose)), calib, **rk)
            hints = pred["hints"].cpu().numpy()
        if guide is not None:
            meas, conf = own(l, r, hints), None
        elif mode == "confidence":
            meas, conf = own(l, r)
        else:
            meas, conf = own(l, r), None
        if fresh:
            assert meas.tobytes() == plain(l, r).tobytes(), "zero hints are the unguided network"
        state = ops.temporal_fuse(pred, dev(meas), mask=dev(conf), mask_min=0.4, **fk)
        before = len(copies)
        got = infer(l, r, pose)
        assert len(copies) == before + 1 and copies[-1] == 9 * h * w, "one read-back of exactly the record's bytes"
        assert isinstance(got, FrameTemporal) and got.disp.shape == got.var.shape == got.age.shape == (h, w)
        assert got.disp.dtype == got.var.dtype == np.float32 and got.age.dtype == np.uint8
        for k in T.STATE_KEYS:
            assert getattr(got, k).tobytes() == state[k].cpu().numpy().tobytes(), f"frame {i}: {k}"
        if fresh:
            if conf is None:
                assert got.disp.tobytes() == plain(l, r).tobytes(), "the first frame is KittiInference's"
            assert not got.age.any()
        else:
            print(f"frame {i}: {int((got.age > 0).sum())} of {h * w} pixels carry on, oldest {int(got.age.max())}")
            assert (got.age > 0).sum() > 100, "the sequence carries a state"
        single.append(got)
        last = None if pose is None else (pose, (h, w))
    assert single[3].age.max() == 3 and single[6].age.max() == 1
    infer.reset()
    again = infer(*pairs[0], poses[0])
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, single[0])), "reset() starts the sequence again"
    infer.reset()
    streamed = list(infer.stream(((l, r, p) for (l, r), p in zip(pairs, poses)), depth=2))
    assert len(streamed) == len(single)
    for i, (a, b) in enumerate(zip(streamed, single)):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), f"stream(), frame {i}"


def test_kitti_inference_temporal_refusals():
    from dcanet_amd.geometry import StereoCalib
    from dcanet_amd.inference import KittiInferenceTemporal
    model, calib = _model(), StereoCalib(40.0, 0.5, 24.5, 13.5)
    infer = KittiInferenceTemporal(model, calib, **WRAP)
    assert infer.guide is None and infer._hot_kwargs() == {} and infer._hot_inputs() == {}
    for bad in (dict(calib=None), dict(device_io=False), dict(mask="nope"), dict(guide=(1.0,)), dict(guide=(10.0, 1.0), mask="lr"),
                dict(meas_var=0.0), dict(q=-1.0), dict(gate=-1.0), dict(occl=(9, 1, 1.0)), dict(hint_min_age=300), dict(min_disp=-1.0),
                dict(guide=(10.0, 1.0), crop_width=62)):
        with pytest.raises((ValueError, RuntimeError, TypeError)):
            KittiInferenceTemporal(model, **{**dict(calib=calib), **WRAP, **bad})
    l = np.zeros((28, 50, 3), np.uint8)
    with pytest.raises(TypeError):
        infer(l, l, np.eye(4), as_uint16=True)
    for pose in (np.eye(3), np.full((4, 4), NAN)):
        with pytest.raises(ValueError):
            infer(l, l, pose)
