"""CPU checks of semi-global matching: the numpy restatement of dcanet_amd/sgm.py against an independent scalar implementation
written here from the definitions of include/dca_hip.h, properties of the result on the synthetic pairs of tests/_sgm_cases.py,
the operators' refusals, the library's symbols, and the host check of csrc/sgm_math.h under sanitizers.  The kernels are
compared with the restatement, bit for bit, in test_gpu_sgm.py."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import _sgm_cases as C
from dcanet_amd import sgm as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the definitions, literally: plain loops over pixel, path and bin, Python integers, nothing shared with sgm.py ---------------
def scalar_grey(img):
    img = np.asarray(img)
    H, W = img.shape[:2]
    if img.ndim == 2:
        return [[int(img[y, x]) for x in range(W)] for y in range(H)]
    return [[(77 * int(img[y, x, 0]) + 150 * int(img[y, x, 1]) + 29 * int(img[y, x, 2]) + 128) >> 8 for x in range(W)] for y in range(H)]


def scalar_census(g):
    H, W = len(g), len(g[0])
    out = [[0] * W for _ in range(H)]
    for y in range(H):
        for x in range(W):
            bit = 61
            for dy in range(-3, 4):
                for dx in range(-4, 5):
                    if dy == 0 and dx == 0:
                        continue
                    yy, xx = y + dy, x + dx
                    if 0 <= yy < H and 0 <= xx < W and g[yy][xx] < g[y][x]:
                        out[y][x] |= 1 << bit
                    bit -= 1
            assert bit == -1
    return out


def scalar_sgm(left, right, D, paths=8, P1=10, P2=120, u=15, min_disp=1):
    cL, cR = scalar_census(scalar_grey(left)), scalar_census(scalar_grey(right))
    H, W = len(cL), len(cL[0])
    cost = lambda y, x, d: bin(cL[y][x] ^ cR[y][x - d]).count("1") if x - d >= 0 else 62
    offsets = [(0, 1), (0, -1), (1, 0), (-1, 0)] + ([(1, 1), (1, -1), (-1, 1), (-1, -1)] if paths == 8 else [])
    S_ = [[[0] * D for _ in range(W)] for _ in range(H)]
    for dy, dx in offsets:
        L = {}
        ys = range(H) if dy >= 0 else range(H - 1, -1, -1)
        xs = range(W) if dx >= 0 else range(W - 1, -1, -1)
        for y in ys:                                         # an order in which the predecessor is always done
            for x in xs:
                py, px = y - dy, x - dx
                if not (0 <= py < H and 0 <= px < W):
                    L[y, x] = [cost(y, x, d) for d in range(D)]
                else:
                    prev = L[py, px]
                    m = min(prev)
                    row = []
                    for d in range(D):
                        terms = [prev[d], m + P2]
                        if d >= 1:
                            terms.append(prev[d - 1] + P1)
                        if d <= D - 2:
                            terms.append(prev[d + 1] + P1)
                        row.append(cost(y, x, d) + min(terms) - m)
                    L[y, x] = row
                for d in range(D):
                    S_[y][x][d] += L[y, x][d]

    def winner(vals):                                        # the present bins, in order
        s = min(vals)
        ds = vals.index(s)
        off = 0
        if 0 < ds < len(vals) - 1:
            den = vals[ds - 1] + vals[ds + 1] - 2 * s
            if den > 0:
                off = (16 * (vals[ds - 1] - vals[ds + 1]) + 17 * den) // (2 * den) - 8
        return ds, s, 16 * ds + off

    out = {k: np.zeros((H, W), np.int32 if k == "cost" else np.float32) for k in S.SGM_OUTPUTS}
    for y in range(H):
        for x in range(W):
            ds, s, q = winner(S_[y][x])
            passes = all(S_[y][x][k] * (100 - u) >= 100 * s for k in range(D) if abs(k - ds) > 1)
            ok = passes and ds >= min_disp
            out["disp"][y, x] = np.float32(q) / np.float32(16) if ok else 0
            out["valid"][y, x] = 1 if ok else 0
            out["cost"][y, x] = s
            _, _, q = winner([S_[y][x + k][k] for k in range(min(D, W - x))])
            out["disp_right"][y, x] = out["disp_right_mirrored"][y, W - 1 - x] = np.float32(q) / np.float32(16)
    census = np.array([[[v for v in row] for row in c] for c in (cL, cR)], np.uint64)
    return out, census


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert got.tobytes() == want.tobytes(), f"{what}: {int((got != want).sum())} elements differ"


@pytest.mark.parametrize("name", ["tiny", "extremes-P1-u0-min0", "extremes-P4095-u99-min5", "flat"])
def test_restatement_equals_the_scalar_definition(name):
    c = C.case(name)
    kw = dict(c.kw)
    want, census = scalar_sgm(c.left, c.right, kw.pop("max_disp"), kw.get("paths", 8), kw.get("P1", 10), kw.get("P2", 120),
                              kw.get("uniqueness", 15), kw.get("min_disp", 1))
    got = C.expected(name)
    same(got["census"], census, "census")
    for k in S.SGM_OUTPUTS:
        same(got[k], want[k], k)


def test_restatement_equals_the_scalar_definition_in_colour_with_four_paths():
    rng = np.random.default_rng(3)
    left, right = C.shifted_pair(rng, 8, 13, 3, 4, noise=6)
    want, census = scalar_sgm(left, right, 9, 4, 3, 17, 30, 2)
    got = S.sgm_host(left, right, 9, 4, 3, 17, 30, 2, outputs=S.SGM_OUTPUTS)
    same(np.stack([S.census_host(left), S.census_host(right)]), census, "census")
    for k in S.SGM_OUTPUTS:
        same(got[k], want[k], k)
    same(S.census_host(left[..., :3]), S.census_host(left), "the alpha channel is ignored")
    grey = S.grey_host(left).astype(np.uint8)
    same(S.census_host(grey), S.census_host(left), "a grey image is taken as it is")


def test_plane_is_recovered():
    """seed 0, P1 = 10, P2 = 120, u = 15: away from the borders (the window's half width, and the shift on the left) every pixel
    of the shifted texture is valid and within half a pixel of the shift, in both views"""
    e, d0, W = C.expected("plane"), C.PLANE_D, 67
    assert (e["valid"][:, d0 + 4:W - 4] == 1).all()
    assert np.abs(e["disp"][:, d0 + 4:W - 4] - d0).max() <= 0.5
    assert np.abs(e["disp_right"][:, 4:W - d0 - 4] - d0).max() <= 0.5
    assert e["cost"].dtype == np.int32 and e["cost"].min() >= 0 and e["cost"].max() <= 8 * (62 + 120)


def test_flat_image_ties_go_to_the_lowest_index():
    e = C.expected("flat")
    assert (e["cost"] == 0).all() and (e["valid"] == 0).all() and (e["disp"] == 0).all(), "d* = 0 < min_disp = 1"
    assert (e["disp_right"] == 0).all()
    c = C.case("flat")
    r = S.sgm_host(c.left, c.right, 16, min_disp=0)
    assert (r["valid"] == 1).all() and (r["disp"] == 0).all(), "with min_disp = 0 the same winner is a measurement"


@pytest.mark.parametrize("name", C.names())
def test_outputs_are_consistent(name):
    """the mirrored right view is the flip of the right view; invalid pixels are +0.0; valid ones lie in [min_disp - 1/2,
    D - 1]; S stays within the uint16 bound; with u = 0 exactly the pixels with d* >= min_disp are valid"""
    c, e = C.case(name), C.expected(name)
    same(e["disp_right_mirrored"], np.ascontiguousarray(e["disp_right"][:, ::-1]), "mirrored")
    D, md = c.kw["max_disp"], c.kw.get("min_disp", 1)
    P2, paths = c.kw.get("P2", 120), c.kw.get("paths", 8)
    inv = e["valid"] == 0
    assert set(np.unique(e["valid"])) <= {0.0, 1.0}
    assert (e["disp"][inv].view(np.uint32) == 0).all(), "+0.0 where invalid"
    assert (e["disp"][~inv] >= md - 0.5).all() and (e["disp"][~inv] <= D - 1).all()
    assert 0 <= e["cost"].min() and e["cost"].max() <= paths * (62 + P2) < 65536
    assert (e["disp_right"] >= 0).all() and (e["disp_right"] <= np.minimum(D, c.left.shape[1] - np.arange(c.left.shape[1])) - 1).all()
    open_ = S.sgm_host(c.left, c.right, **{**c.kw, "uniqueness": 0})
    cL, cR = S.census_host(c.left), S.census_host(c.right)
    Sv = S.aggregate_host(S.cost_volume_host(cL, cR, D), paths, c.kw.get("P1", 10), P2)
    same(open_["valid"], (Sv.argmin(axis=-1) >= md).astype(np.float32), "u = 0: valid iff d* >= min_disp")
    assert (open_["valid"] >= e["valid"]).all(), "the uniqueness test only removes"
    same(open_["cost"], e["cost"], "the cost does not depend on u")


def test_two_planes_scene_statistics():
    """a description of the synthetic scene, printed, not an accuracy claim: what DESIGN.md section 6r quotes.  The one bound: most
    of what is visible in both images is measured"""
    left, right, disp, occluded = C.two_planes_pair(np.random.default_rng(C.SEED))
    assert (left == C.case("two_planes-8").left).all()
    for paths in (8, 4):
        e = C.expected(f"two_planes-{paths}")
        v, seen = e["valid"] > 0, ~occluded
        share = (v & seen).sum() / seen.sum()
        off = ((np.abs(e["disp"] - disp) > 1) & v & seen).sum() / (v & seen).sum()
        print(f"two_planes, {paths} paths: {share:.4f} of the non-occluded pixels valid, {off:.4f} of those off by more than 1 px; "
              f"{(v & occluded).sum() / occluded.sum():.3f} of the occluded ones valid")
        assert share > 0.5


# ---- the library and the operators ---------------------------------------------------------------------------------------------
def test_header_library_and_exports():
    from dcanet_amd import _lib, ops
    i, l, p = ctypes.c_int, ctypes.c_long, ctypes.c_void_p
    with open(os.path.join(ROOT, "include", "dca_hip.h")) as f:
        text = f.read()
    for name in ("dca_sgm_workspace_bytes", "dca_sgm_census", "dca_sgm_disparity"):
        assert name + "(" in text
    lib = _lib.load()
    assert _lib.ABI_VERSION == 21 and lib.dca_abi_version() == 21
    assert _lib.SIGNATURES["dca_sgm_workspace_bytes"] == (l, [i, i, i])
    assert _lib.SIGNATURES["dca_sgm_census"] == (i, [p, p, p, i, i, i, p])
    assert _lib.SIGNATURES["dca_sgm_disparity"] == (i, [p] * 8 + [i] * 9 + [p])
    consts = dict(MIN_DIM=7, MAX_DIM=8192, MIN_DISP=8, MAX_DISP=256, MAX_P=4095, CENSUS_BITS=62, COST_OUT=62)
    assert all(_lib.CONSTANTS["DCA_SGM_" + k] == v for k, v in consts.items())
    assert ops.sgm_disparity is S.sgm_disparity and ops.sgm_census is S.sgm_census and ops.sgm_workspace is S.sgm_workspace
    assert ops.SGM_OUTPUTS == S.SGM_OUTPUTS == tuple(S._SGM_KINDS) == ("disp", "valid", "cost", "disp_right", "disp_right_mirrored")
    assert (S.SGM_PATHS, S.SGM_P1, S.SGM_P2, S.SGM_UNIQUENESS, S.SGM_MIN_DISP) == (8, 10, 120, 15, 1), "the defaults"
    assert lib.dca_sgm_workspace_bytes(375, 1242, 192) == 16 * 375 * 1242 + 2 * 375 * 1242 * 192 == S.sgm_workspace_bytes(375, 1242, 192)
    for bad in ((6, 40, 16), (40, 6, 16), (8193, 40, 16), (40, 8193, 16), (40, 40, 7), (40, 40, 257), (4096, 4096, 64)):
        assert lib.dca_sgm_workspace_bytes(*bad) == -1, bad
    # the library refuses before it launches (1: hipErrorInvalidValue); the pointers are never followed
    x = ctypes.c_void_p(4096)
    good = dict(left=x, right=x, ws=x, disp=x, valid=x, cost=x, dr=x, drm=x, H=12, W=40, C=3, D=16, paths=8, P1=10, P2=120, u=15, md=1)
    call = lambda **kw: lib.dca_sgm_disparity(*{**good, **kw}.values(), None)
    for bad in (dict(left=None), dict(right=None), dict(ws=None), dict(ws=ctypes.c_void_p(4100)), dict(C=2), dict(C=0), dict(H=6),
                dict(W=8193), dict(D=7), dict(D=257), dict(H=4096, W=4096, D=64), dict(paths=5), dict(paths=0), dict(P1=0),
                dict(P1=11, P2=10), dict(P2=4096), dict(u=-1), dict(u=100), dict(md=-1), dict(md=16),
                dict(disp=None, valid=None, cost=None, dr=None, drm=None), dict(disp=ctypes.c_void_p(4098))):
        assert call(**bad) == 1, bad
    for bad in ((None, x, x, 12, 40, 3), (x, None, x, 12, 40, 3), (x, x, None, 12, 40, 3), (x, x, ctypes.c_void_p(4100), 12, 40, 3),
                (x, x, x, 6, 40, 3), (x, x, x, 12, 9000, 3), (x, x, x, 12, 40, 2)):
        assert lib.dca_sgm_census(*bad, None) == 1, bad


def test_sgm_operators_refuse_with_their_names():
    """every refusal of the argument list, raised where the operators validate once -- `sgm.sgm_scalars`, which they call with
    RuntimeError and the restatement with ValueError -- and named; a CPU tensor is refused, never computed on"""
    from dcanet_amd import ops
    a = torch.zeros((12, 40, 3), dtype=torch.uint8)
    for call in (lambda: ops.sgm_disparity(a, a, 16), lambda: ops.sgm_disparity(a[..., 0].contiguous(), a[..., 0].contiguous(), 16)):
        with pytest.raises(RuntimeError, match=r"sgm_disparity: .*no CPU fallback"):
            call()
    with pytest.raises(RuntimeError, match=r"sgm_census: .*no CPU fallback"):
        ops.sgm_census(a, a)
    good = dict(H=12, W=40, max_disp=16, paths=8, P1=10, P2=120, uniqueness=15, min_disp=1)
    assert S.sgm_scalars("sgm_disparity", RuntimeError, **good) == (16, 8, 10, 120, 15, 1)
    assert S.sgm_scalars("sgm_disparity", RuntimeError, 7, 7, 8, 4, 1, 1, 0, 0) == (8, 4, 1, 1, 0, 0)
    assert S.sgm_scalars("sgm_disparity", RuntimeError, 8192, 511, 256, 8, 4095, 4095, 99, 255)[0] == 256
    bads = (dict(max_disp=7), dict(max_disp=257), dict(max_disp=16.5), dict(max_disp="x"), dict(max_disp=None), dict(max_disp=True),
            dict(P1=0), dict(P1=11, P2=10), dict(P2=4096), dict(P1=2.5), dict(uniqueness=100), dict(uniqueness=-1), dict(paths=5),
            dict(paths=2), dict(paths=16), dict(min_disp=-1), dict(min_disp=16), dict(H=6), dict(W=6), dict(H=8193), dict(W=8193),
            dict(H=4096, W=4096, max_disp=64))
    for bad in bads:
        for err, name in ((RuntimeError, "sgm_disparity"), (ValueError, "sgm_host")):
            with pytest.raises(err, match=name + ":"):
                S.sgm_scalars(name, err, **{**good, **bad})
    # ... and through the operator itself, before it looks at the device: the scalars and the names of the outputs
    for bad in bads:
        if not set(bad) & {"H", "W"}:
            with pytest.raises(RuntimeError, match="sgm_disparity:"):
                ops.sgm_disparity(a, a, **{**dict(max_disp=16), **bad})
    for bad in (dict(outputs=("nope",)), dict(outputs=()), dict(outputs=("disp", "depth"))):
        with pytest.raises(RuntimeError, match="sgm_disparity: outputs"):
            ops.sgm_disparity(a, a, 16, **bad)
        with pytest.raises(ValueError, match="sgm_host: outputs"):
            S.sgm_host(a.numpy(), a.numpy(), 16, **bad)
    for bad in (dict(H=6), dict(W=8193), dict(max_disp=7), dict(max_disp=257), dict(H=4096, W=4096, max_disp=64)):
        with pytest.raises(RuntimeError, match="sgm_workspace:"):
            ops.sgm_workspace(**{**dict(H=12, W=40, max_disp=16, device="cpu"), **bad})
    ws = ops.sgm_workspace(12, 40, 16, "cpu")
    assert ws.dtype == torch.uint8 and ws.numel() == 16 * 12 * 40 + 2 * 12 * 40 * 16
    # the restatement's own checks: shapes that differ, other types, other layouts
    z = np.zeros((12, 40, 3), np.uint8)
    for left, right in ((z, z[:, :39]), (z, z[..., 0]), (z.astype(np.float32),) * 2, (z[..., :2],) * 2, (z[None],) * 2, (z[:6],) * 2,
                        (z.astype(np.int8),) * 2):
        with pytest.raises(ValueError, match="sgm_host:"):
            S.sgm_host(left, right, 16)
    with pytest.raises(ValueError, match="census_host:"):
        S.census_host(z.astype(np.uint16))
    r = S.sgm_host(z[:, ::-1], z[:, ::-1], 16, outputs=("cost", "disp_right"))
    assert tuple(r) == ("cost", "disp_right"), "the restatement takes any layout numpy can read; the outputs come in the library's order"


def test_sgm_inference_wrappers_host_logic():
    """SGMInference takes no model; KittiInferenceGuided(sgm=...) takes pairs alone and refuses lidar= next to it"""
    from dcanet_amd.geometry import LidarCalib, StereoCalib
    from dcanet_amd.inference import FramePipeline, KittiInference, KittiInferenceGuided, SGMInference
    s = SGMInference()
    assert isinstance(s, FramePipeline) and not isinstance(s, KittiInference) and not hasattr(s, "net") and s.device_io \
        and not s.has_uint16
    # the frames go through the pipeline's own stages: nothing of them is restated for the class without a network
    for name in ("stream", "_readback", "_result", "_compute", "_call_device"):
        assert getattr(type(s), name) is getattr(FramePipeline, name), name
    assert type(s)._upload is not FramePipeline._upload and type(s).__mro__[1] is FramePipeline, "its _upload extends the pipeline's"
    assert (s.sgm["max_disp"], s.sgm["paths"], s.sgm["P1"], s.sgm["P2"], s.sgm["uniqueness"], s.lr_tau, s.median, s.speckle) == \
        (192, 8, 10, 120, 15, 1.0, 0, None)
    assert [(n, dt) for n, dt, _ in s._fields(30, 101, False)] == [("disp", torch.float32), ("valid", torch.float32)]
    t = SGMInference(64, 4, 3, 30, 0, lr_tau=None, median=3, speckle=(50, 1.5))
    assert (t.sgm["max_disp"], t.sgm["paths"], t.lr_tau, t.median, t.speckle) == (64, 4, None, 3, (50, 1.5))
    for bad in (dict(max_disp=7), dict(max_disp=300), dict(paths=5), dict(P1=20, P2=10), dict(P2=5000), dict(uniqueness=100),
                dict(lr_tau=-1.0), dict(lr_tau=float("nan")), dict(median=4), dict(speckle=(1,)), dict(rectify=object()),
                dict(min_disp=-1)):
        with pytest.raises((ValueError, RuntimeError, TypeError)):
            SGMInference(**bad)
    with pytest.raises(TypeError):
        s(np.zeros((12, 40, 3), np.uint8), np.zeros((12, 40, 3), np.uint8), as_uint16=True)
    net = torch.nn.Linear(1, 1)
    net.maxdisp = 192
    g = KittiInferenceGuided(net, 64, 128, graph=False, sgm=dict(max_disp=64, lr_tau=None))
    assert g.sgm["max_disp"] == 64 and g.sgm_lr_tau is None and g.lidar is None
    h = KittiInferenceGuided(net, 64, 128, graph=False, sgm={})
    assert (h.sgm["max_disp"], h.sgm["paths"], h.sgm_lr_tau) == (192, 8, 1.0)
    assert KittiInferenceGuided(net, 64, 128, graph=False).sgm is None
    lidar = LidarCalib(np.array([[700.0, 0, 60, 0], [0, 700.0, 30, 0], [0, 0, 1, 0]]), StereoCalib(700.0, 0.54, 60.0, 30.0), (64, 128))
    for bad in (dict(sgm=dict(max_disp=64), lidar=lidar), dict(sgm=dict(nope=1)), dict(sgm=dict(max_disp=7)), dict(sgm=5),
                dict(sgm=dict(median=3))):
        with pytest.raises((ValueError, RuntimeError, TypeError)):
            KittiInferenceGuided(net, 64, 128, graph=False, **bad)
    with pytest.raises(TypeError, match="sgm="):
        g(np.zeros((12, 40, 3), np.uint8), np.zeros((12, 40, 3), np.uint8), np.zeros((12, 40), np.float32))


def test_sgm_math_host_check_under_sanitizers(tmp_path):
    """tools/sgm_math_check.cpp: the recursion step of csrc/sgm_math.h along whole paths against the definition, its bounds at
    the extremes, the uniqueness test and the sub-pixel step against exact integers, compiled for the host with AddressSanitizer
    and UBSan as a stand-alone program, exits 0"""
    cxx = next((c for c in (shutil.which("clang++"), "/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++",
                            shutil.which("g++")) if c and os.path.exists(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "sgm_check")
    csrc = os.path.join(ROOT, "cost-volume-aggregation-in-stereo-matching-revisited_amd", "csrc")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc,
           os.path.join(ROOT, "tools", "sgm_math_check.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok"), run.stdout[-2000:] + run.stderr[-2000:]
