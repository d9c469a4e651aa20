"""Geometry from calibrated disparity, the parts that need no GPU: the entry points of csrc/geometry.hip are bound with the
types the header states and refuse bad arguments before anything touches a device, the tile query follows its formula, the
calibration parsers and the PLY exporter do what they document, the operators refuse CPU tensors and bad scalars -- and the
scene the GPU tests compare on (tests/_geometry_reference.py) populates EVERY rejection category and both kept classes on
every shape those tests use, so that none of them can pass vacuously."""
import ctypes
import math

import numpy as np
import pytest
import torch

from _geometry_reference import (CALIB, MASK_MIN, MAX_DEPTH, MIN_DISP, REASONS, SHAPES, TILE, V0, VERTEX, Y0,
                                 geometry_reference, scene)

CARRY_SHAPE = (1100, 1000)       # the scan-carry window of the GPU test


def test_geometry_entry_points_are_bound_and_exported():
    from dcanet_amd import _lib, ops
    lib = _lib.load()
    i, l, f, p = ctypes.c_int, ctypes.c_long, ctypes.c_float, ctypes.c_void_p
    want = {
        "dca_disp_to_depth": (i, [p] * 4 + [i] * 5 + [f] * 6 + [p]),
        "dca_point_cloud_tiles": (l, [i, i]),
        "dca_point_cloud": (i, [p, p, p, i, i, i, p, l, p, p] + [i] * 7 + [f] * 8 + [p]),
    }
    for name, (res, args) in want.items():
        assert _lib.SIGNATURES[name] == (res, args), name
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    assert lib.dca_abi_version() == 21 and _lib.ABI_VERSION == 21
    assert _lib.CONSTANTS["DCA_PC_TILE"] == ops.PC_TILE == TILE
    assert _lib.CONSTANTS["DCA_PC_RECORD_BYTES"] == ops.PC_RECORD_BYTES == VERTEX.itemsize == 16


@pytest.mark.parametrize("pixels", [1, TILE - 1, TILE, TILE + 1, 1301 * 9])
def test_point_cloud_tiles_follows_its_formula(pixels):
    from dcanet_amd import _lib, ops
    lib = _lib.load()
    want = -(-pixels // TILE)
    assert lib.dca_point_cloud_tiles(1, pixels) == want == ops.point_cloud_tiles(1, pixels)
    if pixels == 1301 * 9:
        assert lib.dca_point_cloud_tiles(9, 1301) == want == 12 and lib.dca_point_cloud_tiles(1301, 9) == want
    assert lib.dca_point_cloud_tiles(0, 5) == 0 and lib.dca_point_cloud_tiles(5, -1) == 0
    assert lib.dca_point_cloud_tiles(1 << 16, 1 << 15) == 0                         # 2^31 pixels
    with pytest.raises(RuntimeError):
        ops.point_cloud_tiles(0, 5)


def test_geometry_launchers_refuse_bad_arguments_before_any_launch():
    """hipErrorInvalidValue (1) without touching a device"""
    from dcanet_amd import _lib
    lib = _lib.load()
    p, m, o, u, rgb, vert, offs, cnt = (ctypes.c_void_p(64 * k) for k in range(1, 9))
    cal = dict(fb=380.0, doffs=0.0, min_disp=0.5, max_depth=80.0, mask_min=0.5)

    def depth(pred=p, mask=m, of=o, ou=u, Hc=8, Wc=16, y0=2, rows=4, cols=10, scale=256.0, **kw):
        c = {**cal, **kw}
        return lib.dca_disp_to_depth(pred, mask, of, ou, Hc, Wc, y0, rows, cols, c["fb"], c["doffs"], c["min_disp"],
                                     c["max_depth"], c["mask_min"], scale, None)

    def cloud(pred=p, mask=m, rgb=rgb, C=3, Hs=9, Ws=12, vert=vert, cap=40, offs=offs, cnt=cnt, Hc=8, Wc=16, y0=2, rows=4,
              cols=10, v0=5, stride=1, f=700.0, cx=8.0, cy=4.0, **kw):
        c = {**cal, **kw}
        return lib.dca_point_cloud(pred, mask, rgb, C, Hs, Ws, vert, cap, offs, cnt, Hc, Wc, y0, rows, cols, v0, stride, f,
                                   c["fb"], cx, cy, c["doffs"], c["min_disp"], c["max_depth"], c["mask_min"], None)

    bad_common = [dict(pred=None), dict(y0=-1), dict(rows=0), dict(cols=0), dict(y0=5), dict(cols=17), dict(Hc=0),
                  dict(Wc=-3), dict(fb=0.0), dict(fb=-1.0), dict(fb=math.inf), dict(fb=math.nan), dict(doffs=math.nan),
                  dict(doffs=math.inf), dict(min_disp=-0.5), dict(min_disp=math.inf), dict(min_disp=math.nan),
                  dict(max_depth=0.0), dict(max_depth=-1.0), dict(max_depth=math.inf), dict(max_depth=math.nan),
                  dict(mask_min=math.nan)]
    for bad in bad_common:
        assert depth(**bad) == 1, bad
        assert cloud(**bad) == 1, bad
    for bad in (dict(of=None, ou=None), dict(scale=0.0), dict(scale=math.nan), dict(scale=math.inf)):
        assert depth(**bad) == 1, bad
    for bad in (dict(C=2), dict(C=5), dict(Hs=8), dict(Ws=9), dict(v0=6), dict(v0=-1), dict(vert=None),
                dict(vert=ctypes.c_void_p(8)), dict(cap=-1), dict(offs=None), dict(cnt=None), dict(offs=ctypes.c_void_p(6)),
                dict(cnt=ctypes.c_void_p(12)), dict(stride=0), dict(stride=-2), dict(f=0.0), dict(f=-700.0),
                dict(f=math.nan), dict(f=math.inf), dict(cx=math.nan), dict(cy=math.inf)):
        assert cloud(**bad) == 1, bad


def test_the_scene_reaches_every_category_on_every_gpu_shape():
    """the condition that keeps the GPU comparison from passing vacuously; also: the restatement's own invariants"""
    for rows, cols in SHAPES + (CARRY_SHAPE,):
        pred, mask, rgb = scene(rows, cols)
        assert pred.dtype == mask.dtype == np.float32 and rgb.dtype == np.uint8 and pred.shape == mask.shape
        assert pred.shape[0] > Y0 + rows and pred.shape[1] > cols and rgb.shape[0] > V0 + rows and rgb.shape[1] > cols
        ref = geometry_reference(pred, CALIB, (Y0, rows, cols), V0, 1, mask, rgb=rgb)
        r = ref["reasons"]
        print((rows, cols), r)
        assert sum(r.values()) == rows * cols and r["stride"] == 0 and r["kept"] == ref["count"] == len(ref["vertices"])
        i = np.arange(rows * cols)
        keep = ref["keep"].reshape(-1)
        if rows * cols >= 8:
            for name in REASONS:
                if name != "stride":
                    assert r[name] > 0, ((rows, cols), name)
            # both kept classes, nothing else: Z == max_depth (class 6) and mask == mask_min (class 7) stay in
            assert np.array_equal(keep, i % 8 >= 6) and keep[i % 8 == 6].any() and keep[i % 8 == 7].any()
            z = ref["vertices"]["z"]
            assert (z == np.float32(MAX_DEPTH)).any() and (z > 0).all() and (z <= np.float32(MAX_DEPTH)).all()
        else:
            assert r["nan"] == 1 and ref["count"] == 0
        # the dense map and the records agree; rejected -> +0.0; the offsets are the running count at the tile borders
        assert np.array_equal(ref["depth"][ref["keep"]], ref["vertices"]["z"])
        assert not ref["depth"][~ref["keep"]].view(np.uint32).any()
        assert ref["tile_offsets"][0] == 0 and ref["tile_offsets"][-1] == ref["count"]
        assert len(ref["tile_offsets"]) == -(-rows * cols // TILE) + 1 and (np.diff(ref["tile_offsets"]) >= 0).all()
        assert (ref["vertices"]["alpha"] == 255).all()
        # without the mask the masked-out class is kept too; a stride drops pixels for that reason alone
        nomask = geometry_reference(pred, CALIB, (Y0, rows, cols), V0, 1, None)
        assert nomask["reasons"]["mask"] == 0 and nomask["count"] == ref["count"] + r["mask"]
        assert (nomask["vertices"]["red"] == 255).all()
        for stride in (2, 3):
            s = geometry_reference(pred, CALIB, (Y0, rows, cols), V0, stride, mask, rgb=rgb)
            assert s["reasons"]["stride"] + s["count"] == ref["count"] and s["depth"].tobytes() == ref["depth"].tobytes()
            if rows * cols >= 64:
                assert 0 < s["count"] < ref["count"]
    assert MIN_DISP == 0.5 and CALIB.doffs == -2.0 and MASK_MIN == 0.5


def test_the_restatement_against_plain_float64_formulas():
    """the float32 restatement is the pinhole model: against float64 formulas it differs by rounding only"""
    pred, mask, rgb = scene(5, 67)
    ref = geometry_reference(pred, CALIB, (Y0, 5, 67), V0, 1, mask, rgb=rgb)
    rr, cc = np.nonzero(ref["keep"])
    d = pred[Y0:Y0 + 5, :67][rr, cc].astype(np.float64)
    Z = CALIB.fb / (d + CALIB.doffs)
    X, Y = (cc - CALIB.cx) * Z / CALIB.f, (V0 + rr - CALIB.cy) * Z / CALIB.f
    v = ref["vertices"]
    for got, want in ((v["z"], Z), (v["x"], X), (v["y"], Y)):
        assert np.allclose(got, want, rtol=4 * 2.0 ** -24, atol=0)          # at most four roundings of 2^-24 each
    assert np.array_equal(v["red"], rgb[V0 + rr, cc, 0]) and np.array_equal(v["blue"], rgb[V0 + rr, cc, 2])
    assert np.array_equal(ref["depth_u16"][rr, cc], np.minimum(np.trunc(v["z"] * np.float32(256)), 65535))


KITTI_OBJECT = """P0: 7.215377e+02 0.000000e+00 6.095593e+02 0.000000e+00 0.000000e+00 7.215377e+02 1.728540e+02 0.000000e+00 0.000000e+00 0.000000e+00 1.000000e+00 0.000000e+00
P2: 7.215377e+02 0.000000e+00 6.095593e+02 4.485728e+01 0.000000e+00 7.215377e+02 1.728540e+02 2.163791e-01 0.000000e+00 0.000000e+00 1.000000e+00 2.745884e-03
P3: 7.215377e+02 0.000000e+00 6.095593e+02 -3.395242e+02 0.000000e+00 7.215377e+02 1.728540e+02 2.199936e+00 0.000000e+00 0.000000e+00 1.000000e+00 2.729905e-03
R0_rect: 1 0 0 0 1 0 0 0 1
"""
KITTI_RAW = """calib_time: 09-Jan-2012 13:57:47
S_rect_02: 1.242000e+03 3.750000e+02
P_rect_02: 7.0e+02 0.0 6.0e+02 3.5e+01 0.0 7.0e+02 1.8e+02 0.0 0.0 0.0 1.0 0.0
P_rect_03: 7.0e+02 0.0 6.04e+02 -3.15e+02 0.0 7.0e+02 1.8e+02 0.0 0.0 0.0 1.0 0.0
"""
MIDDLEBURY = """cam0=[3997.684 0 1176.728; 0 3997.684 1011.728; 0 0 1]
cam1=[3997.684 0 1307.839; 0 3997.684 1011.728; 0 0 1]
doffs=131.111
baseline=193.001
width=2964
height=1988
"""


def test_calibration_parsers(tmp_path):
    from dcanet_amd.geometry import StereoCalib
    (tmp_path / "000000.txt").write_text(KITTI_OBJECT)
    for src in (KITTI_OBJECT, str(tmp_path / "000000.txt"), tmp_path / "000000.txt"):
        c = StereoCalib.from_kitti(src)
        assert (c.f, c.cx, c.cy, c.doffs) == (721.5377, 609.5593, 172.854, 0.0)
        assert c.baseline == 44.85728 / 721.5377 - -339.5242 / 721.5377 and abs(c.baseline - 0.5327) < 1e-4
        assert c.fb == float(np.float32(c.f * c.baseline))
    (tmp_path / "calib_cam_to_cam.txt").write_text(KITTI_RAW)
    c = StereoCalib.from_kitti(tmp_path / "calib_cam_to_cam.txt")
    assert (c.f, c.cx, c.cy) == (700.0, 600.0, 180.0) and c.baseline == 0.05 - -0.45 and c.doffs == 4.0
    assert c.fb == 350.0
    grey = StereoCalib.from_kitti(KITTI_OBJECT, left="P0", right="P3")
    assert grey.baseline == 0.0 - -339.5242 / 721.5377
    with pytest.raises(ValueError):
        StereoCalib.from_kitti(KITTI_RAW, left="P0")
    with pytest.raises(ValueError):
        StereoCalib.from_kitti("P2: 1 2 3\nP3: 1 2 3\n")
    (tmp_path / "calib.txt").write_text(MIDDLEBURY)
    for src in (MIDDLEBURY, tmp_path / "calib.txt"):
        m = StereoCalib.from_middlebury(src)
        assert (m.f, m.cx, m.cy, m.doffs) == (3997.684, 1176.728, 1011.728, 131.111) and m.baseline == 193.001 / 1000.0
    with pytest.raises(ValueError):
        StereoCalib.from_middlebury("cam0=[1 0 2; 0 1 3; 0 0 1]\n")
    half = m.scaled(0.5, 0.25)
    assert (half.f, half.cx, half.cy, half.doffs, half.baseline) == (m.f / 2, m.cx / 2, m.cy / 4, m.doffs / 2, m.baseline)
    assert m.scaled(2.0).cy == m.cy * 2
    for bad in (dict(f=0.0), dict(baseline=-0.5), dict(cx=math.nan), dict(doffs=math.inf)):
        with pytest.raises(ValueError):
            StereoCalib(**{**dict(f=700.0, baseline=0.5, cx=1.0, cy=2.0), **bad})


def test_ply_round_trip_and_header(tmp_path):
    from dcanet_amd.geometry import PLY_VERTEX, read_ply, write_ply
    assert PLY_VERTEX == VERTEX and PLY_VERTEX.itemsize == 16
    pred, mask, rgb = scene(5, 67)
    vert = geometry_reference(pred, CALIB, (Y0, 5, 67), V0, 1, mask, rgb=rgb)["vertices"]
    n = len(vert)
    assert n == 83                                                        # 42 + 41 pixels of the two kept classes
    path = tmp_path / "cloud.ply"
    assert write_ply(path, vert) == n
    header = (b"ply\nformat binary_little_endian 1.0\nelement vertex 83\nproperty float x\nproperty float y\n"
              b"property float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\n"
              b"end_header\n")
    data = path.read_bytes()
    assert data == header + vert.tobytes()
    back = read_ply(path)
    assert back.dtype == PLY_VERTEX and back.tobytes() == vert.tobytes()
    # the (n,4) float32 form of ops.point_cloud is the same bytes
    as_f32 = torch.from_numpy(vert.view(np.float32).reshape(-1, 4).copy())
    write_ply(path, as_f32)
    assert path.read_bytes() == data
    write_ply(path, vert[:0])
    assert len(read_ply(path)) == 0
    path.write_bytes(data[:-3])
    with pytest.raises(ValueError):
        read_ply(path)
    path.write_bytes(data.replace(b"binary_little_endian", b"ascii"))
    with pytest.raises(ValueError):
        read_ply(path)
    with pytest.raises(ValueError):
        write_ply(path, np.zeros((3, 3), np.float32))


def test_depth_png(tmp_path):
    from PIL import Image
    from dcanet_amd import inference
    from dcanet_amd.geometry import depth_png
    assert inference.depth_png is depth_png
    depth = np.array([[0.0, 1.0, 2.5], [80.0, 255.999, 300.0]], np.float32)
    depth_png(tmp_path / "d.png", depth)
    got = np.array(Image.open(tmp_path / "d.png"))
    assert got.dtype == np.uint16 and np.array_equal(got, [[0, 256, 640], [20480, 65535, 65535]])
    depth_png(tmp_path / "u.png", got)
    assert np.array_equal(np.array(Image.open(tmp_path / "u.png")), got)


def test_geometry_operators_refuse_cpu_tensors_and_bad_scalars():
    from dcanet_amd import ops
    pred = torch.ones(8, 16)
    for bad in (dict(), dict(min_disp=-1.0), dict(max_depth=0.0), dict(max_depth=math.inf), dict(mask_min=math.nan)):
        with pytest.raises(RuntimeError):
            ops.disp_to_depth(pred, CALIB, **bad)
        with pytest.raises(RuntimeError):
            ops.point_cloud(pred, CALIB, **bad)
    with pytest.raises(RuntimeError):
        ops.point_cloud(pred, CALIB, rgb=torch.zeros(8, 16, 3, dtype=torch.uint8), stride=0)
    with pytest.raises(RuntimeError):
        ops.disp_to_depth(pred, object())


def test_kitti_inference_3d_host_logic():
    """KittiInference's arguments plus the calibration and the filters; device I/O is required"""
    from dcanet_amd.geometry import StereoCalib
    from dcanet_amd.inference import Frame3D, KittiInference, KittiInference3D
    net = torch.nn.Linear(1, 1)
    calib = StereoCalib(700.0, 0.5, 600.0, 180.0)
    a = KittiInference3D(net, calib, 64, 128, graph=False, device_io=True)
    assert isinstance(a, KittiInference) and a.nmaps == 1 and a.confidence is False and a.stride == 1
    assert (a.crop_height, a.crop_width, a.graph) == (64, 128, False)
    b = KittiInference3D(net, calib, mask="confidence", radius=2, mask_min=0.7, device_io=True)
    assert b.nmaps == 2 and b.confidence is True and b.radius == 2 and b.filters["mask_min"] == 0.7
    c = KittiInference3D(net, calib, mask="lr", tau=2.0, stride=3, max_depth=50.0, device_io=True)
    assert c.nmaps == 2 and c.confidence is False and c.tau == 2.0 and c.stride == 3 and c.filters["max_depth"] == 50.0
    assert Frame3D._fields == ("disp", "mask", "depth", "vertices")
    for bad in (dict(), dict(device_io=False)):
        with pytest.raises(ValueError):
            KittiInference3D(net, calib, **bad)
    for bad in (dict(mask="filled"), dict(stride=0), dict(radius=-1), dict(tau=-1.0)):
        with pytest.raises(ValueError):
            KittiInference3D(net, calib, device_io=True, **bad)
    for bad in (dict(min_disp=-1.0), dict(max_depth=math.nan)):
        with pytest.raises(RuntimeError):
            KittiInference3D(net, calib, device_io=True, **bad)
