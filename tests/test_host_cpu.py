"""CPU-only checks of the host side: the C-ABI library loads and exports every symbol include/dca_hip.h
declares (no compute calls without a GPU), the module mirror has the reference's state-dict format, and the
product path refuses to run without the HIP kernels (no CPU fallback)."""
import json
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_capi_exports_every_declared_symbol():
    import dcanet_amd
    from dcanet_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "dca_hip.h")).read()
    declared = set(re.findall(r"^(?:int|long)\s+(dca_\w+)\s*\(", header, flags=re.M))
    assert declared, "no declarations parsed"
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    for name in declared:
        assert getattr(lib, name) is not None


def test_capi_argument_counts_match_header():
    from dcanet_amd import _lib
    header = open(os.path.join(ROOT, "include", "dca_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, (_, args) in _lib.SIGNATURES.items():
        m = re.search(name + r"\s*\((.*?)\)\s*;", header, flags=re.S)
        assert m, name
        assert len([a for a in m.group(1).split(",") if a.strip() and a.strip() != "void"]) == len(args), name


def test_capi_argument_types_are_derived_from_header():
    """types, not only counts: a swapped int / long or float / double loads and runs, with garbage sizes"""
    from ctypes import c_double as d, c_float as f, c_int as i, c_long as l, c_void_p as p
    from dcanet_amd import _lib
    S = _lib.SIGNATURES
    assert S["dca_bn_finalize"] == (i, [p, i, d, p, p, p, p, f, f, i, p, p, p, i, p, i, i, p])
    assert S["dca_train_tables"] == (i, [p, l, p, f, f, p, p, p, p])
    # const float* const*, const int*, void*, unsigned*, hipStream_t
    assert S["dca_cost_volume_fwd"] == (i, [p, p, p, i, p, p, i, p, i, i, i, i, i, i, p, p])
    assert S["dca_eval_state_len"] == (l, [i])
    assert S["dca_abi_version"] == (i, [])
    assert _lib.ABI_VERSION == _lib.CONSTANTS["DCA_ABI_VERSION"]

    sigs, consts = _lib.parse_header(
        "/* int dca_gone(int n); */\n#ifndef DCA_X_H\n#define DCA_X_H\n#define DCA_N 0x10\n#define DCA_M 7  // seven\n"
        "long dca_y(const long n, const double* q,\n           hipStream_t stream);  /* trailing */\nint dca_z(void);\n")
    assert sigs == {"dca_y": (l, [l, p, p]), "dca_z": (i, [])} and consts == {"DCA_N": 16, "DCA_M": 7}
    for bad in ("short n", "unsigned n", "long long n", "hipStream_t"):
        with pytest.raises(RuntimeError, match="dca_x"):
            _lib.parse_header(f"int dca_x({bad});")
    with pytest.raises(RuntimeError):
        _lib.parse_header("#define DCA_N 3\nvoid helper(int n);\n")


def test_every_entry_point_is_defined_against_the_header():
    """C linkage compares nothing: a definition is checked against its declaration only if its file sees the header"""
    csrc = os.path.join(ROOT, "cost-volume-aggregation-in-stereo-matching-revisited_amd", "csrc")
    header = os.path.join(ROOT, "include", "dca_hip.h")
    declared = set(re.findall(r"^(?:int|long)\s+(dca_\w+)\s*\(", open(header).read(), flags=re.M))

    def closure(path, seen):
        path = os.path.normpath(path)
        if path not in seen and os.path.exists(path):
            seen.add(path)
            for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(path).read(), flags=re.M):
                closure(os.path.join(os.path.dirname(path), inc), seen)
        return seen

    defined = set()
    for name in sorted(os.listdir(csrc)):
        if not name.endswith(".hip"):
            continue
        here = re.findall(r'^extern "C" (?:int|long) (dca_\w+)', open(os.path.join(csrc, name)).read(), flags=re.M)
        assert not defined & set(here), (name, defined & set(here))
        defined |= set(here)
        if here:
            assert os.path.normpath(header) in closure(os.path.join(csrc, name), set()), name
    assert defined == declared, defined ^ declared

    ndef = 0
    for d in (csrc, os.path.join(ROOT, "include")):
        for name in os.listdir(d):
            if name.endswith((".h", ".hip")):
                ndef += len(re.findall(r"^\s*#\s*define\s+DCA_AMAX_CSLOTS\b", open(os.path.join(d, name)).read(), flags=re.M))
    assert ndef == 1


# Every size query of the C ABI at shapes that are no tile multiples and sit on both sides of each clip (tiles below and
# above the workgroups the grid rule allows, more channel blocks than CUs, the slot and block caps), on a 256-CU device --
# also what a query assumes when no device can be asked.  Recorded from the library before the queries and the launchers
# were given one geometry function each: a caller allocates with these, the launch indexes with them.
SIZE_QUERIES = {
    "dca_conv3d_x2_stats_chunks": {
        (1, 32, 5, 9, 20): 8,
        (2, 32, 48, 136, 240): 256,
        (2, 64, 48, 136, 240): 128,
        (3, 32, 20, 40, 64): 256,
        (1, 96, 5, 9, 20): 8,
        (1, 8224, 5, 9, 20): 1,
        (8, 8, 48, 136, 240): 256,
    },
    "dca_conv3d_x3_stats_chunks": {
        (1, 32, 5, 9, 20): 8,
        (3, 32, 20, 40, 64): 256,
        (2, 64, 48, 136, 240): 128,
        (1, 8224, 5, 9, 20): 1,
    },
    "dca_conv3d_s2x2_out_slots": {
        (1, 64, 6, 10, 24): 4,
        (4, 64, 48, 136, 240): 256,
        (2, 64, 38, 76, 132): 256,
        (1, 128, 12, 20, 72): 18,
        (2, 128, 38, 76, 132): 128,
    },
    "dca_deconv3d_x3_stats_chunks": {
        (1, 3, 5, 12): 2,
        (2, 19, 38, 68): 256,
        (1, 9, 17, 36): 45,
    },
    "dca_conv1_x3_stats_chunks": {
        (1, 900): 2,
        (1, 4): 1,
        (3, 349184): 2046,
        (3, 349568): 2048,
        (2, 130948): 512,
    },
    "dca_conv3d_wgrad_x2_workspace": {
        (1, 32, 32, 5, 9, 20): 497664,
        (2, 32, 32, 18, 32, 64): 7077888,
        (1, 40, 72, 5, 9, 20): 2985984,
        (2, 64, 64, 18, 32, 64): 7077888,
        (1, 512, 544, 3, 5, 20): 7520256,
    },
    "dca_conv3d_wgrad_x3_workspace": {
        (1, 32, 32, 5, 9, 20): 497664,
        (2, 32, 32, 18, 32, 64): 7077888,
        (1, 40, 72, 5, 9, 20): 2985984,
        (2, 64, 64, 18, 32, 64): 7077888,
        (1, 512, 544, 3, 5, 20): 7520256,
    },
    "dca_conv3d_wgrad_s2_x2_workspace": {
        (1, 32, 64, 6, 10, 24): 331776,
        (2, 32, 64, 36, 64, 128): 14155776,
        (1, 40, 72, 6, 10, 24): 995328,
        (2, 64, 128, 36, 64, 128): 14155776,
    },
    "dca_conv3d_wgrad_workspace": {
        (1, 32, 32, 5, 9, 20, 3, 1): 248832,
        (2, 32, 32, 18, 32, 64, 3, 1): 7077888,
        (1, 32, 64, 3, 5, 12, 3, 2): 497664,
        (1, 32, 32, 5, 9, 20, 1, 1): 4096,
        (1, 32, 32, 5, 9, 48, 3, 1): 497664,
        (1, 40, 72, 5, 9, 20, 3, 1): 1492992,
        (2, 32, 64, 18, 32, 64, 3, 2): 7077888,
        (2, 64, 32, 18, 32, 64, 1, 1): 524288,
        (1, 32, 27, 5, 9, 20, 1, 1): 4096,
        (4, 32, 27, 48, 136, 240, 1, 1): 524288,
        (1, 512, 544, 3, 5, 20, 3, 1): 7520256,
    },
}


def test_size_queries_are_pinned():
    from dcanet_amd import _lib
    if torch.cuda.is_available() and torch.cuda.get_device_properties(0).multi_processor_count != 256:
        pytest.skip("the table holds for 256 CUs")
    lib = _lib.load()
    got = {name: {args: getattr(lib, name)(*args) for args in cases} for name, cases in SIZE_QUERIES.items()}
    assert got == SIZE_QUERIES


@pytest.mark.parametrize("variant", ["g", "gc"])
def test_state_dict_matches_reference(variant):
    """tests/golden/state_dict_keys.json was dumped from the reference model (oracle/make_golden.py)."""
    from dcanet_amd.models.gwcnet_dca_g import GwcNet
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "state_dict_keys.json")))[variant]
    got = {k: list(v.shape) for k, v in GwcNet(192, use_concat_volume=(variant == "gc")).state_dict().items()}
    assert list(got) == list(want)          # same keys, same order
    assert got == want                      # same shapes


def test_factories_and_registry():
    from dcanet_amd.models import __models__, GwcNet_G, GwcNet_GC
    assert __models__["gwcnet-g"] is GwcNet_G and __models__["gwcnet-gc"] is GwcNet_GC
    m = GwcNet_G(64)
    assert m.maxdisp == 64 and m.num_groups == 40 and m.concat_channels == 0 and not m.use_concat_volume
    assert GwcNet_GC(64).concat_channels == 12


def test_no_cpu_fallback():
    from dcanet_amd.models.submodule import build_gwc_volume, disparity_regression
    from dcanet_amd.models.gwcnet_dca_g import GwcNet
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        build_gwc_volume(torch.zeros(1, 8, 2, 4), torch.zeros(1, 8, 2, 4), 2, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        disparity_regression(torch.zeros(1, 4, 2, 2), 4)
    m = GwcNet(32, False).eval()
    with pytest.raises(RuntimeError, match="no CPU fallback"), torch.no_grad():
        m(torch.zeros(1, 3, 32, 64), torch.zeros(1, 3, 32, 64))


def test_reference_asserts_are_kept():
    from dcanet_amd.models.submodule import build_gwc_volume, disparity_regression
    with pytest.raises(AssertionError):
        disparity_regression(torch.zeros(4, 2, 2), 4)          # reference submodule.py:128
    with pytest.raises(AssertionError):
        build_gwc_volume(torch.zeros(1, 9, 2, 4), torch.zeros(1, 9, 2, 4), 2, 4)   # submodule.py:150


def test_product_does_not_import_oracle():
    pkg = os.path.join(ROOT, "cost-volume-aggregation-in-stereo-matching-revisited_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dirpath, f)).read()
                assert "oracle" not in src, os.path.join(dirpath, f)


def test_losses_match_reference(golden=None):
    """models/loss.py mirror vs the reference (tests/golden/losses.npz): `model_loss` is device-agnostic torch code and
    is checked here incl. its NaN behaviour at masked-out pixels; the focal loss is a HIP kernel (GPU test in
    tests/test_gpu_heads.py) and must refuse CPU tensors; the LR schedules are pure host logic."""
    import numpy as np
    from oracle.seeded import seeded_tensor
    from dcanet_amd.models.loss import StereoFocalLoss, focal_loss, model_loss
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "losses.npz")))
    gt = torch.from_numpy(g["gt"])
    ests = [torch.softmax(seeded_tensor(f"loss.e{i}", (2, 8, 8, 16)), 1).requires_grad_() for i in range(5)]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        focal_loss(ests, gt, 32, 5.0, False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        StereoFocalLoss(max_disp=32, focal_coefficient=5.0)(ests[0], gt, variance=1)
    d0 = (seeded_tensor("loss.d0", (2, 1, 32, 64)) * 3 + gt).requires_grad_()
    d1 = (seeded_tensor("loss.d1", (2, 1, 32, 64)) * 0.3 + gt).requires_grad_()
    mask = (gt < 32) & (gt > 0)
    ml = model_loss([d0, d1], gt, mask)
    assert abs(ml.item() - float(g["model"])) < 1e-5 * max(1, abs(float(g["model"])))
    gd = torch.autograd.grad(ml, [d0, d1])
    assert torch.allclose(gd[0], torch.from_numpy(g["gd0"]), atol=1e-7, rtol=1e-4)
    assert torch.allclose(gd[1], torch.from_numpy(g["gd1"]), atol=1e-7, rtol=1e-4)
    # a non-finite estimate at a masked-out pixel must not poison the loss (reference: est[mask] never sees it)
    bad = d0.detach().clone()
    bad[~mask] = float("inf")
    bad.requires_grad_()
    ml2 = model_loss([bad, d1.detach()], gt, mask)
    assert torch.isfinite(ml2) and abs(ml2.item() - ml.item()) < 1e-5 * max(1, abs(ml.item()))
    assert torch.isfinite(torch.autograd.grad(ml2, bad)[0]).all()


def test_lr_schedules():
    """adjust_learning_rate (utils/experiment.py:91-109, main_dca.py:254) and learning_rate_adjust (util.py:132-145)."""
    from dcanet_amd.utils import adjust_learning_rate, learning_rate_adjust
    opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=1.0)
    want = {0: 1e-3, 11: 1e-3, 12: 5e-4, 19: 5e-4, 20: 2.5e-4, 24: 1.25e-4, 27: 1.25e-4, 28: 6.25e-5, 39: 6.25e-5}
    for epoch, lr in want.items():
        assert adjust_learning_rate(opt, epoch, 1e-3, "12,20,24,28:2") == pytest.approx(lr)
        assert opt.param_groups[0]["lr"] == pytest.approx(lr)
    for epoch, lr in {0: 1e-3, 299: 1e-3, 300: 1e-4, 599: 1e-4, 600: 1e-5}.items():
        assert learning_rate_adjust(opt, epoch) == pytest.approx(lr)


def test_frozen_weights_and_batched_counters_host_logic():
    """ops.frozen_weights(): memoised per source-tensor identity inside the context only; ops.batched_bn_counters():
    deferred `num_batches_tracked += 1` applied once at exit (a module used twice counts twice)"""
    import dcanet_amd  # noqa: F401
    from dcanet_amd import ops
    t, u, calls = torch.zeros(3), torch.zeros(3), []

    def build():
        calls.append(1)
        return torch.ones(1)
    with ops.frozen_weights():
        a = ops._memo(("k", 1), (t,), build)
        assert ops._memo(("k", 1), (t,), build) is a and len(calls) == 1          # reused
        assert ops._memo(("k", 2), (t,), build) is not a and len(calls) == 2      # another layout of the same weight
        assert ops._memo(("k", 1), (u,), build) is not a and len(calls) == 3      # another tensor
        with ops.frozen_weights():                                                 # nested context: its own cache
            ops._memo(("k", 1), (t,), build)
            assert len(calls) == 4
        assert ops._memo(("k", 1), (t,), build) is a and len(calls) == 4
    ops._memo(("k", 1), (t,), build)
    assert len(calls) == 5 and getattr(ops._tls, "frozen", None) is None           # outside: always rebuilt

    n1, n2 = torch.zeros((), dtype=torch.long), torch.zeros((), dtype=torch.long)
    with ops.batched_bn_counters():
        ops._tls.pending += [n1, n1, n2]
        assert n1.item() == 0
    assert (n1.item(), n2.item()) == (2, 1) and getattr(ops._tls, "pending", None) is None


def test_weight_init_is_bit_identical_to_reference():
    """a10: under the same torch seed a freshly constructed model has the reference's initial weights, bit for bit
    (gwcnet_dca_g.py:173-185 incl. the ConvTranspose3d / Guidance exceptions and the RNG consumption order);
    fixture = per-key fingerprints of the reference's own freshly constructed model (oracle/make_golden.py::gen_init)."""
    import numpy as np
    import dcanet_amd  # noqa: F401
    from dcanet_amd.models.gwcnet_dca_g import GwcNet
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "init_fingerprint.npz")))
    for variant, concat in (("g", False), ("gc", True)):
        torch.manual_seed(1234)
        sd = GwcNet(64, use_concat_volume=concat).state_dict()
        keys = sorted(sd.keys())
        assert len(keys) == g[f"{variant}_fp"].shape[0]
        for i, k in enumerate(keys):
            v = sd[k].double().flatten()
            head = torch.zeros(4, dtype=torch.float64)
            head[:min(4, v.numel())] = v[:4]
            fp = torch.cat([v.sum().view(1), v.abs().sum().view(1), head]).numpy()
            assert np.array_equal(fp, g[f"{variant}_fp"][i]), f"{variant}: {k} differs from the reference's init"


def test_2d_neighbours_match_reference_on_cpu():
    """the PyTorch 2D modules either side of the path (feature_extraction, Guidance) against the
    reference's outputs (tests/golden/whole_g_eval.npz) -- they are plain torch modules, so this runs without a GPU."""
    import json
    import numpy as np
    import dcanet_amd  # noqa: F401
    from dcanet_amd.models.gwcnet_dca_g import GwcNet
    from oracle import dcanet_oracle as O
    from oracle.seeded import seeded_tensor
    with open(os.path.join(ROOT, "tests", "golden", "state_dict_keys.json")) as f:
        shapes = json.load(f)["g"]
    m = GwcNet(32, use_concat_volume=False)
    m.load_state_dict(O.seeded_state_dict({k: tuple(v) for k, v in shapes.items()}), strict=True)
    m.eval()
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "whole_g_eval.npz")))
    left = seeded_tensor("whole.left", (1, 3, 64, 128))
    with torch.no_grad():
        feat = m.feature_extraction(left)["gwc_feature"]
        guid = m.guidance(left)["g"]
    assert (feat[:, ::16] - torch.from_numpy(g["gwc_feature"])).abs().max() < 2e-5
    assert (guid[:, ::8] - torch.from_numpy(g["guidance"])).abs().max() < 2e-5


def test_kitti_wrapper_host_logic(tmp_path):
    """dcanet_amd.inference: my_img.py:47-110's normalisation / padding / cropping / 16-bit PNG, against an independent
    plain-numpy restatement of those lines."""
    import numpy as np
    from PIL import Image
    from dcanet_amd.inference import crop_back, disparity_png, normalize_pair, pad_or_crop
    rng = np.random.default_rng(3)
    left = rng.integers(0, 256, (37, 121, 3), dtype=np.uint8)
    right = rng.integers(0, 256, (37, 121, 3), dtype=np.uint8)
    t = normalize_pair(left, right)
    assert t.shape == (6, 37, 121) and t.dtype == np.float32
    for i, img in enumerate((left, right)):
        for c in range(3):
            want = ((img[:, :, c] - img[:, :, c].mean()) / img[:, :, c].std()).astype("float32")
            assert np.array_equal(t[3 * i + c], want)
            assert abs(float(t[3 * i + c].mean())) < 1e-5 and abs(float(t[3 * i + c].std()) - 1) < 1e-4
    L, R, h, w = pad_or_crop(t, 48, 128)          # smaller than the frame: bottom-left corner, zeros top / right
    assert (h, w) == (37, 121) and L.shape == R.shape == (1, 3, 48, 128)
    assert np.array_equal(L[0, :, 11:, :121].numpy(), t[0:3]) and np.array_equal(R[0, :, 11:, :121].numpy(), t[3:6])
    assert float(L[0, :, :11].abs().max()) == 0 and float(L[0, :, :, 121:].abs().max()) == 0
    disp = rng.random((48, 128)).astype("float32") * 100
    assert np.array_equal(crop_back(disp, h, w, 48, 128), disp[11:, :121])
    L2, R2, h2, w2 = pad_or_crop(t, 32, 64)       # larger than the frame: vertically centred crop from column 0
    assert (h2, w2) == (37, 121) and np.array_equal(L2[0].numpy(), t[0:3, 2:34, 0:64])
    assert crop_back(disp, h2, w2, 32, 64) is disp
    png = str(tmp_path / "000000_10.png")
    disparity_png(png, disp)
    back = np.asarray(Image.open(png))
    assert back.dtype == np.uint16 and np.array_equal(back, (disp * 256).astype("uint16"))


def test_forward_set_attributes_survive_apply():
    """The operand tags (ops.py, "operand scales of the f16x2 kernels") are Python attributes that an autograd Function sets
    on its outputs inside forward().  That rests on one torch property: what apply() returns still carries them, with the
    version counter the tag was stamped with."""
    import threading

    class Tagging(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            y, aux, xa = x * 2, x + 1, x.view_as(x)
            ctx.mark_non_differentiable(aux)
            for i, t in enumerate((y, aux, xa)):
                t._tag = (i, None if t.is_inference() else t._version)
            return y, aux, xa

    def check():
        x = torch.ones(3, requires_grad=True)
        for i, t in enumerate(Tagging.apply(x)):
            assert t._tag == (i, None if t.is_inference() else t._version), (i, t._tag, t._version)

    check()
    assert Tagging.apply(torch.ones(3, requires_grad=True))[0].grad_fn is not None
    with torch.no_grad():
        check()
    with torch.inference_mode():
        check()
    errors = []

    def worker():
        try:
            check()
        except BaseException as e:      # noqa: BLE001 -- handed to the main thread
            errors.append(e)
    th = threading.Thread(target=worker)
    th.start()
    th.join()
    assert not errors, errors


def test_operand_tag_validity():
    """One validity rule for the versioned tags (ops._tag_ok: stamped with the tensor's current version, payload on its
    device): each setter's tag is seen, an in-place update ends it, and _copy_tags hands only valid tags to an alias."""
    import dcanet_amd  # noqa: F401
    from dcanet_amd import ops
    shape = (2, 8, 2, 2, 4)

    def tagged():
        t = torch.ones(shape)
        slots, exps, twin = torch.zeros(8 * ops.CSLOTS, dtype=torch.int32), torch.zeros(8, dtype=torch.int32), torch.ones(shape)
        ops._tag_cmax(t, slots, 3)
        ops._tag_exps(t, exps)
        ops._tag_twin(t, ops._tag_px2(twin, exps))
        return t, slots, exps, twin

    def valid(t):
        return [k for k in ("_dca_cmax", "_dca_exps", "_dca_twin") if ops._tag_ok(t, k) is not None]

    t, slots, exps, twin = tagged()
    assert valid(t) == ["_dca_cmax", "_dca_exps", "_dca_twin"]
    assert t._dca_cmax[0] is slots and t._dca_cmax[1] == 3 and t._dca_cmax[2] == ops._ver(t)
    assert ops._exps_cached(t) is exps and ops._twin_of(t) is twin
    assert ops._is_packed(twin) and ops._exps_cached(twin) is exps and twin._dca_px2[0] is exps
    before = dict(ops.AMAX_STATS)
    assert ops._slots_of(t) == (slots, 3) and ops.AMAX_STATS["tagged"] == before["tagged"] + 1
    # a valid source: all three travel to the alias, restamped for it; the px2 mark never does
    ops._tag_px2(t, exps)
    ta = t.view_as(t)
    ops._copy_tags(t, ta)
    assert valid(ta) == ["_dca_cmax", "_dca_exps", "_dca_twin"] and not ops._is_packed(ta)
    assert ta._dca_cmax[:2] == (slots, 3) and ta._dca_exps[0] is exps and ops._twin_of(ta) is twin
    # an in-place update ends every versioned tag
    t.mul_(2)
    assert valid(t) == [] and ops._twin_of(t) is None
    del t._dca_px2
    assert ops._exps_cached(t) is None
    # ... and a tag that was already stale on the source does not come back to life on an alias (views share the counter)
    x, _, _, _ = tagged()
    x.mul_(1000.)
    xa = x.view_as(x)
    ops._copy_tags(x, xa)
    assert x._dca_cmax[2] != ops._ver(x)
    assert valid(xa) == [] and ops._exps_cached(xa) is None and ops._twin_of(xa) is None
    assert not any(hasattr(xa, k) for k in ("_dca_cmax", "_dca_exps", "_dca_twin", "_dca_px2"))


def test_no_tag_handoff_state():
    """The operand tags are attached where they are made; no thread-local hand-off from a Function to its wrapper."""
    src = open(os.path.join(ROOT, "cost-volume-aggregation-in-stereo-matching-revisited_amd", "ops.py")).read()
    for name in ("last_vmax", "last_twin", "last_zexps"):
        assert name not in src, name
