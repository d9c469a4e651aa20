"""bench.py's contract: `--steps` timed steps and `ms_per_step` in the one JSON line, no rooflines or CPU oracle without
`--full`, and `--dump-outputs DIR` writing what the last timed step computed as float32 DIR/<name>.npy."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_writes_float32_and_a_fixed_sample_of_large_arrays(tmp_path):
    import bench
    big = torch.arange(3 * bench.DUMP_MAX_NUMEL, dtype=torch.float64)
    arrays = {"small": torch.randn(3, 4), "half": torch.ones(5, dtype=torch.bfloat16),
              "loss": torch.tensor(2.0, requires_grad=True) * 3, "big": big}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays)
    for name, t in arrays.items():
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert a.dtype == np.float32 and np.array_equal(a, b), name
        if t.numel() <= bench.DUMP_MAX_NUMEL:
            assert a.shape == tuple(t.shape) and np.array_equal(a, t.detach().float().numpy()), name
    s = np.load(tmp_path / "a" / "big.npy")
    assert s.shape == (bench.DUMP_MAX_NUMEL,) and np.all(np.diff(s) >= 0) and s[-1] > s[0]
    assert np.array_equal(s, np.round(s)) and s.max() < big.numel()      # elements of the array, in index order


def _bench(*args):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--shape", "64x128x32",
                        "--batch", "1"] + list(args), cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-3000:]
    return json.loads(lines[0])


@pytest.mark.gpu
@pytest.mark.timeout(1200)
@pytest.mark.parametrize("mode", ["fwdbwd", "fwd"])
def test_plain_run_times_the_steps_and_dumps_the_last_step(tmp_path, mode):
    args = ["--mode", mode, "--steps", "3", "--warmup", "1", "--dump-outputs"]
    line = _bench(*args, str(tmp_path / "a"))
    assert line["steps"] == 3 and line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(1e3 / line["ms_per_step"], rel=1e-2)
    for k in ("metric", "unit", "higher_is_better", "dtype"):
        assert k in line
    assert not {"roofline", "roofline_other", "cpu_baseline", "vs_cpu_baseline"} & set(line)
    want = {"pred4", "pred4_q", "prob_volume2"}
    if mode == "fwdbwd":
        want |= {"loss", "pred0", "pred1", "pred2", "pred_dca1", "pred_dca2", "pred_dca3", "grad_fL", "grad_fR",
                 "param_grads", "params"}
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert set(got) == want
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    for name, a in got.items():
        assert a.dtype == np.float32 and np.isfinite(a).all(), name
    assert got["pred4"].ndim == 4 and got["pred4"].shape[:2] == (1, 1)
    # same arguments -> same inputs, weights and training steps -> the same outputs
    _bench(*args, str(tmp_path / "b"))
    for name, a in got.items():
        np.testing.assert_allclose(np.load(tmp_path / "b" / f"{name}.npy"), a, rtol=1e-5, atol=1e-6, err_msg=name)
