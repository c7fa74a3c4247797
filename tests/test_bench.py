"""bench.py's own contract: a plain run times the steps and prints the headline line only; ``--dump-outputs DIR`` writes
what the last timed step computed (float32 / float64 .npy, bounded in size, the same for the same arguments)."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMP_LIMIT = 64 * 10 ** 6


def _load_dump(path):
    arrays = {f[:-4]: np.load(os.path.join(path, f)) for f in sorted(os.listdir(path)) if f.endswith(".npy")}
    total = sum(os.path.getsize(os.path.join(path, f)) for f in os.listdir(path))
    return arrays, total


@pytest.mark.parametrize("n", [1000, 15_000_000])
def test_dump_outputs_budget_and_fixed_sample(tmp_path, n):
    """Small parameter buffers are written whole; beyond the byte budget a sample at a fixed index set, the same on every
    call, keeps the dump under 64 MB."""
    import bench
    model = types.SimpleNamespace(model=types.SimpleNamespace(store=types.SimpleNamespace(w=torch.arange(n, dtype=torch.float32))))
    sums = torch.rand(13, 3)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), model, sums, 12.5)
    a, total = _load_dump(str(tmp_path / "a"))
    b, _ = _load_dump(str(tmp_path / "b"))
    assert total <= DUMP_LIMIT
    assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert np.array_equal(a["loss_sums"], sums.numpy()) and a["loss"].tolist() == [12.5]
    if n == 1000:
        assert np.array_equal(a["params"], np.arange(n, dtype=np.float32))
    else:
        s = a["params_sample"]
        assert "params" not in a and s.size > n // 2
        assert np.all(np.diff(s) > 0) and s[0] >= 0 and s[-1] < n      # distinct entries of w, in index order


@pytest.mark.gpu
def test_bench_plain_run_and_dump_outputs(tmp_path):
    """A plain run carries the headline fields and none of what --full adds; two runs with the same arguments dump the
    same outputs (same inputs, same step count)."""
    lines = {}
    for d in ("a", "b"):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "6", "--warmup", "2", "--batch", "16",
               "--dump-outputs", str(tmp_path / d)]
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stderr[-2000:]
        lines[d] = json.loads(res.stdout.strip().splitlines()[-1])
    line = lines["a"]
    assert line["metric"] == "elements_per_sec_train_step" and line["unit"] == "elements/s" and line["higher_is_better"] is True
    assert line["dtype"] == "bf16" and line["steps"] == 6 and line["value"] > 0 and line["ms_per_step"] > 0
    assert abs(line["value"] - 16 * 128 / (line["ms_per_step"] * 1e-3)) < 1e-6 * line["value"]
    for key in ("roofline", "cpu_baseline", "ms_per_step_median", "bf16_loss_rel_dev"):
        assert key not in line, key
    a, total = _load_dump(str(tmp_path / "a"))
    b, _ = _load_dump(str(tmp_path / "b"))
    assert total <= DUMP_LIMIT and sorted(a) == sorted(b) == ["loss", "loss_sums", "params"]
    assert all(v.dtype in (np.float32, np.float64) and np.isfinite(v).all() for v in a.values())
    assert a["params"].size == line["config"]["params"]
    assert abs(float(a["loss"][0]) - line["final_loss"]) <= 1e-9 * abs(line["final_loss"])
    # (the loss sums are accumulated with float atomics: equal to rounding, not bit for bit)
    for k in a:
        np.testing.assert_allclose(a[k], b[k], rtol=1e-4, atol=1e-6, err_msg=k)
