"""bench.py's plain run (the headline only) and its --dump-outputs files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args, timeout=600):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_bench_times_its_steps_and_dumps_the_last_step(tmp_path):
    """A plain run prints the contract's keys with `steps` timed steps and nothing of --full (no roofline, CPU baseline or extra legs);
    --dump-outputs writes the last timed step's loss, parameters and state samples as float32 .npy files within 64 MB, and a second
    run with the same arguments writes the same values."""
    args = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--global-batch", "8192"]
    runs = []
    for k in range(2):
        j = _bench(*args, "--dump-outputs", str(tmp_path / f"d{k}"))
        assert j["steps"] == 3 and j["warmup"] == 1 and j["n_gpus"] == 1 and j["higher_is_better"] is True
        assert j["unit"] == "poses/s" and j["dtype"] == "bf16" and j["metric"].startswith("poses/sec score-net train step")
        assert j["value"] > 0 and abs(j["value"] - 8192 / (j["ms_per_step"] * 1e-3)) / j["value"] < 1e-6
        assert j["roofline"] is None and j["cpu_baseline"] is None
        assert not {"sampler", "fk_joints", "train_step_fp32_mode", "small_batches", "gemm_kernels"} & set(j["extra"])
        runs.append(j)
    names = sorted(os.listdir(tmp_path / "d0"))
    assert names == ["adam_m_sample.npy", "adam_v_sample.npy", "ema_params_sample.npy", "params.npy", "step_loss.npy"]
    assert sum(os.path.getsize(tmp_path / "d0" / n) for n in names) <= 64 << 20
    a = {n[:-4]: np.load(tmp_path / "d0" / n) for n in names}
    b = {n[:-4]: np.load(tmp_path / "d1" / n) for n in names}
    for n in a:
        assert a[n].dtype == np.float32 and np.isfinite(a[n]).all(), n
        assert np.array_equal(a[n], b[n]), n
    assert a["params"].size == 8277567 and a["ema_params_sample"].size == 1 << 20
    assert float(a["step_loss"][0]) == pytest.approx(runs[0]["extra"]["train_loss_last_step"], rel=1e-6)
