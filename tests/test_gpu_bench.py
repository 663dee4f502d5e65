"""bench.py as a command on the GPU: a plain run (no --full) on a small matrix times exactly
--steps steps, reports the headline fields only and, with --dump-outputs, saves the C its timed
steps computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


@pytest.mark.gpu
def test_plain_run_dumps_the_timed_output(tmp_path):
    n, b, steps = 320, 64, 3
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps",
                        str(steps), "--warmup", "2", "--edge", str(n), "--block", str(b),
                        "--dump-outputs", str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=170, env=env, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["metric"] == bench.METRIC and d["unit"] == "GB/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f64" and d["steps"] == steps and d["warmup"] == 2 and d["verified"] is True
    assert d["ms_per_step"] > 0
    # the library counted --steps transforms' bytes in the timed pass; value = those over its time
    assert d["config"]["bytes_per_step"] == 2 * 8 * n * n
    assert d["value"] == pytest.approx(2 * 8 * n * n / (d["ms_per_step"] * 1e-3) / 1e9, rel=1e-2)
    # nothing of --full in a plain line
    for key in ("roofline", "cpu_baseline", "e2e_host", "baseline_configs", "blocking",
                "with_phase_events", "call_overhead_us"):
        assert key not in d
    assert os.listdir(tmp_path / "out") == ["C.npy"]
    got = np.load(tmp_path / "out" / "C.npy")
    assert got.dtype == np.float64 and got.shape == (n * n,)
    # C = A^T, column-major: C[i + j * n] = A(j, i)
    i = torch.arange(n, dtype=torch.int64)
    want = bench.pos_values(i[:, None], i[None, :], bench.SEED_A, "f64")  # [col j of C][row i]
    assert np.array_equal(got.reshape(n, n), want.numpy())
