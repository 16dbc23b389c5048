"""`python bench.py` as it is run for every change: a plain run times exactly --steps steps, prints the headline line without the
legs of --full, and --dump-outputs writes the last timed step's outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_line_and_dumped_outputs(tmp_path):
    out_dir = tmp_path / "outputs"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2",
                        "--dump-outputs", str(out_dir)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["metric"] == "servo_updates_per_sec" and line["unit"] == "updates/s" and line["higher_is_better"] is True
    assert line["dtype"] == "bf16" and line["steps"] == 7 and line["warmup"] == 2 and line["n_gpus"] == 1
    assert line["ms_per_step"] > 0 and line["value"] == pytest.approx(1e3 / line["ms_per_step"], rel=2e-3)
    for leg in ("sequential", "roofline", "parity", "secondary", "cpu_baseline", "kernels", "latency_ms_with_host_sync"):
        assert leg not in line, f"{leg} belongs to --full"
    v_c = np.load(out_dir / "v_c.npy")
    status = np.load(out_dir / "status.npy")
    assert v_c.dtype == np.float64 and v_c.shape == (1, 6) and status.dtype == np.float64 and status.shape == (1,)
    assert np.all(np.isfinite(v_c)) and status[0] == 0 and line["status"] == [0]
    assert v_c[0].tolist() == line["v_c"]
    assert sorted(os.listdir(out_dir)) == ["status.npy", "v_c.npy"]
