"""bench.py on the GPU: a plain run measures the headline only and ``--dump-outputs``
writes what the last timed step left (``--full`` adds the extra keys and is not run
here: it times every comparator)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
            "vs_baseline", "dtype", "data", "config"}


def test_plain_run_is_headline_only_and_dumps_last_step(tmp_path):
    e = dict(os.environ, PYTHONPATH=ROOT)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "6", "--warmup", "3",
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=120, cwd=ROOT, env=e)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert set(out) == HEADLINE, sorted(set(out) ^ HEADLINE)
    assert out["steps"] == 6 and out["ms_per_step"] > 0 and out["config"]["graph"] is True
    assert "phase=extra:" not in r.stderr
    assert sorted(os.listdir(tmp_path)) == ["loss.npy", "params.npy"]
    loss, params = np.load(tmp_path / "loss.npy"), np.load(tmp_path / "params.npy")
    assert loss.dtype == np.float32 and params.dtype == np.float32
    assert loss.nbytes + params.nbytes <= 64 << 20
    assert abs(float(loss[0]) - out["config"]["final_loss"]) < 1e-5
    assert np.isfinite(params).all() and params.std() > 0
