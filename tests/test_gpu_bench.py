"""bench.py's two modes on a small batch: a plain run prints the headline alone, and its headline update computes what the
headline of a ``--full`` run computes (same sample, same ring leaves and stamps, the last timed update from the initial
parameters and optimiser state)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--global-envs", "16", "--rollout-len", "8"]
# what only a --full run measures (configs / scaling_model and cpu_baseline are left out below: minutes at their own sizes)
FULL_ONLY = {"roofline", "roofline_gae", "roofline_mlp", "kernel_ms_per_step", "launches_per_step", "resident_in_hbm",
             "from_pinned_host", "rollout_inference", "closed_loop", "configs", "scaling_model", "cpu_baseline"}


def _bench(*args):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *SMALL, *args], cwd=ROOT, capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_is_the_headline_of_the_full_run(tmp_path):
    plain = _bench("--dump-outputs", str(tmp_path / "plain"))
    full = _bench("--full", "--no-configs", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / "full"))
    assert not FULL_ONLY & set(plain), sorted(FULL_ONLY & set(plain))
    assert FULL_ONLY - {"configs", "scaling_model", "cpu_baseline"} <= set(full), sorted(set(full))
    for k in ("metric", "unit", "higher_is_better", "dtype", "steps", "warmup", "value_basis"):
        assert plain[k] == full[k], (k, plain[k], full[k])
    pc, fc = dict(plain["config"]), dict(full["config"])
    assert pc.pop("policy_loss") == pytest.approx(fc.pop("policy_loss"), rel=1e-5, abs=1e-7) and pc == fc, (pc, fc)
    assert plain["value"] > 0 and plain["ms_per_step"] > 0
    # the same leaves cross the link in the headline's steps (advantages and returns included), every frame row bound
    assert plain["ring_fed"]["h2d_bytes_per_step_per_gpu"] == full["ring_fed"]["h2d_bytes_per_step_per_gpu"]
    assert plain["ring_fed"]["obs_ring"]["rows_patched"] == 0 and plain["ring_fed"]["obs_ring"]["binds_failed"] == 0
    names = sorted(os.listdir(tmp_path / "plain"))
    assert names and names == sorted(os.listdir(tmp_path / "full"))
    for n in names:
        a, b = np.load(tmp_path / "plain" / n), np.load(tmp_path / "full" / n)
        assert a.shape == b.shape and a.dtype == b.dtype, n
        # one update from the same inputs: equal up to the rounding of its reductions (atomics, stream order)
        np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-6, err_msg=n)
