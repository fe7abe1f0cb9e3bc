"""bench.py's command line on the GPU: a plain run times exactly --steps asks and prints the
headline fields alone (everything else is behind --full), and --dump-outputs writes what the
last timed ask returned as float64 .npy files.  The run is a fresh interpreter (the test is
about the command) with the smallest step counts: 1 warm-up, 2 timed asks."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("roofline", "kernels", "kernel_ms", "sharded_ask", "eval_pass", "qlognehvi", "linalg", "cpu_baseline",
             "gp_posterior_ms", "gp_posterior", "config1")


def test_plain_run_line_and_dumped_outputs(tmp_path):
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--dump-outputs", str(out)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, f"bench.py failed (rc {r.returncode}):\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    res = json.loads(lines[0])
    assert res["steps"] == 2 and res["warmup"] == 1 and res["n_gpus"] == 1
    assert res["unit"] == "candidates/s" and res["higher_is_better"] is True and res["dtype"] == "f64"
    assert res["metric"].startswith("QnehviStrategy.ask() candidates/sec")
    assert res["ms_per_step"] > 0 and res["value"] > 0
    # value = evaluations / wall time of the timed asks, ms_per_step = that wall time / steps
    assert res["value"] == pytest.approx(res["ask"]["evals_per_ask"] / (res["ms_per_step"] * 1e-3), rel=1e-3)
    assert not [k for k in FULL_ONLY if k in res], sorted(res)
    cand = np.load(out / "candidate.npy")
    acq = np.load(out / "acq_value.npy")
    assert cand.dtype == np.float64 and acq.dtype == np.float64
    cols = res["outputs"]["candidate_columns"]
    assert cand.shape == (1, len(cols)) and acq.shape == (1,)
    assert res["outputs"]["files"] == {"candidate.npy": [1, len(cols)], "acq_value.npy": [1]}
    assert cols[:6] == [f"x_{i}" for i in range(6)]
    assert np.isfinite(cand).all() and np.isfinite(acq).all()
    assert ((cand[0, :6] >= 0.0) & (cand[0, :6] <= 1.0)).all()
