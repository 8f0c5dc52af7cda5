"""bench.py's plain run on the GPU: exactly --steps timed steps, the contract's fields in the
last line, and --dump-outputs writing what the last timed step returned -- checked here
against the CPU oracle, since a plain run no longer compares with it itself (--full does)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_dumps_the_timed_outputs(tmp_path):
    import bench  # (for the workload: the run's inputs, rebuilt here for the oracle)
    import oracle_lib as O
    out = tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1",
                        "--steps", "3", "--warmup", "1", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert line["unit"] == "trees/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["value"] == pytest.approx(1000 / (line["ms_per_step"] / 1e3), rel=1e-4)
    assert "cpu_baseline" not in line and "also" not in line  # (--full only)
    ll = np.load(out / "log_likelihoods.npy")
    g = np.load(out / "branch_length_gradients.npy")
    site = np.load(out / "site_model_gradients.npy")
    assert ll.shape == (1000,) and g.shape == (1000, 53) and site.shape == (1000,)
    assert ll.dtype == g.dtype == site.dtype == np.float64
    tips, w, pids, bls = bench.ds1_workload(1000)
    params = np.ones((1000, 2))
    k = 4
    og = O.unrooted_gradients(O.make_spec(27, tips.shape[1], "JC69", "weibull+4"), tips, w,
                              pids[:k], bls[:k], params[:k], False, k)
    assert np.max(np.abs(ll[:k] - og["log_likelihood"]) / np.abs(og["log_likelihood"])) <= 1e-10
    assert (np.max(np.abs(g[:k] - og["branch_lengths"]))
            <= 1e-10 * np.max(np.abs(og["branch_lengths"])))
    assert np.max(np.abs(site[:k] - og["site_model"]) / np.abs(og["site_model"])) <= 1e-10
