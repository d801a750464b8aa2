"""bench.py as the driver runs it on one GPU: a plain run prints the headline only, --dump-outputs writes what the last
timed step computed, and two runs with the same arguments give the same outputs up to rounding, however many steps they time
(the float atomics' summation order makes two trajectories drift apart over thousands of training steps: the dumped step
starts again from the set-up state)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + list(args), cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_run_dumps_the_last_step_and_repeats(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    runs = []
    for name in ("a", "b"):
        out = _bench("--steps", "5000", "--warmup", "10", "--dump-outputs", str(tmp_path / name))
        assert out["steps"] == 5000 and out["warmup"] == 10 and out["dtype"] == "fp32" and out["unit"] == "samples/s"
        assert out["higher_is_better"] is True and out["ms_per_step"] > 0
        # value and ms_per_step describe the same timed steps (ms_per_step is rounded to 0.1 us)
        assert abs(out["value"] - 32e3 / out["ms_per_step"]) <= 2e-3 * out["value"]
        assert "roofline" not in out and "cpu_baseline" not in out
        runs.append({n: np.load(tmp_path / name / (n + ".npy")) for n in ("losses", "params", "grads")})
    a, b = runs
    n_params = out["config"]["params"]
    assert a["params"].shape == a["grads"].shape == (n_params,) and a["losses"].ndim == 1
    for n in a:
        assert a[n].dtype == np.float32 and np.isfinite(a[n]).all(), n
        # the same inputs: equal up to the summation order of the atomics (measured <= 2e-7; different weights, data or
        # dropout masks, or trajectories drifted over the 5000 steps, differ at the size of the values themselves)
        assert np.abs(a[n] - b[n]).max() <= 1e-5 * np.abs(a[n]).max(), n
