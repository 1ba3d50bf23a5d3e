"""bench.py's plain run: the headline line and nothing beyond it (the rest is --full), --steps as the number of
timed steps, and --dump-outputs writing what a step of the timed path computed - the same arrays, to rounding, from
two runs with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("loss", "grads", "params", "buffers")


def _bench(dump):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--batch", "2", "--dump-outputs", str(dump)]
    r = subprocess.run(cmd, env=dict(os.environ, PYTHONPATH=ROOT), cwd=ROOT, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), {n: np.load(dump / (n + ".npy")) for n in NAMES}


def test_plain_bench_line_and_dumped_outputs(tmp_path):
    out, a = _bench(tmp_path / "a")
    assert out["n_gpus"] == 1 and out["steps"] == 3 and out["warmup"] == 1
    assert out["unit"] == "scenes/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
    # value = the scenes of the --steps timed steps over their time; ms_per_step = that time per step
    assert abs(out["value"] - 2 * 3 / (out["ms_per_step"] * 3e-3)) < 1e-6 * out["value"]
    for k in ("repeat_ms_per_step", "roofline", "roofline_step", "secondary", "cpu_baseline", "pmc_live"):
        assert k not in out, k
    for n, v in a.items():
        assert v.dtype == np.float32 and v.size > 0 and np.isfinite(v).all(), n
    assert a["loss"].shape == (1,) and a["grads"].shape == a["params"].shape
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    # a second run with the same arguments: the same inputs, so the same outputs up to the rounding of float
    # atomics (and, in the parameters, AdamW's first step turning gradients that are rounding noise into +-lr)
    _, b = _bench(tmp_path / "b")
    for n, tol in (("loss", 1e-5), ("grads", 1e-4), ("buffers", 1e-4), ("params", 1e-3)):
        x, y = a[n].astype(np.float64), b[n].astype(np.float64)
        assert x.shape == y.shape, n
        assert np.linalg.norm(x - y) <= tol * np.linalg.norm(x), (n, np.linalg.norm(x - y) / np.linalg.norm(x))
