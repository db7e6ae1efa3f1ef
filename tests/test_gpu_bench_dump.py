"""`bench.py --dump-outputs DIR` at a reduced size: the line reports the timed steps it was asked for, and two runs with the same
arguments write the same arrays (float64, well under 64 MB) -- what a comparison of two builds output for output relies on."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def _bench(out_dir, steps):
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--ny", "64",
           "--no-cpu-baseline", "--no-strict-leg", "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def test_bench_dump_outputs_are_reproducible(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    line = _bench(a, 3)
    assert line["steps"] == 3 and line["ms_per_step"] > 0
    _bench(b, 2)
    names = sorted(p.name for p in a.glob("*.npy"))
    assert names == ["alphas.npy", "basis.npy", "betas.npy", "residual.npy"]
    assert sorted(p.name for p in b.glob("*.npy")) == names
    assert sum(p.stat().st_size for p in a.glob("*.npy")) <= 64 << 20
    for n in names:
        x, y = np.load(a / n), np.load(b / n)
        assert x.dtype == np.float64 and np.all(np.isfinite(x))
        np.testing.assert_allclose(y, x, rtol=1e-12, atol=1e-12 * np.abs(x).max(), err_msg=n)
    assert np.load(a / "basis.npy").shape[1] == 100
    assert np.load(a / "alphas.npy")[-1] == line["last_alpha"]
