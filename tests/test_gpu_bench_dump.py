"""GPU: bench.py's plain run and --dump-outputs.  A plain run prints the headline line without the --full legs; the
timed steps start from the set-up state whatever ran before them (the clock settle runs a number of untimed steps
that depends on the machine), so two runs that differ only in their untimed steps (--warmup 1 / 4) dump
bit-identical outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("reward", "entropy", "timesteps", "norm2", "grad", "theta", "update")


def _bench(out, warmup):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "FDR_BENCH_REHEARSE")}
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", str(warmup), "--settle-ms", "0",
           "--perturbations", "512", "--episode-len", "50", "--dump-outputs", out]
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_dumps_reproducible_outputs(tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    d = _bench(a, 1)
    d2 = _bench(b, 4)
    assert d["warmup"] == 1 and d2["warmup"] == 4                  # different histories before the timed steps
    assert d["steps"] == 3 and d["value"] > 0 and d["ms_per_step"] > 0
    assert d["unit"] == "env steps/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert abs(d["value"] - 512 * 50 * 3 / (3 * d["ms_per_step"] * 1e-3)) <= 1e-3 * d["value"]
    # the legs behind --full did not run
    assert d["full"] is False and d["roofline"] is None and d["cpu_baseline"] is None and d["variants"] is None
    assert sorted(os.listdir(a)) == sorted(n + ".npy" for n in NAMES)
    total = 0
    for n in NAMES:
        x, y = np.load(os.path.join(a, n + ".npy")), np.load(os.path.join(b, n + ".npy"))
        assert x.dtype in (np.float32, np.float64) and np.all(np.isfinite(x))
        assert np.array_equal(x, y), n
        total += x.nbytes
    assert total <= 64 << 20
    assert np.load(os.path.join(a, "reward.npy")).shape == (512,)
    assert np.load(os.path.join(a, "update.npy"))[1] > 0            # ||grad|| of the last timed step
