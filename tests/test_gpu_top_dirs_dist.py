"""GPU: the sharded top-b direction step equals the single process (tools/dist_check.py, as
tests/test_gpu_dist_equivalence.py drives it for the z-score and the centred rank).

weighting "top_directions:0.25" takes the gather form -- one all-gather of the returns, the selection over the
directions of ALL ranks on every rank, one all-reduce of g.  Preset "small": Worker.evaluate(lane_range="auto") +
FiniteDifferences.step on FDBatches, 96 antithetic directions over 2 ranks; preset "uneven": lists of FDReturn split
unevenly, one rank empty in two of the three steps (every return a direction of its own).  Both ranks' theta must be
bitwise equal, and within 1e-6 of the single-process theta."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(ROOT, "tools", "dist_check.py")
WEIGHTING = "top_directions:0.25"

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("port,preset", [(29571, "small"), (29572, "uneven")])
def test_two_rank_top_directions_steps_equal_one_rank(tmp_path, port, preset):
    out = str(tmp_path)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    p = subprocess.run([sys.executable, SCRIPT, "single", WEIGHTING, out, preset], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=180)
    assert p.returncode == 0, p.stderr[-2000:]
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", str(port), SCRIPT, "multi", WEIGHTING, out,
                        preset], cwd=ROOT, env=env, capture_output=True, text=True, timeout=180)
    assert p.returncode == 0, p.stderr[-2000:]
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import dist_check
    finally:
        sys.path.pop(0)
    err = dist_check.compare(out)       # asserts the ranks bitwise equal
    assert err <= 1e-6, err
    u1 = np.load(os.path.join(out, "upd_single.npy"))
    u0 = np.load(os.path.join(out, "upd_rank0.npy"))
    np.testing.assert_array_equal(u0, np.load(os.path.join(out, "upd_rank1.npy")))
    np.testing.assert_allclose(u0, u1, rtol=1e-6)
    assert np.all(u0 > 0)
