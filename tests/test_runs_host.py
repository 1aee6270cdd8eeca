"""Run batches without a GPU: the refusals of fdr_rollout_runs / fdr_obs_stats_merge_runs / fdr_fd_step_runs (before any
device work), the PopulationRunner's id layout as pure numpy functions, its statistics -> (mean, std) step against
WelfordRunningStat bit for bit, and the conditioning of the learner cases tests/test_gpu_runs.py runs."""
import ctypes

import numpy as np
import pytest
import torch

import learner_cases as lc
import runs_ref as rr

ONE = 1     # a non-NULL pointer value that no refused call dereferences


@pytest.fixture(scope="module")
def L():
    from fdr import _lib
    return _lib


def _err(L):
    return L.lib.fdr_last_error().decode()


# ---- 1. refusals ---------------------------------------------------------------------------------------------------
def _rollout(L, policy=None, env=None, R=2, lanes=3, theta=ONE, sigma=ONE, off=ONE, ret=ONE, steps=ONE, K=1, om=None,
             osd=None):
    pd = L.PolicyDesc(L.FDR_POLICY_LINEAR, 4, 2, 0, 8, None, None) if policy is None else policy
    ed = L.EnvDesc(L.FDR_ENV_CARTPOLE, 4, 2, 100, None, None, None, None, 0, 0, 0.0, 0) if env is None else env
    return L.lib.fdr_rollout_runs(None, ctypes.byref(pd), ctypes.byref(ed), R, lanes, theta, sigma, om, osd, off, None, 0,
                                  None, None, 5, 0, K, None, ret, None, None, steps, None, None, None, None, 0.0, None)


def test_rollout_runs_invalid(L):
    for kw in (dict(theta=None), dict(sigma=None), dict(off=None), dict(ret=None), dict(steps=None), dict(R=0),
               dict(R=-1), dict(lanes=0), dict(K=0), dict(K=1025), dict(om=ONE), dict(R=1 << 20, lanes=1 << 12)):
        assert _rollout(L, **kw) == L.FDR_ERR_INVALID, kw
    assert L.lib.fdr_rollout_runs(None, None, None, 1, 1, ONE, ONE, None, None, ONE, None, 0, None, None, 5, 0, 1, None,
                                  ONE, None, None, ONE, None, None, None, None, 0.0, None) == L.FDR_ERR_INVALID


def test_rollout_runs_unsupported(L):
    for kind, hidden, P in ((L.FDR_POLICY_DISCRETE, 64, 4610), (L.FDR_POLICY_MUJOCO, 64, 4610)):
        assert _rollout(L, policy=L.PolicyDesc(kind, 4, 2, hidden, P, None, None)) == L.FDR_ERR_UNSUPPORTED
        assert "linear" in _err(L)
    # a non-physics env (the synthetic one, with its matrices given)
    synth = L.EnvDesc(L.FDR_ENV_SYNTH, 4, 2, 100, ONE, ONE, ONE, None, 0, 0, 0.0, 0)
    assert _rollout(L, env=synth) == L.FDR_ERR_UNSUPPORTED
    assert "physics" in _err(L)
    # a shape that is not the env's own
    assert _rollout(L, policy=L.PolicyDesc(L.FDR_POLICY_LINEAR, 3, 2, 0, 6, None, None)) == L.FDR_ERR_UNSUPPORTED
    assert "own" in _err(L)


def _step(L, table=ONE, table_size=100, idx=ONE, R=2, n_train=8, lpd=2, P=8, stride=8, theta=ONE, lr=ONE, out=ONE):
    return L.lib.fdr_fd_step_runs(None, table, table_size, idx, ONE, ONE, ONE, stride, R, n_train, lpd, P, None, ONE, None,
                                  theta, lr, 1.0, None, out, None)


def test_fd_step_runs_refusals(L):
    for kw in (dict(table=None), dict(idx=None), dict(theta=None), dict(lr=None), dict(out=None), dict(R=0),
               dict(stride=7), dict(n_train=7), dict(n_train=0), dict(lpd=0), dict(table_size=7)):
        assert _step(L, **kw) == L.FDR_ERR_INVALID, kw
    assert _step(L, P=33, table_size=100) == L.FDR_ERR_UNSUPPORTED
    assert "32" in _err(L) and "n_params" in _err(L)
    assert _step(L, n_train=4098, stride=4098) == L.FDR_ERR_UNSUPPORTED
    assert "4096" in _err(L)


def test_obs_stats_merge_runs_refusals(L):
    f = L.lib.fdr_obs_stats_merge_runs
    assert f(None, ONE, ONE, ONE, 0, 3, 4, ONE, ONE, ONE, None) == L.FDR_ERR_INVALID
    assert f(None, ONE, ONE, ONE, 2, 0, 4, ONE, ONE, ONE, None) == L.FDR_ERR_INVALID
    assert f(None, ONE, ONE, ONE, 2, 3, 0, ONE, ONE, ONE, None) == L.FDR_ERR_INVALID
    assert f(None, None, ONE, ONE, 2, 3, 4, ONE, ONE, ONE, None) == L.FDR_ERR_INVALID
    assert f(None, ONE, ONE, ONE, 2, 3, 4, ONE, ONE, None, None) == L.FDR_ERR_INVALID
    assert f(None, ONE, ONE, ONE, 2, 3, 1025, ONE, ONE, ONE, None) == L.FDR_ERR_UNSUPPORTED


def test_engine_wrappers_exist():
    from fdr import engine
    assert callable(engine.rollout_runs) and callable(engine.obs_stats_merge_runs) and callable(engine.fd_step_runs)


# ---- 2. the runner's id layout -------------------------------------------------------------------------------------
def test_ids_are_distinct_across_runs_and_bounded():
    import run_population as rp
    seeds, D, lpd, E, K = [0, 1, 5, 1000, 4321], 16, 2, 4, 3
    Lr = D * lpd + E
    s = rp.check_seeds(seeds, Lr, K)
    ids = np.concatenate([rp.direction_ids(s, e, D) for e in range(4)], 1)
    assert ids.dtype == np.int64 and ids.min() >= 0 and np.unique(ids).size == ids.size
    for r, seed in enumerate(seeds):
        assert np.all(ids[r] >> 32 == seed) and np.all((ids[r] & 0xffffffff) == np.arange(4 * D))
    for crn in (False, "pair"):
        st = rp.stream_ids(s, D, lpd, E, K, crn)
        if crn is False:
            assert st is None       # the kernel's default: (offset + l) K + e
            st = np.concatenate([(o + np.arange(Lr))[:, None] * K + np.arange(K)[None, :]
                                 for o in rp.run_lane_offsets(s, Lr)])
        st = st.reshape(len(seeds), Lr, K)
        assert st.min() >= 0 and st.max() < (1 << 32)
        per_run = [set(st[r].reshape(-1).tolist()) for r in range(len(seeds))]
        for a in range(len(seeds)):
            for b in range(a + 1, len(seeds)):
                assert not (per_run[a] & per_run[b])
        if crn == "pair":
            np.testing.assert_array_equal(st[:, 0:2 * D:2], st[:, 1:2 * D:2])       # +- pairs share their streams
            assert np.unique(st[:, 2 * D:].reshape(len(seeds), -1), axis=1).shape[1] == E * K
    np.testing.assert_array_equal(rp.run_lane_offsets(s, Lr), np.asarray(seeds) * Lr)


def test_a_seeds_ids_do_not_depend_on_the_population():
    import run_population as rp
    D, lpd, E, K = 8, 2, 2, 2
    Lr = D * lpd + E
    alone = (rp.direction_ids([7], 3, D)[0], rp.run_lane_offsets([7], Lr)[0], rp.stream_ids([7], D, lpd, E, K, "pair"))
    for seeds in ([7, 1, 2, 3, 4], [1, 2, 7, 3, 4], [4, 3, 2, 1, 7]):
        r = seeds.index(7)
        np.testing.assert_array_equal(rp.direction_ids(seeds, 3, D)[r], alone[0])
        assert rp.run_lane_offsets(seeds, Lr)[r] == alone[1]
        np.testing.assert_array_equal(rp.stream_ids(seeds, D, lpd, E, K, "pair").reshape(5, Lr, K)[r], alone[2])
    assert rp.launch_key(3, 5) == rp.launch_key(3, 5) != rp.launch_key(3, 6)


def test_overlarge_seeds_are_refused():
    import run_population as rp
    Lr, K = 520, 1
    ok = (1 << 32) // (Lr * K) - 1
    rp.check_seeds([ok], Lr, K)
    for bad in ([ok + 1], [-1], [1 << 31], [3, 3], []):
        with pytest.raises(ValueError):
            rp.check_seeds(bad, Lr, K)
    with pytest.raises(ValueError):
        rp.direction_ids([1], (1 << 32) // 256, 256)
    with pytest.raises(ValueError):
        rp.PopulationRunner(seeds=[ok + 1], batch_size=256, eval_lanes=8, device="cpu")
    with pytest.raises(ValueError):
        rp.PopulationRunner(env_id="Walker2d-v2", n_runs=2, device="cpu")


# ---- 3. statistics -> (mean, std) ----------------------------------------------------------------------------------
def test_obs_norm_matches_welford_bitwise():
    import run_population as rp
    from utils.math_helpers import WelfordRunningStat
    rs = np.random.RandomState(5)
    d = 6
    counts = [0, 1, 2, 1000]
    stats = []
    for n in counts:
        w = WelfordRunningStat((d,))
        x = rs.randn(max(n, 1), d).astype(np.float32) * np.float32(3)
        x[:, 2] = np.float32(0.5)           # an element with zero variance
        for i in range(n):
            w.update(x[i])
        stats.append(w)
    mean = torch.from_numpy(np.stack([w.running_mean for w in stats]))
    m2 = torch.from_numpy(np.stack([w.running_variance for w in stats]))
    cnt = torch.tensor(counts, dtype=torch.int64)
    om, osd = rp.obs_norm_from_stats(mean, m2, cnt)
    assert om.dtype == torch.float32 and osd.dtype == torch.float32
    for r, w in enumerate(stats):
        want_m, want_s = np.asarray(w.mean, np.float32), np.asarray(w.std, np.float32)
        assert om[r].numpy().tobytes() == want_m.tobytes(), counts[r]
        assert osd[r].numpy().tobytes() == want_s.tobytes(), counts[r]
    assert np.all(osd[:2].numpy() == 1) and np.all(om[:2].numpy() == 0)
    assert osd[2, 2] == 1 and osd[3, 2] == 1 and m2[3, 2] == 0


def test_row_sums_depend_on_the_row_alone():
    import run_population as rp
    x = torch.from_numpy(np.random.RandomState(2).randn(5, 517))
    s = rp.row_sums(x)
    for r in range(5):
        assert rp.row_sums(x[r:r + 1].clone())[0].item() == s[r].item()
    np.testing.assert_allclose(s.numpy(), x.numpy().sum(1), rtol=1e-13)


# ---- 4. the learner cases of the GPU test are well conditioned -------------------------------------------------------
@pytest.mark.parametrize("shape", rr.LEARNER_SHAPES, ids=lambda s: "D%d-lpd%d-P%d-R%d" % s[:4])
def test_learner_cases_are_conditioned(shape):
    D, lpd, P, R, first = shape
    table, runs = rr.learner_batch(*shape)
    assert len(runs) == R and table.size == P + rr.ROOM
    if R == 130:
        assert {u.kind for u in runs} == set(rr.KINDS)
    for u in runs:
        assert u.idx.max() <= rr.ROOM and u.idx.min() >= 0
        if u.kind in rr.POISONED or u.kind == "zero":
            continue
        assert u.kappa() <= lc.KAPPA_MAX, (u.kind, u.kappa())
        if u.kind == "ties" and D >= 255:
            import top_dirs_ref as tref
            s = tref.scores(u.r, lpd)
            keep = tref.selected(u.r, lpd, u.b)
            assert s[keep].min() == s[~keep].max()      # tied scores across the cut
