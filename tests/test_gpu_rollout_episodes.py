"""GPU: fdr_rollout_episodes -- K episodes per lane in one launch, random streams chosen by the caller.

Episode e of lane l must be exactly the episode the one-lane kernel runs for global lane id id(l, e).  The new kernel
inlines the same env step functions as rollout_kernel, so K = 1 and the K-launch decomposition are compared bit for
bit; the CartPole oracle comparisons use tests/episodes_ref.py (seeds verified in tests/test_rollout_episodes_ref.py).
"""
import numpy as np
import pytest
import torch

import episodes_ref as eref
from oracle import obs_stats as ostats
from test_gpu_physics_envs import (DEV, SIGMA, _CACHE, _code, _dev, case_short, lanes_mixed, policy_and_table)

pytestmark = pytest.mark.gpu

# env -> (policy kind, n_in, n_act, short time limit): terminating and time-limited lanes both occur
ENVS = {"CartPoleEnv": ("discrete", 4, 2, 60), "PendulumEnv": ("mujoco", 3, 1, 65),
        "AcrobotEnv": ("discrete", 6, 3, 40), "MountainCarEnv": ("discrete", 2, 3, 70),
        "MountainCarContinuousEnv": ("mujoco", 2, 1, 70)}
OBS_NORM = {4: ([0.01, -0.1, 0.005, 0.2], [0.05, 0.5, 0.04, 0.7]), 3: ([0.1, -0.2, 0.3], [0.7, 0.6, 2.0]),
            6: ([0.9, 0.0, 0.9, 0.0, 0.1, -0.1], [0.1, 0.2, 0.1, 0.3, 0.5, 0.8]), 2: ([-0.5, 0.0], [0.1, 0.01])}


@pytest.fixture(scope="module")
def eng():
    from fdr import engine
    assert hasattr(engine, "rollout_episodes")
    return engine


def _env(name, T=None):
    import envs
    return getattr(envs, name)(ENVS[name][3] if T is None else T)


def _lanes(eng, kind, n_in, n_act, idx, sign, det, lane_offset=0):
    theta, tab = policy_and_table(kind, n_in, n_act)
    key = ("table", kind, n_in, n_act)
    if key not in _CACHE:
        _CACHE[key] = (_dev(theta), _dev(tab.table))
    theta_d, tab_d = _CACHE[key]
    spec = eng.PolicySpec(kind, n_in, n_act, theta.size)
    return spec, eng.lanes_desc(theta_d, 0, tab_d, _dev(idx), _dev(sign), SIGMA, _dev(det), lane_offset=lane_offset)


def _host(res):
    torch.cuda.synchronize()
    out = dict(ret=res.reward.cpu().numpy(), ent=res.entropy.cpu().numpy(), steps=res.timesteps.cpu().numpy(),
               norm2=res.norm2.cpu().numpy())
    if getattr(res, "reward_sq", None) is not None:
        out["ret_sq"] = res.reward_sq.cpu().numpy()
    if getattr(res, "obs_mean", None) is not None:
        out.update(os_mean=res.obs_mean.cpu().numpy(), os_m2=res.obs_m2.cpu().numpy(),
                   os_count=res.obs_count.cpu().numpy())
    return out


def _parent(eng, name, idx, sign, det, seed, lane_offset=0, T=None, jiggle=False, **kw):
    kind, n_in, n_act, _ = ENVS[name]
    spec, lanes = _lanes(eng, kind, n_in, n_act, idx, sign, det, lane_offset)
    return _host(eng.rollout(spec, _env(name, T), lanes, len(idx), seed, jiggle=jiggle, **kw))


def _episodes(eng, name, idx, sign, det, seed, K, ids=None, lane_offset=0, T=None, jiggle=False, **kw):
    kind, n_in, n_act, _ = ENVS[name]
    spec, lanes = _lanes(eng, kind, n_in, n_act, idx, sign, det, lane_offset)
    ids_d = None if ids is None else _dev(np.ascontiguousarray(ids, np.int64))
    return _host(eng.rollout_episodes(spec, _env(name, T), lanes, len(idx), seed, K, episode_ids=ids_d, jiggle=jiggle,
                                      **kw))


def _norm(n_in, on):
    if not on:
        return {}
    m, s = OBS_NORM[n_in]
    return dict(obs_mean=_dev(np.array(m, np.float32)), obs_std=_dev(np.array(s, np.float32)))


def _case61(name):
    kind, n_in, n_act, _ = ENVS[name]
    _, tab = policy_and_table(kind, n_in, n_act)
    return lanes_mixed(tab, 24, 8, 5, idx_seed=15)


# ---- 1. K = 1, no ids: the present entry ------------------------------------------------------------------------
@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("lane_offset", [0, 1000])
@pytest.mark.parametrize("name", list(ENVS))
def test_one_episode_equals_rollout(eng, name, lane_offset, norm):
    idx, sign, det = _case61(name)
    assert len(idx) == 61
    kw = _norm(ENVS[name][1], norm)
    for extra in ({}, {"obs_stats": 0.5}):
        want = _parent(eng, name, idx, sign, det, 81, lane_offset, **kw, **extra)
        got = _episodes(eng, name, idx, sign, det, 81, 1, lane_offset=lane_offset, **kw, **extra)
        assert set(got) == set(want)
        for k in want:
            bad = np.nonzero(np.any((got[k] != want[k]).reshape(61, -1), axis=1))[0]
            if len(bad):
                print("%s %s: lanes %s differ: %s vs %s" % (name, k, bad[:4], got[k][bad[:4]], want[k][bad[:4]]))
        for k in want:
            np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    if name == "CartPoleEnv":
        assert len(np.unique(want["steps"])) > 1      # early terminations and the time limit both occur


# ---- 2. decomposition into K parent launches --------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ENVS))
def test_three_episodes_are_three_launches(eng, name):
    idx, sign, det = _case61(name)
    L, K = len(idx), 3
    ids = 64 * np.arange(K, dtype=np.int64)[None, :] + np.arange(L, dtype=np.int64)[:, None]
    got = _episodes(eng, name, idx, sign, det, 82, K, ids=ids, ret_sq=True, obs_stats=0.5)
    eps = [_parent(eng, name, idx, sign, det, 82, lane_offset=64 * e, obs_stats=0.5) for e in range(K)]
    rsum, rsq, esum, steps = np.zeros(L), np.zeros(L), np.zeros(L), np.zeros(L, np.int64)
    for ep in eps:
        rsum = rsum + ep["ret"]
        rsq = rsq + ep["ret"] * ep["ret"]
        esum = esum + ep["ent"] * ep["steps"]
        steps += ep["steps"]
    np.testing.assert_array_equal(got["steps"], steps)
    np.testing.assert_array_equal(got["norm2"], eps[0]["norm2"])
    np.testing.assert_array_equal(got["ret"], rsum / 3.0)
    np.testing.assert_allclose(got["ret_sq"], rsq, rtol=1e-12, atol=0)
    np.testing.assert_allclose(got["ent"], esum / steps, rtol=1e-5, atol=1e-5)
    # one Welford stat running on across the episodes == the per-episode stats merged
    np.testing.assert_array_equal(got["os_count"], sum(ep["os_count"] for ep in eps))
    assert got["os_count"].sum() > 0.3 * steps.sum()
    n_in = ENVS[name][1]
    for l in range(L):
        w = ostats.Welford(n_in)
        for ep in eps:
            w.merge(ep["os_mean"][l], ep["os_m2"][l], ep["os_count"][l])
        if w.count:
            np.testing.assert_allclose(got["os_mean"][l], w.mean_, rtol=1e-5, atol=1e-5)
            np.testing.assert_allclose(got["os_m2"][l], w.m2, rtol=1e-5, atol=1e-5)


# ---- 3. against the CPU oracle, shared streams ------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_runs(eng):
    """(mode, seed) -> (lanes, ids, oracle fold, GPU outputs of the whole 62-lane launch, jiggle off)."""
    runs = {}
    for mode, seed, _ in eref.ORACLE_CASES:
        (idx, sign, det), ids, o = eref.cartpole_case(mode, seed)
        g = _episodes(eng, "CartPoleEnv", idx, sign, det, seed, eref.CASE_K, ids=None if mode is False else ids,
                      T=500, ret_sq=True)
        runs[(mode, seed)] = ((idx, sign, det), ids, o, g)
    return runs


@pytest.mark.parametrize("mode,seed,n_border", eref.ORACLE_CASES)
def test_cartpole_against_the_oracle(oracle_runs, mode, seed, n_border):
    (idx, sign, det), ids, o, g = oracle_runs[(mode, seed)]
    from worker.worker import episode_stream_ids
    built = episode_stream_ids(mode, sign, 0, eref.CASE_K, 2)
    if mode is False:
        assert built is None
    else:
        np.testing.assert_array_equal(built, ids)
    keep = ~o["borderline"]
    assert (~keep).sum() <= 2
    np.testing.assert_array_equal(g["steps"][keep], o["steps"][keep])
    np.testing.assert_array_equal(g["ret"][keep], o["ret"][keep])
    np.testing.assert_allclose(g["ret_sq"][keep], o["ret_sq"][keep], rtol=1e-12, atol=0)
    np.testing.assert_allclose(g["ent"][keep], o["ent"][keep], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(g["norm2"], o["norm2"], rtol=1e-9, atol=0)


# ---- 4. coupling ------------------------------------------------------------------------------------------------
def test_partners_share_streams_and_keep_their_own_jiggle(eng):
    from worker.worker import episode_stream_ids
    L, K = 32, 3
    idx, sign, det = np.zeros(L, np.int64), np.zeros(L, np.int8), np.zeros(L, np.int8)   # theta itself, sampled
    # sign 0 would keep a lane's own stream: the pairing is by direction, so build it from signed lanes' rule
    ids = episode_stream_ids("pair", np.tile(np.array([1, -1], np.int8), L // 2), 0, K, 2)
    g = _episodes(eng, "CartPoleEnv", idx, sign, det, 91, K, ids=ids, T=500, ret_sq=True, obs_stats=0.5)
    for k, v in g.items():
        v = v.reshape(L, -1)
        np.testing.assert_array_equal(v[0::2], v[1::2], err_msg=k)
    pairs = np.stack([g["steps"][0::2], g["ret_sq"][0::2]], axis=1)
    assert len(np.unique(pairs, axis=0)) > L // 4                 # pairs differ from each other
    assert len(np.unique(g["os_mean"][0::2], axis=0)) == L // 2
    j = _episodes(eng, "CartPoleEnv", idx, sign, det, 91, K, ids=ids, T=500, jiggle=True)
    d = j["ret"] - g["ret"]
    assert np.all(np.abs(np.abs(d) - 1e-12) < 5e-13)              # every lane moved by +-1e-12 ...
    dp = np.round((j["ret"][0::2] - j["ret"][1::2]) / 1e-12).astype(int)
    assert set(dp.tolist()) <= {-2, 0, 2} and np.any(dp != 0)     # ... by its own coin, not its partner's


# ---- 5. shard invariance ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,seed", [("pair", 71), (False, 71)])
def test_shard_invariance(eng, oracle_runs, mode, seed):
    (idx, sign, det), ids, _, whole = oracle_runs[(mode, seed)]
    part = _episodes(eng, "CartPoleEnv", idx[32:], sign[32:], det[32:], seed, eref.CASE_K,
                     ids=None if mode is False else ids[32:], lane_offset=32, T=500, ret_sq=True)
    for k in whole:
        np.testing.assert_array_equal(part[k], whole[k][32:], err_msg=k)


# ---- 6. edges ---------------------------------------------------------------------------------------------------
def test_edges(eng):
    idx, sign, det = case_short(8)
    # episode_len 1, K = 5: every CartPole episode is its first step (reward 1) -- 5 steps, the episode returns sum
    # to 5, and ret is their mean
    g = _episodes(eng, "CartPoleEnv", idx, sign, det, 5, 5, T=1, ret_sq=True)
    np.testing.assert_array_equal(g["steps"], 5)
    np.testing.assert_array_equal(g["ret"] * 5, 5.0)
    np.testing.assert_array_equal(g["ret"], 1.0)
    np.testing.assert_array_equal(g["ret_sq"], 5.0)
    g = _episodes(eng, "CartPoleEnv", idx, sign, det, 5, 1024, T=1)
    np.testing.assert_array_equal(g["steps"], 1024)
    np.testing.assert_array_equal(g["ret"], 1.0)
    # Pendulum: T = 65 crosses one 64-step draw batch in every episode
    _, tab = policy_and_table("mujoco", 3, 1)
    pidx, psign, pdet = lanes_mixed(tab, 4, 1, 1, idx_seed=16)
    g = _episodes(eng, "PendulumEnv", pidx, psign, pdet, 6, 2, T=65)
    np.testing.assert_array_equal(g["steps"], 130)
    ids = 2 * np.arange(10, dtype=np.int64)[:, None] + np.arange(2, dtype=np.int64)[None, :]
    g2 = _episodes(eng, "PendulumEnv", pidx, psign, pdet, 6, 2, ids=ids, T=65)
    np.testing.assert_array_equal(g2["ret"], g["ret"])             # the default ids are (g) K + e
    one = _parent(eng, "PendulumEnv", pidx, psign, pdet, 6, T=65)
    e0 = _episodes(eng, "PendulumEnv", pidx, psign, pdet, 6, 1, ids=np.arange(10, dtype=np.int64)[:, None], T=65)
    np.testing.assert_array_equal(e0["ret"], one["ret"])
    # one lane
    g = _episodes(eng, "CartPoleEnv", idx[:1], sign[:1], det[:1], 5, 3, T=500)
    assert g["ret"].shape == (1,) and 3 <= g["steps"][0] <= 1500
    assert abs(g["ret"][0] * 3 - g["steps"][0]) < 1e-9


# ---- 7. refusals ------------------------------------------------------------------------------------------------
class _Desc(object):
    def __init__(self, desc, episode_len):
        self._d, self.episode_len = desc, episode_len

    def desc(self):
        return self._d


def _refused(eng, spec, env, K, partial_welford=False):
    from fdr import _lib
    n = 8
    base = torch.zeros(spec.n_params, dtype=torch.float32, device=DEV)
    buf = torch.full((4, n), -7.0, dtype=torch.float64, device=DEV)
    steps = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    osb = torch.full((2, n, spec.n_in), -7.0, dtype=torch.float32, device=DEV)
    lanes = eng.lanes_desc(base, 0)
    pd, ed = spec.desc(), env.desc()
    import ctypes
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rc = _lib.lib.fdr_rollout_episodes(None, ctypes.byref(pd), ctypes.byref(ed), ctypes.byref(lanes), n,
                                       ctypes.c_uint64(1), 0, None, None, K, None, p(buf[0]), p(buf[3]), p(buf[1]),
                                       p(steps), p(buf[2]), p(osb[0]) if partial_welford else None,
                                       p(osb[1]) if partial_welford else None, None, 0.5, None)
    torch.cuda.synchronize()
    assert torch.all(buf == -7.0) and torch.all(steps == -7) and torch.all(osb == -7.0), "a refused call launched"
    assert rc != _lib.FDR_OK and _lib.lib.fdr_last_error()
    return rc


def test_refusals(eng):
    from envs import CartPoleEnv, SyntheticEnv, TrapEnv
    from fdr import _lib
    P = policy_and_table("discrete", 4, 2)[0].size
    spec = eng.PolicySpec("discrete", 4, 2, P)
    assert _refused(eng, spec, CartPoleEnv(10), 0) == _lib.FDR_ERR_INVALID
    assert _refused(eng, spec, CartPoleEnv(10), 1025) == _lib.FDR_ERR_INVALID
    assert _refused(eng, spec, SyntheticEnv(4, 2, True, 10, device=DEV), 2) == _lib.FDR_ERR_UNSUPPORTED
    assert b"physics" in _lib.lib.fdr_last_error()
    Pt = policy_and_table("discrete", 2, 9)[0].size
    assert _refused(eng, eng.PolicySpec("discrete", 2, 9, Pt), TrapEnv(device=DEV), 2) == _lib.FDR_ERR_UNSUPPORTED
    assert _refused(eng, eng.PolicySpec("mujoco", 17, 6, 6092), CartPoleEnv(10), 2) == _lib.FDR_ERR_UNSUPPORTED
    assert _refused(eng, eng.PolicySpec("mujoco", 4, 2, 4740), CartPoleEnv(10), 2) == _lib.FDR_ERR_UNSUPPORTED
    assert _refused(eng, spec, CartPoleEnv(10), 2, partial_welford=True) == _lib.FDR_ERR_INVALID
    # the Python layer checks the id array
    idx, sign, det = case_short(8)
    for bad in (torch.zeros((8, 2), dtype=torch.int32, device=DEV), torch.zeros((8, 3), dtype=torch.int64, device=DEV),
                torch.zeros((2, 8), dtype=torch.int64, device=DEV).t()):
        with pytest.raises(ValueError):
            _, lanes = _lanes(eng, "discrete", 4, 2, idx, sign, det)
            eng.rollout_episodes(spec, CartPoleEnv(10), lanes, 8, 1, 2, episode_ids=bad)


# ---- 8. worker and runner ---------------------------------------------------------------------------------------
def _spy(monkeypatch, eng):
    calls = {"rollout": [], "episodes": []}
    real_r, real_e = eng.rollout, eng.rollout_episodes

    def rollout(*a, **kw):
        calls["rollout"].append((a, kw))
        return real_r(*a, **kw)

    def rollout_episodes(*a, **kw):
        res = real_e(*a, **kw)
        calls["episodes"].append((a, kw, res))
        return res

    monkeypatch.setattr(eng, "rollout", rollout)
    monkeypatch.setattr(eng, "rollout_episodes", rollout_episodes)
    return calls


def test_runner_trains_with_episodes_and_shared_streams(eng, monkeypatch):
    from run_sequential import SequentialRunner
    calls = _spy(monkeypatch, eng)
    r = SequentialRunner(env_id="CartPole-v1", physics=True, antithetic=True, batch_size=32, episodes_per_lane=3,
                         common_random_numbers=True, noise_table_size=1 << 20, verbose=False, eval_prob=0.2)
    before = r.policy.get_trainable_flat().copy()
    r.train(2)
    after = r.policy.get_trainable_flat()
    assert np.all(np.isfinite(after)) and np.any(after != before)
    train_calls = [c for c in calls["episodes"] if c[0][3] >= 64]
    assert len(train_calls) == 2
    total = 0
    saw_eval = False
    for a, kw, res in train_calls:
        n, K = a[3], a[5]
        assert K == 3
        ids = kw["episode_ids"].cpu().numpy()
        assert ids.shape == (n, 3)
        tr = ids[:64]
        np.testing.assert_array_equal(tr[0::2], tr[1::2])                      # equal within each +- pair
        assert len(np.unique(tr[0::2, 0])) == 32                               # distinct across pairs
        np.testing.assert_array_equal(tr[:, 1:] - tr[:, :1], [[1, 2]] * 64)
        ev = ids[64:]
        saw_eval |= len(ev) > 0
        np.testing.assert_array_equal(ev, (np.arange(64, n)[:, None] * 3 + np.arange(3)[None, :]))   # own ids
        assert len(np.unique(ids[:, 0])) == 32 + len(ev)
        assert ids.min() >= 0 and ids.max() < 2 ** 32
        total += int(res.timesteps.sum().item())
    assert saw_eval
    assert r.agent.cumulative_timesteps == total
    assert len(r.history) == 2
    for h in r.history:
        s = h["Noisy Reward Within-Lane Std"]
        assert np.isfinite(s) and s > 0


def test_runner_defaults_stay_on_rollout(eng, monkeypatch):
    from run_sequential import SequentialRunner
    calls = _spy(monkeypatch, eng)
    r = SequentialRunner(env_id="CartPole-v1", physics=True, antithetic=True, batch_size=32,
                         noise_table_size=1 << 20, verbose=False)
    r.train(1)
    assert not calls["episodes"] and calls["rollout"]
    assert set(r.history[0]) == {"Epoch", "Epoch Time", "Cumulative Timesteps", "Policy Reward", "Policy Entropy",
                                 "Policy Novelty", "Noisy Reward", "Noisy Novelty", "Update Magnitude", "Omega", "idx",
                                 "rewards"}


def _worker(**kw):
    from envs import CartPoleEnv
    from policies import DiscretePolicy
    from utils import SharedNoiseTable
    from worker import Agent, Worker
    pol = DiscretePolicy(4, 2, seed=7, device=DEV)
    src = SharedNoiseTable(1 << 20, pol.num_params, random_seed=7)
    return Worker(pol, Agent(pol, CartPoleEnv(500), 7), src, None, sigma=SIGMA, random_seed=7, **kw)


def test_worker_default_launch_calls_rollout_exactly_as_before(eng, monkeypatch):
    calls = _spy(monkeypatch, eng)
    w = _worker()
    b = w.evaluate(8, antithetic=True, seed=5)
    assert len(b.reward) == 16 and not calls["episodes"] and len(calls["rollout"]) == 1
    a, kw = calls["rollout"][0]
    assert a[3] == 16 and a[4] == 5
    assert set(kw) == {"jiggle", "obs_mean", "obs_std", "bn_mean", "bn_var", "out", "device", "obs_stats"}


def test_worker_evaluate_shards_reproduce_the_whole(eng):
    whole = _worker(episodes_per_lane=3, common_random_numbers="pair").evaluate(8, antithetic=True, seed=5)
    torch.cuda.synchronize()
    parts = []
    for rng in ((0, 8), (8, 16)):
        w = _worker(episodes_per_lane=3, common_random_numbers="pair")
        b = w.evaluate(8, antithetic=True, seed=5, lane_range=rng)
        parts.append((b.reward.cpu().numpy(), b.timesteps.cpu().numpy(), b.entropy.cpu().numpy()))
        assert w.agent.cumulative_timesteps == int(parts[-1][1].sum())
    for k, name in enumerate(("reward", "timesteps", "entropy")):
        np.testing.assert_array_equal(np.concatenate([p[k] for p in parts]), getattr(whole, name).cpu().numpy())
    # partners share their episodes' resets: under a near-uniform initial policy most play to the same length
    steps = whole.timesteps.cpu().numpy()
    assert np.sum(steps[0::2] == steps[1::2]) >= 1


def test_unsupported_combinations_are_value_errors():
    from envs import SyntheticEnv
    from policies import DiscretePolicy
    from utils import SharedNoiseTable
    from utils.noise_sources import SimpleNoiseSource
    from worker import Agent, Worker
    pol = DiscretePolicy(4, 2, seed=7, device=DEV)
    src = SharedNoiseTable(1 << 20, pol.num_params, random_seed=7)
    with pytest.raises(ValueError, match="physics envs only"):
        Worker(pol, Agent(pol, SyntheticEnv(4, 2, True, 10, device=DEV), 7), src, None, episodes_per_lane=2)
    from envs import CartPoleEnv
    with pytest.raises(ValueError, match="host noise"):
        Worker(pol, Agent(pol, CartPoleEnv(500), 7), SimpleNoiseSource(pol.num_params, random_seed=7), None,
               common_random_numbers="batch")
    with pytest.raises(ValueError, match="multiple of lanes_per_dir"):
        w = Worker(pol, Agent(pol, CartPoleEnv(500), 7), src, None, common_random_numbers="pair")
        w.launch(np.zeros(4, np.int64), np.array([1, -1, 1, -1], np.int8), np.zeros(4, np.int8), seed=1,
                 lane_offset=1, lanes_per_dir=2)
