"""GPU: CartPole-v1 and Pendulum-v1 inside the one-lane rollout kernel (FDR_ENV_CARTPOLE / FDR_ENV_PENDULUM).

Parity is against tests/physics_ref.py, the numpy restatement of gym's published classic_control formulas (its own f32
error is pinned in tests/test_physics_ref.py), driven by the project's oracle (oracle.agent.evaluate_lanes,
oracle.policies.lanes_forward, oracle.rng).

Closed-loop comparison of long balanced CartPole episodes is not meaningful (argmax margins of a near-uniform policy
fall below the forward tolerance within a few hundred steps), so long episodes are checked transition by transition
along the GPU's own recorded trajectory, and whole episodes are compared only where they are short (sampled lanes
from a random init: ~22 steps).

Seeds (each verified on the CPU restatement, see the helpers' docstrings):
  SEED_LONG   the 61-lane launch: no visited state of any lane within 1e-5 of a failure threshold (0 lanes skipped)
  SEED_SHORT  the 64 sampled lanes: at most 2 borderline lanes
  SEED_X*     the 16-lane extras: no borderline lane
"""
import re

import numpy as np
import pytest
import torch

import physics_ref as ref
from oracle import agent as oagent
from oracle import noise as onoise
from oracle import policies as opol
from oracle import rng as crng

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SIGMA = 0.02
SEED_LONG, SEED_SHORT = 31, 41
SEED_XENV, SEED_XACT, SEED_XNORM, SEED_XSTAT = 51, 52, 53, 54
SEED_PEND = 61
LN2 = float(np.log(2.0))


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


# ---- cases (pure numpy: also used to verify the seeds on the CPU) -----------------------------------------------
_CACHE = {}


def policy_and_table(kind, n_in, n_act):
    key = (kind, n_in, n_act)
    if key not in _CACHE:
        theta = opol.TorchPolicy(kind, n_in, n_act, seed=124).get_flat()
        _CACHE[key] = (theta, onoise.NoiseTable(1 << 20, theta.size, 124))
    return _CACHE[key]


def lanes_mixed(tab, n_pairs, n_theta, n_pert, idx_seed):
    """n_pairs sampled +-pairs, n_theta deterministic sign-0 lanes of theta itself, n_pert deterministic perturbed."""
    rs = np.random.RandomState(idx_seed)
    pidx = rs.randint(0, tab.max_idx, size=n_pairs).astype(np.int64)
    didx = rs.randint(0, tab.max_idx, size=n_pert).astype(np.int64)
    idx = np.concatenate([np.repeat(pidx, 2), np.zeros(n_theta, np.int64), didx])
    sign = np.concatenate([np.tile(np.array([1, -1], np.int8), n_pairs), np.zeros(n_theta, np.int8),
                           np.where(np.arange(n_pert) % 2 == 0, 1, -1).astype(np.int8)])
    det = np.concatenate([np.zeros(2 * n_pairs, np.int8), np.ones(n_theta + n_pert, np.int8)])
    return idx, sign, det


def cartpole_oracle(idx, sign, det, seed, T=500, lane_ids=None, env_seed=None, obs_mean=None, obs_std=None,
                    obs_chance=None):
    """evaluate_lanes on BatchedCartPole, plus per lane the borderline flag of the restatement: at some step
    |u tot - p0| < 2e-5 (twice the engine's 1e-5 forward tolerance; sampled lanes), or a visited state within 1e-5 of
    a failure threshold.  -> dict(ret, ent, steps, norm2, states, borderline, env[, stats])."""
    theta, tab = policy_and_table("discrete", 4, 2)
    L = len(idx)
    lanes = np.arange(L, dtype=np.uint64) if lane_ids is None else np.asarray(lane_ids, np.uint64)
    env = ref.BatchedCartPole(L, seed if env_seed is None else env_seed, lanes, T)
    out = oagent.evaluate_lanes("discrete", 4, 2, theta, tab.table, idx, sign, SIGMA, env, seed,
                                deterministic=det.astype(bool), jiggle=False, record_states=True, lane_ids=lanes,
                                obs_mean=obs_mean, obs_std=obs_std, obs_chance=obs_chance)
    ret, ent, steps, norm2 = out[:4]
    states = out[-1]
    thetas = onoise.perturb(theta, tab.table, idx, sign, SIGMA)
    border = env.min_margin < 1e-5
    for t in range(int(steps.max())):
        alive = (steps > t) & (det == 0)
        if not alive.any():
            continue
        x = states[alive, t]
        if obs_mean is not None:
            x = np.clip((x - obs_mean) / obs_std, -10, 10).astype(np.float32)
        p = opol.lanes_forward("discrete", 4, 2, thetas[alive], x)
        u = crng.uniform(seed, lanes[alive], t, 0)
        tot = (p[:, 0] + p[:, 1]).astype(np.float32)
        border[np.nonzero(alive)[0]] |= np.abs((u * tot).astype(np.float32) - p[:, 0]) < 2e-5
    res = dict(ret=ret, ent=ent, steps=steps, norm2=norm2, states=states, borderline=border, env=env)
    if obs_chance is not None:
        res["stats"] = out[4]
    return res


def case_long():
    """The 61-lane launch of tests 2, 3: 24 sampled +-pairs, 8 deterministic lanes of theta, 5 deterministic perturbed
    (on the CPU restatement the theta lanes average ~450 steps: long episodes and the time limit)."""
    _, tab = policy_and_table("discrete", 4, 2)
    return lanes_mixed(tab, 24, 8, 5, idx_seed=5)


def case_short(L=64, idx_seed=6):
    _, tab = policy_and_table("discrete", 4, 2)
    return lanes_mixed(tab, L // 2, 0, 0, idx_seed=idx_seed)


def case_theta_lanes(n=8):
    return np.zeros(n, np.int64), np.zeros(n, np.int8), np.ones(n, np.int8)


# ---- GPU launches -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    from fdr import engine
    return engine


def _launch(eng, kind, n_in, n_act, env, idx, sign, det, seed, lane_offset=0, record=True, **kw):
    theta, tab = policy_and_table(kind, n_in, n_act)
    L = len(idx)
    spec = eng.PolicySpec(kind, n_in, n_act, theta.size)
    key = ("table", kind, n_in, n_act)
    if key not in _CACHE:
        _CACHE[key] = (_dev(theta), _dev(tab.table))
    theta_d, tab_d = _CACHE[key]
    lanes = eng.lanes_desc(theta_d, 0, tab_d, _dev(idx), _dev(sign), SIGMA, _dev(det), lane_offset=lane_offset)
    states = None
    if record:
        states = torch.full((L, env.episode_len, n_in), float("nan"), dtype=torch.float32, device=DEV)
    res = eng.rollout(spec, env, lanes, L, seed, jiggle=False, states=states, **kw)
    torch.cuda.synchronize()
    out = dict(ret=res.reward.cpu().numpy(), ent=res.entropy.cpu().numpy(), steps=res.timesteps.cpu().numpy(),
               norm2=res.norm2.cpu().numpy(), states=None if states is None else states.cpu().numpy(), res=res)
    return out


@pytest.fixture(scope="module")
def cart_long(eng):
    from envs import CartPoleEnv
    idx, sign, det = case_long()
    return (idx, sign, det), _launch(eng, "discrete", 4, 2, CartPoleEnv(500), idx, sign, det, SEED_LONG)


@pytest.fixture(scope="module")
def cart_short(eng):
    from envs import CartPoleEnv
    idx, sign, det = case_short()
    return (idx, sign, det), _launch(eng, "discrete", 4, 2, CartPoleEnv(500), idx, sign, det, SEED_SHORT)


# ---- 1. resets --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lane_offset", [0, 1000])
def test_cartpole_resets_bitwise(eng, lane_offset):
    from envs import CartPoleEnv
    idx, sign, det = case_short()
    got = _launch(eng, "discrete", 4, 2, CartPoleEnv(4), idx, sign, det, SEED_SHORT, lane_offset=lane_offset)
    want = ref.cartpole_reset(SEED_SHORT, lane_offset + np.arange(64))
    np.testing.assert_array_equal(got["states"][:, 0, :].view(np.uint32), want.view(np.uint32))
    assert len(np.unique(want[:, 0])) == 64          # every lane its own state


# ---- 2. one-step consistency ------------------------------------------------------------------------------------
def _transitions(states, steps):
    """(lane, t) of every recorded transition states[l, t] -> states[l, t + 1], t + 1 < steps[l]."""
    ll, tt = [], []
    for l, n in enumerate(steps):
        ll.append(np.full(max(int(n) - 1, 0), l))
        tt.append(np.arange(max(int(n) - 1, 0)))
    return np.concatenate(ll), np.concatenate(tt)


def test_cartpole_one_step_consistency(cart_long):
    (idx, sign, det), g = cart_long
    S, steps = g["states"], g["steps"]
    assert len(steps) == 61
    ll, tt = _transitions(S, steps)
    assert len(ll) > 3000, "the deterministic lanes should run long episodes"
    cur, nxt = S[ll, tt], S[ll, tt + 1]
    assert np.all(np.isfinite(cur)) and np.all(np.isfinite(nxt))
    m = [np.all(np.abs(ref.cartpole_step_f32(cur, np.full(len(ll), a)) - nxt) <= 2e-6, axis=-1) for a in (0, 1)]
    err = np.minimum(*[np.abs(ref.cartpole_step_f32(cur, np.full(len(ll), a)) - nxt).max(axis=-1) for a in (0, 1)])
    print("cartpole one-step: %d transitions, max |gpu - restated| = %.3g" % (len(ll), err.max()))
    assert np.all(m[0] ^ m[1]), "transitions matching neither / both actions: %d" % int((~(m[0] ^ m[1])).sum())
    # deterministic lanes take the argmax wherever the oracle's margin is above the forward tolerance
    theta, tab = policy_and_table("discrete", 4, 2)
    thetas = onoise.perturb(theta, tab.table, idx, sign, SIGMA)
    checked = 0
    for l in np.nonzero(det)[0]:
        sel = ll == l
        if not sel.any():
            continue
        p = opol.lanes_forward("discrete", 4, 2, np.broadcast_to(thetas[l], (int(sel.sum()), theta.size)), cur[sel])
        clear = np.abs(p[:, 0] - p[:, 1]) > 1e-4
        act = np.where(m[1][sel], 1, 0)
        np.testing.assert_array_equal(act[clear], np.argmax(p, axis=-1)[clear], err_msg="lane %d" % l)
        checked += int(clear.sum())
    # (a normc-initialised policy is near-uniform: most margins on the long balanced episodes are below 1e-4)
    print("cartpole argmax: %d clear-margin deterministic steps checked" % checked)
    assert checked > 0


# ---- 3. termination and return ----------------------------------------------------------------------------------
def test_cartpole_termination_and_return(cart_long):
    (idx, sign, det), g = cart_long
    S, steps, T = g["states"], g["steps"], 500
    assert steps.min() >= 1 and steps.max() <= T
    assert (steps < T).sum() >= 40 and steps[det == 1].max() > 100
    np.testing.assert_array_equal(g["ret"], steps.astype(np.float64))       # reward 1 per step taken, jiggle off
    # (0, ln 2], to the precision the kernel reports entropies in: an f32 sum scaled by fl32(ln 2), which itself lies
    # 1.9e-9 above ln 2 -- a uniform policy's entropy is not representable below it.  The project's entropy
    # tolerance (atol 1e-5, as in test 4) bounds the excess; measured 2.3e-8.
    print("cartpole entropy: max %.10f, excess over ln 2 %.3g" % (g["ent"].max(), g["ent"].max() - LN2))
    assert np.all(np.isfinite(g["ent"])) and np.all(g["ent"] > 0) and np.all(g["ent"] <= LN2 + 1e-5)
    skipped = 0
    for l, n in enumerate(steps):
        n = int(n)
        assert not ref.cartpole_failed(S[l, :n]).any(), "lane %d recorded a state outside the bounds" % l
        assert np.all(np.isnan(S[l, n:])), "lane %d wrote a state after its last step" % l
        if n == T:
            continue
        cand = np.stack([ref.cartpole_step_f32(S[l, n - 1], a) for a in (0, 1)])
        if ref.cartpole_margin(cand).min() < 1e-5:
            skipped += 1
            continue
        assert ref.cartpole_failed(cand).any(), "lane %d stopped at %d inside the bounds" % (l, n)
    assert skipped <= 1


# ---- 4. whole short episodes ------------------------------------------------------------------------------------
def test_cartpole_short_episodes_vs_oracle(cart_short):
    (idx, sign, det), g = cart_short
    o = cartpole_oracle(idx, sign, det, SEED_SHORT)
    keep = ~o["borderline"]
    assert (~keep).sum() <= 2
    assert o["steps"].max() < 500 and 10 < o["steps"].mean() < 60
    np.testing.assert_array_equal(g["steps"][keep], o["steps"][keep])
    np.testing.assert_array_equal(g["ret"][keep], o["ret"][keep])
    np.testing.assert_allclose(g["ent"][keep], o["ent"][keep], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(g["norm2"], o["norm2"], rtol=1e-9, atol=0)


# ---- 5. time limit ----------------------------------------------------------------------------------------------
def test_cartpole_time_limit(eng):
    from envs import CartPoleEnv
    idx, sign, det = case_theta_lanes(8)
    o = cartpole_oracle(idx, sign, det, SEED_LONG, T=60)
    alive = o["steps"] > 30
    assert alive.sum() >= 4
    g = _launch(eng, "discrete", 4, 2, CartPoleEnv(episode_len=30), idx, sign, det, SEED_LONG)
    assert np.all(g["steps"] <= 30)
    np.testing.assert_array_equal(g["steps"][alive], 30)
    np.testing.assert_array_equal(g["ret"][alive], 30.0)


# ---- 6. extras --------------------------------------------------------------------------------------------------
def test_cartpole_u_inject_replays_oracle_episodes(eng):
    """Action draws injected from another stream than the launch's seed: resets still come from the seed."""
    from envs import CartPoleEnv
    idx, sign, det = case_short(16, idx_seed=7)
    o = cartpole_oracle(idx, sign, det, SEED_XACT, env_seed=SEED_XENV)
    assert not o["borderline"].any()
    T = 500
    u = np.stack([crng.uniform(SEED_XACT, np.arange(16, dtype=np.uint64), t, 0) for t in range(T)], axis=1)
    g = _launch(eng, "discrete", 4, 2, CartPoleEnv(T), idx, sign, det, SEED_XENV,
                u_inject=_dev(u.reshape(16, T, 1).astype(np.float32)))
    np.testing.assert_array_equal(g["steps"], o["steps"])
    np.testing.assert_array_equal(g["ret"], o["ret"])
    np.testing.assert_array_equal(g["states"][:, 0], o["states"][:, 0])


def test_cartpole_obs_normalisation(eng):
    from envs import CartPoleEnv
    idx, sign, det = case_short(16, idx_seed=8)
    mean = np.array([0.01, -0.1, 0.005, 0.2], np.float32)
    std = np.array([0.05, 0.5, 0.04, 0.7], np.float32)
    o = cartpole_oracle(idx, sign, det, SEED_XNORM, obs_mean=mean, obs_std=std)
    keep = ~o["borderline"]
    assert (~keep).sum() <= 2
    g = _launch(eng, "discrete", 4, 2, CartPoleEnv(500), idx, sign, det, SEED_XNORM, obs_mean=_dev(mean),
                obs_std=_dev(std))
    np.testing.assert_array_equal(g["steps"][keep], o["steps"][keep])
    # recorded states are the raw observations
    np.testing.assert_array_equal(g["states"][:, 0], ref.cartpole_reset(SEED_XNORM, np.arange(16)))


def test_cartpole_welford_statistics(eng):
    from envs import CartPoleEnv
    idx, sign, det = case_short(16, idx_seed=9)
    o = cartpole_oracle(idx, sign, det, SEED_XSTAT, obs_chance=0.5)
    assert not o["borderline"].any()
    g = _launch(eng, "discrete", 4, 2, CartPoleEnv(500), idx, sign, det, SEED_XSTAT, record=False, obs_stats=0.5)
    res = g["res"]
    np.testing.assert_array_equal(g["steps"], o["steps"])
    cnt = res.obs_count.cpu().numpy()
    np.testing.assert_array_equal(cnt, [s.count for s in o["stats"]])
    assert cnt.sum() > 0.3 * o["steps"].sum()
    gm, g2 = res.obs_mean.cpu().numpy(), res.obs_m2.cpu().numpy()
    for l, s in enumerate(o["stats"]):
        if s.count:
            np.testing.assert_allclose(gm[l], s.mean_, rtol=1e-5, atol=1e-5)
            np.testing.assert_allclose(g2[l], s.m2, rtol=1e-5, atol=1e-5)


def _code(excinfo):
    return int(re.search(r"\(code (\d+)\)", str(excinfo.value)).group(1))


def test_u_inject_with_statistics_is_still_refused(eng):
    from envs import CartPoleEnv
    from fdr import _lib
    idx, sign, det = case_short(16, idx_seed=7)
    with pytest.raises(_lib.FDRError) as ei:
        _launch(eng, "discrete", 4, 2, CartPoleEnv(20), idx, sign, det, 1, record=False, obs_stats=0.5,
                u_inject=torch.zeros((16, 20, 1), dtype=torch.float32, device=DEV))
    assert _code(ei) == _lib.FDR_ERR_UNSUPPORTED


# ---- 7. shard invariance ----------------------------------------------------------------------------------------
def test_cartpole_shard_invariance(eng, cart_short):
    from envs import CartPoleEnv
    (idx, sign, det), whole = cart_short
    part = _launch(eng, "discrete", 4, 2, CartPoleEnv(500), idx[32:], sign[32:], det[32:], SEED_SHORT, lane_offset=32)
    np.testing.assert_array_equal(part["steps"], whole["steps"][32:])
    np.testing.assert_array_equal(part["ret"], whole["ret"][32:])
    np.testing.assert_array_equal(part["states"].view(np.uint32), whole["states"][32:].view(np.uint32))


# ---- 8. Pendulum ------------------------------------------------------------------------------------------------
def test_pendulum(eng):
    from envs import PendulumEnv
    T, L = 200, 64
    theta, tab = policy_and_table("mujoco", 3, 1)
    assert theta.size == 4546
    idx, sign, det = lanes_mixed(tab, 24, 8, 8, idx_seed=10)
    g = _launch(eng, "mujoco", 3, 1, PendulumEnv(T), idx, sign, det, SEED_PEND)
    S = g["states"]
    np.testing.assert_array_equal(g["steps"], T)
    assert np.all(np.isfinite(S)) and np.all(np.isfinite(g["ent"]))
    # reset: thetadot bit for bit; (cos, sin) are the accurate f32 functions of the bit-exact restated theta (an
    # ulp of values in [0.5, 1]: the observation shows theta only through cosf / sinf)
    th0, thd0 = ref.pendulum_reset(SEED_PEND, np.arange(L))
    np.testing.assert_array_equal(S[:, 0, 2].view(np.uint32), thd0.view(np.uint32))
    np.testing.assert_allclose(S[:, 0, 0], np.cos(th0.astype(np.float64)), rtol=0, atol=2.0 ** -23)
    np.testing.assert_allclose(S[:, 0, 1], np.sin(th0.astype(np.float64)), rtol=0, atol=2.0 ** -23)
    np.testing.assert_allclose(S[..., 0].astype(np.float64) ** 2 + S[..., 1].astype(np.float64) ** 2, 1.0, rtol=0,
                               atol=1e-6)
    assert np.all(np.abs(S[..., 2]) <= 8)
    # one-step consistency and the return, along the GPU's own trajectory
    thetas = onoise.perturb(theta, tab.table, idx, sign, SIGMA)
    worst, n_checked, beyond = 0.0, 0, np.zeros(2, np.int64)
    for l in range(L):
        obs = S[l]
        mean, std = opol.lanes_forward("mujoco", 3, 1, np.broadcast_to(thetas[l], (T, theta.size)), obs)
        a = mean[:, 0]
        if not det[l]:
            z = crng.normal(SEED_PEND, np.uint64(l), np.arange(T, dtype=np.uint64), 0)
            a = (mean[:, 0] + std[:, 0] * z).astype(np.float32)
        th = np.arctan2(obs[:, 1], obs[:, 0]).astype(np.float32)
        nth, nthd, rew = ref.pendulum_step_f32(th, obs[:, 2], a)
        want = ref.pendulum_obs(nth, nthd)
        ok = np.abs(np.abs(a[:-1]) - 2.0) >= 1e-4
        err = np.abs(want[:-1] - obs[1:]).max(axis=-1)
        worst = max(worst, float(err[ok].max()))
        n_checked += int(ok.sum())
        beyond += [int((a > 2.0).sum()), int((a < -2.0).sum())]
        assert np.all(err[ok] <= 5e-6), "lane %d: max one-step error %.3g" % (l, err[ok].max())
        assert abs(g["ret"][l] - rew.astype(np.float64).sum()) <= 4e-3, \
            "lane %d: ret %.6f, restated %.6f" % (l, g["ret"][l], rew.astype(np.float64).sum())
    print("pendulum one-step: %d transitions, max |gpu - restated| = %.3g" % (n_checked, worst))
    # the census of tests/branch_cases.py for this launch (printed, not required: the sampled noise decides)
    print("pendulum branches: torque beyond +2 / -2 at %d / %d steps, speed at +8 / -8 in %d / %d recorded states"
          % (beyond[0], beyond[1], int((S[..., 2] == 8).sum()), int((S[..., 2] == -8).sum())))
    assert n_checked > 0.9 * L * (T - 1)
    assert len(np.unique(np.round(g["ret"], 3))) > 40       # every lane its own episode


# ---- 9. refusals ------------------------------------------------------------------------------------------------
class _Desc(object):
    def __init__(self, desc, episode_len):
        self._d, self.episode_len = desc, episode_len

    def desc(self):
        return self._d


def _refused(eng, spec, env, n_params):
    from fdr import _lib
    base = torch.zeros(n_params, dtype=torch.float32, device=DEV)
    buf = torch.full((4, 8), -7.0, dtype=torch.float64, device=DEV)
    out = eng.RolloutResult(buf[0], buf[1], torch.full((8,), -7, dtype=torch.int32, device=DEV), buf[2])
    with pytest.raises(_lib.FDRError) as ei:
        eng.rollout(spec, env, eng.lanes_desc(base, 0), 8, 1, out=out)
    torch.cuda.synchronize()
    assert torch.all(buf == -7.0) and torch.all(out.timesteps == -7), "a refused call launched"
    return _code(ei)


def test_refusals(eng):
    from envs import CartPoleEnv, PendulumEnv
    from fdr import _lib
    assert _refused(eng, eng.PolicySpec("mujoco", 17, 6, 6092), CartPoleEnv(10), 6092) == _lib.FDR_ERR_UNSUPPORTED
    assert _refused(eng, eng.PolicySpec("discrete", 3, 1, 4546), PendulumEnv(10), 4546) == _lib.FDR_ERR_UNSUPPORTED
    assert _refused(eng, eng.PolicySpec("mujoco", 4, 2, 4740), CartPoleEnv(10), 4740) == _lib.FDR_ERR_UNSUPPORTED
    m = torch.zeros(16, dtype=torch.float32, device=DEV)
    d = CartPoleEnv(10).desc()
    d.M = m.data_ptr()
    P = policy_and_table("discrete", 4, 2)[0].size
    spec = eng.PolicySpec("discrete", 4, 2, P)
    assert _refused(eng, spec, _Desc(d, 10), P) == _lib.FDR_ERR_INVALID
    for field, value in (("done_threshold", 0.5), ("obs_dim", 3), ("episode_len", 10001), ("episode_len", 0)):
        d = CartPoleEnv(10).desc()
        setattr(d, field, value)
        assert _refused(eng, spec, _Desc(d, 10), P) == _lib.FDR_ERR_INVALID, field
    # the synthetic env has no (3, 1) instance
    from envs import SyntheticEnv
    assert _refused(eng, eng.PolicySpec("mujoco", 3, 1, 4546), SyntheticEnv(3, 1, False, 10, device=DEV), 4546) \
        == _lib.FDR_ERR_UNSUPPORTED


# ---- the (3, 1) policy's other kernels --------------------------------------------------------------------------
def test_pendulum_policy_forward_and_loader(eng):
    theta, tab = policy_and_table("mujoco", 3, 1)
    idx, sign, det = lanes_mixed(tab, 6, 1, 0, idx_seed=11)
    L = len(idx)
    spec = eng.PolicySpec("mujoco", 3, 1, theta.size)
    lanes = eng.lanes_desc(_dev(theta), 0, _dev(tab.table), _dev(idx), _dev(sign), SIGMA)
    x = np.random.RandomState(3).randn(L, 3).astype(np.float32)
    mean, std = eng.policy_forward(spec, lanes, L, _dev(x))
    thetas = onoise.perturb(theta, tab.table, idx, sign, SIGMA)
    rmean, rstd = opol.lanes_forward("mujoco", 3, 1, thetas, x)
    np.testing.assert_allclose(mean.cpu().numpy(), rmean, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(std.cpu().numpy(), rstd, rtol=1e-5, atol=1e-5)
    out, reads, counted, n2 = eng.theta_prime(spec, lanes, L, "lane")
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), thetas.view(np.uint32))
    assert torch.all(reads >= 1) and torch.all(counted == 1)
    from fdr import _lib
    with pytest.raises(_lib.FDRError) as ei:
        eng.theta_prime(spec, lanes, L, "pair")
    assert _code(ei) == _lib.FDR_ERR_UNSUPPORTED


# ---- 10. runner -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env_id", ["CartPole-v1", "Pendulum-v1"])
def test_runner_trains_on_physics_envs(env_id):
    from envs import CartPoleEnv, PendulumEnv
    from run_sequential import SequentialRunner
    r = SequentialRunner(env_id=env_id, physics=True, batch_size=32, antithetic=True, noise_table_size=1 << 20,
                         verbose=False)
    assert isinstance(r.env, CartPoleEnv if env_id.startswith("CartPole") else PendulumEnv)
    before = r.policy.get_trainable_flat().copy()
    seen = []
    launch = r.worker.launch

    def spy(*a, **kw):
        out = launch(*a, **kw)
        seen.append(out[0].timesteps.clone())
        return out
    r.worker.launch = spy
    r.train(2)
    torch.cuda.synchronize()
    after = r.policy.get_trainable_flat()
    assert np.all(np.isfinite(after)) and not np.array_equal(before, after)
    assert len(seen) == 2
    total = int(sum(int(s.sum()) for s in seen))
    n_lanes = int(sum(s.numel() for s in seen))
    assert r.agent.cumulative_timesteps == total
    if env_id.startswith("CartPole"):
        assert n_lanes >= 128 and total < n_lanes * 500
    else:
        assert total == n_lanes * 200


def test_runner_default_keeps_the_synthetic_env():
    from envs import SyntheticEnv
    from run_sequential import SequentialRunner
    r = SequentialRunner(env_id="CartPole-v1", batch_size=4, noise_table_size=1 << 20, verbose=False)
    assert isinstance(r.env, SyntheticEnv) and (r.env.obs_dim, r.env.act_dim, r.env.episode_len) == (4, 2, 500)
