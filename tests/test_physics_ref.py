"""CPU: the numpy restatement of CartPole-v1 / Pendulum-v1 (tests/physics_ref.py) and the host layers of the physics
envs -- ids, descriptors, constants.  The GPU parity tests (tests/test_gpu_physics_envs.py) lean on this restatement, so
its own f32 error against f64 is pinned here: measured max over 10^6 random states 3.3e-7 (CartPole, any component),
5.4e-7 (Pendulum state, theta compared on the circle) and 3.1e-6 (Pendulum reward) with these seeds; asserted at
1e-6 / 1e-6 / 1e-5."""
import numpy as np
import pytest

import physics_ref as ref

N = 1000000


def test_cartpole_f32_step_error_vs_f64():
    rs = np.random.RandomState(0)
    s = np.stack([rs.uniform(-2.4, 2.4, N), rs.uniform(-4, 4, N), rs.uniform(-0.21, 0.21, N),
                  rs.uniform(-4, 4, N)], axis=-1).astype(np.float32)
    a = rs.randint(0, 2, N)
    err = np.abs(ref.cartpole_step_f32(s, a).astype(np.float64) - ref.cartpole_step_f64(s.astype(np.float64), a))
    print("cartpole f32 vs f64 one-step max error per component:", err.max(axis=0))
    assert err.max() <= 1e-6


def test_pendulum_f32_step_error_vs_f64():
    rs = np.random.RandomState(1)
    th = rs.uniform(-np.pi, np.pi, N).astype(np.float32)
    thd = rs.uniform(-8, 8, N).astype(np.float32)
    u = rs.uniform(-3, 3, N).astype(np.float32)
    t32, d32, r32 = ref.pendulum_step_f32(th, thd, u)
    t64, d64, r64 = ref.pendulum_step_f64(th.astype(np.float64), thd.astype(np.float64), u.astype(np.float64))
    # theta lives on the circle: the two wraps may land on opposite ends of [-pi, pi)
    dth = np.abs((t32.astype(np.float64) - t64 + np.pi) % (2 * np.pi) - np.pi)
    e_state = max(dth.max(), np.abs(d32.astype(np.float64) - d64).max())
    e_rew = np.abs(r32.astype(np.float64) - r64).max()
    print("pendulum f32 vs f64 one-step max error: state %.3g reward %.3g" % (e_state, e_rew))
    assert e_state <= 1e-6
    assert e_rew <= 1e-5
    assert np.all(t32 >= -np.float32(np.pi)) and np.all(t32 <= np.float32(np.pi))
    assert np.all(np.abs(d32) <= 8)


def test_cartpole_step_known_values():
    """One hand-checked step: upright at rest, push right -> xacc = 10 / 1.1 - ..., theta accelerates negative."""
    s = ref.cartpole_step_f64(np.zeros(4), 1)
    temp = 10.0 / 1.1
    thacc = -temp / (0.5 * (4.0 / 3.0 - 0.1 / 1.1))
    np.testing.assert_allclose(s, [0.0, 0.02 * (temp - 0.05 * thacc / 1.1), 0.0, 0.02 * thacc], rtol=1e-12)
    # explicit Euler: positions advance with the OLD velocities
    s = ref.cartpole_step_f64(np.array([0.0, 1.0, 0.0, 2.0]), 0)
    assert s[0] == 0.02 and s[2] == 0.04
    assert not ref.cartpole_failed(np.array([2.4, 0, 0.2, 0], np.float32))
    assert ref.cartpole_failed(np.array([2.41, 0, 0, 0], np.float32))
    assert ref.cartpole_failed(np.array([0, 0, -0.21, 0], np.float32))


def test_pendulum_step_known_values():
    th, thd, r = ref.pendulum_step_f64(np.pi / 2, 1.0, 5.0)      # torque clamps to 2
    assert thd == 1.0 + (15.0 + 6.0) * 0.05
    np.testing.assert_allclose(th, np.pi / 2 + thd * 0.05, rtol=1e-12)
    np.testing.assert_allclose(r, -((np.pi / 2) ** 2 + 0.1 + 0.004), rtol=1e-12)
    _, thd, _ = ref.pendulum_step_f64(np.pi / 2, 7.9, 2.0)       # speed clamps to 8
    assert thd == 8.0
    th, _, _ = ref.pendulum_step_f64(3.1, 8.0, 0.0)              # crosses +pi: wrapped
    assert -np.pi <= th < -np.pi + 0.5


def test_resets_lie_in_range_and_depend_on_the_lane():
    lanes = np.arange(5000, dtype=np.uint64)
    s = ref.cartpole_reset(7, lanes)
    assert s.dtype == np.float32 and s.shape == (5000, 4)
    assert np.all(s >= -0.05) and np.all(s < 0.05)
    assert abs(float(s.mean())) < 2e-3 and len(np.unique(s[:, 0])) > 4900
    th, thd = ref.pendulum_reset(7, lanes)
    assert np.all(th >= -np.float32(np.pi)) and np.all(th <= np.float32(np.pi))
    assert np.all(thd >= -1) and np.all(thd < 1)
    assert th.min() < -3.0 and th.max() > 3.0
    # keyed by the global lane id: a shard sees the same states
    np.testing.assert_array_equal(ref.cartpole_reset(7, lanes[1000:1010]), s[1000:1010])
    np.testing.assert_array_equal(ref.BatchedCartPole(10, 7, lanes[1000:1010]).reset(), s[1000:1010])
    assert not np.array_equal(ref.cartpole_reset(8, lanes), s)
    env = ref.BatchedPendulum(16, 7)
    o = env.reset()
    np.testing.assert_array_equal(o[:, 2], thd[:16])
    np.testing.assert_allclose(o[:, 0] ** 2 + o[:, 1] ** 2, 1.0, atol=1e-6)


def test_batched_envs_serve_the_oracle_episode_loop():
    """evaluate_lanes runs them unchanged: CartPole's return is its step count, episodes end on failure."""
    from oracle import agent as oagent
    from oracle import noise as onoise
    from oracle import policies as opol
    theta = opol.TorchPolicy("discrete", 4, 2, seed=124).get_flat()
    tab = onoise.NoiseTable(1 << 16, theta.size, 124)
    L = 8
    idx = np.repeat(tab.sample_indices(L // 2), 2)
    sign = np.tile(np.array([1, -1], np.int8), L // 2)
    env = ref.BatchedCartPole(L, 5, T=60)
    ret, ent, steps, _ = oagent.evaluate_lanes("discrete", 4, 2, theta, tab.table, idx, sign, 0.02, env, 5, jiggle=False)
    np.testing.assert_array_equal(ret, steps)
    assert steps.min() >= 8 and steps.max() <= 60 and np.all((ent > 0) & (ent <= np.log(2) + 1e-12))
    theta = opol.TorchPolicy("mujoco", 3, 1, seed=124).get_flat()
    assert theta.size == 4546
    tab = onoise.NoiseTable(1 << 16, theta.size, 124)
    env = ref.BatchedPendulum(L, 5, T=20)
    ret, ent, steps, _ = oagent.evaluate_lanes("mujoco", 3, 1, theta, tab.table, idx, sign, 0.02, env, 5, jiggle=False)
    assert np.all(steps == 20) and np.all(ret < 0) and np.all(np.isfinite(ent))


def test_lib_has_the_env_constants():
    from fdr import _lib
    assert (_lib.FDR_ENV_SYNTH, _lib.FDR_ENV_TRAP, _lib.FDR_ENV_CARTPOLE, _lib.FDR_ENV_PENDULUM) == (0, 1, 2, 3)
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fdr.h")).read()
    assert "#define FDR_ENV_CARTPOLE 2" in hdr and "#define FDR_ENV_PENDULUM 3" in hdr


def test_env_descriptors():
    from envs import CartPoleEnv, PendulumEnv
    from fdr import _lib
    for env, kind, obs, act, T, disc, term in ((CartPoleEnv(), _lib.FDR_ENV_CARTPOLE, 4, 2, 500, True, True),
                                               (PendulumEnv(), _lib.FDR_ENV_PENDULUM, 3, 1, 200, False, False),
                                               (CartPoleEnv(episode_len=30), _lib.FDR_ENV_CARTPOLE, 4, 2, 30, True,
                                                True)):
        assert (env.obs_dim, env.act_dim, env.episode_len, env.discrete, env.terminates) == (obs, act, T, disc, term)
        d = env.desc()
        assert (d.kind, d.obs_dim, d.act_dim, d.episode_len) == (kind, obs, act, T)
        assert d.M is None and d.K is None and d.s0 is None and d.walkable is None
        assert (d.map_w, d.map_h, d.done_threshold, d.done_dim) == (0, 0, 0.0, 0)
    for bad in (0, -1, 10001):
        with pytest.raises(ValueError):
            CartPoleEnv(episode_len=bad)
        with pytest.raises(ValueError):
            PendulumEnv(episode_len=bad)


def test_make_env_physics_ids():
    from envs import CartPoleEnv, PendulumEnv
    from run_sequential import make_env
    e = make_env("CartPole-v1", physics=True)
    assert isinstance(e, CartPoleEnv) and e.episode_len == 500
    e = make_env("CartPole-v0", physics=True)
    assert isinstance(e, CartPoleEnv) and e.episode_len == 200
    for i in ("Pendulum-v1", "Pendulum-v0"):
        e = make_env(i, physics=True)
        assert isinstance(e, PendulumEnv) and e.episode_len == 200
    assert make_env("CartPole-v1", physics=True, episode_len=77).episode_len == 77
    assert make_env("Pendulum-v1", physics=True, episode_len=50).episode_len == 50
    for i in ("Walker2d-v2", "HalfCheetah-v2", "SimpleTrapEnv-v0", "CartPole-v2", "PongNoFrameskip-v4"):
        with pytest.raises(ValueError) as ei:
            make_env(i, physics=True)
        assert "CartPole-v1" in str(ei.value) and "Pendulum" in str(ei.value)
