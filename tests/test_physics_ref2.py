"""CPU: the numpy restatement of Acrobot-v1 / MountainCar-v0 / MountainCarContinuous-v0 (tests/physics_ref2.py) and the
host layers of these envs -- ids, descriptors, constants.  The GPU parity tests (tests/test_gpu_physics_envs2.py) lean
on this restatement, so its own f32 error against f64 is pinned here, over 10^6 random states per env with these seeds,
each figure asserted at the measured value rounded up to one digit:

  MountainCar-v0            position 6.6e-8, velocity 6.1e-9                      asserted 7e-8 / 7e-9
  MountainCarContinuous-v0  position 6.7e-8, velocity 7.6e-9, reward 3.9e-6       asserted 7e-8 / 8e-9 / 4e-6
                            (actions in [-3, 3])
  Acrobot-v1                (th1, th2, thd1, thd2) 6.0e-7, 7.4e-7, 2.2e-6, 4.3e-6   asserted 7e-7 / 8e-7 / 3e-6 / 5e-6
                            on the box |thd1| <= 6, |thd2| <= 10 (angles anywhere in [-pi, pi]).

The Acrobot box is the one the GPU test's episodes visit: on this restatement the 61-lane case of
test_gpu_physics_envs2.py keeps its random-init lanes (sampled and deterministic) within |thd1| <= 4.9, |thd2| <= 9.5,
and only the last swings of the bang-bang controller lanes leave the box (|thd1| up to 6.3, |thd2| up to 11.4: 0.004 %
of its 27,112 transitions; the GPU test leaves those out).  Over the full clamp box (+-4 pi, +-9 pi) the f32 step is far
worse (about 1e-2 in the velocities: the dynamics amplify rounding with the square of the speed), so the box is part of
the statement."""
import os

import numpy as np
import pytest

import physics_ref2 as ref

N = 1000000
ACROBOT_BOX, ACROBOT_ERR, MC_ERR, MCC_ERR = ref.ACROBOT_BOX, ref.ACROBOT_ERR, ref.MC_ERR, ref.MCC_ERR


def test_the_pinned_figures():
    """The bounds the GPU tests scale by 10 are the ones stated above."""
    assert ACROBOT_BOX == (6.0, 10.0) and ACROBOT_ERR == (7e-7, 8e-7, 3e-6, 5e-6)
    assert MC_ERR == (7e-8, 7e-9) and MCC_ERR == (7e-8, 8e-9, 4e-6)


# ---- restatement error ------------------------------------------------------------------------------------------
def test_acrobot_f32_step_error_vs_f64():
    rs = np.random.RandomState(0)
    s = np.stack([rs.uniform(-np.pi, np.pi, N), rs.uniform(-np.pi, np.pi, N),
                  rs.uniform(-ACROBOT_BOX[0], ACROBOT_BOX[0], N), rs.uniform(-ACROBOT_BOX[1], ACROBOT_BOX[1], N)],
                 axis=-1).astype(np.float32)
    a = rs.randint(0, 3, N)
    d = ref.acrobot_step_f32(s, a).astype(np.float64) - ref.acrobot_step_f64(s.astype(np.float64), a)
    d[:, :2] = (d[:, :2] + np.pi) % (2 * np.pi) - np.pi      # the angles live on the circle
    err = np.abs(d).max(axis=0)
    print("acrobot f32 vs f64 one-step max error per component:", err)
    for e, bound in zip(err, ACROBOT_ERR):
        assert e <= bound


@pytest.mark.parametrize("cont", [False, True])
def test_mountaincar_f32_step_error_vs_f64(cont):
    rs = np.random.RandomState(3)
    p = rs.uniform(-1.2, 0.6, N).astype(np.float32)
    v = rs.uniform(-0.07, 0.07, N).astype(np.float32)
    a = rs.uniform(-3, 3, N).astype(np.float32) if cont else rs.randint(0, 3, N)
    p32, v32, d32, r32 = ref.mountaincar_step_f32(p, v, a, cont)
    p64, v64, d64, r64 = ref.mountaincar_step_f64(p.astype(np.float64), v.astype(np.float64),
                                                  a.astype(np.float64) if cont else a, cont)
    e_pos, e_vel = np.abs(p32 - p64).max(), np.abs(v32 - v64).max()
    same = d32 == d64                                        # the +100 is not a rounding error
    e_rew = np.abs(r32.astype(np.float64) - r64)[same].max()
    print("mountaincar cont=%s f32 vs f64 one-step max error: pos %.3g vel %.3g reward %.3g (%d goal tests differ)"
          % (cont, e_pos, e_vel, e_rew, int((~same).sum())))
    bound = MCC_ERR if cont else MC_ERR
    assert e_pos <= bound[0]
    assert e_vel <= bound[1]
    assert (~same).sum() <= 2
    if cont:
        assert e_rew <= bound[2]
    else:
        assert np.all(r32 == -1.0) and np.all(r64 == -1.0)
    assert np.all(np.abs(v32) <= np.float32(0.07)) and np.all(p32 >= np.float32(-1.2)) and np.all(p32 <= np.float32(0.6))


# ---- known values -----------------------------------------------------------------------------------------------
def test_mountaincar_known_values():
    # one step from rest at the valley's bottom (cos(3 pos) = 0 at pos = -pi / 6), push right
    p, v, done, r = ref.mountaincar_step_f64(-np.pi / 6, 0.0, 2)
    np.testing.assert_allclose(v, 0.001, rtol=0, atol=1e-18)
    np.testing.assert_allclose(p, -np.pi / 6 + v, rtol=1e-15)
    assert not done and r == -1.0
    # gravity alone: vel -= 0.0025 cos(3 pos)
    p, v, _, _ = ref.mountaincar_step_f64(0.0, 0.0, 1)
    assert v == -0.0025 and p == -0.0025
    # the speed clamps to 0.07, the position to [-1.2, 0.6]
    _, v, _, _ = ref.mountaincar_step_f64(-0.5, 0.0699, 2)
    assert v == 0.07
    p, v, done, _ = ref.mountaincar_step_f64(0.58, 0.07, 2)
    assert p == 0.6 and done
    # the left wall stops the car: position clamped to -1.2 with a leftward velocity -> velocity 0
    p, v, done, _ = ref.mountaincar_step_f64(-1.19, -0.05, 0)
    assert p == -1.2 and v == 0.0 and not done
    p32, v32, _, _ = ref.mountaincar_step_f32(np.float32(-1.19), np.float32(-0.05), 0)
    assert p32 == np.float32(-1.2) and v32 == 0.0 and p32.dtype == np.float32
    # the goal: position >= 0.5 AND velocity >= 0 (0.49 + 0.0112.. crosses it; from above moving left it does not count)
    p, v, done, r = ref.mountaincar_step_f64(0.49, 0.01, 2)
    assert p >= 0.5 and v > 0 and done and r == -1.0          # -1 on the finishing step too
    p, v, done, _ = ref.mountaincar_step_f64(0.52, -0.005, 0)
    assert p >= 0.5 and v < 0 and not done
    p, v, done, _ = ref.mountaincar_step_f64(0.45, 0.01, 2)
    assert 0.45 < p < 0.5 and not done                        # MountainCar-v0's goal is 0.5, not 0.45


def test_mountaincar_continuous_known_values():
    # the force is the action clamped to +-1 (power 0.0015); the cost is 0.1 a^2 of the UNCLIPPED action
    p, v, done, r = ref.mountaincar_step_f64(-np.pi / 6, 0.0, 2.5, cont=True)
    np.testing.assert_allclose(v, 0.0015, rtol=0, atol=1e-18)
    assert not done
    np.testing.assert_allclose(r, -0.1 * 2.5 ** 2, rtol=1e-15)
    p, v, _, r = ref.mountaincar_step_f64(-np.pi / 6, 0.0, -0.5, cont=True)
    np.testing.assert_allclose(v, -0.00075, rtol=0, atol=1e-18)
    np.testing.assert_allclose(r, -0.025, rtol=1e-15)
    # the goal is 0.45 here; +100 arrives with that step's action cost
    p, v, done, r = ref.mountaincar_step_f64(0.44, 0.02, 3.0, cont=True)
    assert p >= 0.45 and v > 0 and done
    np.testing.assert_allclose(r, 100.0 - 0.9, rtol=1e-15)
    p, v, done, r = ref.mountaincar_step_f64(0.40, 0.01, 1.0, cont=True)
    assert not done
    np.testing.assert_allclose(r, -0.1, rtol=1e-15)
    # the same wall
    p, v, done, _ = ref.mountaincar_step_f64(-1.19, -0.05, -1.0, cont=True)
    assert p == -1.2 and v == 0.0 and not done


def test_acrobot_known_values():
    # hanging at rest, no torque: an equilibrium
    s = ref.acrobot_step_f64(np.zeros(4), 1)
    np.testing.assert_allclose(s, 0.0, atol=1e-15)
    # hanging at rest: the accelerations under torque tq are those of gym's expressions at th = 0,
    #   d1 = 0.25 + 2.25 + 2 = 4.5, d2 = 0.75 + 1 = 1.75, phi1 = phi2 = 0
    #   ddth2 = tq / (1.25 - d2^2 / d1), ddth1 = -d2 ddth2 / d1
    for act in (0, 2):
        k = ref._acrobot_dsdt(np.zeros(4), np.float64(act - 1), np.float64, True)
        dd2 = (act - 1) / (1.25 - 1.75 ** 2 / 4.5)
        np.testing.assert_allclose(k, [0.0, 0.0, -1.75 * dd2 / 4.5, dd2], rtol=1e-12, atol=1e-15)
    # gym's literal cos(th - pi / 2) and the sine form agree to rounding
    s0 = np.array([0.7, -1.1, 0.3, -0.4])
    np.testing.assert_allclose(ref._acrobot_step(s0, 2, np.float64, True), ref._acrobot_step(s0, 2, np.float64, False),
                               rtol=0, atol=1e-14)
    # the torque is action - 1: opposite actions mirror the mirrored state
    a, b = ref.acrobot_step_f64(s0, 0), ref.acrobot_step_f64(-s0, 2)
    np.testing.assert_allclose(a, -b, rtol=0, atol=1e-14)
    # wraps: an angle crossing +pi comes back near -pi (one 2 pi), the other way round too
    s = ref.acrobot_step_f64(np.array([3.1, 0.0, 2.0, 0.0]), 1)
    assert -np.pi <= s[0] < -np.pi + 0.6
    s = ref.acrobot_step_f64(np.array([0.0, -3.1, 0.0, -3.0]), 1)
    assert np.pi - 0.8 < s[1] <= np.pi
    # clamps: 4 pi on thd1, 9 pi on thd2
    rs = np.random.RandomState(2)
    fast = np.stack([rs.uniform(-np.pi, np.pi, 2000), rs.uniform(-np.pi, np.pi, 2000),
                     rs.choice([-1, 1], 2000) * 4 * np.pi, rs.choice([-1, 1], 2000) * 9 * np.pi], -1)
    raw, s = ref._acrobot_rk4(fast, 2, np.float64, True), ref.acrobot_step_f64(fast, 2)
    over1, over2 = np.abs(raw[:, 2]) > 4 * np.pi, np.abs(raw[:, 3]) > 9 * np.pi
    assert over1.sum() > 100 and over2.sum() > 100 and (~over1).sum() > 100
    np.testing.assert_array_equal(s[over1, 2], np.sign(raw[over1, 2]) * 4 * np.pi)
    np.testing.assert_array_equal(s[over2, 3], np.sign(raw[over2, 3]) * 9 * np.pi)
    np.testing.assert_array_equal(s[~over1, 2], raw[~over1, 2])
    s32 = ref.acrobot_step_f32(fast.astype(np.float32), 2)
    assert s32.dtype == np.float32 and np.all(np.abs(s32[:, 2]) <= np.float32(4) * np.float32(np.pi))
    # the single conditional 2 pi is gym's while-loop wrap wherever the angle moves less than 2 pi in a step: on the
    # pinned box (|thd1| <= 6, |thd2| <= 10) it moves less than 4 rad
    slow = fast * np.array([1.0, 1.0, 6 / (4 * np.pi), 10 / (9 * np.pi)])
    assert np.all(np.abs(ref._acrobot_rk4(slow, 2, np.float64, True)[:, :2] - slow[:, :2]) < 4.0)
    assert np.all(np.abs(ref.acrobot_step_f32(slow.astype(np.float32), 2)[:, :2]) <= np.float32(np.pi))
    # terminal: the free end above the bar by one link; upright is 2, hanging -2, horizontal 0
    assert ref.acrobot_terminal(np.array([np.pi, 0.0, 0, 0])) and ref.acrobot_height(np.array([np.pi, 0.0, 0, 0])) == 2
    assert not ref.acrobot_terminal(np.zeros(4)) and not ref.acrobot_terminal(np.array([np.pi / 2, 0.0, 0, 0]))
    assert not ref.acrobot_terminal(np.array([2 * np.pi / 3, 0.0, 0, 0]))      # exactly (up to rounding) 1: not above
    assert ref.acrobot_terminal(np.array([2 * np.pi / 3 + 1e-3, 0.0, 0, 0]))
    # the batched env pays -1 per step and 0 on the terminal step
    env = ref.BatchedAcrobot(2, 3)
    env.s = np.array([[np.pi - 0.05, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0]], np.float32)
    _, r = env.step(np.array([1, 1]))
    np.testing.assert_array_equal(env.failed(), [True, False])
    np.testing.assert_array_equal(r, [0.0, -1.0])
    # observation
    np.testing.assert_allclose(ref.acrobot_obs(np.array([0.5, -0.25, 1.5, -2.5]), np.float64),
                               [np.cos(0.5), np.sin(0.5), np.cos(0.25), -np.sin(0.25), 1.5, -2.5], rtol=1e-15)
    st = ref.acrobot_state_from_obs(ref.acrobot_obs(np.array([[3.0, -2.0, 1.5, -2.5]], np.float32)))
    np.testing.assert_allclose(st, [[3.0, -2.0, 1.5, -2.5]], rtol=0, atol=3e-7)


# ---- resets -----------------------------------------------------------------------------------------------------
def test_resets_lie_in_range_and_depend_on_the_lane():
    lanes = np.arange(5000, dtype=np.uint64)
    s = ref.acrobot_reset(7, lanes)
    assert s.dtype == np.float32 and s.shape == (5000, 4)
    assert np.all(s >= -0.1) and np.all(s < 0.1)
    assert abs(float(s.mean())) < 4e-3 and len(np.unique(s[:, 0])) > 4900
    p, v = ref.mountaincar_reset(7, lanes)
    assert p.dtype == np.float32 and np.all(p >= np.float32(-0.6)) and np.all(p < -0.4) and np.all(v == 0)
    assert p.min() < -0.59 and p.max() > -0.41 and len(np.unique(p)) > 4900
    # keyed by the global lane id: a shard sees the same states; another seed does not
    np.testing.assert_array_equal(ref.acrobot_reset(7, lanes[1000:1010]), s[1000:1010])
    np.testing.assert_array_equal(ref.mountaincar_reset(7, lanes[1000:1010])[0], p[1000:1010])
    assert not np.array_equal(ref.acrobot_reset(8, lanes), s)
    o = ref.BatchedAcrobot(10, 7, lanes[1000:1010]).reset()
    np.testing.assert_array_equal(o[:, 4:], s[1000:1010, 2:])
    np.testing.assert_allclose(o[:, 0] ** 2 + o[:, 1] ** 2, 1.0, atol=1e-6)
    for cls in (ref.BatchedMountainCar, ref.BatchedMountainCarContinuous):
        o = cls(10, 7, lanes[1000:1010]).reset()
        np.testing.assert_array_equal(o[:, 0], p[1000:1010])
        assert np.all(o[:, 1] == 0)
    # both MountainCars share the reset; it is draw 0 of the slot Acrobot's th1 uses, scaled to another range
    u = (s[:, 0].astype(np.float64) + 0.1) / 0.2
    np.testing.assert_allclose((p.astype(np.float64) + 0.6) / 0.2, u, rtol=0, atol=1e-6)


# ---- controllers ------------------------------------------------------------------------------------------------
CONTROLLERS = {
    # env: (kind, n_in, n_act, batched env, controller, T, steps-to-finish range on 16 resets)
    "acrobot": ("discrete", 6, 3, ref.BatchedAcrobot, ref.acrobot_controller, 500, (60, 300)),
    "mountaincar": ("discrete", 2, 3, ref.BatchedMountainCar, ref.mountaincar_controller, 200, (100, 135)),
    "mountaincar_cont": ("mujoco", 2, 1, ref.BatchedMountainCarContinuous, ref.mountaincar_cont_controller, 999,
                         (70, 125)),
}


@pytest.mark.parametrize("name", sorted(CONTROLLERS))
def test_controllers_finish_on_the_restatement(name):
    """Deterministic sign-0 lanes of the hand-built controllers reach the goal closed-loop through evaluate_lanes;
    the returns follow from the step counts."""
    from oracle import agent as oagent
    from oracle import policies as opol
    kind, n_in, n_act, Env, ctrl, T, (lo, hi) = CONTROLLERS[name]
    theta = ctrl()
    assert theta.dtype == np.float32 and theta.size == opol.num_params(kind, n_in, n_act)
    L = 16
    env = Env(L, 5, T=T)
    ret, ent, steps, norm2 = oagent.evaluate_lanes(kind, n_in, n_act, theta, np.zeros(theta.size, np.float32),
                                                   np.zeros(L, np.int64), np.zeros(L, np.int8), 0.02, env, 5,
                                                   deterministic=True, jiggle=False)
    print(name, "controller steps:", steps)
    assert np.all(steps >= lo) and np.all(steps <= hi) and np.all(steps < T)
    assert np.all(norm2 == 0)
    if name == "acrobot":
        np.testing.assert_array_equal(ret, -(steps - 1.0))
    elif name == "mountaincar":
        np.testing.assert_array_equal(ret, -steps.astype(np.float64))
    else:
        assert np.all(ret > 100 - 0.1 * steps) and np.all(ret < 100)      # |mean| < 1: cost below 0.1 per step
    assert np.all(np.isfinite(ent))


def test_discrete_controller_is_bang_bang():
    from oracle import policies as opol
    theta = ref.discrete3_controller(2, [0.0, 1.0], gain=2000.0)
    x = np.array([[-0.5, 0.03], [-0.5, -0.03], [0.2, 1e-3], [0.2, -1e-3], [-0.5, 0.0]], np.float32)
    p = opol.lanes_forward("discrete", 2, 3, np.broadcast_to(theta, (5, theta.size)), x)
    np.testing.assert_array_equal(np.argmax(p, -1), [2, 0, 2, 0, 2])          # the tie at rest goes to action 2
    assert np.all(p.max(-1)[:4] > 0.99)
    theta = ref.mountaincar_cont_controller()
    mean, std = opol.lanes_forward("mujoco", 2, 1, np.broadcast_to(theta, (3, theta.size)),
                                   np.array([[-0.5, 0.03], [-0.5, -0.03], [-0.5, 0.0]], np.float32))
    assert 0.9 < mean[0, 0] < 1 and -1 < mean[1, 0] < -0.9 and mean[2, 0] > 0
    np.testing.assert_allclose(std, 0.55, rtol=1e-6)


def test_random_init_lanes_do_not_finish():
    """Why the controllers exist: sampled lanes of a random-init policy run to the time limit."""
    from oracle import agent as oagent
    from oracle import noise as onoise
    from oracle import policies as opol
    theta = opol.TorchPolicy("discrete", 2, 3, seed=124).get_flat()
    assert theta.size == 4807
    tab = onoise.NoiseTable(1 << 16, theta.size, 124)
    L = 8
    idx = np.repeat(tab.sample_indices(L // 2), 2)
    sign = np.tile(np.array([1, -1], np.int8), L // 2)
    env = ref.BatchedMountainCar(L, 5)
    ret, ent, steps, _ = oagent.evaluate_lanes("discrete", 2, 3, theta, tab.table, idx, sign, 0.02, env, 5, jiggle=False)
    assert np.all(steps == 200) and np.all(ret == -200.0) and np.all((ent > 0) & (ent <= np.log(3) + 1e-12))
    assert opol.TorchPolicy("discrete", 6, 3, seed=124).get_flat().size == 5071
    assert opol.TorchPolicy("mujoco", 2, 1, seed=124).get_flat().size == 4482


# ---- host layers ------------------------------------------------------------------------------------------------
def test_lib_has_the_env_constants():
    from fdr import _lib
    assert (_lib.FDR_ENV_ACROBOT, _lib.FDR_ENV_MOUNTAINCAR, _lib.FDR_ENV_MOUNTAINCAR_CONT) == (4, 5, 6)
    assert (_lib.FDR_ENV_SYNTH, _lib.FDR_ENV_TRAP, _lib.FDR_ENV_CARTPOLE, _lib.FDR_ENV_PENDULUM) == (0, 1, 2, 3)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fdr.h")).read()
    for line in ("#define FDR_ENV_ACROBOT 4", "#define FDR_ENV_MOUNTAINCAR 5", "#define FDR_ENV_MOUNTAINCAR_CONT 6"):
        assert line in hdr


def test_env_descriptors():
    from envs import AcrobotEnv, MountainCarContinuousEnv, MountainCarEnv
    from fdr import _lib
    for env, kind, obs, act, T, disc in ((AcrobotEnv(), _lib.FDR_ENV_ACROBOT, 6, 3, 500, True),
                                         (MountainCarEnv(), _lib.FDR_ENV_MOUNTAINCAR, 2, 3, 200, True),
                                         (MountainCarContinuousEnv(), _lib.FDR_ENV_MOUNTAINCAR_CONT, 2, 1, 999, False),
                                         (AcrobotEnv(episode_len=30), _lib.FDR_ENV_ACROBOT, 6, 3, 30, True)):
        assert (env.obs_dim, env.act_dim, env.episode_len, env.discrete, env.terminates) == (obs, act, T, disc, True)
        d = env.desc()
        assert (d.kind, d.obs_dim, d.act_dim, d.episode_len) == (kind, obs, act, T)
        assert d.M is None and d.K is None and d.s0 is None and d.walkable is None
        assert (d.map_w, d.map_h, d.done_threshold, d.done_dim) == (0, 0, 0.0, 0)
    for cls in (AcrobotEnv, MountainCarEnv, MountainCarContinuousEnv):
        for bad in (0, -1, 10001):
            with pytest.raises(ValueError):
                cls(episode_len=bad)


def test_make_env_physics_ids():
    from envs import AcrobotEnv, MountainCarContinuousEnv, MountainCarEnv
    import run_sequential
    from run_sequential import make_env
    for env_id, cls, T in (("Acrobot-v1", AcrobotEnv, 500), ("MountainCar-v0", MountainCarEnv, 200),
                           ("MountainCarContinuous-v0", MountainCarContinuousEnv, 999)):
        e = make_env(env_id, physics=True)
        assert type(e) is cls and e.episode_len == T
        assert make_env(env_id, physics=True, episode_len=77).episode_len == 77
        assert env_id in run_sequential.PHYSICS_IDS
    for i in ("Acrobot-v0", "MountainCar-v1", "MountainCarContinuous", "Walker2d-v2"):
        with pytest.raises(ValueError) as ei:
            make_env(i, physics=True)
        msg = str(ei.value)
        assert "CartPole-v1" in msg and "Pendulum" in msg and "Acrobot-v1" in msg and "MountainCar-v0" in msg
