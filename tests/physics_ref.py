"""numpy restatement of gym's classic_control CartPole-v1 and Pendulum-v1, as the rollout kernel runs them.

TEST INFRASTRUCTURE ONLY.  gym is not a dependency; these are its published formulas (cartpole.py: gravity 9.8,
masscart 1, masspole 0.1, half-length 0.5, force 10, tau 0.02, explicit Euler, failure at |x| > 2.4 or |theta| >
12 degrees; pendulum.py: g 10, m = l = 1, dt 0.05, max torque 2, max speed 8).  One-step functions in f32 (what the
kernel computes) and in f64 (the yardstick of the f32 error), and batched envs with the interface
oracle.agent.evaluate_lanes consumes: reset(), step(actions) -> (obs, reward), failed(), episode_len.

Resets are per lane, from the counter stream's reserved slot t = JIGGLE_T, k = i (k = 15 there is the jiggle's):
    CartPole  state[i] = fl32(fl32(0.1 u_i) - 0.05),  i = 0..3           (gym: U(-0.05, 0.05))
    Pendulum  theta = fl32(fl32(2 pi_f u_0) - pi_f),  thetadot = fl32(fl32(2 u_1) - 1)   (U(-pi, pi), U(-1, 1))
Pendulum keeps theta wrapped to [-pi, pi) after every step (gym leaves it unwrapped: the observation differs by
rounding only).
"""
import numpy as np

from oracle import rng as crng

F = np.float32
PI_F = F(np.pi)
TWO_PI_F = F(2.0 * np.pi)
X_THR = F(2.4)
THETA_THR = F(12 * 2 * np.pi / 360)


# ---- CartPole ---------------------------------------------------------------------------------------------------
def _cartpole_step(state, action, dt):
    """state [..., 4] (x, xdot, theta, thetadot) of dtype dt, action in {0, 1} -> next state (explicit Euler)."""
    c = lambda v: dt(v)  # noqa: E731
    x, xd, th, thd = (state[..., i] for i in range(4))
    force = np.where(np.asarray(action) == 1, c(10.0), c(-10.0)).astype(dt)
    sn, cs = np.sin(th).astype(dt), np.cos(th).astype(dt)
    temp = (force + c(0.05) * thd * thd * sn) / c(1.1)
    thacc = (c(9.8) * sn - cs * temp) / (c(0.5) * (c(4.0) / c(3.0) - c(0.1) * cs * cs / c(1.1)))
    xacc = temp - c(0.05) * thacc * cs / c(1.1)
    out = np.stack([x + c(0.02) * xd, xd + c(0.02) * xacc, th + c(0.02) * thd, thd + c(0.02) * thacc], axis=-1)
    return out.astype(dt)


def cartpole_step_f32(state, action):
    return _cartpole_step(np.asarray(state, F), action, F)


def cartpole_step_f64(state, action):
    return _cartpole_step(np.asarray(state, np.float64), action, np.float64)


def cartpole_failed(state):
    s = np.asarray(state)
    return (s[..., 0] < -X_THR) | (s[..., 0] > X_THR) | (s[..., 2] < -THETA_THR) | (s[..., 2] > THETA_THR)


def cartpole_margin(state):
    """Distance of a state from the nearest failure threshold (>= 0 inside the bounds)."""
    s = np.asarray(state, np.float64)
    return np.minimum(np.abs(np.abs(s[..., 0]) - float(X_THR)), np.abs(np.abs(s[..., 2]) - float(THETA_THR)))


def cartpole_reset(seed, lane_ids):
    lanes = np.asarray(lane_ids, np.uint64)
    u = np.stack([crng.uniform(seed, lanes, crng.JIGGLE_T, i) for i in range(4)], axis=-1)
    return ((F(0.1) * u).astype(F) - F(0.05)).astype(F)


# ---- Pendulum ---------------------------------------------------------------------------------------------------
def _wrap(th, dt):
    pi, two_pi = (PI_F, TWO_PI_F) if dt is F else (np.pi, 2.0 * np.pi)
    return (np.mod((th + pi).astype(dt), dt(two_pi)) - dt(pi)).astype(dt)


def _pendulum_step(theta, thetadot, action, dt):
    """-> (theta', thetadot', reward): reward = -cost of the pre-step state; theta' wrapped to [-pi, pi)."""
    c = lambda v: dt(v)  # noqa: E731
    th, thd = np.asarray(theta, dt), np.asarray(thetadot, dt)
    u = np.clip(np.asarray(action, dt), c(-2.0), c(2.0))
    w = _wrap(th, dt)
    cost = w * w + c(0.1) * thd * thd + c(0.001) * u * u
    nthd = np.clip(thd + (c(15.0) * np.sin(th).astype(dt) + c(3.0) * u) * c(0.05), c(-8.0), c(8.0)).astype(dt)
    nth = _wrap((th + nthd * c(0.05)).astype(dt), dt)
    return nth, nthd, (-cost).astype(dt)


def pendulum_step_f32(theta, thetadot, action):
    return _pendulum_step(theta, thetadot, action, F)


def pendulum_step_f64(theta, thetadot, action):
    return _pendulum_step(theta, thetadot, action, np.float64)


def pendulum_obs(theta, thetadot, dt=F):
    th = np.asarray(theta, dt)
    return np.stack([np.cos(th).astype(dt), np.sin(th).astype(dt), np.asarray(thetadot, dt)], axis=-1)


def pendulum_reset(seed, lane_ids):
    lanes = np.asarray(lane_ids, np.uint64)
    u0, u1 = crng.uniform(seed, lanes, crng.JIGGLE_T, 0), crng.uniform(seed, lanes, crng.JIGGLE_T, 1)
    theta = ((TWO_PI_F * u0).astype(F) - PI_F).astype(F)
    thetadot = ((F(2.0) * u1).astype(F) - F(1.0)).astype(F)
    return theta, thetadot


# ---- batched envs (oracle.agent.evaluate_lanes) -----------------------------------------------------------------
class BatchedCartPole(object):
    obs_dim, act_dim, discrete = 4, 2, True

    def __init__(self, n, seed, lane_ids=None, T=500):
        self.n, self.seed, self.episode_len = int(n), seed, int(T)
        self.lane_ids = np.arange(n, dtype=np.uint64) if lane_ids is None else np.asarray(lane_ids, np.uint64)
        assert len(self.lane_ids) == self.n
        self.min_margin = np.full(self.n, np.inf)   # closest any visited state came to a threshold, per lane
        self.reset()

    def reset(self):
        self.s = cartpole_reset(self.seed, self.lane_ids)
        return self.s.copy()

    def step(self, actions):
        self.s = cartpole_step_f32(self.s, np.asarray(actions, np.int64))
        self.min_margin = np.minimum(self.min_margin, cartpole_margin(self.s))
        return self.s.copy(), np.ones(self.n, np.float64)

    def failed(self):
        return cartpole_failed(self.s)


class BatchedPendulum(object):
    obs_dim, act_dim, discrete = 3, 1, False

    def __init__(self, n, seed, lane_ids=None, T=200):
        self.n, self.seed, self.episode_len = int(n), seed, int(T)
        self.lane_ids = np.arange(n, dtype=np.uint64) if lane_ids is None else np.asarray(lane_ids, np.uint64)
        assert len(self.lane_ids) == self.n
        self.reset()

    def reset(self):
        self.theta, self.thetadot = pendulum_reset(self.seed, self.lane_ids)
        return pendulum_obs(self.theta, self.thetadot)

    def step(self, actions):
        a = np.asarray(actions, F).reshape(self.n)
        self.theta, self.thetadot, r = pendulum_step_f32(self.theta, self.thetadot, a)
        return pendulum_obs(self.theta, self.thetadot), r.astype(np.float64)

    def failed(self):
        return np.zeros(self.n, bool)
