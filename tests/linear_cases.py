"""The seeded cases of the linear-policy tests (pure numpy: tests/test_linear_ref.py pins their conditions on the CPU,
tests/test_gpu_linear_policy.py runs them on the GPU).

A case is 64 lanes of one env: theta = N(0, 1) * scale, lane l runs theta' = theta + sign_l * fl32(sigma * eps_l) from a
shared 65,536-float noise table, sigma of the order of scale so that the lanes are 64 different controllers and their
episodes spread from a few steps to the time limit inside one wave.  Conditions pinned on the CPU for every case: the
f32 restatement and its f64 twin agree on the step count of every lane not flagged borderline (a visited state within
1e-5 of a termination threshold, or a visited discrete y whose top-two gap is below 1e-4 max|y|), and at most 2 of the
64 lanes are borderline.
"""
import numpy as np

import linear_ref as lref

TABLE_SIZE = 1 << 16
L = 64


class Case(object):
    def __init__(self, env, seed, T, scale, sigma, obs_mean=None, obs_std=None, obs_chance=None, theta_seed=7,
                 lane_offset=0, K=1, theta=None):
        self.env, self.seed, self.T, self.scale, self.sigma = env, seed, T, scale, sigma
        self.kind, self.n_in, self.n_act, self.discrete = lref.ENVS[env]
        self.P = self.n_in * self.n_act
        self.obs_mean = None if obs_mean is None else np.asarray(obs_mean, np.float32)
        self.obs_std = None if obs_std is None else np.asarray(obs_std, np.float32)
        self.obs_chance = obs_chance
        self.lane_offset = lane_offset
        rs = np.random.RandomState(theta_seed)
        self.theta = (rs.randn(self.P) * scale).astype(np.float32)
        if theta is not None:                                     # a controller: scale * theta, perturbed by sigma
            self.theta = (np.asarray(theta, np.float64).reshape(self.P) * scale).astype(np.float32)
        self.table = table()
        self.idx = rs.randint(0, TABLE_SIZE - self.P + 1, size=L).astype(np.int64)
        self.idx[0], self.idx[1] = 0, TABLE_SIZE - self.P        # both table edges
        self.sign = np.where(np.arange(L) % 2 == 0, 1, -1).astype(np.int8)
        self.sign[[5, 40]] = 0                                    # two lanes of theta itself
        self.K = K                                                # episodes per lane: stream ids (lane_offset + l) K + e
        g = lane_offset + np.arange(L, dtype=np.uint64)
        self.ids = g[:, None] * np.uint64(K) + np.arange(K, dtype=np.uint64)[None, :]

    def thetas(self):
        return lref.theta_prime(self.theta, self.table, self.idx, self.sign, self.sigma)

    def run(self, dt=np.float32, e=0):
        """Episode e of every lane."""
        W, _ = self.thetas()
        return lref.run(self.env, W, self.seed, self.ids[:, e], self.T, obs_mean=self.obs_mean, obs_std=self.obs_std,
                        obs_chance=self.obs_chance if dt is np.float32 else None, dt=dt)


_TABLE = []


def table():
    if not _TABLE:
        _TABLE.append(np.random.RandomState(99).randn(TABLE_SIZE).astype(np.float32))
    return _TABLE[0]


CART_MEAN, CART_STD = [0.01, -0.1, 0.005, 0.2], [0.05, 0.5, 0.04, 0.7]
ACRO_MEAN, ACRO_STD = [0.9, 0.0, 0.9, 0.05, 0.1, -0.2], [0.2, 0.4, 0.3, 0.5, 1.0, 2.0]

# Controllers (theta of a case = scale * these, before the perturbation): CartPole pushes along a weighted sum of the
# state; the MountainCars push along the velocity; Acrobot's torque opposes the first link's velocity.
CART_CTRL = [[0, 0, 0, 0], [0.3, 1.0, 5.0, 1.5]]
MC_CTRL = [[0, -1], [0, 0], [0, 1]]
MCC_CTRL = [[0, 1]]
ACRO_CTRL = [[0, 0, 0, 0, 1, 0], [0, 0, 0, 0, 0, 0], [0, 0, 0, 0, -1, 0]]

# name -> constructor arguments (cases are built on demand and cached)
_SPECS = {
    # whole episodes against the restatement (short: closed-loop CartPole and Acrobot episodes amplify rounding).  The
    # MountainCars are not chaotic: their cases run to the goal (86 .. 160 steps).  Pendulum: T = 16, where the f32
    # restatement's return stays within 6e-5 of its f64 twin's (the tolerance there is 16 x 2e-5).
    "cartpole": dict(env="cartpole", seed=201, T=64, scale=1.0, sigma=3.0, theta=CART_CTRL),
    "pendulum": dict(env="pendulum", seed=102, T=16, scale=1.0, sigma=1.0),
    "acrobot": dict(env="acrobot", seed=103, T=64, scale=1.0, sigma=1.0),
    "mountaincar": dict(env="mountaincar", seed=104, T=160, scale=1.0, sigma=0.02, theta=MC_CTRL),
    "mountaincar_cont": dict(env="mountaincar_cont", seed=104, T=160, scale=30.0, sigma=0.6, theta=MCC_CTRL),
    # recorded trajectories checked step by step: CartPole to T = 200 and Acrobot reaching its goal
    "cartpole_long": dict(env="cartpole", seed=102, T=200, scale=1.0, sigma=1.0, theta=CART_CTRL),
    "acrobot_ctrl": dict(env="acrobot", seed=104, T=200, scale=1.0, sigma=1.0, theta=ACRO_CTRL),
    # normalised observations, and the Welford statistics
    "cartpole_norm": dict(env="cartpole", seed=111, T=64, scale=1.0, sigma=1.0, obs_mean=CART_MEAN, obs_std=CART_STD),
    "acrobot_norm": dict(env="acrobot", seed=112, T=64, scale=1.0, sigma=1.0, obs_mean=ACRO_MEAN, obs_std=ACRO_STD),
    "cartpole_stats": dict(env="cartpole", seed=113, T=64, scale=1.0, sigma=3.0, theta=CART_CTRL, obs_chance=0.5),
    "acrobot_stats": dict(env="acrobot", seed=114, T=64, scale=1.0, sigma=1.0, obs_chance=0.25, obs_mean=ACRO_MEAN,
                          obs_std=ACRO_STD),
    # the K = 3 fold reads the stream ids (lane_offset + l) * 3 + e
    "cartpole_k3": dict(env="cartpole", seed=121, T=64, scale=1.0, sigma=3.0, theta=CART_CTRL, K=3, lane_offset=1000),
}
GPU_CASES = tuple(_SPECS)
_CACHE = {}


def case(name):
    if name not in _CACHE:
        _CACHE[name] = Case(**_SPECS[name])
    return _CACHE[name]
