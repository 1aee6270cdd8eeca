"""numpy restatement of the linear policy (FDR_POLICY_LINEAR) and its episode loop on the five physics envs.

TEST INFRASTRUCTURE ONLY.  Everything the kernel defines is restated here operation for operation in f32:
    theta'   fl32(theta + sign * fl32(sigma * eps)), norm2 the f64 sum over ascending p of the squared f32 increment
             (NaN, and the lane unperturbed, for an offset outside [0, table_size - P])
    y        y_i = (((W'[i,0] x_0) + W'[i,1] x_1) + ...), every product and sum rounded to f32
    action   discrete: the smallest i attaining max y; continuous: y itself
    episode  reset from the counter stream (physics_ref / physics_ref2), state t recorded and offered to the Welford
             coin uniform(seed, id, t, 14) < chance before step t, rewards added in f64 in step order
The envs are the batched ones of physics_ref.py / physics_ref2.py.  run(..., dt=np.float64) is the f64 twin: the same
theta' and reset values, every later operation in f64 (the *_f64 step functions): the yardstick that tells which lanes'
step counts f32 rounding can move.
"""
import numpy as np

import physics_ref as ref
import physics_ref2 as ref2
from oracle import rng as crng

F = np.float32

# name -> (FDR_ENV_* kind, n_in, n_act, discrete)
ENVS = {"cartpole": (2, 4, 2, True), "pendulum": (3, 3, 1, False), "acrobot": (4, 6, 3, True),
        "mountaincar": (5, 2, 3, True), "mountaincar_cont": (6, 2, 1, False)}
_BATCHED = {"cartpole": ref.BatchedCartPole, "pendulum": ref.BatchedPendulum, "acrobot": ref2.BatchedAcrobot,
            "mountaincar": ref2.BatchedMountainCar, "mountaincar_cont": ref2.BatchedMountainCarContinuous}


def theta_prime(base, table, idx, sign, sigma, base_stride=0):
    """base [P] (stride 0) or [L, P] (stride P); -> theta' [L, P] f32, norm2 [L] f64."""
    base = np.asarray(base, F)
    L = len(idx)
    P = base.shape[-1]
    rows = np.broadcast_to(base, (L, P)) if base_stride == 0 else base.reshape(L, P)
    out = np.array(rows, F)
    n2 = np.zeros(L, np.float64)
    if table is None:
        return out, n2
    max_idx = len(table) - P
    s32 = F(sigma)
    for l in range(L):
        ix, sg = int(idx[l]), int(sign[l])
        if ix < 0 or ix > max_idx:
            n2[l] = np.nan
            continue
        if sg == 0:
            continue
        inc = (s32 * table[ix:ix + P]).astype(F)
        out[l] = (rows[l] + inc).astype(F) if sg > 0 else (rows[l] - inc).astype(F)
        acc = 0.0
        for v in inc.astype(np.float64):
            acc += v * v
        n2[l] = acc
    return out, n2


def dot_ordered(W, x, dt=F):
    """W [L, A, I], x [L, I] -> y [L, A] in dtype dt: the product of j = 0, then + the product of j, ascending."""
    W, x = np.asarray(W, dt), np.asarray(x, dt)
    acc = (W[:, :, 0] * x[:, None, 0]).astype(dt)
    for j in range(1, W.shape[2]):
        acc = (acc + (W[:, :, j] * x[:, None, j]).astype(dt)).astype(dt)
    return acc


def first_argmax(y):
    """The scan of the kernel: i replaces the choice where y_i > best."""
    act = np.zeros(len(y), np.int64)
    best = y[:, 0].copy()
    for i in range(1, y.shape[1]):
        gt = y[:, i] > best
        act[gt] = i
        best = np.maximum(best, y[:, i])
    return act


def normalise(s, mean, std, dt=F):
    if mean is None:
        return np.asarray(s, dt)
    return np.clip((np.asarray(s, dt) - np.asarray(mean, dt)) / np.asarray(std, dt), dt(-10), dt(10)).astype(dt)


def top_two_gap_small(y):
    """Discrete y [L, A]: the top-two gap is below 1e-4 max|y|."""
    s = np.sort(np.asarray(y, np.float64), axis=1)
    return (s[:, -1] - s[:, -2]) < 1e-4 * np.abs(y).max(axis=1)


class _Env(object):
    """One interface over the five systems in dtype dt: reset() -> obs, step(a) -> (obs, reward f64, done), and
    near() -> the state reached lies within 1e-5 of the termination test's boundary."""

    def __init__(self, name, seed, ids, dt):
        self.name, self.dt, self.f32 = name, dt, dt is F
        self.b = _BATCHED[name](len(ids), seed, np.asarray(ids, np.uint64), 1)   # the f32 batched env: resets, f32 steps

    def _obs(self):
        n, dt, b = self.name, self.dt, self.b
        if n == "cartpole":
            return np.asarray(self.s, dt)
        if n == "pendulum":
            return ref.pendulum_obs(self.th, self.thd, dt)
        if n == "acrobot":
            return ref2.acrobot_obs(self.s, dt)
        return np.stack([self.pos, self.vel], -1).astype(dt)

    def reset(self):
        n, dt, b = self.name, self.dt, self.b
        b.reset()
        if n in ("cartpole", "acrobot"):
            self.s = b.s.astype(dt)
        elif n == "pendulum":
            self.th, self.thd = b.theta.astype(dt), b.thetadot.astype(dt)
        else:
            self.pos, self.vel = b.pos.astype(dt), b.vel.astype(dt)
        return self._obs()

    def step(self, a):
        n, dt, b = self.name, self.dt, self.b
        L = b.n
        if self.f32:     # through the batched env itself
            obs, r = b.step(a)
            done = b.failed()
            if n in ("cartpole", "acrobot"):
                self.s = b.s
            elif n == "pendulum":
                self.th, self.thd = b.theta, b.thetadot
            else:
                self.pos, self.vel = b.pos, b.vel
            return obs, np.asarray(r, np.float64), done
        if n == "cartpole":
            self.s = ref.cartpole_step_f64(self.s, a)
            return self._obs(), np.ones(L), ref.cartpole_failed(self.s)
        if n == "pendulum":
            self.th, self.thd, r = ref.pendulum_step_f64(self.th, self.thd, np.asarray(a, dt).reshape(L))
            return self._obs(), r, np.zeros(L, bool)
        if n == "acrobot":
            self.s = ref2.acrobot_step_f64(self.s, a)
            done = ref2.acrobot_terminal(self.s)
            return self._obs(), np.where(done, 0.0, -1.0), done
        cont = n == "mountaincar_cont"
        a = np.asarray(a, dt).reshape(L) if cont else a
        self.pos, self.vel, done, r = ref2.mountaincar_step_f64(self.pos, self.vel, a, cont)
        return self._obs(), np.asarray(r, np.float64), done

    def near(self):
        n = self.name
        if n == "cartpole":
            return ref.cartpole_margin(self.s) < 1e-5
        if n == "acrobot":
            return ref2.acrobot_margin(self.s) < 1e-5
        if n == "pendulum":
            return np.zeros(self.b.n, bool)
        return ref2.mountaincar_borderline(self.pos, self.vel, cont=n == "mountaincar_cont")


def run(name, W, seed, ids, T, obs_mean=None, obs_std=None, obs_chance=None, dt=F):
    """One episode per lane: lane l plays theta' = W[l] ([L, A * I] f32) on stream id ids[l].  -> dict(ret f64, steps,
    states [L, T, I] (NaN where not visited), borderline, stats (WelfordRunningStat per lane, with obs_chance))."""
    _, n_in, n_act, disc = ENVS[name]
    ids = np.asarray(ids, np.uint64)
    L = len(ids)
    Wm = np.asarray(W, F).reshape(L, n_act, n_in)
    env = _Env(name, seed, ids, dt)
    obs = env.reset()
    states = np.full((L, T, n_in), np.nan, dt)
    alive = np.ones(L, bool)
    steps = np.full(L, T, np.int64)
    ret = np.zeros(L, np.float64)
    border = np.zeros(L, bool)
    stats = None
    if obs_chance is not None:
        from utils.math_helpers import WelfordRunningStat
        stats = [WelfordRunningStat(n_in) for _ in range(L)]
    for t in range(T):
        if not alive.any():
            break
        states[alive, t] = obs[alive]
        if stats is not None:
            coin = (crng.uniform(seed, ids, t, 14) < F(obs_chance)) & alive
            for l in np.nonzero(coin)[0]:
                stats[l].update(np.asarray(obs[l], F))
        y = dot_ordered(Wm, normalise(obs, obs_mean, obs_std, dt), dt)
        if disc:
            border |= alive & top_two_gap_small(y)
            a = first_argmax(y)
        else:
            a = y[:, 0]
        obs, r, done = env.step(a)
        border |= alive & env.near()
        ret[alive] += r[alive]
        steps[alive & done] = t + 1
        alive &= ~done
    return dict(ret=ret, steps=steps, states=states, borderline=border, stats=stats)


def run_episodes(name, W, seed, ids, T, **kw):
    """K episodes per lane, ids [L, K]: -> dict(ret = (((R_0 + R_1) + ..) + R_{K-1}) / K, ret_sq, steps, borderline)."""
    ids = np.asarray(ids, np.uint64)
    L, K = ids.shape
    rsum, rsq, nsum, border = np.zeros(L), np.zeros(L), np.zeros(L, np.int64), np.zeros(L, bool)
    for e in range(K):
        o = run(name, W, seed, ids[:, e], T, **kw)
        rsum = rsum + o["ret"]
        rsq = rsq + o["ret"] * o["ret"]
        nsum += o["steps"]
        border |= o["borderline"]
    return dict(ret=rsum / float(K), ret_sq=rsq, steps=nsum, borderline=border)
