"""numpy restatement of gym's classic_control Acrobot-v1, MountainCar-v0 and MountainCarContinuous-v0, as the rollout
kernel runs them (the companion of physics_ref.py, same style and interface).

TEST INFRASTRUCTURE ONLY.  gym is not a dependency; these are its published formulas:
  acrobot.py                  "book" dynamics, m1 = m2 = 1, l1 = 1, lc1 = lc2 = 0.5, I1 = I2 = 1, g = 9.8, dt = 0.2, no
                              torque noise; torque = action - 1; one classical RK4 step of dsdt over [0, dt]; the angles
                              wrapped into [-pi, pi], the velocities clamped to +-4 pi / +-9 pi; terminal when
                              -cos th1 - cos(th1 + th2) > 1; reward -1, 0 on the terminal step; 500 steps.
  mountain_car.py             vel += (a - 1) 0.001 - 0.0025 cos(3 pos), clamped to +-0.07; pos += vel, clamped to
                              [-1.2, 0.6]; vel = 0 at the left wall; done at pos >= 0.5 (vel >= 0); reward -1; 200 steps.
  continuous_mountain_car.py  force = clamp(a, +-1), power 0.0015, goal 0.45; reward (done ? 100 : 0) - 0.1 a^2 with the
                              unclipped a; 999 steps.
One-step functions in f32 (what the kernel computes) and in f64 (the yardstick of the f32 error), and batched envs with
the interface oracle.agent.evaluate_lanes consumes: reset(), step(actions) -> (obs, reward), failed(), episode_len.
The f64 Acrobot form is gym's literal cos(th - pi / 2); the f32 one takes the sine, as the kernel does.

Resets are per lane, from the counter stream's reserved slot t = JIGGLE_T, k = i (k = 15 there is the jiggle's):
    Acrobot      state[i] = fl32(fl32(0.2 u_i) - 0.1), i = 0..3     (gym: U(-0.1, 0.1))
    MountainCar  pos = fl32(fl32(0.2 u_0) - 0.6), vel = 0           (gym: U(-0.6, -0.4)), both variants

Controller policies: hand-built parameter vectors that make the MLP a bang-bang controller, so the envs' success
terminations are reached closed-loop (uniformly random actions essentially never finish these tasks).
"""
import numpy as np

from oracle import policies as opol
from oracle import rng as crng

F = np.float32
PI_F = F(np.pi)
TWO_PI_F = F(2.0 * np.pi)

# The f32 one-step error of this restatement against f64, as tests/test_physics_ref2.py pins it (max over 10^6 random
# states, rounded up to one digit); the GPU tests allow ten times these.
ACROBOT_BOX = (6.0, 10.0)                  # |thd1|, |thd2| of the pre-step states the Acrobot figures hold on
ACROBOT_ERR = (7e-7, 8e-7, 3e-6, 5e-6)     # th1, th2, thd1, thd2
# The same over the whole legal box |thd1| <= 4 pi, |thd2| <= 9 pi (tests/test_physics_branches_ref.py pins it: measured
# 2.0e-5, 2.8e-5, 1.3e-2, 1.7e-2; the dynamics amplify rounding with the square of the speed)
ACROBOT_ERR_WIDE = (2e-5, 3e-5, 2e-2, 2e-2)
MC_ERR = (7e-8, 7e-9)                      # MountainCar-v0: position, velocity
MCC_ERR = (7e-8, 8e-9, 4e-6)               # MountainCarContinuous-v0: position, velocity, reward (|a| <= 3)


# ---- Acrobot ----------------------------------------------------------------------------------------------------
def _acrobot_dsdt(s, tq, dt, literal):
    c = dt
    th1, th2, d1, d2 = (s[..., i] for i in range(4))
    g = c(9.8)
    cos2, sin2 = np.cos(th2).astype(dt), np.sin(th2).astype(dt)
    dd1 = c(0.25) + (c(1.0) + c(0.25) + cos2) + c(2.0)   # m1 lc1^2 + m2 (l1^2 + lc2^2 + 2 l1 lc2 cos th2) + I1 + I2
    dd2 = (c(0.25) + c(0.5) * cos2) + c(1.0)             # m2 (lc2^2 + l1 lc2 cos th2) + I2
    if literal:
        hp = c(np.pi / 2.0)
        phi2 = c(0.5) * g * np.cos(th1 + th2 - hp).astype(dt)
        ct = np.cos(th1 - hp).astype(dt)
    else:
        phi2 = c(0.5) * g * np.sin(th1 + th2).astype(dt)
        ct = np.sin(th1).astype(dt)
    phi1 = -c(0.5) * d2 * d2 * sin2 - c(1.0) * d2 * d1 * sin2 + c(1.5) * g * ct + phi2
    ddth2 = (tq + dd2 / dd1 * phi1 - c(0.5) * d1 * d1 * sin2 - phi2) / (c(0.25) + c(1.0) - dd2 * dd2 / dd1)
    ddth1 = -(dd2 * ddth2 + phi1) / dd1
    return np.stack([d1, d2, ddth1, ddth2], -1).astype(dt)


def _wrap1(x, dt):
    """gym's wrap(x, -pi, pi) as one conditional +-2 pi (|thetadot| dt < 2 pi: its while loops run at most once)."""
    pi, two = (PI_F, TWO_PI_F) if dt is F else (np.pi, 2.0 * np.pi)
    return np.where(x > pi, x - dt(two), np.where(x < -pi, x + dt(two), x)).astype(dt)


def _acrobot_rk4(state, action, dt, literal):
    """One classical RK4 step of dsdt over [0, 0.2], before the wrap and the clamp."""
    s = np.asarray(state, dt)
    tq = (np.asarray(action) - 1).astype(dt)
    h = dt(0.2)
    k1 = _acrobot_dsdt(s, tq, dt, literal)
    k2 = _acrobot_dsdt((s + h / dt(2) * k1).astype(dt), tq, dt, literal)
    k3 = _acrobot_dsdt((s + h / dt(2) * k2).astype(dt), tq, dt, literal)
    k4 = _acrobot_dsdt((s + h * k3).astype(dt), tq, dt, literal)
    return (s + h / dt(6) * (k1 + dt(2) * k2 + dt(2) * k3 + k4)).astype(dt)


def _acrobot_step(state, action, dt, literal):
    ns = _acrobot_rk4(state, action, dt, literal)
    pi = PI_F if dt is F else np.pi
    return np.stack([_wrap1(ns[..., 0], dt), _wrap1(ns[..., 1], dt),
                     np.clip(ns[..., 2], dt(-4) * dt(pi), dt(4) * dt(pi)),
                     np.clip(ns[..., 3], dt(-9) * dt(pi), dt(9) * dt(pi))], -1).astype(dt)


def acrobot_step_f32(state, action):
    """state [..., 4] (th1, th2, thd1, thd2), action in {0, 1, 2} -> next state."""
    return _acrobot_step(state, action, F, False)


def acrobot_step_f64(state, action):
    return _acrobot_step(state, action, np.float64, True)


def acrobot_height(state):
    """-cos th1 - cos(th1 + th2): the free end's height above the pivot; terminal above 1."""
    s = np.asarray(state)
    return -np.cos(s[..., 0]) - np.cos(s[..., 1] + s[..., 0])


def acrobot_terminal(state):
    return acrobot_height(state) > 1.0


def acrobot_margin(state):
    return np.abs(acrobot_height(np.asarray(state, np.float64)) - 1.0)


def acrobot_obs(state, dt=F):
    s = np.asarray(state, dt)
    return np.stack([np.cos(s[..., 0]), np.sin(s[..., 0]), np.cos(s[..., 1]), np.sin(s[..., 1]), s[..., 2],
                     s[..., 3]], -1).astype(dt)


def acrobot_state_from_obs(obs):
    """The state an observation shows (angles through atan2: exact to an ulp of the cos / sin pair)."""
    o = np.asarray(obs, np.float64)
    return np.stack([np.arctan2(o[..., 1], o[..., 0]), np.arctan2(o[..., 3], o[..., 2]), o[..., 4], o[..., 5]],
                    -1).astype(F)


def acrobot_reset(seed, lane_ids):
    lanes = np.asarray(lane_ids, np.uint64)
    u = np.stack([crng.uniform(seed, lanes, crng.JIGGLE_T, i) for i in range(4)], axis=-1)
    return ((F(0.2) * u).astype(F) - F(0.1)).astype(F)


# ---- MountainCar (both variants) --------------------------------------------------------------------------------
GOAL, GOAL_CONT = 0.5, 0.45


def _mountaincar_step(pos, vel, action, dt, cont):
    """-> (pos', vel', done, reward).  action: {0, 1, 2}, or the continuous policy's (unclipped) action."""
    c = dt
    p, v = np.asarray(pos, dt), np.asarray(vel, dt)
    if cont:
        a = np.asarray(action, dt)
        push = np.clip(a, c(-1.0), c(1.0)) * c(0.0015)
    else:
        push = (np.asarray(action) - 1).astype(dt) * c(0.001)
    v = (v + push - c(0.0025) * np.cos(c(3.0) * p).astype(dt)).astype(dt)
    v = np.clip(v, c(-0.07), c(0.07)).astype(dt)
    p = np.clip((p + v).astype(dt), c(-1.2), c(0.6)).astype(dt)
    v = np.where((p == c(-1.2)) & (v < 0), c(0.0), v).astype(dt)
    done = (p >= c(GOAL_CONT if cont else GOAL)) & (v >= 0)
    if cont:
        rew = (np.where(done, c(100.0), c(0.0)) - c(0.1) * a * a).astype(dt)
    else:
        rew = np.full(np.shape(p), -1.0, dt)
    return p, v, done, rew


def mountaincar_step_f32(pos, vel, action, cont=False):
    return _mountaincar_step(pos, vel, action, F, cont)


def mountaincar_step_f64(pos, vel, action, cont=False):
    return _mountaincar_step(pos, vel, action, np.float64, cont)


def mountaincar_done(pos, vel, cont=False):
    return (np.asarray(pos) >= F(GOAL_CONT if cont else GOAL)) & (np.asarray(vel) >= 0)


def mountaincar_borderline(pos, vel, cont=False, eps=1e-5):
    """A state within eps of the goal test's boundary: pos near the goal, or at / past it with vel near 0."""
    p, v = np.asarray(pos, np.float64), np.asarray(vel, np.float64)
    goal = float(F(GOAL_CONT if cont else GOAL))
    return (np.abs(p - goal) < eps) | ((p >= goal - eps) & (np.abs(v) < eps))


def mountaincar_reset(seed, lane_ids):
    lanes = np.asarray(lane_ids, np.uint64)
    u = crng.uniform(seed, lanes, crng.JIGGLE_T, 0)
    return ((F(0.2) * u).astype(F) - F(0.6)).astype(F), np.zeros(len(lanes), F)


# ---- batched envs (oracle.agent.evaluate_lanes) -----------------------------------------------------------------
class _Batched(object):
    def __init__(self, n, seed, lane_ids, T):
        self.n, self.seed, self.episode_len = int(n), seed, int(T)
        self.lane_ids = np.arange(n, dtype=np.uint64) if lane_ids is None else np.asarray(lane_ids, np.uint64)
        assert len(self.lane_ids) == self.n
        self.borderline = np.zeros(self.n, bool)   # some visited state within 1e-5 of the termination test's boundary
        self.done = np.zeros(self.n, bool)
        self.reset()

    def failed(self):
        """'done' of the state reached by the last step (a success here, not a failure)."""
        return self.done.copy()


class BatchedAcrobot(_Batched):
    obs_dim, act_dim, discrete = 6, 3, True

    def __init__(self, n, seed, lane_ids=None, T=500):
        self.max_speed = np.zeros((int(n), 2))     # largest |thd1|, |thd2| any PRE-step state of the lane had
        super().__init__(n, seed, lane_ids, T)

    def reset(self):
        self.s = acrobot_reset(self.seed, self.lane_ids)
        return acrobot_obs(self.s)

    def step(self, actions):
        self.max_speed = np.maximum(self.max_speed, np.abs(self.s[:, 2:].astype(np.float64)))
        self.s = acrobot_step_f32(self.s, np.asarray(actions, np.int64))
        self.done = acrobot_terminal(self.s)
        self.borderline |= acrobot_margin(self.s) < 1e-5
        return acrobot_obs(self.s), np.where(self.done, 0.0, -1.0)


class BatchedMountainCar(_Batched):
    obs_dim, act_dim, discrete, cont = 2, 3, True, False

    def __init__(self, n, seed, lane_ids=None, T=200):
        super().__init__(n, seed, lane_ids, T)

    def reset(self):
        self.pos, self.vel = mountaincar_reset(self.seed, self.lane_ids)
        return np.stack([self.pos, self.vel], -1)

    def step(self, actions):
        a = np.asarray(actions, F).reshape(self.n) if self.cont else np.asarray(actions, np.int64)
        self.pos, self.vel, self.done, r = mountaincar_step_f32(self.pos, self.vel, a, self.cont)
        self.borderline |= mountaincar_borderline(self.pos, self.vel, self.cont)
        return np.stack([self.pos, self.vel], -1), r.astype(np.float64)


class BatchedMountainCarContinuous(BatchedMountainCar):
    obs_dim, act_dim, discrete, cont = 2, 1, False, True

    def __init__(self, n, seed, lane_ids=None, T=999):
        super().__init__(n, seed, lane_ids, T)


# ---- controller policies ----------------------------------------------------------------------------------------
def _flat(kind, n_in, n_act, parts):
    out = []
    for name, shape in opol.layout(kind, n_in, n_act):
        a = np.asarray(parts.get(name, np.zeros(shape)), np.float32)
        assert a.shape == tuple(shape), name
        out.append(a.reshape(-1))
    return np.concatenate(out)


def discrete3_controller(n_in, w, gain=200.0, head=50.0, bias=0.01):
    """DiscretePolicy(n_in, 3) parameters that take action 2 where gain * (w . obs) + bias >= 0 and action 0
    elsewhere: two ReLU units per layer carry the positive and the negative part of that sum (the BatchNorms are the
    identity up to 1 / sqrt(1 + 1e-5)), and the head turns their difference into logits +-head * (..) for actions 2 /
    0 against 0 for action 1.  The small bias breaks the tie at w . obs = 0 (a car at rest) towards action 2."""
    H = opol.HIDDEN
    w = np.asarray(w, np.float32)
    l1w, l1b = np.zeros((H, n_in), np.float32), np.zeros(H, np.float32)
    l1w[0], l1w[1] = gain * w, -gain * w
    l1b[0], l1b[1] = bias, -bias
    l2w = np.zeros((H, H), np.float32)
    l2w[0, 0] = l2w[1, 1] = 1.0
    l3w = np.zeros((3, H), np.float32)
    l3w[2, 0], l3w[2, 1] = head, -head
    l3w[0, 0], l3w[0, 1] = -head, head
    ones = lambda n: np.ones(n, np.float32)  # noqa: E731
    return _flat("discrete", n_in, 3, {"bn0.w": ones(n_in), "l1.w": l1w, "l1.b": l1b, "bn1.w": ones(H), "l2.w": l2w,
                                       "bn2.w": ones(H), "l3.w": l3w})


def mountaincar_controller():
    """Push along the velocity (obs element 1); velocities are <= 0.07, so the gain is large."""
    return discrete3_controller(2, [0.0, 1.0], gain=2000.0, head=50.0, bias=0.01)


def acrobot_controller():
    """Torque -sign(thetadot1) (obs element 4)."""
    return discrete3_controller(6, [0, 0, 0, 0, -1.0, 0], gain=20.0, head=50.0, bias=0.001)


def mountaincar_cont_controller(gain=2000.0, bias=0.01, head=2.0):
    """MujocoPolicy(2, 1) parameters with mean = tanh(head * tanh(4 tanh(gain * vel + bias))) ~ 0.96 sign(vel) (inside
    the force clamp) and std = 0.55 (the std head is zero)."""
    H = opol.HIDDEN
    l1w, l1b = np.zeros((H, 2), np.float32), np.zeros(H, np.float32)
    l1w[0, 1], l1b[0] = gain, bias
    l2w = np.zeros((H, H), np.float32)
    l2w[0, 0] = 4.0
    l3w = np.zeros((2, H), np.float32)
    l3w[0, 0] = head
    return _flat("mujoco", 2, 1, {"l1.w": l1w, "l1.b": l1b, "l2.w": l2w, "l3.w": l3w})
