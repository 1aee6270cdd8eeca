"""The branches of the five physics systems (cartpole_step, pendulum_step, acrobot_step, mountaincar_step, wrap_pi), the
seeded cases that drive the rollout kernels through them, and the checker of a recorded launch (pure numpy:
tests/test_physics_branches_ref.py pins everything here on the CPU, tests/test_gpu_physics_branches.py runs the cases).

ROWS     one row per decision of a step function, both signs where it has two.  A row's predicate
         taken(cur, action, nxt) is written from gym's published formulas in f64 on a RECORDED transition (cur and nxt
         are observations); it returns how far past its threshold the decision's own operand lies (> 0: taken), so a
         caller can tell a decision that rounding could move from a firm one.  A terminal row is evaluated on the
         transition out of a lane's last recorded state, whose nxt is the restated step.
census   counts every row over a trajectory: (times taken, lanes that took it).
CASES    linear_cases.Case specs (64 lanes, a controller times a scale, a small sigma so that the lanes differ), each
         aimed at rows the cases of linear_cases.py miss.
simulate the f32 episode loop of linear_ref.run restated with every constant of a branch as a knob (MUTATIONS): with
         no knob turned it is linear_ref.run bit for bit (pinned), with one turned it is a subtly wrong kernel.
check    the comparison of the GPU test on host arrays: raises AssertionError on a launch that is not the restatement's.

Rows that no case reaches are listed in UNREACHABLE with the argument and the largest value a CPU search found, rows
reached too rarely to aim at in SPARSE (DESIGN.md 3.1.5 has the table).  MlpCase carries the same controllers as
deterministic sign-0 lanes of a hand-built DiscretePolicy for the MLP kernels.
"""
import numpy as np

import linear_cases as lc
import linear_ref as lref
import physics_ref as ref
import physics_ref2 as ref2

F = np.float32
PI_F = ref.PI_F
L = lc.L
AC1, AC2 = F(4) * PI_F, F(9) * PI_F            # fl32(4 fl32(pi)), fl32(9 fl32(pi))
MIN_TIMES, MIN_LANES = 8, 4                    # a row counts as taken by a case: >= 8 times in >= 4 lanes

# One-step tolerances of the existing GPU tests, per observation component (tests/test_gpu_linear_policy.py states where
# each comes from); Acrobot outside the pinned box of ACROBOT_ERR: ten times ACROBOT_ERR_WIDE.
PEND_STEP_TOL, PEND_RET_PER_STEP = 5e-6, 4e-3 / 200
CART_STEP_TOL = 2e-6
_e, _w = ref2.ACROBOT_ERR, ref2.ACROBOT_ERR_WIDE
ACRO_STEP_TOL = 10 * np.array([_e[0], _e[0], _e[1], _e[1], _e[2], _e[3]])
ACRO_STEP_TOL_WIDE = 10 * np.array([_w[0], _w[0], _w[1], _w[1], _w[2], _w[3]])
MC_STEP_TOL = 10 * np.array(ref2.MC_ERR)
MCC_STEP_TOL = 10 * np.array(ref2.MCC_ERR[:2])
MCC_RET_PER_STEP = ref2.MCC_ERR[2]
STEP_TOL = {"cartpole": CART_STEP_TOL, "pendulum": PEND_STEP_TOL, "acrobot": ACRO_STEP_TOL, "mountaincar": MC_STEP_TOL,
            "mountaincar_cont": MCC_STEP_TOL}
FORCE_CLAMP = {"pendulum": 2.0, "mountaincar_cont": 1.0}


# ---- the rows ---------------------------------------------------------------------------------------------------
def _pend(cur, a):
    """Pendulum's unclamped new speed and unwrapped new angle from a recorded observation (f64)."""
    o = np.asarray(cur, np.float64)
    th = np.arctan2(o[:, 1], o[:, 0])
    u = np.clip(np.asarray(a, np.float64), -2.0, 2.0)
    raw = o[:, 2] + (15.0 * o[:, 1] + 3.0 * u) * 0.05
    return raw, th + np.clip(raw, -8.0, 8.0) * 0.05


def _acro(cur, a):
    """Acrobot's RK4 step before the wrap and the clamp (f64, gym's literal form)."""
    return ref2._acrobot_rk4(ref2.acrobot_state_from_obs(cur).astype(np.float64), np.asarray(a), np.float64, True)


def _acro_height(obs):
    o = np.asarray(obs, np.float64)
    return -o[:, 0] - (o[:, 0] * o[:, 2] - o[:, 1] * o[:, 3])      # -cos th1 - cos(th1 + th2)


def _mc(cur, a, cont):
    """The MountainCars' unclamped new velocity, and the unclamped new position under the clamped one (f64)."""
    o = np.asarray(cur, np.float64)
    push = np.clip(np.asarray(a, np.float64), -1.0, 1.0) * 0.0015 if cont else (np.asarray(a) - 1) * 0.001
    v = o[:, 1] + push - 0.0025 * np.cos(3.0 * o[:, 0])
    return v, o[:, 0] + np.clip(v, -0.07, 0.07)


def _mc_rows(cont):
    goal = ref2.GOAL_CONT if cont else ref2.GOAL
    rows = [
        ("v_hi", lambda c, a, n: _mc(c, a, cont)[0] - 0.07, (1, F(0.07)), False),
        ("v_lo", lambda c, a, n: -0.07 - _mc(c, a, cont)[0], (1, F(-0.07)), False),
        # the wall: the position clamps to -1.2 and the (leftward) velocity becomes 0
        ("wall", lambda c, a, n: -1.2 - _mc(c, a, cont)[1], (0, F(-1.2)), False),
        ("pos_hi", lambda c, a, n: _mc(c, a, cont)[1] - 0.6, (0, F(0.6)), False),
        ("goal", lambda c, a, n: np.where(np.asarray(n, np.float64)[:, 1] >= 0, np.asarray(n, np.float64)[:, 0] - goal,
                                          -1.0), None, True),
    ]
    if cont:
        rows += [("f_hi", lambda c, a, n: np.asarray(a, np.float64) - 1.0, None, False),
                 ("f_lo", lambda c, a, n: -1.0 - np.asarray(a, np.float64), None, False)]
    return rows


# env -> [(row, excess(cur, action, nxt) -> f64 [n], pinned (component, constant) or None, terminal)]
_ROWS = {
    "cartpole": [
        ("x_hi", lambda c, a, n: np.asarray(n, np.float64)[:, 0] - float(ref.X_THR), None, True),
        ("x_lo", lambda c, a, n: -float(ref.X_THR) - np.asarray(n, np.float64)[:, 0], None, True),
        ("th_hi", lambda c, a, n: np.asarray(n, np.float64)[:, 2] - float(ref.THETA_THR), None, True),
        ("th_lo", lambda c, a, n: -float(ref.THETA_THR) - np.asarray(n, np.float64)[:, 2], None, True),
    ],
    "pendulum": [
        ("u_hi", lambda c, a, n: np.asarray(a, np.float64) - 2.0, None, False),
        ("u_lo", lambda c, a, n: -2.0 - np.asarray(a, np.float64), None, False),
        ("thd_hi", lambda c, a, n: _pend(c, a)[0] - 8.0, (2, F(8)), False),
        ("thd_lo", lambda c, a, n: -8.0 - _pend(c, a)[0], (2, F(-8)), False),
        # wrap_pi of the new angle: past +pi it comes down by 2 pi, below -pi it goes up
        ("wrap_down", lambda c, a, n: _pend(c, a)[1] - np.pi, None, False),
        ("wrap_up", lambda c, a, n: -np.pi - _pend(c, a)[1], None, False),
    ],
    "acrobot": [
        ("th1_down", lambda c, a, n: _acro(c, a)[:, 0] - np.pi, None, False),
        ("th1_up", lambda c, a, n: -np.pi - _acro(c, a)[:, 0], None, False),
        ("th2_down", lambda c, a, n: _acro(c, a)[:, 1] - np.pi, None, False),
        ("th2_up", lambda c, a, n: -np.pi - _acro(c, a)[:, 1], None, False),
        ("thd1_hi", lambda c, a, n: _acro(c, a)[:, 2] - 4 * np.pi, (4, AC1), False),
        ("thd1_lo", lambda c, a, n: -4 * np.pi - _acro(c, a)[:, 2], (4, -AC1), False),
        ("thd2_hi", lambda c, a, n: _acro(c, a)[:, 3] - 9 * np.pi, (5, AC2), False),
        ("thd2_lo", lambda c, a, n: -9 * np.pi - _acro(c, a)[:, 3], (5, -AC2), False),
        # some velocity clamp: the four rows above are rare events of a chaotic system (see SPARSE)
        ("thd_any", lambda c, a, n: np.max(np.abs(_acro(c, a)[:, 2:]) - np.array([4 * np.pi, 9 * np.pi]), axis=1), None,
         False),
        ("goal", lambda c, a, n: _acro_height(n) - 1.0, None, True),
    ],
    "mountaincar": _mc_rows(False),
    "mountaincar_cont": _mc_rows(True) + [
        # the +100 of the finishing step: the goal row's transition, seen in the return
        ("bonus", lambda c, a, n: np.where(np.asarray(n, np.float64)[:, 1] >= 0,
                                          np.asarray(n, np.float64)[:, 0] - ref2.GOAL_CONT, -1.0), None, True),
    ],
}
ROWS = {env: [r[0] for r in rows] for env, rows in _ROWS.items()}


def taken(env, row, cur, action, nxt):
    """Row `row` of env acted on the recorded transitions (cur, action, nxt)."""
    return excess(env, row, cur, action, nxt) > 0


def excess(env, row, cur, action, nxt):
    for name, fn, _, _ in _ROWS[env]:
        if name == row:
            return np.asarray(fn(cur, action, nxt), np.float64)
    raise KeyError((env, row))


# Rows that cannot act through the API: the argument, and what the CPU search found (test_physics_branches_ref.py
# recomputes the figures).
UNREACHABLE = {
    ("pendulum", "cost_wrap"): "wrap_pi in the cost's w sees a theta that the reset and the previous step's wrap_pi "
                               "already hold in [-pi, pi): it is the identity there (both directions), and the "
                               "observation shows theta by its cosine and sine only",
    ("mountaincar", "v_hi"): "the fastest run to the right starts at rest at the left wall (the wall zeroes the velocity) "
                             "and pushes right all the way: v^2 / 2 = 0.0025 / 3 (sin 3.6 + sin 3 p) + 0.001 (p + 1.2) "
                             "peaks at cos 3 p = 0.4 with v = 0.0624; the restated runs and the searched "
                             "controllers give up to 0.06239",
    ("mountaincar_cont", "v_hi"): "the same run under power 0.0015 peaks at cos 3 p = 0.6 with v = 0.0689; the restated "
                                  "run and the searched controllers give 0.06891",
    ("mountaincar", "pos_hi"): "a position >= the goal is only entered with vel > 0, which ends the episode, and from "
                               "below the goal 0.6 needs vel > 0.1 > 0.07; for the same reason the vel >= 0 half of the "
                               "goal test never decides",
    ("mountaincar_cont", "pos_hi"): "as MountainCar-v0 with the goal 0.45: 0.6 needs vel > 0.15",
}
MAX_V_RIGHT = {"mountaincar": 0.0626, "mountaincar_cont": 0.0692}      # bounds on the restated runs and the cases, < 0.07
# Rows that act, but as rare events of a chaotic system: about 16,000 sign(w . obs) controllers were searched on the CPU
# (random w over the six observation elements, T = 500, 16 .. 256 resets each).  Each sign of both clamps is reached, but
# no controller found takes all four 8 times in 4 lanes, not even over four launches.  acro_whirl is the best found: over
# its four launches the four rows together act MIN_TIMES times in MIN_LANES lanes (row thd_any), every occurrence is
# checked bit for bit, no recorded speed may exceed a clamp, and the CPU census of each sign is pinned as it stands.
SPARSE = {("acrobot", r): "a rare event of the whirling mode; counted in thd_any" for r in
          ("thd1_hi", "thd1_lo", "thd2_hi", "thd2_lo")}


# ---- trajectories -----------------------------------------------------------------------------------------------
def weights(case):
    return case.thetas()[0].reshape(L, case.n_act, case.n_in)


def actions_of(case, Wm, obs):
    """The recomputed action of recorded observations obs [n, n_in] under Wm [n, A, I] (discrete: index; else y)."""
    y = lref.dot_ordered(Wm, lref.normalise(obs, case.obs_mean, case.obs_std))
    return lref.first_argmax(y) if case.discrete else y[:, 0]


def lane_actions(case, lanes, obs, nxt=None):
    """The action of lanes `lanes` at recorded observations obs [n, n_in]: the linear policy's recomputed one, or an
    MlpCase's controller rule."""
    if isinstance(case, MlpCase):
        return case.actions(obs, nxt)
    return actions_of(case, weights(case)[lanes], obs)


def step_candidates(env, cur, acts):
    """Next observation of recorded observations cur under acts in the f32 restatement (test_gpu_linear_policy.py's)."""
    if env == "cartpole":
        return ref.cartpole_step_f32(cur, acts)
    if env == "acrobot":
        return ref2.acrobot_obs(ref2.acrobot_step_f32(ref2.acrobot_state_from_obs(cur), acts))
    if env == "pendulum":
        th = np.arctan2(cur[:, 1], cur[:, 0]).astype(F)
        nth, nthd, _ = ref.pendulum_step_f32(th, cur[:, 2], acts)
        return ref.pendulum_obs(nth, nthd)
    p, v, _, _ = ref2.mountaincar_step_f32(cur[:, 0], cur[:, 1], acts, cont=env == "mountaincar_cont")
    return np.stack([p, v], -1)


def transitions(steps, last=False):
    """(lane, t) of the recorded transitions t -> t + 1; last: of every lane's last recorded state instead."""
    if last:
        return np.arange(len(steps), dtype=np.int64), np.asarray(steps, np.int64) - 1
    ll = np.concatenate([np.full(max(int(n) - 1, 0), l) for l, n in enumerate(steps)])
    tt = np.concatenate([np.arange(max(int(n) - 1, 0)) for n in steps])
    return ll.astype(np.int64), tt.astype(np.int64)


def census(case, states, steps, min_excess=0.0):
    """-> {row: (times, lanes)} over a trajectory of case (states [L, T, n_in] with NaN behind each lane's steps).
    Non-terminal rows are counted on the recorded transitions, terminal rows on the transition out of the last state
    of a lane that stopped short of T (its nxt restated).  min_excess > 0 counts only decisions firmer than that."""
    ll, tt = transitions(steps)
    cur, nxt = states[ll, tt], states[ll, tt + 1]
    act = lane_actions(case, ll, cur, nxt)
    early = np.nonzero(np.asarray(steps) < case.T)[0]
    lcur = states[early, np.asarray(steps)[early] - 1]
    lact = lane_actions(case, early, lcur)
    lnxt = step_candidates(case.env, lcur, lact)
    out = {}
    for name, fn, _, terminal in _ROWS[case.env]:
        if terminal:
            hit, lanes = fn(lcur, lact, lnxt) > min_excess, early
        else:
            hit, lanes = fn(cur, act, nxt) > min_excess, ll
        out[name] = (int(hit.sum()), len(np.unique(lanes[hit])))
    return out


def reached(cen, row):
    return cen[row][0] >= MIN_TIMES and cen[row][1] >= MIN_LANES


# ---- the restatement with its constants as knobs ----------------------------------------------------------------
KNOBS = dict(x_thr=ref.X_THR, thd_hi=F(8), thd_lo=F(-8), wrap_down=True, wrap_up=True, ac1=AC1, ac2=AC2,
             mc_hi=F(0.07), mc_lo=F(-0.07), wall_zero=True, cost_clipped=False, bonus=F(100), goal_cont=F(ref2.GOAL_CONT))
# name -> (knobs turned, the case whose check must raise)
MUTATIONS = {
    "cartpole x bound 4.8 (right)": (dict(x_thr=F(4.8)), "cart_x_hi"),
    "cartpole x bound 4.8 (left)": (dict(x_thr=F(4.8)), "cart_x_lo"),
    "pendulum speed clamp only above": (dict(thd_lo=F(-np.inf)), "pend_speed"),
    "pendulum speed clamp only below": (dict(thd_hi=F(np.inf)), "pend_speed"),
    "pendulum speed clamp at +8.5": (dict(thd_hi=F(8.5)), "pend_speed"),
    "pendulum speed clamp at -8.5": (dict(thd_lo=F(-8.5)), "pend_speed"),
    "wrap_pi without the way down": (dict(wrap_down=False), "pend_speed"),
    "wrap_pi without the way up": (dict(wrap_up=False), "pend_speed"),
    "acrobot 4 pi and 9 pi swapped": (dict(ac1=AC2, ac2=AC1), "acro_whirl"),
    "acrobot without clamps": (dict(ac1=F(np.inf), ac2=F(np.inf)), "acro_whirl"),
    "mountaincar speed limit -0.08": (dict(mc_lo=F(-0.08)), "mc_wall"),
    "mountaincar_cont speed limit -0.08": (dict(mc_lo=F(-0.08)), "mcc_wall"),
    "mountaincar wall keeps the velocity": (dict(wall_zero=False), "mc_wall"),
    "mountaincar_cont wall keeps the velocity": (dict(wall_zero=False), "mcc_wall"),
    "mountaincar_cont cost of the clamped force": (dict(cost_clipped=True), "mcc_goal"),
    "mountaincar_cont without the +100": (dict(bonus=F(0)), "mcc_goal"),
    "mountaincar_cont goal 0.5": (dict(goal_cont=F(0.5)), "mcc_goal"),
}


def _wrap_f32(th, k):
    """physics_ref._wrap in f32, each direction on its knob."""
    w = (np.mod((th + PI_F).astype(F), ref.TWO_PI_F) - PI_F).astype(F)
    y = (th + PI_F).astype(F)
    keep = np.zeros(np.shape(th), bool)
    if not k["wrap_down"]:
        keep |= y >= ref.TWO_PI_F
    if not k["wrap_up"]:
        keep |= y < 0
    return np.where(keep, th, w).astype(F)


class _Sim(object):
    """The five systems in f32 with KNOBS: reset() -> obs, step(a) -> (obs, reward f64, done)."""

    def __init__(self, env, seed, ids, knobs):
        self.env, self.k, self.seed, self.ids = env, knobs, seed, np.asarray(ids, np.uint64)

    def obs(self):
        if self.env == "cartpole":
            return self.s.copy()
        if self.env == "pendulum":
            return ref.pendulum_obs(self.th, self.thd)
        if self.env == "acrobot":
            return ref2.acrobot_obs(self.s)
        return np.stack([self.pos, self.vel], -1)

    def reset(self):
        if self.env == "cartpole":
            self.s = ref.cartpole_reset(self.seed, self.ids)
        elif self.env == "pendulum":
            self.th, self.thd = ref.pendulum_reset(self.seed, self.ids)
        elif self.env == "acrobot":
            self.s = ref2.acrobot_reset(self.seed, self.ids)
        else:
            self.pos, self.vel = ref2.mountaincar_reset(self.seed, self.ids)
        return self.obs()

    def step(self, a):
        k, n = self.k, len(self.ids)
        if self.env == "cartpole":
            s = self.s = ref.cartpole_step_f32(self.s, a)
            done = (s[:, 0] < -k["x_thr"]) | (s[:, 0] > k["x_thr"]) | (s[:, 2] < -ref.THETA_THR) | (s[:, 2] > ref.THETA_THR)
            return self.obs(), np.ones(n), done
        if self.env == "pendulum":          # physics_ref._pendulum_step, line for line
            th, thd = self.th, self.thd
            u = np.clip(np.asarray(a, F), F(-2.0), F(2.0))
            w = _wrap_f32(th, k)
            cost = w * w + F(0.1) * thd * thd + F(0.001) * u * u
            raw = thd + (F(15.0) * np.sin(th).astype(F) + F(3.0) * u) * F(0.05)
            self.thd = np.minimum(np.maximum(raw, k["thd_lo"]), k["thd_hi"]).astype(F)
            self.th = _wrap_f32((th + self.thd * F(0.05)).astype(F), k)
            return self.obs(), (-cost).astype(F).astype(np.float64), np.zeros(n, bool)
        if self.env == "acrobot":
            ns = ref2._acrobot_rk4(self.s, a, F, False)
            self.s = np.stack([ref2._wrap1(ns[:, 0], F), ref2._wrap1(ns[:, 1], F), np.clip(ns[:, 2], -k["ac1"], k["ac1"]),
                               np.clip(ns[:, 3], -k["ac2"], k["ac2"])], -1).astype(F)
            done = ref2.acrobot_terminal(self.s)
            return self.obs(), np.where(done, 0.0, -1.0), done
        cont = self.env == "mountaincar_cont"           # physics_ref2._mountaincar_step, line for line
        p, v = self.pos, self.vel
        if cont:
            a = np.asarray(a, F)
            ac = np.clip(a, F(-1.0), F(1.0))
            push = ac * F(0.0015)
        else:
            push = (np.asarray(a) - 1).astype(F) * F(0.001)
        v = (v + push - F(0.0025) * np.cos(F(3.0) * p).astype(F)).astype(F)
        v = np.clip(v, k["mc_lo"], k["mc_hi"]).astype(F)
        p = np.clip((p + v).astype(F), F(-1.2), F(0.6)).astype(F)
        if k["wall_zero"]:
            v = np.where((p == F(-1.2)) & (v < 0), F(0.0), v).astype(F)
        done = (p >= (k["goal_cont"] if cont else F(ref2.GOAL))) & (v >= 0)
        if cont:
            c = ac if k["cost_clipped"] else a
            rew = (np.where(done, k["bonus"], F(0.0)) - F(0.1) * c * c).astype(F)
        else:
            rew = np.full(n, -1.0, F)
        self.pos, self.vel = p, v
        return self.obs(), rew.astype(np.float64), done


def simulate(case, mutation=None, e=0, lane_offset=None):
    """Episode e of every lane of case in the f32 restatement, `mutation` (a dict of KNOBS) applied: -> the host
    arrays of a recorded launch, dict(states [L, T, n_in] NaN where not visited, steps, ret, ent)."""
    k = dict(KNOBS, **(mutation or {}))
    ids = case.ids[:, e] if lane_offset is None else lane_offset + np.arange(L, dtype=np.uint64)
    sim = _Sim(case.env, case.seed, ids, k)
    obs = sim.reset()
    T = case.T
    states = np.full((L, T, case.n_in), np.nan, F)
    alive = np.ones(L, bool)
    steps = np.full(L, T, np.int64)
    ret = np.zeros(L, np.float64)
    for t in range(T):
        if not alive.any():
            break
        states[alive, t] = obs[alive]
        obs, r, done = sim.step(lane_actions(case, np.arange(L), obs))
        ret[alive] += r[alive]
        steps[alive & done] = t + 1
        alive &= ~done
    return dict(states=states, steps=steps, ret=ret, ent=np.zeros(L))


# ---- the cases --------------------------------------------------------------------------------------------------
# CartPole: linear_cases.CART_CTRL balances the pole; obs_mean = (+-3, 0, 0, 0) makes x = +-3 its set point, so the
# cart walks out through the x bound with the pole upright.  Pendulum: y = 5 thd saturates the torque along the spin.
# MountainCars: push along k vel - g (pos + 0.5) (obs_mean = (-0.5, 0)): the car pumps itself up both slopes, hits the
# wall, runs down into the speed limit and never reaches the goal.  Acrobot: torque sign(w . obs) on the odd features.
PEND_SPIN = [[0, 0, 5]]
MC_PUMP = [[10, -50], [0, 0], [-10, 50]]
MCC_PUMP = [[-50, 200]]
_ONE = [1, 1]


ACRO_W = [0.0, -0.302, 0.0, 0.0, 0.559, 0.223]
ACRO_WHIRL = [[-v for v in ACRO_W], [0] * 6, ACRO_W]
MC_T = 300
_SPECS = {
    "cart_x_hi": dict(env="cartpole", seed=7, T=250, scale=1.0, sigma=0.02, theta=lc.CART_CTRL, obs_mean=[3, 0, 0, 0],
                      obs_std=[1, 1, 1, 1]),
    "cart_x_lo": dict(env="cartpole", seed=7, T=250, scale=1.0, sigma=0.02, theta=lc.CART_CTRL, obs_mean=[-3, 0, 0, 0],
                      obs_std=[1, 1, 1, 1]),
    "cart_theta": dict(env="cartpole", seed=201, T=64, scale=1.0, sigma=3.0, theta=lc.CART_CTRL),
    "pend_speed": dict(env="pendulum", seed=7, T=100, scale=1.0, sigma=0.05, theta=PEND_SPIN),
    "acro_whirl": dict(env="acrobot", seed=7, T=500, scale=1.0, sigma=0.02, theta=ACRO_WHIRL),
    "mc_wall": dict(env="mountaincar", seed=7, T=MC_T, scale=1.0, sigma=0.05, theta=MC_PUMP, obs_mean=[-0.5, 0],
                    obs_std=_ONE),
    "mc_goal": dict(env="mountaincar", seed=104, T=160, scale=1.0, sigma=0.02, theta=lc.MC_CTRL),
    "mcc_wall": dict(env="mountaincar_cont", seed=7, T=MC_T, scale=1.0, sigma=0.5, theta=MCC_PUMP, obs_mean=[-0.5, 0],
                     obs_std=_ONE),
    "mcc_goal": dict(env="mountaincar_cont", seed=104, T=160, scale=30.0, sigma=0.6, theta=lc.MCC_CTRL),
}
# the rows a case is aimed at: its own trajectory takes each at least MIN_TIMES times in at least MIN_LANES lanes
AIMS = {
    "cart_x_hi": ("x_hi",), "cart_x_lo": ("x_lo",), "cart_theta": ("th_hi", "th_lo"),
    "pend_speed": ("u_hi", "u_lo", "thd_hi", "thd_lo", "wrap_down", "wrap_up"),
    "acro_whirl": ("th1_down", "th1_up", "th2_down", "th2_up", "thd_any", "goal"),
    "mc_wall": ("v_lo", "wall"), "mc_goal": ("goal",),
    "mcc_wall": ("v_lo", "wall", "f_hi", "f_lo"), "mcc_goal": ("goal", "bonus", "f_hi", "f_lo"),
}
# the recorded launches of a case: lane offsets (lane l of a launch plays stream id offset + l under theta'_l); the
# census of a case is the sum over its launches.  Two at least: fdr_rollout_episodes with K = 2 folds the first two.
OFFSETS = {name: (0, 64) for name in _SPECS}
OFFSETS["acro_whirl"] = (0, 64, 128, 192)
NAMES = tuple(_SPECS)
_CACHE = {}


def case(name, offset=0):
    if (name, offset) not in _CACHE:
        _CACHE[(name, offset)] = (MlpCase(lane_offset=offset, **_MLP_SPECS[name]) if name in _MLP_SPECS else
                                  lc.Case(lane_offset=offset, **_SPECS[name]))
    return _CACHE[(name, offset)]


# ---- the MLP kernels (rollout_kernel, lane form): controller lanes ----------------------------------------------
def bang_controller(n_in, n_act, w, gain, head=50.0, bias=0.01):
    """DiscretePolicy(n_in, n_act) parameters that take the last action where gain (w . x) + bias >= 0 and action 0
    elsewhere: physics_ref2.discrete3_controller, and its two-action sibling (the same two ReLU units; the head gives
    logits +-head (..) to the last action and -+ to action 0)."""
    if n_act == 3:
        return ref2.discrete3_controller(n_in, w, gain=gain, head=head, bias=bias)
    from oracle import policies as opol
    assert n_act == 2
    H = opol.HIDDEN
    w = np.asarray(w, F)
    l1w, l1b = np.zeros((H, n_in), F), np.zeros(H, F)
    l1w[0], l1w[1] = gain * w, -gain * w
    l1b[0], l1b[1] = bias, -bias
    l2w = np.zeros((H, H), F)
    l2w[0, 0] = l2w[1, 1] = 1.0
    l3w = np.zeros((2, H), F)
    l3w[1, 0], l3w[1, 1] = head, -head
    l3w[0, 0], l3w[0, 1] = -head, head
    return ref2._flat("discrete", n_in, 2, {"bn0.w": np.ones(n_in, F), "l1.w": l1w, "l1.b": l1b, "bn1.w": np.ones(H, F),
                                            "l2.w": l2w, "bn2.w": np.ones(H, F), "l3.w": l3w})


class MlpCase(object):
    """64 deterministic sign-0 lanes of one bang_controller (every lane its own reset), in the shape of
    linear_cases.Case.  actions(): the controller's rule on the normalised observation; where gain (w . x) + bias lies
    within AMBIGUOUS gain of zero the forward's rounding decides, and the action is read off the recorded transition
    (the candidate nearest to it), as tests/test_gpu_physics_envs2.py reads every action."""
    AMBIGUOUS = 1e-4

    def __init__(self, env, seed, T, w, gain, obs_mean=None, obs_std=None, lane_offset=0, bias=0.01):
        self.env, self.seed, self.T, self.w, self.gain, self.bias = env, seed, T, np.asarray(w, np.float64), gain, bias
        self.kind, self.n_in, self.n_act, self.discrete = lref.ENVS[env]
        assert self.discrete
        self.obs_mean = None if obs_mean is None else np.asarray(obs_mean, F)
        self.obs_std = None if obs_std is None else np.asarray(obs_std, F)
        self.obs_chance, self.lane_offset, self.K = None, lane_offset, 1
        self.ids = (lane_offset + np.arange(L, dtype=np.uint64))[:, None]

    def theta(self):
        return bang_controller(self.n_in, self.n_act, self.w, self.gain, bias=self.bias)

    def actions(self, obs, nxt=None):
        x = lref.normalise(obs, self.obs_mean, self.obs_std).astype(np.float64)
        s = self.gain * (x @ self.w) + self.bias
        act = np.where(s >= 0, self.n_act - 1, 0)
        unsure = np.abs(s) < self.AMBIGUOUS * self.gain
        if nxt is not None and unsure.any():
            both = np.stack([step_candidates(self.env, obs[unsure], np.full(int(unsure.sum()), a))
                             for a in (0, self.n_act - 1)])
            err = np.abs(both.astype(np.float64) - np.asarray(nxt)[unsure][None]).max(-1)
            act[unsure] = np.where(err[1] <= err[0], self.n_act - 1, 0)
        return act


# The MLP suite's own cases (cart_long and the three case_long of test_gpu_physics_envs{,2}.py) miss the CartPole x exits
# on a named side and MountainCar's -0.07; these lanes carry the controllers of cart_x_hi / cart_x_lo / mc_wall.
_MLP_SPECS = {
    "mlp_cart_x_hi": dict(env="cartpole", seed=7, T=250, w=[0.3, 1.0, 5.0, 1.5], gain=200.0, obs_mean=[3, 0, 0, 0],
                          obs_std=[1, 1, 1, 1]),
    "mlp_cart_x_lo": dict(env="cartpole", seed=7, T=250, w=[0.3, 1.0, 5.0, 1.5], gain=200.0, obs_mean=[-3, 0, 0, 0],
                          obs_std=[1, 1, 1, 1]),
    "mlp_mc_wall": dict(env="mountaincar", seed=7, T=MC_T, w=[-0.2, 1.0], gain=1000.0, obs_mean=[-0.5, 0], obs_std=_ONE),
}
MLP_NAMES = tuple(_MLP_SPECS)
AIMS.update({"mlp_cart_x_hi": ("x_hi",), "mlp_cart_x_lo": ("x_lo",), "mlp_mc_wall": ("v_lo", "wall")})
OFFSETS.update({name: (0,) for name in _MLP_SPECS})


def add_census(total, cen):
    for row, (times, lanes) in cen.items():
        t, l = total.get(row, (0, 0))
        total[row] = (t + times, l + lanes)
    return total


# ---- the checker ------------------------------------------------------------------------------------------------
def terminal_recorded(env, obs):
    """Recorded observations that the env's termination test ends an episode on: the kernel tests the f32 values it
    records (CartPole, the MountainCars: exact here); Acrobot's height comes from the angles, here from their
    recorded cosines and sines: above 1 by more than 1e-5, the suite's borderline margin."""
    if env == "cartpole":
        return ref.cartpole_failed(obs)
    if env == "acrobot":
        return _acro_height(obs) > 1.0 + 1e-5
    if env == "pendulum":
        return np.zeros(len(obs), bool)
    return ref2.mountaincar_done(obs[:, 0], obs[:, 1], cont=env == "mountaincar_cont")


# the values a recorded observation component can take: the clamps, exact in f32
RANGES = {"pendulum": {2: F(8)}, "acrobot": {4: AC1, 5: AC2}, "mountaincar": {1: F(0.07)}, "mountaincar_cont": {1: F(0.07)}}


def check(c, got, aims=(), count=True):
    """One recorded launch of case c against the restatement, along the launch's own trajectory.  got: host arrays
    states [L, T, n_in] (NaN where nothing was written), steps [L], ret [L] f64, ent [L].  Raises AssertionError;
    -> a report (census, the largest deviations) for the caller to print."""
    env, T = c.env, c.T
    S, steps, ret = np.asarray(got["states"]), np.asarray(got["steps"]).astype(np.int64), np.asarray(got["ret"])
    Wm = None if isinstance(c, MlpCase) else weights(c)
    rep = {}
    assert S.shape == (L, T, c.n_in) and S.dtype == F
    assert steps.min() >= 1 and steps.max() <= T
    # nothing is written after a lane's last step, and everything before it
    for l, n in enumerate(steps):
        assert np.all(np.isfinite(S[l, :n])) and np.all(np.isnan(S[l, n:])), "lane %d wrote after its last step" % l
    # no recorded state is terminal, and every one lies inside the clamps
    rl = np.concatenate([np.full(int(n), l) for l, n in enumerate(steps)])
    rt = np.concatenate([np.arange(int(n)) for n in steps])
    rec = S[rl, rt]
    term = terminal_recorded(env, rec)
    assert not term.any(), "%d recorded states are terminal: lane %d went on from step %d" % (
        term.sum(), rl[term][0], rt[term][0])
    for comp, bound in RANGES.get(env, {}).items():
        assert np.all(np.abs(rec[:, comp]) <= bound), "component %d leaves +-%r" % (comp, bound)
    if env in ("mountaincar", "mountaincar_cont"):
        assert np.all(rec[:, 0] >= F(-1.2)) and np.all(rec[:, 0] <= F(0.6))
    # every transition: the restatement under the recomputed action, and under no other distinct candidate
    ll, tt = transitions(steps)
    cur, nxt = S[ll, tt], S[ll, tt + 1]
    ar = np.arange(len(ll))
    act = lane_actions(c, ll, cur, nxt)
    tol = np.broadcast_to(np.asarray(STEP_TOL[env], np.float64), (len(ll), c.n_in))
    inbox = np.ones(len(ll), bool)
    if env == "acrobot":        # no exclusion: outside the pinned box of ACROBOT_ERR the wide tolerance
        st = ref2.acrobot_state_from_obs(cur)
        inbox = (np.abs(st[:, 2]) <= ref2.ACROBOT_BOX[0]) & (np.abs(st[:, 3]) <= ref2.ACROBOT_BOX[1])
        tol = np.where(inbox[:, None], ACRO_STEP_TOL, ACRO_STEP_TOL_WIDE)
        rep["outside_box"] = int((~inbox).sum())
    ok = np.ones(len(ll), bool)
    if c.discrete:
        cand = np.stack([step_candidates(env, cur, np.full(len(ll), a)) for a in range(c.n_act)])
        err = np.abs(cand.astype(np.float64) - nxt[None])
        m = np.all(err <= tol[None], axis=-1)                         # [A, n]
        chosen = err[act, ar]
        rep["max_err"] = chosen[inbox].max(0) if inbox.any() else None
        rep["max_err_outside_box"] = chosen[~inbox].max(0) if (~inbox).any() else None
        assert np.all(m[act, ar]), "transitions off the recomputed action: %d (first: lane %d step %d, error %s)" % (
            (~m[act, ar]).sum(), ll[~m[act, ar]][0], tt[~m[act, ar]][0], chosen[~m[act, ar]][0])
        # another action's candidate matches only where it is the same state; under the wide tolerance only where it
        # lies within twice that tolerance of the chosen one (farther apart, one recorded state cannot match both)
        same = np.all(cand == cand[act, ar][None], axis=-1)
        assert np.all((m == same)[:, inbox]), "transitions that also match another action's distinct next state"
        close = np.all(np.abs(cand.astype(np.float64) - cand[act, ar][None]) <= 2 * tol[None], axis=-1)
        assert not np.any((m & ~close)[:, ~inbox])
        if env != "mountaincar":
            assert (same.sum(0) == 1).all()
    else:
        ok = np.abs(np.abs(act) - FORCE_CLAMP[env]) >= 1e-4            # at the clamp the restated force may differ
        err = np.abs(step_candidates(env, cur, act).astype(np.float64) - nxt)
        rep["max_err"], rep["checked"] = err[ok].max(0), (int(ok.sum()), len(ll))
        assert ok.mean() > 0.9, "more than 10 % of the steps lie within 1e-4 of the force clamp"
        bad = ok & ~np.all(err <= tol, axis=-1)
        assert not bad.any(), "transitions off the restatement: %d (first: lane %d step %d, error %s)" % (
            bad.sum(), ll[bad][0], tt[bad][0], err[bad][0])
    # where a clamp or the wall acts, the clamped component is the constant, bit for bit.  "Acts": the decision's
    # operand (f64, from the recorded state) lies past its threshold by more than the component's one-step tolerance,
    # so that no rounding of the kernel's own operand can land it on the other side.
    rep["pinned"] = {}
    wall = excess(env, "wall", cur, act, nxt) if "wall" in ROWS[env] else None
    for name, fn, pinned, terminal in _ROWS[env]:
        if pinned is None:
            continue
        comp, const = pinned
        ex = fn(cur, act, nxt)
        firm = ok & (ex > tol[:, comp])
        if name in ("v_lo", "v_hi") and wall is not None:              # the wall zeroes a clamped leftward velocity
            firm &= wall < -tol[:, 0]
        rep["pinned"][name] = int(firm.sum())
        v = np.ascontiguousarray(nxt[firm, comp])
        assert np.all(v.view(np.uint32) == np.asarray(const, F).view(np.uint32)), \
            "%s acted and left %r, not %r" % (name, v[v != const][:3], const)
        if name == "wall":
            assert np.all(nxt[firm, 1] == 0), "the wall left a velocity %r" % nxt[firm, 1][nxt[firm, 1] != 0][:3]
    # a lane that ended early: the recomputed action's next state is terminal (or borderline, at most 2 lanes)
    early = np.nonzero(steps < T)[0]
    if len(early):
        lcur = S[early, steps[early] - 1]
        lact = lane_actions(c, early, lcur)
        nx = step_candidates(env, lcur, lact)
        if env == "cartpole":
            near, termc = ref.cartpole_margin(nx) < 1e-5, ref.cartpole_failed(nx)
        elif env == "acrobot":
            st = ref2.acrobot_state_from_obs(nx)
            near, termc = ref2.acrobot_margin(st) < 1e-5, ref2.acrobot_terminal(st)
        else:
            assert env != "pendulum", "Pendulum never ends early"
            cont = env == "mountaincar_cont"
            near = ref2.mountaincar_borderline(nx[:, 0], nx[:, 1], cont=cont)
            termc = ref2.mountaincar_done(nx[:, 0], nx[:, 1], cont=cont)
        assert near.sum() <= 2
        assert np.all(termc | near), "lane %d stopped at %d short of its termination" % (
            early[~(termc | near)][0], steps[early[~(termc | near)][0]])
        for side, sgn in (("x_hi", 1.0), ("x_lo", -1.0)):
            if side in aims:     # the x test ends every one of them, on this side, the pole upright
                x, th = nx[:, 0].astype(np.float64), nx[:, 2].astype(np.float64)
                rep["exit_theta"] = float(np.abs(th).max())
                assert np.all(sgn * x > float(ref.X_THR)) and np.all(np.abs(th) < 0.5 * float(ref.THETA_THR)), \
                    "a lane of %s left otherwise: x %s, theta %s" % (side, x, th)
    # the census of this trajectory
    rep["census"] = census(c, S, steps)
    rep["steps"] = (int(steps.min()), int(steps.max()))
    # returns along the recorded trajectory
    if isinstance(c, MlpCase):      # (a softmax policy: the entropy of a saturated bang-bang head is tiny, not zero)
        assert np.all(np.isfinite(got["ent"])) and np.all(np.asarray(got["ent"]) >= 0.0)
    else:
        assert np.all(np.asarray(got["ent"]) == 0.0)
    if env == "cartpole":
        np.testing.assert_array_equal(ret, steps.astype(np.float64))
    elif env == "mountaincar":
        np.testing.assert_array_equal(ret, -steps.astype(np.float64))
    elif env == "acrobot":
        np.testing.assert_array_equal(ret, np.where(steps < T, -(steps - 1.0), -float(T)))
    else:
        worst = 0.0
        for l, n in enumerate(steps):
            obs = S[l, :n]
            a = actions_of(c, np.broadcast_to(Wm[l], (n, c.n_act, c.n_in)), obs)
            if env == "pendulum":
                th = np.arctan2(obs[:, 1], obs[:, 0]).astype(F)
                rew = ref.pendulum_step_f32(th, obs[:, 2], a)[2].astype(np.float64)
                tol_r = T * PEND_RET_PER_STEP
            else:
                rew = (-(F(0.1) * a * a)).astype(F).astype(np.float64)
                # the +100 belongs to a last step that reaches the goal (at step T itself too)
                p, v, dn, _ = ref2.mountaincar_step_f32(obs[-1:, 0], obs[-1:, 1], a[-1:], cont=True)
                if ref2.mountaincar_borderline(p, v, cont=True)[0]:
                    continue
                assert dn[0] or n == T
                if dn[0]:
                    rew[-1] = float(F(100.0) - F(0.1) * a[-1] * a[-1])
                tol_r = T * MCC_RET_PER_STEP
            worst = max(worst, abs(ret[l] - rew.sum()))
            assert abs(ret[l] - rew.sum()) <= tol_r, "lane %d: ret %.6f, restated %.6f" % (l, ret[l], rew.sum())
        rep["max_ret_err"], rep["ret_tol"] = worst, tol_r
    if count:
        assert_reached(rep["census"], aims)
    return rep


def assert_reached(cen, aims):
    for row in aims:
        assert reached(cen, row), "row %s is taken %d times in %d lanes" % ((row,) + cen[row])


def check_case(name, launches, mutation=None):
    """Every recorded launch of case `name` (launches: offset -> host arrays; None: the restatement's, under
    `mutation`), and the census summed over them against the case's aims.  -> (reports, census)."""
    total, reports = {}, {}
    for off in OFFSETS[name]:
        c = case(name, off)
        got = simulate(c, mutation) if launches is None else launches[off]
        reports[off] = check(c, got, AIMS[name], count=False)
        add_census(total, reports[off]["census"])
    assert_reached(total, AIMS[name])
    return reports, total
