"""GPU: Acrobot-v1, MountainCar-v0 and MountainCarContinuous-v0 inside the one-lane rollout kernel (FDR_ENV_ACROBOT /
FDR_ENV_MOUNTAINCAR / FDR_ENV_MOUNTAINCAR_CONT).

Parity is against tests/physics_ref2.py, the numpy restatement of gym's published classic_control formulas (its own
f32 error is pinned in tests/test_physics_ref2.py), driven by the project's oracle (oracle.agent.evaluate_lanes,
oracle.policies.lanes_forward, oracle.rng).  One-step tolerances are 10 x the CPU-pinned f32-vs-f64 error of the
restatement, the ratio the CartPole / Pendulum tests use.

A random-init policy essentially never finishes these tasks, so the launches carry CONTROLLER lanes: deterministic
sign-0 lanes whose base vector is a hand-built bang-bang controller (physics_ref2.*_controller; every lane has its own
base row, base_stride = P).  They reach the goal closed-loop on the GPU and so exercise the success terminations.

Acrobot is chaotic: it is checked transition by transition along the GPU's own recorded trajectory, never as whole
episodes.  MountainCar-v0 is not, and its whole episodes are compared with evaluate_lanes.

Seeds (verified on the CPU restatement with the helpers below): SEED_LONG -- the 61-lane cases: no MountainCar lane
borderline, 0.004 % of Acrobot's 27,112 transitions start outside the pinned box (the controller lanes' last swings);
SEED_SHORT / SEED_X* -- no borderline lane.
"""
import re

import numpy as np
import pytest
import torch

import physics_ref2 as ref
from oracle import agent as oagent
from oracle import noise as onoise
from oracle import policies as opol
from oracle import rng as crng

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SIGMA = 0.02
SEED_LONG, SEED_SHORT = 31, 41
SEED_XENV, SEED_XACT, SEED_XNORM, SEED_XSTAT = 51, 55, 53, 58

ENVS = {
    # name: policy kind, n_in, n_act, P, time limit, envs class, batched restatement, controller
    "acrobot": ("discrete", 6, 3, 5071, 500, "AcrobotEnv", ref.BatchedAcrobot, ref.acrobot_controller),
    "mountaincar": ("discrete", 2, 3, 4807, 200, "MountainCarEnv", ref.BatchedMountainCar, ref.mountaincar_controller),
    "mountaincar_cont": ("mujoco", 2, 1, 4482, 999, "MountainCarContinuousEnv", ref.BatchedMountainCarContinuous,
                         ref.mountaincar_cont_controller),
}


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def _env(name, T=None):
    import envs
    cls = getattr(envs, ENVS[name][5])
    return cls() if T is None else cls(T)


# ---- cases (pure numpy: also used to verify the seeds on the CPU) -----------------------------------------------
_CACHE = {}


def policy_and_table(name):
    kind, n_in, n_act, P = ENVS[name][:4]
    if name not in _CACHE:
        theta = opol.TorchPolicy(kind, n_in, n_act, seed=124).get_flat()
        assert theta.size == P
        _CACHE[name] = (theta, onoise.NoiseTable(1 << 20, theta.size, 124))
    return _CACHE[name]


def lanes_mixed(tab, n_pairs, n_ctrl, n_pert, idx_seed):
    """n_pairs sampled +-pairs of the random-init theta, n_ctrl deterministic sign-0 controller lanes, n_pert
    deterministic perturbed lanes of theta.  -> idx, sign, det, ctrl (bool: the lane's base is the controller)."""
    rs = np.random.RandomState(idx_seed)
    pidx = rs.randint(0, tab.max_idx, size=n_pairs).astype(np.int64)
    didx = rs.randint(0, tab.max_idx, size=n_pert).astype(np.int64)
    idx = np.concatenate([np.repeat(pidx, 2), np.zeros(n_ctrl, np.int64), didx])
    sign = np.concatenate([np.tile(np.array([1, -1], np.int8), n_pairs), np.zeros(n_ctrl, np.int8),
                           np.where(np.arange(n_pert) % 2 == 0, 1, -1).astype(np.int8)])
    det = np.concatenate([np.zeros(2 * n_pairs, np.int8), np.ones(n_ctrl + n_pert, np.int8)])
    ctrl = np.concatenate([np.zeros(2 * n_pairs, bool), np.ones(n_ctrl, bool), np.zeros(n_pert, bool)])
    return idx, sign, det, ctrl


def case_long(name):
    """The 61-lane launch of tests 2 and 3: 24 sampled +-pairs, 8 controller lanes, 5 deterministic perturbed."""
    return lanes_mixed(policy_and_table(name)[1], 24, 8, 5, idx_seed=5)


def case_short(name, L=64, n_ctrl=0, idx_seed=6):
    return lanes_mixed(policy_and_table(name)[1], (L - n_ctrl) // 2, n_ctrl, 0, idx_seed=idx_seed)


def lane_thetas(name, idx, sign, ctrl):
    """theta' of every lane [L, P]."""
    theta, tab = policy_and_table(name)
    out = onoise.perturb(theta, tab.table, idx, sign, SIGMA)
    out[ctrl] = ENVS[name][7]()
    return out


def oracle_episodes(name, idx, sign, det, ctrl, seed, T=None, lane_ids=None, env_seed=None, obs_mean=None,
                    obs_std=None, obs_chance=None):
    """evaluate_lanes on the batched restatement (the random-init lanes and the controller lanes as two calls, each
    lane under its global id), plus per lane the borderline flag, defined as the CartPole test's: a visited state
    within 1e-5 of the termination test's boundary, or at some step a sampled lane's u tot within 2e-5 (twice the
    engine's 1e-5 forward tolerance) of a partial sum of the probabilities / a deterministic lane's two largest
    probabilities within 2e-5 of each other.  -> dict(ret, ent, steps, norm2, states, borderline[, stats, max_speed])."""
    kind, n_in, n_act, P, T0, _, Batched, ctrl_fn = ENVS[name]
    T = T0 if T is None else T
    theta, tab = policy_and_table(name)
    L = len(idx)
    lanes = np.arange(L, dtype=np.uint64) if lane_ids is None else np.asarray(lane_ids, np.uint64)
    res = dict(ret=np.zeros(L), ent=np.zeros(L), steps=np.zeros(L, np.int32), norm2=np.zeros(L),
               states=np.zeros((L, T, n_in), np.float32), borderline=np.zeros(L, bool), stats=[None] * L,
               max_speed=np.zeros((L, 2)))
    for sel, th in ((~ctrl, theta), (ctrl, ctrl_fn())):
        if not sel.any():
            continue
        env = Batched(int(sel.sum()), seed if env_seed is None else env_seed, lanes[sel], T)
        out = oagent.evaluate_lanes(kind, n_in, n_act, th, tab.table, idx[sel], sign[sel], SIGMA, env, seed,
                                    deterministic=det[sel].astype(bool), jiggle=False, record_states=True,
                                    lane_ids=lanes[sel], obs_mean=obs_mean, obs_std=obs_std, obs_chance=obs_chance)
        for k, v in zip(("ret", "ent", "steps", "norm2"), out[:4]):
            res[k][sel] = v
        res["states"][sel] = out[-1]
        res["borderline"][sel] = env.borderline
        if obs_chance is not None:
            for l, s in zip(np.nonzero(sel)[0], out[4]):
                res["stats"][l] = s
        if name == "acrobot":
            res["max_speed"][sel] = env.max_speed
    if kind == "discrete":
        thetas = lane_thetas(name, idx, sign, ctrl)
        steps, states = res["steps"], res["states"]
        for t in range(int(steps.max())):
            alive = steps > t
            x = states[alive, t]
            if obs_mean is not None:
                x = np.clip((x - obs_mean) / obs_std, -10, 10).astype(np.float32)
            p = opol.lanes_forward(kind, n_in, n_act, thetas[alive], x)
            u = crng.uniform(seed, lanes[alive], t, 0)
            c = np.cumsum(p, axis=-1, dtype=np.float32)
            target = (u * c[:, -1]).astype(np.float32)
            near = (np.abs(target[:, None] - c[:, :-1]) < 2e-5).any(axis=-1)
            top = np.sort(p, axis=-1)
            tie = (top[:, -1] - top[:, -2]) < 2e-5
            res["borderline"][np.nonzero(alive)[0]] |= np.where(det[alive] == 1, tie, near)
    return res


# ---- GPU launches -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    from fdr import engine
    return engine


def _launch(eng, name, idx, sign, det, ctrl, seed, T=None, lane_offset=0, record=True, **kw):
    kind, n_in, n_act, P = ENVS[name][:4]
    theta, tab = policy_and_table(name)
    env = _env(name, T)
    L = len(idx)
    spec = eng.PolicySpec(kind, n_in, n_act, P)
    if ("table", name) not in _CACHE:
        _CACHE[("table", name)] = _dev(tab.table)
    base = np.tile(theta, (L, 1))
    base[ctrl] = ENVS[name][7]()
    lanes = eng.lanes_desc(_dev(base), P, _CACHE[("table", name)], _dev(idx), _dev(sign), SIGMA, _dev(det),
                           lane_offset=lane_offset)
    states = None
    if record:
        states = torch.full((L, env.episode_len, n_in), float("nan"), dtype=torch.float32, device=DEV)
    res = eng.rollout(spec, env, lanes, L, seed, jiggle=False, states=states, **kw)
    torch.cuda.synchronize()
    return dict(ret=res.reward.cpu().numpy(), ent=res.entropy.cpu().numpy(), steps=res.timesteps.cpu().numpy(),
                norm2=res.norm2.cpu().numpy(), states=None if states is None else states.cpu().numpy(), res=res)


_LONG = {}


@pytest.fixture
def long_case(eng, request):
    """The 61-lane launch of an env (one per module run, shared by tests 2 to 4)."""
    name = request.param
    if name not in _LONG:
        case = case_long(name)
        _LONG[name] = (case, _launch(eng, name, *case, SEED_LONG))
    return (name,) + _LONG[name]


def _transitions(steps):
    """(lane, t) of every recorded transition states[l, t] -> states[l, t + 1], t + 1 < steps[l]."""
    ll = [np.full(max(int(n) - 1, 0), l) for l, n in enumerate(steps)]
    tt = [np.arange(max(int(n) - 1, 0)) for n in steps]
    return np.concatenate(ll), np.concatenate(tt)


def _continuous_actions(name, g, idx, sign, det, ctrl, seed, lane_offset=0):
    """MountainCarContinuous: the action of every recorded step [L, T], recomputed from the recorded observations
    with the oracle's forward and the counter stream's normals (as the Pendulum test does)."""
    kind, n_in, n_act, P, T = ENVS[name][:5]
    thetas = lane_thetas(name, idx, sign, ctrl)
    S = g["states"]
    act = np.full(S.shape[:2], np.nan, np.float32)
    for l, n in enumerate(g["steps"]):
        n = int(n)
        mean, std = opol.lanes_forward(kind, n_in, n_act, np.broadcast_to(thetas[l], (n, P)), S[l, :n])
        a = mean[:, 0]
        if not det[l]:
            z = crng.normal(seed, np.uint64(lane_offset + l), np.arange(n, dtype=np.uint64), 0)
            a = (mean[:, 0] + std[:, 0] * z).astype(np.float32)
        act[l, :n] = a
    return act


# ---- 1. resets --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lane_offset", [0, 1000])
@pytest.mark.parametrize("name", sorted(ENVS))
def test_resets(eng, name, lane_offset):
    case = case_short(name)
    got = _launch(eng, name, *case, SEED_SHORT, T=4, lane_offset=lane_offset)["states"][:, 0, :]
    ids = lane_offset + np.arange(64)
    if name == "acrobot":
        want = ref.acrobot_reset(SEED_SHORT, ids)
        np.testing.assert_array_equal(got[:, 4:].view(np.uint32), want[:, 2:].view(np.uint32))
        # (cos, sin) are the accurate f32 functions of the bit-exact restated angles
        w64 = want.astype(np.float64)
        for col, f, th in ((0, np.cos, 0), (1, np.sin, 0), (2, np.cos, 1), (3, np.sin, 1)):
            np.testing.assert_allclose(got[:, col], f(w64[:, th]), rtol=0, atol=2.0 ** -23)
        assert len(np.unique(want[:, 0])) == 64
    else:
        pos, vel = ref.mountaincar_reset(SEED_SHORT, ids)
        np.testing.assert_array_equal(got.view(np.uint32), np.stack([pos, vel], -1).view(np.uint32))
        assert len(np.unique(pos)) == 64          # every lane its own state


# ---- 2. one-step consistency ------------------------------------------------------------------------------------
@pytest.mark.parametrize("long_case", ["acrobot"], indirect=True)
def test_acrobot_one_step_consistency(long_case):
    """Every recorded transition whose pre-state lies in the pinned box (|thd1| <= 6, |thd2| <= 10) matches the f32
    restatement under exactly one torque, each observation component within 10 x the pinned f32 error of the state
    component it shows: 7e-6 (cos / sin th1), 8e-6 (cos / sin th2), 3e-5 (thd1), 5e-5 (thd2).  The next states of two
    torques differ by >= 0.08 in thd2 (0.19 on these states).  Measured GPU maximum over the 27,111 checked transitions
    (printed): 2.4e-7 on every cos / sin, 4.8e-7 on thd1, 9.5e-7 on thd2."""
    name, (idx, sign, det, ctrl), g = long_case
    S, steps = g["states"], g["steps"]
    assert len(steps) == 61
    ll, tt = _transitions(steps)
    cur, nxt = ref.acrobot_state_from_obs(S[ll, tt]), S[ll, tt + 1]
    assert np.all(np.isfinite(S[ll, tt])) and np.all(np.isfinite(nxt))
    inbox = (np.abs(cur[:, 2]) <= ref.ACROBOT_BOX[0]) & (np.abs(cur[:, 3]) <= ref.ACROBOT_BOX[1])
    print("acrobot: %d transitions, %d (%.2f %%) start outside the pinned box"
          % (len(ll), int((~inbox).sum()), 100.0 * (~inbox).mean()))
    assert len(ll) > 20000 and (~inbox).mean() <= 0.05
    e = ref.ACROBOT_ERR
    tol = 10 * np.array([e[0], e[0], e[1], e[1], e[2], e[3]])
    cand = np.stack([ref.acrobot_obs(ref.acrobot_step_f32(cur, np.full(len(ll), a))) for a in range(3)])
    sep = np.abs(cand[[0, 1]] - cand[[1, 2]])[..., 5].min()
    assert sep >= 0.08, sep
    err = np.abs(cand - nxt[None])                              # [3, n, 6]
    m = np.all(err <= tol, axis=-1)
    closest = err[(err / tol).max(axis=-1).argmin(axis=0), np.arange(len(ll))]      # [n, 6]: the nearest candidate's
    print("acrobot one-step: %d transitions checked, max |gpu - restated| per component %s (tolerance %s)"
          % (int(inbox.sum()), closest[inbox].max(axis=0), tol))
    assert np.all(m.sum(axis=0)[inbox] == 1), \
        "transitions matching no / several torques: %d" % int((m.sum(axis=0)[inbox] != 1).sum())
    # the controller lanes apply torque -sign(thd1): action 0 where thd1 is clearly positive, 2 where negative
    act = m.argmax(axis=0)
    c = ctrl[ll] & inbox & (np.abs(cur[:, 2]) > 1e-2)
    assert c.sum() > 300
    np.testing.assert_array_equal(act[c], np.where(cur[c, 2] > 0, 0, 2))


@pytest.mark.parametrize("long_case", ["mountaincar"], indirect=True)
def test_mountaincar_one_step_consistency(long_case):
    """Every recorded transition matches the f32 restatement under exactly one action, within 10 x the pinned f32
    error: 7e-7 in position, 7e-8 in velocity.  Two actions are 0.001 apart in velocity -- except where a clamp (the
    speed limit, the left wall) makes their next states the same state: such coinciding candidates count as one (3 of
    the 11,500 transitions).  Measured GPU maximum (printed): position 0 (bitwise), velocity 1.9e-9."""
    name, (idx, sign, det, ctrl), g = long_case
    S, steps = g["states"], g["steps"]
    ll, tt = _transitions(steps)
    cur, nxt = S[ll, tt], S[ll, tt + 1]
    assert len(ll) > 10000 and np.all(np.isfinite(cur)) and np.all(np.isfinite(nxt))
    tol = 10 * np.array(ref.MC_ERR)
    cand = np.stack([np.stack(ref.mountaincar_step_f32(cur[:, 0], cur[:, 1], np.full(len(ll), a))[:2], -1)
                     for a in range(3)])
    err = np.abs(cand - nxt[None])
    m = np.all(err <= tol, axis=-1)
    closest = err[(err / tol).max(axis=-1).argmin(axis=0), np.arange(len(ll))]
    print("mountaincar one-step: %d transitions, max |gpu - restated| pos %.3g vel %.3g"
          % (len(ll), closest[:, 0].max(), closest[:, 1].max()))
    assert np.all(m.any(axis=0)), "transitions matching no action: %d" % int((~m.any(axis=0)).sum())
    first = m.argmax(axis=0)
    same = np.all(cand == cand[first, np.arange(len(ll))][None], axis=-1)       # candidates equal to the matched one
    assert np.all(m == same), "transitions matching two distinct candidates: %d" % int((m != same).any(axis=0).sum())
    print("mountaincar one-step: %d transitions with coinciding candidates" % int((same.sum(axis=0) > 1).sum()))
    assert (same.sum(axis=0) > 1).mean() < 0.02
    # the controller pushes along its velocity
    c = ctrl[ll] & (np.abs(cur[:, 1]) > 1e-4) & (same.sum(axis=0) == 1)
    assert c.sum() > 500
    np.testing.assert_array_equal(first[c], np.where(cur[c, 1] > 0, 2, 0))


@pytest.mark.parametrize("long_case", ["mountaincar_cont"], indirect=True)
def test_mountaincar_cont_one_step_consistency(long_case):
    """Every recorded transition matches the f32 restatement under the action recomputed from the oracle's forward
    and the counter stream, within 10 x the pinned f32 error: 7e-7 in position, 8e-8 in velocity.  Steps with
    ||a| - 1| < 1e-4 (at the force clamp) are left out; more than 90 % of all steps are checked (53,609 of 53,614).
    Measured GPU maximum (printed): position 6.0e-8, velocity 3.7e-9."""
    name, (idx, sign, det, ctrl), g = long_case
    S, steps = g["states"], g["steps"]
    act = _continuous_actions(name, g, idx, sign, det, ctrl, SEED_LONG)
    ll, tt = _transitions(steps)
    cur, nxt, a = S[ll, tt], S[ll, tt + 1], act[ll, tt]
    assert np.all(np.isfinite(cur)) and np.all(np.isfinite(nxt)) and np.all(np.isfinite(a))
    ok = np.abs(np.abs(a) - 1.0) >= 1e-4
    p, v, _, _ = ref.mountaincar_step_f32(cur[:, 0], cur[:, 1], a, cont=True)
    err = np.abs(np.stack([p, v], -1) - nxt)
    print("mountaincar_cont one-step: %d of %d transitions checked, max |gpu - restated| pos %.3g vel %.3g"
          % (int(ok.sum()), len(ll), err[ok, 0].max(), err[ok, 1].max()))
    assert ok.sum() > 0.9 * len(ll) and len(ll) > 40000
    tol = 10 * np.array(ref.MCC_ERR[:2])
    assert np.all(err[ok] <= tol), "transitions off the restatement: %d" % int((err[ok] > tol).any(axis=-1).sum())
    # sampled actions do leave the clamp: the unclipped action is what the cost sees
    assert (np.abs(a) > 1.0).mean() > 0.05


# ---- 3. termination and return ----------------------------------------------------------------------------------
def _termination(name, g, ctrl, det, T, terminal, candidates, margin_small):
    """Controller lanes end before T, random-init sampled lanes run to T; no recorded state is terminal, nothing is
    written after the last step, and a lane that ended early has a terminal candidate next state."""
    S, steps = g["states"], g["steps"]
    assert steps.min() >= 1 and steps.max() <= T
    assert np.all(steps[ctrl] < T), steps[ctrl]
    assert np.all(steps[(~ctrl) & (det == 0)] == T)
    skipped = 0
    for l, n in enumerate(steps):
        n = int(n)
        assert not terminal(S[l, :n]).any(), "lane %d recorded a terminal state" % l
        assert np.all(np.isnan(S[l, n:])), "lane %d wrote a state after its last step" % l
        if n == T:
            continue
        cand = candidates(l, n - 1)
        if margin_small(cand).any():
            skipped += 1
            continue
        assert terminal(cand).any(), "lane %d stopped at %d short of the goal" % (l, n)
    assert skipped <= 1
    assert np.all(np.isfinite(g["ent"]))


@pytest.mark.parametrize("long_case", ["acrobot"], indirect=True)
def test_acrobot_termination_and_return(long_case):
    name, (idx, sign, det, ctrl), g = long_case
    S, steps, T = g["states"], g["steps"], 500
    st = ref.acrobot_state_from_obs
    _termination(name, g, ctrl, det, T, lambda o: ref.acrobot_terminal(st(o)),
                 lambda l, t: ref.acrobot_obs(np.stack([ref.acrobot_step_f32(st(S[l, t]), a) for a in range(3)])),
                 lambda o: ref.acrobot_margin(st(o)) < 1e-5)
    # -1 per step, 0 on the terminal one: exact integers
    np.testing.assert_array_equal(g["ret"], np.where(steps < T, -(steps - 1.0), -float(T)))
    assert 60 <= steps[ctrl].min() and steps[ctrl].max() <= 300
    assert np.all(g["ent"] > 0) and np.all(g["ent"][~ctrl] <= np.log(3.0) + 1e-5)


@pytest.mark.parametrize("long_case", ["mountaincar"], indirect=True)
def test_mountaincar_termination_and_return(long_case):
    name, (idx, sign, det, ctrl), g = long_case
    S, steps, T = g["states"], g["steps"], 200
    _termination(name, g, ctrl, det, T, lambda o: ref.mountaincar_done(o[..., 0], o[..., 1]),
                 lambda l, t: np.stack([np.stack(ref.mountaincar_step_f32(S[l, t, 0], S[l, t, 1], a)[:2], -1)
                                        for a in range(3)]),
                 lambda o: ref.mountaincar_borderline(o[..., 0], o[..., 1]))
    np.testing.assert_array_equal(g["ret"], -steps.astype(np.float64))          # -1 per step taken, exact
    assert 100 <= steps[ctrl].min() and steps[ctrl].max() <= 135
    assert np.all(g["ent"] >= 0) and np.all(g["ent"][~ctrl] <= np.log(3.0) + 1e-5)


@pytest.mark.parametrize("long_case", ["mountaincar_cont"], indirect=True)
def test_mountaincar_cont_termination_and_return(long_case):
    """The return against the restated reward sum along the GPU's own trajectory (f32 rewards summed in f64, the
    recomputed actions, +100 on the finishing step).  Tolerance: the restatement's own f32-versus-f64 reward error,
    pinned at 4e-6 per step, over the T = 999 steps: 4e-3.  Measured GPU maximum (printed): 3.4e-6."""
    name, (idx, sign, det, ctrl), g = long_case
    S, steps, T = g["states"], g["steps"], 999
    act = _continuous_actions(name, g, idx, sign, det, ctrl, SEED_LONG)

    def cand(l, t):
        p, v, _, _ = ref.mountaincar_step_f32(S[l, t, 0], S[l, t, 1], act[l, t], cont=True)
        return np.array([[p, v]])
    _termination(name, g, ctrl, det, T, lambda o: ref.mountaincar_done(o[..., 0], o[..., 1], cont=True), cand,
                 lambda o: ref.mountaincar_borderline(o[..., 0], o[..., 1], cont=True))
    assert 70 <= steps[ctrl].min() and steps[ctrl].max() <= 125
    tol = T * ref.MCC_ERR[2]
    worst = 0.0
    for l, n in enumerate(steps):
        n = int(n)
        a = act[l, :n]
        rew = (-(np.float32(0.1) * a * a)).astype(np.float32).astype(np.float64)
        if n < T:
            rew[-1] = float(np.float32(100.0) - np.float32(0.1) * a[-1] * a[-1])
        worst = max(worst, abs(g["ret"][l] - rew.sum()))
        assert abs(g["ret"][l] - rew.sum()) <= tol, "lane %d: ret %.6f, restated %.6f" % (l, g["ret"][l], rew.sum())
    print("mountaincar_cont return: max |gpu - restated| = %.3g (tolerance %.3g)" % (worst, tol))
    assert np.all(g["ret"][ctrl] > 80) and np.all(g["ret"][~ctrl] < 0)           # the +100 arrived, and only there


# ---- 4. MountainCar whole episodes ------------------------------------------------------------------------------
def _compare_whole(g, o):
    keep = ~o["borderline"]
    assert (~keep).sum() <= 2
    np.testing.assert_array_equal(g["steps"][keep], o["steps"][keep])
    np.testing.assert_array_equal(g["ret"][keep], o["ret"][keep])
    np.testing.assert_allclose(g["ent"][keep], o["ent"][keep], rtol=0, atol=1e-5)
    np.testing.assert_allclose(g["norm2"], o["norm2"], rtol=1e-9, atol=0)
    return keep


@pytest.mark.parametrize("long_case", ["mountaincar"], indirect=True)
def test_mountaincar_whole_episodes_vs_oracle(long_case, eng):
    """Not chaotic: the controller lanes (and the rest of the 61-lane case) and 64 sampled lanes against
    evaluate_lanes -- steps and returns exact, entropies to 1e-5, norm2 to 1e-9 relative, <= 2 borderline lanes."""
    name, case, g = long_case
    o = oracle_episodes(name, *case, SEED_LONG)
    keep = _compare_whole(g, o)
    ctrl = case[3]
    assert keep[ctrl].sum() >= 6 and np.all(o["steps"][ctrl] < 200)
    case = case_short(name)
    g = _launch(eng, name, *case, SEED_SHORT)
    o = oracle_episodes(name, *case, SEED_SHORT)
    _compare_whole(g, o)
    assert np.all(o["steps"] == 200)


# ---- 5. extras on MountainCar-v0 --------------------------------------------------------------------------------
def case_extras(idx_seed):
    """16 lanes: 6 sampled +-pairs and 4 controller lanes."""
    return case_short("mountaincar", 16, n_ctrl=4, idx_seed=idx_seed)


def test_mountaincar_u_inject_replays_oracle_episodes(eng):
    """Action draws injected from another stream than the launch's seed: resets still come from the seed."""
    name, case = "mountaincar", case_extras(7)
    o = oracle_episodes(name, *case, SEED_XACT, env_seed=SEED_XENV)
    assert not o["borderline"].any()
    T = 200
    u = np.stack([crng.uniform(SEED_XACT, np.arange(16, dtype=np.uint64), t, 0) for t in range(T)], axis=1)
    g = _launch(eng, name, *case, SEED_XENV, u_inject=_dev(u.reshape(16, T, 1).astype(np.float32)))
    np.testing.assert_array_equal(g["steps"], o["steps"])
    np.testing.assert_array_equal(g["ret"], o["ret"])
    np.testing.assert_array_equal(g["states"][:, 0], o["states"][:, 0])
    assert np.all(g["steps"][case[3]] < T)
    # the draws matter: the same launch on its own stream takes other actions
    g2 = _launch(eng, name, *case, SEED_XENV)
    assert not np.array_equal(g2["states"][:12, 5], g["states"][:12, 5])


def test_mountaincar_obs_normalisation(eng):
    name, case = "mountaincar", case_extras(8)
    mean = np.array([-0.5, 0.0], np.float32)         # velocity mean 0: the controller still sees its sign
    std = np.array([0.3, 0.03], np.float32)
    o = oracle_episodes(name, *case, SEED_XNORM, obs_mean=mean, obs_std=std)
    keep = ~o["borderline"]
    assert (~keep).sum() <= 2 and np.all(o["steps"][case[3]] < 200)
    g = _launch(eng, name, *case, SEED_XNORM, obs_mean=_dev(mean), obs_std=_dev(std))
    np.testing.assert_array_equal(g["steps"][keep], o["steps"][keep])
    np.testing.assert_allclose(g["ent"][keep], o["ent"][keep], rtol=0, atol=1e-5)
    # recorded states are the raw observations
    pos, vel = ref.mountaincar_reset(SEED_XNORM, np.arange(16))
    np.testing.assert_array_equal(g["states"][:, 0], np.stack([pos, vel], -1))


def test_mountaincar_welford_statistics(eng):
    name, case = "mountaincar", case_extras(9)
    o = oracle_episodes(name, *case, SEED_XSTAT, obs_chance=0.5)
    assert not o["borderline"].any()
    g = _launch(eng, name, *case, SEED_XSTAT, record=False, obs_stats=0.5)
    res = g["res"]
    np.testing.assert_array_equal(g["steps"], o["steps"])
    cnt = res.obs_count.cpu().numpy()
    np.testing.assert_array_equal(cnt, [s.count for s in o["stats"]])           # counts exact
    assert cnt.sum() > 0.3 * o["steps"].sum()
    gm, g2 = res.obs_mean.cpu().numpy(), res.obs_m2.cpu().numpy()
    for l, s in enumerate(o["stats"]):
        if s.count:
            np.testing.assert_allclose(gm[l], s.mean_, rtol=1e-5, atol=1e-5)
            np.testing.assert_allclose(g2[l], s.m2, rtol=1e-5, atol=1e-5)


def test_mountaincar_time_limit(eng):
    """A time limit shorter than the controller's finish: every lane runs exactly that long."""
    name, case = "mountaincar", case_extras(7)
    g = _launch(eng, name, *case, SEED_LONG, T=60)
    np.testing.assert_array_equal(g["steps"], 60)
    np.testing.assert_array_equal(g["ret"], -60.0)
    assert not ref.mountaincar_done(g["states"][..., 0], g["states"][..., 1]).any()


def test_mountaincar_shard_invariance(eng):
    name, case = "mountaincar", case_extras(7)
    whole = _launch(eng, name, *case, SEED_SHORT)
    part = _launch(eng, name, *[c[8:] for c in case], SEED_SHORT, lane_offset=8)
    np.testing.assert_array_equal(part["steps"], whole["steps"][8:])
    np.testing.assert_array_equal(part["ret"], whole["ret"][8:])
    np.testing.assert_array_equal(part["states"].view(np.uint32), whole["states"][8:].view(np.uint32))
    assert np.all(part["steps"][-4:] < 200)


def _code(excinfo):
    return int(re.search(r"\(code (\d+)\)", str(excinfo.value)).group(1))


def test_u_inject_with_statistics_is_still_refused(eng):
    from fdr import _lib
    with pytest.raises(_lib.FDRError) as ei:
        _launch(eng, "mountaincar", *case_extras(7), 1, T=20, record=False, obs_stats=0.5,
                u_inject=torch.zeros((16, 20, 1), dtype=torch.float32, device=DEV))
    assert _code(ei) == _lib.FDR_ERR_UNSUPPORTED


# ---- 6. the three shapes' other kernels -------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ENVS))
def test_policy_forward_and_loader(eng, name):
    from envs import SyntheticEnv
    from fdr import _lib
    kind, n_in, n_act, P = ENVS[name][:4]
    theta, tab = policy_and_table(name)
    idx, sign, det, _ = lanes_mixed(tab, 6, 0, 1, idx_seed=11)
    sign[-1] = 0
    L = len(idx)
    spec = eng.PolicySpec(kind, n_in, n_act, P)
    lanes = eng.lanes_desc(_dev(theta), 0, _dev(tab.table), _dev(idx), _dev(sign), SIGMA)
    x = np.random.RandomState(3).randn(L, n_in).astype(np.float32)
    thetas = onoise.perturb(theta, tab.table, idx, sign, SIGMA)
    got = eng.policy_forward(spec, lanes, L, _dev(x))
    want = opol.lanes_forward(kind, n_in, n_act, thetas, x)
    if kind == "discrete":
        np.testing.assert_allclose(got.cpu().numpy(), want, rtol=1e-5, atol=1e-5)
    else:
        np.testing.assert_allclose(got[0].cpu().numpy(), want[0], rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(got[1].cpu().numpy(), want[1], rtol=1e-5, atol=1e-5)
    out, reads, counted, n2 = eng.theta_prime(spec, lanes, L, "lane")
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), thetas.view(np.uint32))
    assert torch.all(reads >= 1) and torch.all(counted == 1)
    with pytest.raises(_lib.FDRError) as ei:
        eng.theta_prime(spec, lanes, L, "pair")
    assert _code(ei) == _lib.FDR_ERR_UNSUPPORTED
    # the synthetic env has no instance at these shapes
    assert _refused(eng, spec, SyntheticEnv(n_in, n_act, kind == "discrete", 10, device=DEV), P) \
        == _lib.FDR_ERR_UNSUPPORTED


# ---- 7. refusals ------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("name", sorted(ENVS))
def test_refusals(eng, name):
    from fdr import _lib
    kind, n_in, n_act, P = ENVS[name][:4]
    # any policy other than the env's one, the other new shapes and the compiled MLP shapes included
    others = [(k, i, a, p) for k, i, a, p in [v[:4] for v in ENVS.values()] if (k, i, a) != (kind, n_in, n_act)]
    flip = "mujoco" if kind == "discrete" else "discrete"
    others += [("mujoco", 17, 6, 6092), ("discrete", 4, 2, opol.num_params("discrete", 4, 2)),
               (flip, n_in, n_act, opol.num_params(flip, n_in, n_act))]
    for k, i, a, p in others:
        assert _refused(eng, eng.PolicySpec(k, i, a, p), _env(name, 10), p) == _lib.FDR_ERR_UNSUPPORTED, (k, i, a)
    spec = eng.PolicySpec(kind, n_in, n_act, P)
    m = torch.zeros(64, dtype=torch.float32, device=DEV)
    for ptr in ("M", "K", "s0", "walkable"):
        d = _env(name, 10).desc()
        setattr(d, ptr, m.data_ptr())
        assert _refused(eng, spec, _Desc(d, 10), P) == _lib.FDR_ERR_INVALID, ptr
    for field, value in (("done_threshold", 0.5), ("obs_dim", n_in + 1), ("act_dim", n_act + 1),
                         ("episode_len", 10001), ("episode_len", 0)):
        d = _env(name, 10).desc()
        setattr(d, field, value)
        assert _refused(eng, spec, _Desc(d, 10), P) == _lib.FDR_ERR_INVALID, field


# ---- 8. runner --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env_id", ["Acrobot-v1", "MountainCar-v0", "MountainCarContinuous-v0"])
def test_runner_trains_on_physics_envs(env_id):
    import envs
    from run_sequential import SequentialRunner
    r = SequentialRunner(env_id=env_id, physics=True, batch_size=32, antithetic=True, noise_table_size=1 << 20,
                         verbose=False)
    cls, T = {"Acrobot-v1": (envs.AcrobotEnv, 500), "MountainCar-v0": (envs.MountainCarEnv, 200),
              "MountainCarContinuous-v0": (envs.MountainCarContinuousEnv, 999)}[env_id]
    assert type(r.env) is cls and r.env.episode_len == T
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
    assert n_lanes >= 128 and 0 < total <= n_lanes * T
