"""GPU: the linear policy (FDR_POLICY_LINEAR) on the five physics envs, one lane per thread (rollout_linear_kernel,
policy_forward_linear_kernel).

Parity is against tests/linear_ref.py over the seeded cases of tests/linear_cases.py, whose conditions (which lanes
are borderline, at most 2 of 64) tests/test_linear_ref.py pins on the CPU.  theta', y, the action, resets, step
counts, +-1 returns, Welford counts and shards are compared bit for bit; transitions and the two continuous envs'
returns at the tolerances tests/test_gpu_physics_envs.py and test_gpu_physics_envs2.py already use for these envs.
"""
import re

import numpy as np
import pytest
import torch

import branch_cases as bc
import linear_cases as lc
import linear_ref as lref
import physics_ref as ref
import physics_ref2 as ref2

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SENT = -7.0
# One-step tolerances of the existing physics tests, per observation component
PEND_STEP_TOL, PEND_RET_PER_STEP = 5e-6, 4e-3 / 200       # test_gpu_physics_envs.py::test_pendulum (T = 200: 4e-3)
CART_STEP_TOL = 2e-6                                       # ::test_cartpole_one_step_consistency
_e = ref2.ACROBOT_ERR
ACRO_STEP_TOL = 10 * np.array([_e[0], _e[0], _e[1], _e[1], _e[2], _e[3]])
MC_STEP_TOL = 10 * np.array(ref2.MC_ERR)
MCC_STEP_TOL = 10 * np.array(ref2.MCC_ERR[:2])
MCC_RET_PER_STEP = ref2.MCC_ERR[2]


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def _code(excinfo):
    return int(re.search(r"\(code (\d+)\)", str(excinfo.value)).group(1))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


@pytest.fixture(scope="module")
def eng():
    from fdr import engine
    return engine


def _env(name, T):
    import envs
    return {"cartpole": envs.CartPoleEnv, "pendulum": envs.PendulumEnv, "acrobot": envs.AcrobotEnv,
            "mountaincar": envs.MountainCarEnv, "mountaincar_cont": envs.MountainCarContinuousEnv}[name](T)


def _launch(eng, c, n=None, lane_lo=0, record=False, stats=False, episodes=None, ids=None, ret_sq=False, jiggle=False,
            idx=None, sign=None, pad=0, T=None):
    """Lanes [lane_lo, lane_lo + n) of case c in one launch; outputs are allocated for n + pad lanes and prefilled
    with a sentinel (states: NaN).  episodes = K routes through fdr_rollout_episodes."""
    n = lc.L - lane_lo if n is None else n
    T = c.T if T is None else T
    sl = slice(lane_lo, lane_lo + n)
    idx = c.idx if idx is None else idx
    sign = c.sign if sign is None else sign
    spec = eng.PolicySpec("linear", c.n_in, c.n_act, c.P)
    lanes = eng.lanes_desc(_dev(c.theta), 0, _dev(c.table), _dev(idx[sl]), _dev(sign[sl]), c.sigma,
                           lane_offset=c.lane_offset + lane_lo)
    m = n + pad
    buf = torch.full((3, m), SENT, dtype=torch.float64, device=DEV)
    out = eng.RolloutResult(buf[0], buf[1], torch.full((m,), int(SENT), dtype=torch.int32, device=DEV), buf[2])
    kw = dict(jiggle=jiggle, obs_mean=None if c.obs_mean is None else _dev(c.obs_mean),
              obs_std=None if c.obs_std is None else _dev(c.obs_std), out=out)
    states = None
    if stats:
        kw["obs_stats"] = c.obs_chance
    if episodes is None:
        if record:
            states = torch.full((m, T, c.n_in), float("nan"), dtype=torch.float32, device=DEV)
            kw["states"] = states[:n]
        res = eng.rollout(spec, _env(c.env, T), lanes, n, c.seed, **kw)
    else:
        if ret_sq:
            out.reward_sq = torch.full((m,), SENT, dtype=torch.float64, device=DEV)
        res = eng.rollout_episodes(spec, _env(c.env, T), lanes, n, c.seed, episodes,
                                   episode_ids=None if ids is None else _dev(ids), ret_sq=ret_sq, **kw)
    torch.cuda.synchronize()
    g = dict(ret=buf[0].cpu().numpy(), ent=buf[1].cpu().numpy(), norm2=buf[2].cpu().numpy(),
             steps=out.timesteps.cpu().numpy(), states=None if states is None else states.cpu().numpy(), res=res, n=n)
    if ret_sq:
        g["ret_sq"] = out.reward_sq.cpu().numpy()
    for k in ("ret", "ent", "norm2", "steps") + (("ret_sq",) if ret_sq else ()):
        assert np.all(g[k][n:] == SENT), "%s was written behind n_lanes" % k
        g[k] = g[k][:n]
    if states is not None:
        assert np.all(np.isnan(g["states"][n:])), "states were written behind n_lanes"
        g["states"] = g["states"][:n]
    return g


_RUNS = {}


def _recorded(eng, name):
    """The recorded launch of a case, shared by the tests that read it."""
    if name not in _RUNS:
        _RUNS[name] = _launch(eng, lc.case(name), record=True, pad=3)
    return _RUNS[name]


_REF = {}


def _restated(name, e=0):
    if (name, e) not in _REF:
        _REF[(name, e)] = lc.case(name).run(np.float32, e)
    return _REF[(name, e)]


# ---- 1. theta' and the forward, bit for bit ---------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cartpole", "acrobot"])
def test_theta_prime_bitwise_through_unit_vectors(eng, name):
    c = lc.case(name)
    spec = eng.PolicySpec("linear", c.n_in, c.n_act, c.P)
    max_idx = lc.TABLE_SIZE - c.P
    idx = np.concatenate([[0, 0, 0, max_idx, max_idx, max_idx], c.idx[:10]]).astype(np.int64)
    sign = np.array([1, -1, 0] * 2 + [1, -1] * 4 + [0, 1], np.int8)
    want, _ = lref.theta_prime(c.theta, c.table, idx, sign, c.sigma)
    n = len(idx)
    for j in range(c.n_in):
        x = np.zeros((n, c.n_in), np.float32)
        x[:, j] = 1.0
        lanes = eng.lanes_desc(_dev(c.theta), 0, _dev(c.table), _dev(idx), _dev(sign), c.sigma)
        y = eng.policy_forward(spec, lanes, n, _dev(x)).cpu().numpy()
        assert y.shape == (n, c.n_act)
        # 1 * w is w; the zero products add +0.0: -0.0 + 0.0 is +0.0, so compare values (== treats the zeros alike) and
        # the bits wherever the weight is not a zero
        w = want.reshape(n, c.n_act, c.n_in)[:, :, j]
        np.testing.assert_array_equal(y, w)
        nz = w != 0
        np.testing.assert_array_equal(_bits(y)[nz], _bits(w)[nz])
    # the row form: every lane its own base row, no table
    rows = want.copy()
    lanes = eng.lanes_desc(_dev(rows), c.P, None, _dev(idx), _dev(sign), c.sigma)
    x = np.random.RandomState(3).randn(n, c.n_in).astype(np.float32)
    y = eng.policy_forward(spec, lanes, n, _dev(x)).cpu().numpy()
    np.testing.assert_array_equal(_bits(y), _bits(lref.dot_ordered(rows.reshape(n, c.n_act, c.n_in), x)))
    # a general x through the table form
    lanes = eng.lanes_desc(_dev(c.theta), 0, _dev(c.table), _dev(idx), _dev(sign), c.sigma)
    y = eng.policy_forward(spec, lanes, n, _dev(x)).cpu().numpy()
    np.testing.assert_array_equal(_bits(y), _bits(lref.dot_ordered(want.reshape(n, c.n_act, c.n_in), x)))


@pytest.mark.parametrize("n_in,n_act,n", [(1, 1, 1), (5, 3, 257), (64, 16, 65), (17, 6, 300)])
def test_forward_any_shape(eng, n_in, n_act, n):
    """The forward is runtime-shaped (n_in <= 64, n_act <= 16); the output behind n_lanes stays untouched."""
    rs = np.random.RandomState(n_in)
    P = n_in * n_act
    theta, table = rs.randn(P).astype(np.float32), lc.table()
    idx = rs.randint(0, lc.TABLE_SIZE - P + 1, size=n).astype(np.int64)
    sign = rs.choice(np.array([-1, 0, 1], np.int8), size=n)
    x = rs.randn(n, n_in).astype(np.float32)
    from fdr import _lib
    spec = eng.PolicySpec("linear", n_in, n_act, P)
    lanes = eng.lanes_desc(_dev(theta), 0, _dev(table), _dev(idx), _dev(sign), 0.3)
    out = torch.full((n + 2, n_act), SENT, dtype=torch.float32, device=DEV)
    pd = spec.desc()
    import ctypes
    _lib.check(_lib.lib.fdr_policy_forward(None, ctypes.byref(pd), ctypes.byref(lanes), n, _dev(x).data_ptr(),
                                           out.data_ptr(), None, None), "fdr_policy_forward")
    torch.cuda.synchronize()
    W, _ = lref.theta_prime(theta, table, idx, sign, 0.3)
    got = out.cpu().numpy()
    np.testing.assert_array_equal(_bits(got[:n]), _bits(lref.dot_ordered(W.reshape(n, n_act, n_in), x)))
    assert np.all(got[n:] == SENT)


# ---- 2. lane-count edges and shards -----------------------------------------------------------------------------
def _many(c, n):
    rs = np.random.RandomState(11)
    idx = np.concatenate([c.idx, rs.randint(0, lc.TABLE_SIZE - c.P + 1, size=n - lc.L)]).astype(np.int64)
    sign = np.concatenate([c.sign, rs.choice(np.array([-1, 0, 1], np.int8), size=n - lc.L)])
    return idx, sign


@pytest.fixture(scope="module")
def whole300(eng):
    c = lc.case("cartpole_stats")
    idx, sign = _many(c, 300)
    return idx, sign, _launch(eng, c, n=300, idx=idx, sign=sign, record=True, stats=True, pad=5)


def _same_lanes(part, whole, lo, n, stats=True):
    for k in ("ret", "ent", "norm2"):
        np.testing.assert_array_equal(_bits(part[k]), _bits(whole[k][lo:lo + n]), err_msg=k)
    np.testing.assert_array_equal(part["steps"], whole["steps"][lo:lo + n])
    a, b = part["states"], whole["states"][lo:lo + n]
    np.testing.assert_array_equal(np.isnan(a), np.isnan(b))
    np.testing.assert_array_equal(_bits(np.nan_to_num(a)), _bits(np.nan_to_num(b)))
    if stats:
        for k in ("obs_mean", "obs_m2", "obs_count"):
            np.testing.assert_array_equal(getattr(part["res"], k).cpu().numpy(),
                                          getattr(whole["res"], k).cpu().numpy()[lo:lo + n], err_msg=k)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_lane_count_edges(eng, whole300, n):
    idx, sign, whole = whole300
    c = lc.case("cartpole_stats")
    part = _launch(eng, c, n=n, idx=idx, sign=sign, record=True, stats=True, pad=5)
    _same_lanes(part, whole, 0, n)


def test_whole_launch_is_sane(whole300):
    idx, sign, g = whole300
    assert g["steps"].min() >= 1 and g["steps"].max() == 64 and len(np.unique(g["steps"])) >= 10
    np.testing.assert_array_equal(g["ent"], 0.0)
    np.testing.assert_array_equal(g["ret"], g["steps"].astype(np.float64))


@pytest.mark.parametrize("lo,n", [(32, 32), (255, 45), (1, 256)])
def test_shard_equals_the_slice_of_the_whole_launch(eng, whole300, lo, n):
    idx, sign, whole = whole300
    part = _launch(eng, lc.case("cartpole_stats"), n=n, lane_lo=lo, idx=idx, sign=sign, record=True, stats=True, pad=1)
    _same_lanes(part, whole, lo, n)


# ---- 3. resets --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cartpole", "pendulum", "acrobot", "mountaincar", "mountaincar_cont", "cartpole_k3"])
def test_resets_bitwise(eng, name):
    """State 0 against the restatement's reset of the same stream ids.  Pendulum and Acrobot show their angles through
    cosf / sinf of the bit-exact reset angle: those two columns to an ulp of values in [0.5, 1], as the existing tests."""
    c = lc.case(name)
    g = _recorded(eng, name) if c.K == 1 else _launch(eng, c, record=True)
    S0 = g["states"][:, 0]
    ids = c.lane_offset + np.arange(lc.L)          # fdr_rollout keys lane l by lane_offset + l
    if c.env == "cartpole":
        np.testing.assert_array_equal(_bits(S0), _bits(ref.cartpole_reset(c.seed, ids)))
    elif c.env == "pendulum":
        th, thd = ref.pendulum_reset(c.seed, ids)
        np.testing.assert_array_equal(_bits(S0[:, 2]), _bits(thd))
        np.testing.assert_allclose(S0[:, 0], np.cos(th.astype(np.float64)), rtol=0, atol=2.0 ** -23)
        np.testing.assert_allclose(S0[:, 1], np.sin(th.astype(np.float64)), rtol=0, atol=2.0 ** -23)
    elif c.env == "acrobot":
        s = ref2.acrobot_reset(c.seed, ids)
        np.testing.assert_array_equal(_bits(S0[:, 4:]), _bits(s[:, 2:]))
        w = s.astype(np.float64)
        for col, f, k in ((0, np.cos, 0), (1, np.sin, 0), (2, np.cos, 1), (3, np.sin, 1)):
            np.testing.assert_allclose(S0[:, col], f(w[:, k]), rtol=0, atol=2.0 ** -23)
    else:
        pos, vel = ref2.mountaincar_reset(c.seed, ids)
        np.testing.assert_array_equal(_bits(S0), _bits(np.stack([pos, vel], -1)))
    assert len(np.unique(S0[:, -1 if c.env in ("pendulum", "acrobot") else 0])) >= 60     # every lane its own state


# ---- 4. per-step consistency on the recorded states -------------------------------------------------------------
def _transitions(steps):
    ll = np.concatenate([np.full(max(int(n) - 1, 0), l) for l, n in enumerate(steps)])
    tt = np.concatenate([np.arange(max(int(n) - 1, 0)) for n in steps])
    return ll.astype(np.int64), tt.astype(np.int64)


def _step_candidates(env, cur, acts):
    """Next observation of recorded observations cur under each action of acts ([k, n] or [n]) in the f32 restatement."""
    if env == "cartpole":
        return ref.cartpole_step_f32(cur, acts)
    if env == "acrobot":
        return ref2.acrobot_obs(ref2.acrobot_step_f32(ref2.acrobot_state_from_obs(cur), acts))
    if env == "pendulum":
        th = np.arctan2(cur[:, 1], cur[:, 0]).astype(np.float32)
        nth, nthd, _ = ref.pendulum_step_f32(th, cur[:, 2], acts)
        return ref.pendulum_obs(nth, nthd)
    p, v, _, _ = ref2.mountaincar_step_f32(cur[:, 0], cur[:, 1], acts, cont=env == "mountaincar_cont")
    return np.stack([p, v], -1)


@pytest.mark.parametrize("name", ["cartpole", "cartpole_long", "pendulum", "acrobot", "acrobot_ctrl", "mountaincar",
                                  "mountaincar_cont", "cartpole_norm", "acrobot_norm"])
def test_per_step_consistency(eng, name):
    """Along the GPU's own recorded trajectory: y recomputed from recorded state t gives the action; the transition to
    recorded state t + 1 matches the f32 restatement under THAT action within the env's existing one-step tolerance,
    and (discrete envs) under no other action unless the candidates coincide; nothing is written after the last step
    and no recorded state is one the env ends an episode on."""
    c = lc.case(name)
    g = _recorded(eng, name)
    S, steps = g["states"], g["steps"]
    W, _ = c.thetas()
    Wm = W.reshape(lc.L, c.n_act, c.n_in)
    assert steps.min() >= 1 and steps.max() <= c.T
    for l, n in enumerate(steps):
        assert np.all(np.isfinite(S[l, :n])) and np.all(np.isnan(S[l, n:])), "lane %d wrote after its last step" % l
    # no recorded state is terminal: a lane that should have stopped and went on would record one
    rec = np.concatenate([S[l, :n] for l, n in enumerate(steps)])
    assert not bc.terminal_recorded(c.env, rec).any(), "a lane went on from a terminal state"
    ll, tt = _transitions(steps)
    cur, nxt = S[ll, tt], S[ll, tt + 1]
    y = lref.dot_ordered(Wm[ll], lref.normalise(cur, c.obs_mean, c.obs_std))
    tol = {"cartpole": CART_STEP_TOL, "pendulum": PEND_STEP_TOL, "acrobot": ACRO_STEP_TOL, "mountaincar": MC_STEP_TOL,
           "mountaincar_cont": MCC_STEP_TOL}[c.env]
    ok = np.ones(len(ll), bool)
    if c.env == "acrobot":          # the pinned box of ACROBOT_ERR
        st = ref2.acrobot_state_from_obs(cur)
        ok = (np.abs(st[:, 2]) <= ref2.ACROBOT_BOX[0]) & (np.abs(st[:, 3]) <= ref2.ACROBOT_BOX[1])
        assert ok.mean() >= 0.95
    if c.discrete:
        act = lref.first_argmax(y)
        cand = np.stack([_step_candidates(c.env, cur, np.full(len(ll), a)) for a in range(c.n_act)])
        err = np.abs(cand - nxt[None])
        m = np.all(err <= tol, axis=-1)                                  # [A, n]
        chosen = err[act, np.arange(len(ll))]
        print("%s: %d transitions, max |gpu - restated| per component %s" % (name, int(ok.sum()), chosen[ok].max(0)))
        assert np.all(m[act, np.arange(len(ll))][ok]), \
            "transitions off the recomputed action: %d" % int((~m[act, np.arange(len(ll))][ok]).sum())
        same = np.all(cand == cand[act, np.arange(len(ll))][None], axis=-1)
        assert np.all((m == same)[:, ok]), "transitions that also match another action's distinct next state"
        if c.env != "mountaincar":
            assert (same.sum(0) == 1).all()
    else:
        a = y[:, 0]
        clamp = 2.0 if c.env == "pendulum" else 1.0
        ok &= np.abs(np.abs(a) - clamp) >= 1e-4                           # at the clamp the restated force may differ
        err = np.abs(_step_candidates(c.env, cur, a) - nxt)
        print("%s: %d of %d transitions, max |gpu - restated| per component %s" % (name, int(ok.sum()), len(ll),
                                                                                   err[ok].max(0)))
        assert ok.mean() > 0.9 and np.all(err[ok] <= tol)
    # the last step of a lane that stopped early: the recomputed action's next state is terminal (or borderline)
    early = np.nonzero(steps < c.T)[0]
    if c.env != "pendulum":
        assert len(early) >= (10 if name in ("cartpole", "cartpole_long", "acrobot_ctrl", "mountaincar",
                                             "mountaincar_cont", "cartpole_norm") else 0)
    skipped = 0
    for l in early:
        last = S[l, steps[l] - 1][None]
        yl = lref.dot_ordered(Wm[l][None], lref.normalise(last, c.obs_mean, c.obs_std))
        a = lref.first_argmax(yl) if c.discrete else yl[:, 0]
        nx = _step_candidates(c.env, last, a)
        if c.env == "cartpole":
            near, term = ref.cartpole_margin(nx) < 1e-5, ref.cartpole_failed(nx)
        elif c.env == "acrobot":
            st = ref2.acrobot_state_from_obs(nx)
            near, term = ref2.acrobot_margin(st) < 1e-5, ref2.acrobot_terminal(st)
        else:
            cont = c.env == "mountaincar_cont"
            near = ref2.mountaincar_borderline(nx[:, 0], nx[:, 1], cont=cont)
            term = ref2.mountaincar_done(nx[:, 0], nx[:, 1], cont=cont)
        if near[0]:
            skipped += 1
            continue
        assert term[0], "lane %d stopped at %d short of its termination" % (l, steps[l])
    assert skipped <= 2
    # returns along the recorded trajectory
    np.testing.assert_array_equal(g["ent"], 0.0)
    if c.env == "cartpole":
        np.testing.assert_array_equal(g["ret"], steps.astype(np.float64))
    elif c.env == "mountaincar":
        np.testing.assert_array_equal(g["ret"], -steps.astype(np.float64))
    elif c.env == "acrobot":
        np.testing.assert_array_equal(g["ret"], np.where(steps < c.T, -(steps - 1.0), -float(c.T)))
    else:
        worst = 0.0
        for l, n in enumerate(steps):
            obs = S[l, :n]
            a = lref.dot_ordered(np.broadcast_to(Wm[l], (n, c.n_act, c.n_in)), lref.normalise(obs, c.obs_mean,
                                                                                              c.obs_std))[:, 0]
            if c.env == "pendulum":
                th = np.arctan2(obs[:, 1], obs[:, 0]).astype(np.float32)
                rew = ref.pendulum_step_f32(th, obs[:, 2], a)[2].astype(np.float64)
                tol_r = c.T * PEND_RET_PER_STEP
            else:
                rew = (-(np.float32(0.1) * a * a)).astype(np.float32).astype(np.float64)
                # the +100 belongs to a last step that reaches the goal (at step T itself too)
                p, v, dn, _ = ref2.mountaincar_step_f32(obs[-1:, 0], obs[-1:, 1], a[-1:], cont=True)
                if ref2.mountaincar_borderline(p, v, cont=True)[0]:
                    continue
                assert dn[0] or n == c.T
                if dn[0]:
                    rew[-1] = float(np.float32(100.0) - np.float32(0.1) * a[-1] * a[-1])
                tol_r = c.T * MCC_RET_PER_STEP
            worst = max(worst, abs(g["ret"][l] - rew.sum()))
            assert abs(g["ret"][l] - rew.sum()) <= tol_r, "lane %d: ret %.6f, restated %.6f" % (l, g["ret"][l],
                                                                                              rew.sum())
        print("%s return along the trajectory: max |gpu - restated| = %.3g (tolerance %.3g)" % (name, worst, tol_r))


# ---- 5. whole episodes against the restatement ------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cartpole", "pendulum", "acrobot", "mountaincar", "mountaincar_cont"])
def test_episodes_against_the_restatement(eng, name):
    c = lc.case(name)
    g, o = _recorded(eng, name), _restated(name)
    keep = ~o["borderline"]
    assert (~keep).sum() <= 2
    np.testing.assert_array_equal(g["steps"][keep], o["steps"][keep])
    diff = np.abs(g["ret"] - o["ret"])[keep]
    print("%s: steps %d .. %d, max |ret - restated| = %.3g" % (name, g["steps"].min(), g["steps"].max(), diff.max()))
    if c.env == "pendulum":
        assert np.all(diff <= c.T * PEND_RET_PER_STEP)
    elif c.env == "mountaincar_cont":
        assert np.all(diff <= c.T * MCC_RET_PER_STEP)
    else:
        np.testing.assert_array_equal(g["ret"][keep], o["ret"][keep])
    np.testing.assert_array_equal(g["ent"], 0.0)
    _, n2 = c.thetas()
    assert n2[5] == 0.0 and g["norm2"][5] == 0.0                    # a sign-0 lane
    np.testing.assert_allclose(g["norm2"], n2, rtol=1e-12, atol=0)


def test_out_of_range_offset_runs_unperturbed_with_nan_norm2(eng):
    c = lc.case("cartpole")
    idx = c.idx.copy()
    idx[2], idx[3], idx[10] = -1, lc.TABLE_SIZE - c.P + 1, 1 << 40
    g = _launch(eng, c, idx=idx, record=True)
    assert np.all(np.isnan(g["norm2"][[2, 3, 10]])) and np.all(np.isfinite(np.delete(g["norm2"], [2, 3, 10])))
    # lanes 5 and 40 run theta itself: the bad lanes play their own resets under the same theta
    W = np.broadcast_to(c.theta, (3, c.P))
    o = lref.run(c.env, W, c.seed, c.ids[[2, 3, 10], 0], c.T)
    assert not o["borderline"].any()
    np.testing.assert_array_equal(g["steps"][[2, 3, 10]], o["steps"])
    np.testing.assert_array_equal(g["ret"][[2, 3, 10]], o["ret"])
    whole = _recorded(eng, "cartpole")
    others = np.delete(np.arange(lc.L), [2, 3, 10])
    np.testing.assert_array_equal(g["steps"][others], whole["steps"][others])


def test_jiggle_is_the_mlp_kernels(eng):
    from oracle import rng as crng
    c = lc.case("cartpole")
    g = _launch(eng, c, jiggle=True)
    whole = _recorded(eng, "cartpole")
    np.testing.assert_array_equal(g["ret"], whole["ret"] + crng.jiggle(c.seed, np.arange(lc.L, dtype=np.uint64)))


# ---- 6. observation normalisation and the Welford statistics ----------------------------------------------------
@pytest.mark.parametrize("name", ["cartpole_norm", "acrobot_norm"])
def test_normalised_run_against_the_restatement(eng, name):
    g, o = _recorded(eng, name), _restated(name)
    keep = ~o["borderline"]
    assert (~keep).sum() <= 2
    np.testing.assert_array_equal(g["steps"][keep], o["steps"][keep])
    np.testing.assert_array_equal(g["ret"][keep], o["ret"][keep])
    # the recorded states are the raw observations
    np.testing.assert_array_equal(np.isnan(g["states"][keep]), np.isnan(o["states"][keep]))
    if name == "cartpole_norm":
        np.testing.assert_array_equal(g["states"][:, 0], o["states"][:, 0])


@pytest.mark.parametrize("name", ["cartpole_stats", "acrobot_stats"])
def test_welford_statistics(eng, name):
    """Counts exact; mean and m2 at the rtol / atol of the existing Welford tests (1e-5 / 1e-5)."""
    c = lc.case(name)
    g = _launch(eng, c, stats=True, pad=2)
    o = _restated(name)
    keep = ~o["borderline"]
    assert (~keep).sum() <= 2
    np.testing.assert_array_equal(g["steps"][keep], o["steps"][keep])
    res = g["res"]
    cnt, gm, g2 = res.obs_count.cpu().numpy(), res.obs_mean.cpu().numpy(), res.obs_m2.cpu().numpy()
    assert cnt.shape == (lc.L,) and gm.shape == (lc.L, c.n_in)
    want = np.array([s.count for s in o["stats"]])
    np.testing.assert_array_equal(cnt[keep], want[keep])
    assert 0.5 * c.obs_chance * o["steps"].sum() < want.sum() < 1.5 * c.obs_chance * o["steps"].sum()
    for l in np.nonzero(keep)[0]:
        s = o["stats"][l]
        np.testing.assert_allclose(gm[l], s.running_mean, rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(g2[l], s.running_variance, rtol=1e-5, atol=1e-5)


# ---- 7. fdr_rollout_episodes ------------------------------------------------------------------------------------
def test_one_episode_equals_the_rollout(eng):
    c = lc.case("cartpole_stats")
    a = _launch(eng, c, stats=True)
    b = _launch(eng, c, stats=True, episodes=1, ret_sq=True, pad=2)
    for k in ("ret", "ent", "norm2"):
        np.testing.assert_array_equal(_bits(a[k]), _bits(b[k]), err_msg=k)
    np.testing.assert_array_equal(a["steps"], b["steps"])
    np.testing.assert_array_equal(b["ret_sq"], a["ret"] * a["ret"])
    for k in ("obs_mean", "obs_m2", "obs_count"):
        np.testing.assert_array_equal(getattr(a["res"], k).cpu().numpy(), getattr(b["res"], k).cpu().numpy())


@pytest.mark.parametrize("n", [64, 37])
def test_three_episodes_fold_three_launches(eng, n):
    """K = 3, episode_ids NULL: lane l's episodes are the single episodes of stream ids (lane_offset + l) 3 + e."""
    c = lc.case("cartpole_k3")
    g = _launch(eng, c, n=n, episodes=3, ret_sq=True, pad=1)
    rsum, rsq, nsum = np.zeros(n), np.zeros(n), np.zeros(n, np.int64)
    for e in range(3):
        one = _launch(eng, c, n=n, episodes=1, ids=c.ids[:n, e:e + 1].astype(np.int64))
        rsum, rsq, nsum = rsum + one["ret"], rsq + one["ret"] * one["ret"], nsum + one["steps"]
        np.testing.assert_array_equal(_bits(one["norm2"]), _bits(g["norm2"]))
    np.testing.assert_array_equal(g["ret"], rsum / 3.0)
    np.testing.assert_array_equal(g["ret_sq"], rsq)
    np.testing.assert_array_equal(g["steps"], nsum)
    np.testing.assert_array_equal(g["ent"], 0.0)
    # and the restatement, on the lanes the CPU conditions keep
    o = lref.run_episodes(c.env, c.thetas()[0][:n], c.seed, c.ids[:n], c.T)
    keep = ~o["borderline"]
    assert (~keep).sum() <= 2
    np.testing.assert_array_equal(g["steps"][keep], o["steps"][keep])
    np.testing.assert_array_equal(g["ret"][keep], o["ret"][keep])
    np.testing.assert_array_equal(g["ret_sq"][keep], o["ret_sq"][keep])


def test_equal_ids_give_equal_returns(eng):
    """Common random numbers: lanes of theta itself (sign 0) on equal stream ids return the same bits, jiggle off; with
    the jiggle on they differ by the physical lanes' tie-breakers only."""
    c = lc.case("mountaincar_cont")
    sign = np.zeros(lc.L, np.int8)
    ids = np.tile(np.array([[7, 8, 9]], np.int64), (lc.L, 1))
    ids[1::2] = [[7, 8, 9]]
    ids[10] = [70, 80, 90]
    g = _launch(eng, c, sign=sign, episodes=3, ids=ids, ret_sq=True)
    same = np.delete(np.arange(lc.L), 10)
    assert len(np.unique(_bits(g["ret"][same]))) == 1 and len(np.unique(g["steps"][same])) == 1
    assert len(np.unique(_bits(g["ret_sq"][same]))) == 1
    assert g["ret"][10] != g["ret"][0]
    j = _launch(eng, c, sign=sign, episodes=3, ids=ids, jiggle=True)
    d = j["ret"] - g["ret"]
    assert np.all(np.abs(np.abs(d) - 1e-12) < 1e-13) and len(np.unique(np.sign(d))) == 2


# ---- 8. refusals ------------------------------------------------------------------------------------------------
def _refused(eng, fn):
    from fdr import _lib
    buf = torch.full((4, 8), SENT, dtype=torch.float64, device=DEV)
    out = eng.RolloutResult(buf[0], buf[1], torch.full((8,), int(SENT), dtype=torch.int32, device=DEV), buf[2])
    with pytest.raises(_lib.FDRError) as ei:
        fn(out)
    torch.cuda.synchronize()
    assert torch.all(buf == SENT) and torch.all(out.timesteps == int(SENT)), "a refused call launched"
    return _code(ei)


def test_refusals(eng):
    import envs
    from fdr import _lib
    UNS, INV = _lib.FDR_ERR_UNSUPPORTED, _lib.FDR_ERR_INVALID
    base = torch.zeros(64, dtype=torch.float32, device=DEV)
    lanes = eng.lanes_desc(base, 0)
    lin = lambda i, a: eng.PolicySpec("linear", i, a, i * a)  # noqa: E731
    # the synthetic and trap envs
    syn = envs.SyntheticEnv(4, 2, True, 10, device=DEV)
    assert _refused(eng, lambda out: eng.rollout(lin(4, 2), syn, lanes, 8, 1, out=out)) == UNS
    assert _refused(eng, lambda out: eng.rollout(lin(2, 9), envs.TrapEnv(device=DEV), lanes, 8, 1, out=out)) == UNS
    # a shape that is not the env's own
    for spec, env in ((lin(3, 2), envs.CartPoleEnv(10)), (lin(4, 3), envs.CartPoleEnv(10)),
                      (lin(4, 2), envs.AcrobotEnv(10)), (lin(2, 3), envs.MountainCarContinuousEnv(10)),
                      (lin(3, 1), envs.MountainCarContinuousEnv(10))):
        assert _refused(eng, lambda out: eng.rollout(spec, env, lanes, 8, 1, out=out)) == UNS
        assert _refused(eng, lambda out: eng.rollout_episodes(spec, env, lanes, 8, 1, 2, out=out)) == UNS
    assert _refused(eng, lambda out: eng.rollout_episodes(lin(4, 2), syn, lanes, 8, 1, 2, out=out)) == UNS
    # nothing to inject
    u = torch.zeros((8, 10, 2), dtype=torch.float32, device=DEV)      # the binding sizes a non-discrete kind's by n_act
    assert _refused(eng, lambda out: eng.rollout(lin(4, 2), envs.CartPoleEnv(10), lanes, 8, 1, out=out,
                                                 u_inject=u)) == UNS
    # the MLP policies keep their own refusals, and the env's own policy still runs
    assert _refused(eng, lambda out: eng.rollout(eng.PolicySpec("mujoco", 4, 2, 4740), envs.CartPoleEnv(10), lanes,
                                                 8, 1, out=out)) == UNS
    # forward: one output
    import ctypes
    x = torch.zeros((8, 4), dtype=torch.float32, device=DEV)
    o0 = torch.full((8, 2), SENT, dtype=torch.float32, device=DEV)
    o1 = torch.full((8, 2), SENT, dtype=torch.float32, device=DEV)
    pd = lin(4, 2).desc()
    rc = _lib.lib.fdr_policy_forward(None, ctypes.byref(pd), ctypes.byref(lanes), 8, x.data_ptr(), o0.data_ptr(),
                                     o1.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == INV and torch.all(o0 == SENT) and torch.all(o1 == SENT)
    # the forward's own limits
    for i, a in ((65, 1), (1, 17), (0, 1)):
        with pytest.raises(_lib.FDRError) as ei:
            eng.policy_forward(lin(i, a), lanes, 1, torch.zeros((1, max(i, 1)), dtype=torch.float32, device=DEV))
        assert _code(ei) == UNS
    # no theta' read-back
    with pytest.raises(_lib.FDRError) as ei:
        eng.theta_prime(lin(4, 2), lanes, 8, "lane")
    assert _code(ei) == UNS
    with pytest.raises(_lib.FDRError) as ei:
        eng.theta_prime(lin(4, 2), lanes, 8, "dyn")
    assert _code(ei) == UNS


# ---- 9. runner --------------------------------------------------------------------------------------------------
def _mean_return(eng, r, theta, n=64):
    """Mean deterministic return of theta over n fixed reset ids, one rollout_episodes call, under the observation
    statistics the workers normalise with."""
    p = r.policy
    lanes = eng.lanes_desc(theta.contiguous(), 0)
    ids = torch.arange(5000, 5000 + n, dtype=torch.int64, device=DEV).reshape(n, 1)
    om, osd = r.agent.obs_norm_tensors(r.worker.fixed_obs_stats.mean, r.worker.fixed_obs_stats.std)
    res = eng.rollout_episodes(p.spec, r.env, lanes, n, 12345, 1, episode_ids=ids, jiggle=False, obs_mean=om,
                               obs_std=osd, device=DEV)
    torch.cuda.synchronize()
    return float(res.reward.mean().item())


def test_runner_trains_a_linear_policy_on_cartpole(eng):
    from policies import LinearPolicy
    from run_sequential import SequentialRunner
    r = SequentialRunner(env_id="CartPole-v1", physics=True, policy="linear", normalize_obs=True, antithetic=True,
                         batch_size=256, weighting="top_directions", top_directions=0.25, noise_source="counter",
                         verbose=False)
    p = r.policy
    assert isinstance(p, LinearPolicy) and p.KIND == "linear" and p.num_params == 8 and p.discrete
    assert r.strategy_handler.kind == "l2"
    before = p.get_trainable_flat().copy()
    np.testing.assert_array_equal(before, 0.0)                   # ARS starts at zero
    assert p.get_entropy(np.zeros((1, 4), np.float32)) == 0.0 and p.get_action(np.ones((1, 4), np.float32)) == 0
    zero = _mean_return(eng, r, torch.zeros(8, dtype=torch.float32, device=DEV))
    assert zero < 15                                             # theta = 0 always pushes left
    r.train(30)
    torch.cuda.synchronize()
    after = p.get_trainable_flat()
    assert np.all(np.isfinite(after)) and not np.array_equal(before, after)
    trained = _mean_return(eng, r, p.flat)
    print("linear CartPole-v1: mean deterministic return over 64 resets %.2f at theta = 0, %.2f after 30 epochs"
          % (zero, trained))
    assert trained > zero
    y = p.forward(np.ones((3, 4), np.float32)).cpu().numpy()
    np.testing.assert_array_equal(y, lref.dot_ordered(np.broadcast_to(after.reshape(1, 2, 4), (3, 2, 4)),
                                                      np.ones((3, 4), np.float32)))
    np.testing.assert_array_equal(p.get_strategy(np.ones((3, 4), np.float32)), y)


@pytest.mark.parametrize("variant", ["mixed", "adam", "table_k2_crn", "pendulum"])
def test_runner_variants_move_theta(variant):
    from run_sequential import SequentialRunner
    kw = dict(env_id="CartPole-v1", physics=True, policy="linear", normalize_obs=True, antithetic=True, batch_size=32,
              weighting="top_directions", top_directions=0.25, noise_source="counter", verbose=False, eval_prob=0.2)
    if variant == "mixed":
        # (the mixed objective standardises each channel: it is built for the z-score weighting)
        kw.update(objective="mixed", omega_default_value=0.5, weighting="zscore", top_directions=None)
    elif variant == "adam":
        kw.update(opt_fn=torch.optim.Adam)
    elif variant == "table_k2_crn":
        kw.update(noise_source="table", noise_table_size=1 << 16, episodes_per_lane=2, common_random_numbers=True,
                  weighting="zscore", top_directions=None)
    else:
        kw.update(env_id="Pendulum-v1", normalize_obs=False)
    r = SequentialRunner(**kw)
    before = r.policy.get_trainable_flat().copy()
    r.train(2 if variant == "mixed" else 1)
    torch.cuda.synchronize()
    after = r.policy.get_trainable_flat()
    assert np.all(np.isfinite(after)) and not np.array_equal(before, after)
    assert r.agent.cumulative_timesteps > 0
