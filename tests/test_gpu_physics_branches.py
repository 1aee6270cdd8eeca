"""GPU: the rollout kernels through every reachable branch of the five physics systems (cartpole_step, pendulum_step,
acrobot_step, mountaincar_step, wrap_pi of fdr_rollout_parts.h), with the linear policy as the driver.

The cases, the branch table and the checker are tests/branch_cases.py; tests/test_physics_branches_ref.py pins on the
CPU which rows each case takes on the f32 restatement and that check() raises on restatements with one constant of
one branch changed -- that, not a wrong kernel, is the evidence that these tests would notice one.  Closed-loop
bang-bang episodes are chaotic, so nothing here compares whole episodes: everything is checked along the GPU's own
recorded trajectory, and the census is counted again on it.

(a) fdr_rollout (rollout_linear_kernel), recorded: branch_cases.check on every launch of every case -- each
    transition is the restatement's under the recomputed action and no other's (Acrobot without a box exclusion: ten
    times ACROBOT_ERR_WIDE outside the box of ACROBOT_ERR), the clamped component is the constant bit for bit where a
    clamp or the wall acts, no recorded state is terminal or outside a clamp, nothing is written after a lane's last
    step, a lane that ended early has a terminal candidate (the x-exit cases: through the x test on the aimed side,
    |theta| below half its bound), the returns follow from the recorded steps and actions, and the trajectory takes
    every row the case is aimed at at least 8 times in at least 4 lanes.
(b) fdr_rollout_runs (rollout_runs_kernel): two runs of 32 lanes in one launch, the run boundary inside a wave, bit
    for bit (a)'s returns, steps and norm2 -- the +3 and -3 CartPole cases as the two runs of ONE launch with their
    own obs_mean_runs rows.
(c) fdr_rollout_episodes (rollout_episodes_kernel), K = 2: the episodes of stream ids l and 64 + l fold (a)'s first
    two launches bit for bit.
(d) rollout_kernel (the MLP lane form): deterministic sign-0 lanes of hand-built bang-bang DiscretePolicy vectors carry
    the x-exit and the MountainCar controllers (branch_cases.MlpCase), the rows the MLP suite's own cases miss; the
    same check.  (The MLP Pendulum launch of test_gpu_physics_envs.py prints its own count: +8 / -8 in 54 / 41 states.)

Measured on an MI355X (printed by the tests; profiles/r16a_gpu_physics_branches.txt), everything else in this file's
story -- the census of the restatement, the wide Acrobot error, the mutations -- only on the CPU:
  largest |gpu - restated| of a transition, per component: CartPole 2.4e-7 (tolerance 2e-6); Pendulum 8.3e-7 (5e-6);
  MountainCar-v0 6.0e-8 / 3.7e-9 (7e-7 / 7e-8); MountainCarContinuous-v0 1.2e-7 / 7.5e-9 (7e-7 / 8e-8); Acrobot inside
  the old box 5.5e-7 on cos / sin, 1.6e-6 thd1, 2.4e-6 thd2 (7e-6 / 8e-6 / 3e-5 / 5e-5), outside it (11,387 transitions
  of the four launches) 8.1e-7, 3.8e-6 and 5.7e-6 (2e-4 / 3e-4 / 2e-1 / 2e-1: the kernel is five orders closer to the
  f32 restatement than that restatement is to f64 there).
  Returns along the trajectory: Pendulum within 1.6e-5 (2e-3), MountainCarContinuous 7.6e-6 (1.2e-3).
  Census on the GPU's trajectories: identical to the CPU's for every case but acro_whirl (x_hi 102 lanes of 128, x_lo
  107; Pendulum +8 / -8 at 1948 / 2019 transitions; -0.07 at 411 (mc_wall) and 1324 (mcc_wall) transitions, the wall
  at 210 and 240), whose velocity clamps acted 12 times in 8 lanes (CPU: 31 in 12), 10 of them past the tolerance
  and bit-equal to +-fl32(4 fl32(pi)) / fl32(9 fl32(pi)).
  (d): all 64 lanes leave through x > 2.4 (steps 224 .. 242) and x < -2.4 (217 .. 243), 2.4e-7 from the restatement;
  mlp_mc_wall meets -0.07 at 193 transitions in 52 lanes and the wall at 102 in 64, every one bit-equal.
"""
import numpy as np
import pytest
import torch

import branch_cases as bc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SENT = -7.0
L = bc.L


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


@pytest.fixture(scope="module")
def eng():
    from fdr import engine
    return engine


def _env(name, T):
    import envs
    return {"cartpole": envs.CartPoleEnv, "pendulum": envs.PendulumEnv, "acrobot": envs.AcrobotEnv,
            "mountaincar": envs.MountainCarEnv, "mountaincar_cont": envs.MountainCarContinuousEnv}[name](T)


def _outputs(n, pad):
    from fdr import engine
    buf = torch.full((4, n + pad), SENT, dtype=torch.float64, device=DEV)
    steps = torch.full((n + pad,), int(SENT), dtype=torch.int32, device=DEV)
    out = engine.RolloutResult(buf[0, :n], buf[1, :n], steps[:n], buf[2, :n])
    out.reward_sq = buf[3, :n]
    return out, buf, steps


def _host(buf, steps, n, sq=False):
    torch.cuda.synchronize()
    b, s = buf.cpu().numpy(), steps.cpu().numpy()
    assert np.all(b[:3, n:] == SENT) and np.all(s[n:] == int(SENT)), "written behind n_lanes"
    g = dict(ret=b[0, :n], ent=b[1, :n], norm2=b[2, :n], steps=s[:n])
    if sq:
        assert np.all(b[3, n:] == SENT)
        g["ret_sq"] = b[3, :n]
    return g


_RUNS = {}


def _recorded(eng, name, off):
    """(a): the recorded launch of case `name` at lane offset off, shared by the tests that read it."""
    if (name, off) not in _RUNS:
        c = bc.case(name, off)
        spec = eng.PolicySpec("linear", c.n_in, c.n_act, c.P)
        lanes = eng.lanes_desc(_dev(c.theta), 0, _dev(c.table), _dev(c.idx), _dev(c.sign), c.sigma, lane_offset=off)
        out, buf, steps = _outputs(L, 3)
        states = torch.full((L + 3, c.T, c.n_in), float("nan"), dtype=torch.float32, device=DEV)
        eng.rollout(spec, _env(c.env, c.T), lanes, L, c.seed, jiggle=False, out=out, states=states[:L],
                    obs_mean=None if c.obs_mean is None else _dev(c.obs_mean),
                    obs_std=None if c.obs_std is None else _dev(c.obs_std))
        g = _host(buf, steps, L)
        S = states.cpu().numpy()
        assert np.all(np.isnan(S[L:])), "states were written behind n_lanes"
        g["states"] = S[:L]
        _RUNS[(name, off)] = g
    return _RUNS[(name, off)]


def _fmt(v):
    return "none" if v is None else np.array2string(np.asarray(v), precision=2, separator=", ")


# ---- (a) fdr_rollout ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", bc.NAMES)
def test_rollout_takes_the_branches(eng, name):
    launches = {off: _recorded(eng, name, off) for off in bc.OFFSETS[name]}
    reports, cen = bc.check_case(name, launches)
    print("%s: rows taken on the GPU's trajectories (times, lanes): %s" % (name, {k: v for k, v in cen.items() if v[0]}))
    for off, r in reports.items():
        print("  offset %3d: steps %d .. %d, max |gpu - restated| %s%s%s%s" % (
            off, r["steps"][0], r["steps"][1], _fmt(r["max_err"]),
            "; outside the old box (%d transitions) %s" % (r["outside_box"], _fmt(r["max_err_outside_box"]))
            if "outside_box" in r else "",
            "; bit-equal constants %s" % r["pinned"] if r["pinned"] else "",
            "; max |ret - restated| %.3g (tolerance %.3g)" % (r["max_ret_err"], r["ret_tol"]) if "ret_tol" in r else ""))
    for off, g in launches.items():
        _, n2 = bc.case(name, off).thetas()
        np.testing.assert_allclose(g["norm2"], n2, rtol=1e-12, atol=0)


# ---- (b) fdr_rollout_runs -------------------------------------------------------------------------------------------
def _runs(eng, halves):
    """One fdr_rollout_runs launch of R = 2 runs x 32 lanes: run r plays lanes [32 r, 32 r + 32) of case halves[r]."""
    ca, cb = (bc.case(n) for n in halves)
    assert ca.env == cb.env and ca.T == cb.T and ca.seed == cb.seed and (ca.obs_mean is None) == (cb.obs_mean is None)
    spec = eng.PolicySpec("linear", ca.n_in, ca.n_act, ca.P)
    h = L // 2
    idx = np.concatenate([ca.idx[:h], cb.idx[h:]])
    sign = np.concatenate([ca.sign[:h], cb.sign[h:]])
    out, buf, steps = _outputs(L, 3)
    norm = ca.obs_mean is not None
    eng.rollout_runs(spec, _env(ca.env, ca.T), _dev(np.stack([ca.theta, cb.theta])),
                     _dev(np.array([ca.sigma, cb.sigma], np.float32)), _dev(np.array([0, h], np.int64)), h, ca.seed,
                     table=_dev(ca.table), idx=_dev(idx), sign=_dev(sign), jiggle=False,
                     obs_mean_runs=_dev(np.stack([ca.obs_mean, cb.obs_mean])) if norm else None,
                     obs_std_runs=_dev(np.stack([ca.obs_std, cb.obs_std])) if norm else None, out=out)
    return _host(buf, steps, L)


def _same_lanes(g, a, sl, what):
    for k in ("ret", "ent", "norm2"):
        assert np.ascontiguousarray(g[k][sl]).tobytes() == np.ascontiguousarray(a[k][sl]).tobytes(), "%s: %s" % (what, k)
    np.testing.assert_array_equal(g["steps"][sl], a["steps"][sl], err_msg=what)


def test_runs_walk_the_cart_out_of_both_sides_in_one_launch(eng):
    """Run 0 with obs_mean (+3, 0, 0, 0) and run 1 with (-3, 0, 0, 0), the boundary at lane 32 of the one wave: each
    half is (a)'s, so run 0's lanes left through x > 2.4 and run 1's through x < -2.4 (checked there)."""
    g = _runs(eng, ("cart_x_hi", "cart_x_lo"))
    hi, lo = _recorded(eng, "cart_x_hi", 0), _recorded(eng, "cart_x_lo", 0)
    _same_lanes(g, hi, slice(0, 32), "run 0")
    _same_lanes(g, lo, slice(32, 64), "run 1")
    for got, c, side in ((hi, bc.case("cart_x_hi"), "x_hi"), (lo, bc.case("cart_x_lo"), "x_lo")):
        sl = slice(0, 32) if side == "x_hi" else slice(32, 64)
        cen = bc.census(c, got["states"], got["steps"])
        assert cen[side][0] >= bc.MIN_TIMES and (got["steps"][sl] < c.T).sum() >= bc.MIN_TIMES
    assert np.any(g["steps"][:32] != g["steps"][32:])


@pytest.mark.parametrize("name", [n for n in bc.NAMES if not n.startswith("cart_x")])
def test_runs_are_the_rollout(eng, name):
    g = _runs(eng, (name, name))
    _same_lanes(g, _recorded(eng, name, 0), slice(0, 64), name)


# ---- (c) fdr_rollout_episodes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", bc.NAMES)
def test_two_episodes_fold_two_rollouts(eng, name):
    c = bc.case(name)
    a0, a1 = _recorded(eng, name, 0), _recorded(eng, name, 64)
    spec = eng.PolicySpec("linear", c.n_in, c.n_act, c.P)
    lanes = eng.lanes_desc(_dev(c.theta), 0, _dev(c.table), _dev(c.idx), _dev(c.sign), c.sigma)
    ids = np.stack([np.arange(L), 64 + np.arange(L)], -1).astype(np.int64)
    out, buf, steps = _outputs(L, 3)
    eng.rollout_episodes(spec, _env(c.env, c.T), lanes, L, c.seed, 2, episode_ids=_dev(ids), jiggle=False, ret_sq=True,
                         out=out, obs_mean=None if c.obs_mean is None else _dev(c.obs_mean),
                         obs_std=None if c.obs_std is None else _dev(c.obs_std))
    g = _host(buf, steps, L, sq=True)
    np.testing.assert_array_equal(g["ret"], (a0["ret"] + a1["ret"]) / 2.0)
    # the sum of the squared episode returns: two products and a sum in f64, fused or not (2 ulp); the +-1-return envs
    # have integer returns, whose squares and sum are exact
    sq = a0["ret"] * a0["ret"] + a1["ret"] * a1["ret"]
    if c.env in bc.FORCE_CLAMP:
        np.testing.assert_allclose(g["ret_sq"], sq, rtol=2.0 ** -51, atol=0)
    else:
        np.testing.assert_array_equal(g["ret_sq"], sq)
    np.testing.assert_array_equal(g["steps"], a0["steps"] + a1["steps"])
    np.testing.assert_array_equal(g["ent"], 0.0)
    assert g["norm2"].tobytes() == a0["norm2"].tobytes() == a1["norm2"].tobytes()


# ---- (d) the MLP kernels: rollout_kernel, lane form -----------------------------------------------------------------
@pytest.mark.parametrize("name", bc.MLP_NAMES)
def test_mlp_controller_lanes_take_the_branches(eng, name):
    """64 deterministic sign-0 lanes of a hand-built bang-bang DiscretePolicy (every lane its own base row and its own
    reset), recorded: the same check, with the MLP suite's tolerances (CartPole 2e-6, MountainCar 10 x MC_ERR)."""
    import linear_cases as lc
    c = bc.case(name)
    theta = c.theta()
    P = theta.size
    spec = eng.PolicySpec("discrete", c.n_in, c.n_act, P)
    lanes = eng.lanes_desc(_dev(np.tile(theta, (L, 1))), P, _dev(lc.table()), _dev(np.zeros(L, np.int64)),
                           _dev(np.zeros(L, np.int8)), 0.02, _dev(np.ones(L, np.int8)))
    out, buf, steps = _outputs(L, 3)
    states = torch.full((L + 3, c.T, c.n_in), float("nan"), dtype=torch.float32, device=DEV)
    eng.rollout(spec, _env(c.env, c.T), lanes, L, c.seed, jiggle=False, out=out, states=states[:L],
                obs_mean=_dev(c.obs_mean), obs_std=_dev(c.obs_std))
    g = _host(buf, steps, L)
    S = states.cpu().numpy()
    assert np.all(np.isnan(S[L:])), "states were written behind n_lanes"
    g["states"] = S[:L]
    assert np.all(g["norm2"] == 0.0)
    reports, cen = bc.check_case(name, {0: g})
    r = reports[0]
    print("%s: rows taken on the GPU's trajectory (times, lanes): %s; steps %d .. %d, max |gpu - restated| %s%s" % (
        name, {k: v for k, v in cen.items() if v[0]}, r["steps"][0], r["steps"][1], _fmt(r["max_err"]),
        "; bit-equal constants %s" % r["pinned"] if r["pinned"] else ""))
