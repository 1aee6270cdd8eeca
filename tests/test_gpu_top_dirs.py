"""Top-b direction selection (fdr_top_dirs.hip in front of fd_grad_fused_kernel<FDR_WEIGHT_CENTERED_RANK>) on the GPU,
against the extended-precision restatement tests/top_dirs_ref.py.  Cases: tests/top_dirs_cases.py; the CPU side
(tests/test_top_dirs_ref.py) builds every one of them and holds it to learner_cases.KAPPA_MAX.

1. fdr_top_dir_weights: `selected` exact, unselected lanes exactly 0.0, a kept NaN -> every weight NaN; D over the
   256-thread and 2048-score tile edges, lanes_per_dir 1..3, b in {1, 2, ceil(D/2), D-1, D}, the whole range, a middle
   slice off the 256 grid and the last slice; ties across tiles, all equal, the maximum in the last lane, NaN, +-0.0.
2. fdr_fd_grad_fused_top against learner_ref.grad at the project's rel-L2 1e-12 (the weights are judged here).
3. b == D: g is fdr_fd_grad_fused(FDR_WEIGHT_ZSCORE)'s, bit for bit.
4. fdr_fd_step_top: g at 1e-12, theta / theta_hist bit-equal to learner_ref.dsgd_mirror (test_gpu_learner_edges'
   check); fdr_fd_step_top_opt (Adam): bit-equal to fdr_fd_grad_fused_top followed by fdr_opt_step, counters left zero,
   theta and state within optim_ref's allowance (test_gpu_optim's check).
5. FiniteDifferences(weighting="top_directions") end to end; 7. SequentialRunner.  (6, sharded: its own file.)

The device table is test_gpu_learner_edges' NaN-guarded buffer: a read outside the table turns the result NaN.

Worst measured on an MI355X (each test prints its own; profiles/p2x_top_dirs_gpu_tests.txt), next to the tolerance:
    fd_grad_fused_top, small grid (P 1 / 255 / 257 / 1000)   7.0e-16 / 8.3e-16 / 2.3e-16 / 1.9e-16   1e-12
    fd_grad_fused_top (2304, 1500, 2), b 1152                 2.6e-16   1e-12
    fd_step_top g / ||d theta|| relative                      9.0e-17 / 1.9e-16   1e-12 / P 2^-52
    fd_step_top_opt (Adam) g, k                               2.2e-16, 2.33   1e-12, allowance 17.2
    learner FDBatch step (b 24 / 29 / 96)                     1.5e-16 / 2.0e-16 / 2.2e-16   1e-12  (kappa 1.2 .. 1.9)
    learner list route: current / one epoch old               4.0e-16 / 5.3e-16   1e-12  (kappa 3.7)
    selected, unselected zeros, b == D vs z-score, theta      exact / bit-equal
"""
import numpy as np
import pytest
import torch

import learner_cases as lc
import learner_ref as ref
import optim_ref as oref
import test_gpu_learner_edges as edges
import test_gpu_optim as topt
import top_dirs_cases as tc
import top_dirs_ref as tref
from learner_cases import PR, SIGMA

pytestmark = pytest.mark.gpu

TOL = 1e-12
NAN = float("nan")
LD = np.longdouble
dev, Dev = edges.dev, edges.Dev


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from fdr import engine
    return engine


# ---- 1. the selection and the weights' structure -----------------------------------------------------------------
@pytest.mark.parametrize("D", tc.SEL_D)
def test_selection_is_exact(eng, D):
    n_calls = 0
    for lpd in tc.SEL_LPD:
        for kind in tc.SEL_RETURNS:
            r = tc.sel_returns(D, lpd, kind)
            rd = dev(r)
            for b in tc.sel_bs(D):
                keep = tref.selected(r, lpd, b)
                lane_keep = np.repeat(keep, lpd)
                poisoned = bool(np.isnan(r[lane_keep]).any())
                assert poisoned == (kind == "nan" and b == D)
                for lo, n in tc.sel_shards(D, lpd):
                    w, sel = eng.top_dir_weights(rd, PR, lpd, b, lo, n, selected=True)
                    w, sel = w.cpu().numpy(), sel.cpu().numpy()
                    msg = "D %d lpd %d %s b %d window (%d, %d)" % (D, lpd, kind, b, lo, n)
                    np.testing.assert_array_equal(sel, keep[lo // lpd:(lo + n) // lpd].astype(np.int8), err_msg=msg)
                    if poisoned:
                        assert np.isnan(w).all(), msg
                        continue
                    lk = lane_keep[lo:lo + n]
                    assert np.all(w[~lk] == 0.0) and not np.signbit(w[~lk]).any(), msg      # exactly +0.0
                    assert np.isfinite(w).all(), msg
                    if kind in ("equal", "signed_zero"):    # sd == 0 over the kept lanes: w = r - pr, exactly
                        np.testing.assert_array_equal(w[lk], (r - PR)[lo:lo + n][lk], err_msg=msg)
                    n_calls += 1
    print("top_dir_weights D %d: %d calls, selected exact" % (D, n_calls))


def test_selected_is_optional_and_empty_window_launches_nothing(eng):
    r = dev(tc.sel_returns(257, 2, "normal"))
    w = eng.top_dir_weights(r, PR, 2, 100, 0, 514)
    w2, _ = eng.top_dir_weights(r, PR, 2, 100, 0, 514, selected=True)
    assert w.cpu().numpy().tobytes() == w2.cpu().numpy().tobytes()
    # the statistics do not depend on the window: a slice's weights are the whole range's, bit for bit
    part = eng.top_dir_weights(r, PR, 2, 100, 300, 200).cpu().numpy()
    assert part.tobytes() == w.cpu().numpy()[300:500].tobytes()
    assert eng.top_dir_weights(r, PR, 2, 100, 514, 0).numel() == 0


# ---- 2. the gradient ---------------------------------------------------------------------------------------------
def run_top(eng, c, d, b):
    return eng.fd_grad_fused_top(d.table, d.idx, d.r_all, PR, c.lane_lo, d.sign, d.n2, c.lpd, SIGMA, c.P, b).cpu().numpy()


@pytest.mark.parametrize("P", tc.GRAD_P)
def test_grad_small_grid(eng, P):
    worst = 0.0
    for n_dirs in tc.GRAD_DIRS:
        c, b = tc.grad_case(n_dirs, P, 2, shard=(n_dirs % 2 == 1))
        d = Dev(c)
        e = ref.rel_l2(run_top(eng, c, d, b), ref.grad(c.table, P, c.idx_dirs, tc.coefs(c, b)))
        assert e <= TOL, (edges.what(c), b, e)
        worst = max(worst, e)
    print("fd_grad_fused_top P %d: worst rel-L2 %.2e (tolerance %.0e)" % (P, worst, TOL))


def test_grad_multi_chunk(eng):
    n_dirs, P, lpd = tc.GRAD_BIG
    assert lc.fused_plan(n_dirs, P) == lc.PLAN_TABLE[(n_dirs, P)] and lc.fused_plan(n_dirs, P)[2] > 1
    c, b = tc.grad_case(n_dirs, P, lpd)
    assert c.n_all == 4608
    d = Dev(c)
    out = run_top(eng, c, d, b)
    np.testing.assert_array_equal(run_top(eng, c, d, b), out)       # the tickets were left at zero
    e = ref.rel_l2(out, ref.grad(c.table, P, c.idx_dirs, tc.coefs(c, b)))
    print("fd_grad_fused_top (%d, %d) lpd %d b %d: rel-L2 %.2e (tolerance %.0e)" % (n_dirs, P, lpd, b, e, TOL))
    assert e <= TOL


@pytest.mark.parametrize("bad", ["past", "negative"])
def test_bad_offset_poisons_g_selected_or_not(eng, bad):
    """An out-of-range offset poisons g as in every mode, whether its direction is kept or not; the next clean call
    on the same workspace meets the reference."""
    c, b = tc.grad_case(130, 1000, 2)
    keep = tref.selected(c.r_all, 2, b)
    for where in (int(np.flatnonzero(keep)[len(keep) // 4]), int(np.flatnonzero(~keep)[len(keep) // 4])):
        assert np.all(np.isnan(run_top(eng, c, Dev(c, edges._bad_dirs(c, where, bad)), b))), where
    assert ref.rel_l2(run_top(eng, c, Dev(c), b), ref.grad(c.table, c.P, c.idx_dirs, tc.coefs(c, b))) <= TOL


# ---- 3. every direction kept: the z-score instance's bits -------------------------------------------------------
@pytest.mark.parametrize("n_dirs,P,lpd", tc.BIT_CASES)
def test_all_kept_is_bitwise_the_zscore_instance(eng, n_dirs, P, lpd):
    c = lc.make_case(n_dirs, P, lpd)
    assert c.lane_lo == 0 and c.n_all == n_dirs * lpd
    if n_dirs == 2304:
        assert c.n_all == 4608 > 4096       # past the z-score instance's 16 register values per thread
    d = Dev(c)
    z = eng.fd_grad_fused(d.table, d.idx, d.r_all, PR, 0, d.sign, d.n2, lpd, SIGMA, P, mode="zscore").cpu().numpy()
    t = run_top(eng, c, d, n_dirs)
    assert np.isfinite(z).all()
    assert t.tobytes() == z.tobytes(), "b == D differs from FDR_WEIGHT_ZSCORE in %d of %d" % ((t != z).sum(), P)


# ---- 4. the fused steps ------------------------------------------------------------------------------------------
def test_fd_step_top(eng):
    n_dirs, P, lpd = tc.STEP_CASE
    c, b = tc.grad_case(n_dirs, P, lpd)
    assert c.lane_lo == 0 and c.n_all == c.n_local
    d = Dev(c)
    g_ref = ref.grad(c.table, P, c.idx_dirs, tc.coefs(c, b))
    theta = lc.dsgd_inputs(P)[0]
    t = dev(theta)
    for _ in range(2):      # two steps on the same workspace
        g = torch.full((P,), NAN, dtype=torch.float64, device="cuda")
        hist = torch.full((P,), NAN, dtype=torch.float32, device="cuda")
        out = eng.fd_step_top(d.table, d.idx, d.r_all, PR, d.sign, d.n2, lpd, SIGMA, t, lc.DSGD_LR, lc.DSGD_SCALE, b,
                              g=g, theta_hist=hist).cpu().numpy()
        gd = g.cpu().numpy()
        e = ref.rel_l2(gd, g_ref)
        assert e <= TOL, e
        rel = edges.check_dsgd(theta, gd, t, out, hist)
        theta = t.cpu().numpy()
    print("fd_step_top P %d b %d: g rel-L2 %.2e, ||d theta|| relative %.2e" % (P, b, e, rel))


def test_fd_step_top_opt_adam(eng):
    from fdr import _lib
    n_dirs, P, lpd = tc.STEP_OPT_CASE
    kind, kw = oref.CASES["adam"]
    h, t = oref.hyper(kind, **kw), 7
    c, b = tc.grad_case(n_dirs, P, lpd)
    d = Dev(c)
    theta0 = lc.dsgd_inputs(P)[0]
    s0_in, s1_in = topt.state_inputs(kind, h, P, t)
    res = []
    for fused in (True, False):
        th, s0, s1 = dev(theta0), dev(s0_in), dev(s1_in)
        g = torch.full((P,), NAN, dtype=torch.float64, device="cuda")
        hist = torch.full((P,), NAN, dtype=torch.float32, device="cuda")
        sp = topt.spec(eng, kind, h, t, s0, s1)
        if fused:
            out = eng.fd_step_top_opt(d.table, d.idx, d.r_all, PR, d.sign, d.n2, lpd, SIGMA, th, sp, b, g=g,
                                      theta_hist=hist)
        else:
            eng.fd_grad_fused_top(d.table, d.idx, d.r_all, PR, 0, d.sign, d.n2, lpd, SIGMA, P, b, out=g)
            out = eng.opt_step(th, g, False, sp, theta_hist=hist)
        cb = int(_lib.lib.fdr_fd_grad_fused_counter_bytes(n_dirs, P))
        assert not topt.fused_counter(eng, _lib.FDR_WEIGHT_TOP_DIRS)[:cb].any().item(), "fused counters left non-zero"
        res.append([topt.host(x) for x in (g, th, s0, s1, hist, out)])
    for name, a, bb in zip(("g", "theta", "state0", "state1", "theta_hist", "out"), *res):
        assert a.tobytes() == bb.tobytes(), name
    e = ref.rel_l2(res[0][0], ref.grad(c.table, P, c.idx_dirs, tc.coefs(c, b)))
    assert e <= TOL, e
    assert np.isfinite(res[0][1]).all() and res[0][4].tobytes() == res[0][1].tobytes()
    ks = topt.check_step(kind, h, t, theta0, res[0][0], s0_in, s1_in, dev(res[0][1]), dev(res[0][2]), dev(res[0][3]),
                         res[0][5], "fd_step_top_opt adam")
    print("fd_step_top_opt adam: g rel-L2 %.2e, k %.2f (allowance %.1f)" % (e, max(ks), oref.K[kind]))


# ---- 5. the learner ----------------------------------------------------------------------------------------------
N_DIRS, T = 96, 50


def make_learner(top, opt="dsgd", seed=124, weighting="top_directions", **kw):
    from dsgd import DSGD
    from envs import SyntheticEnv
    from learner import FiniteDifferences
    from policies import MujocoPolicy
    from utils import AdaptiveOmega, SharedNoiseTable
    from worker import Agent, Worker
    devc = torch.device("cuda", 0)
    torch.manual_seed(seed)
    policy = MujocoPolicy(17, 6, seed=seed, device=devc)       # HalfCheetah's shape
    env = SyntheticEnv(17, 6, False, T, device=devc)
    table = SharedNoiseTable(1 << 20, policy.num_params, random_seed=seed)
    worker = Worker(policy, Agent(policy, env, random_seed=7), table, None, sigma=SIGMA, random_seed=seed)
    o = DSGD(policy.parameters(), lr=0.01) if opt == "dsgd" else torch.optim.Adam(policy.parameters(), lr=1e-3)
    learner = FiniteDifferences(policy, o, AdaptiveOmega(), table, noise_std=SIGMA, weighting=weighting,
                                top_directions=top, **kw)
    return learner, worker, table


def batch_reference(table, P, batch, b, lpd=2):
    """g from the batch's own returns and norms (longdouble) and the conditioning of its coefficients."""
    r = batch.reward.double().cpu().numpy()
    n2 = batch.norm2.cpu().numpy()
    idx_dirs = batch.idx_host[::lpd]
    w, keep = tref.weights(r, PR, lpd, b)
    k = tref.coef_condition(r, PR, lpd, b, 0, batch.sign_host, n2, SIGMA)
    return ref.grad(table._table, P, idx_dirs, ref.coef_d(w, batch.sign_host, n2, lpd, SIGMA)), keep, k


@pytest.mark.parametrize("top,b", [(24, 24), (0.25, 24), (0.3, 29), (500, 96)])
def test_learner_batch_step(eng, top, b):
    """A step from an FDBatch against the reference built from the batch's own returns and norms; int and float
    top_directions resolve as specified (0.3 x 96 = 28.8 -> 29; 500 is clipped to the 96 directions)."""
    learner, worker, table = make_learner(top)
    P = learner.policy.num_params
    batch = worker.evaluate(N_DIRS, antithetic=True, seed=1000)
    assert batch.lanes_per_dir == 2 and batch.reward.numel() == 2 * N_DIRS
    g_ref, keep, k = batch_reference(table, P, batch, b)
    assert keep.sum() == b
    theta0 = learner.policy.flat.cpu().numpy().copy()
    assert learner.step(batch, PR, 0.0, 0.0) > 0
    e = ref.rel_l2(learner.gradient_memory.cpu().numpy(), g_ref)
    print("learner top_directions=%r (b %d): g rel-L2 %.2e (tolerance %.0e), kappa %.1f" % (top, b, e, TOL, k))
    assert e <= TOL
    assert learner.policy.flat.cpu().numpy().tobytes() != theta0.tobytes() and learner.epoch == 1


def test_learner_routes_agree(eng):
    """DSGD above the fused step's parameter limit (fd_grad_fused_top + the apply) and Adam in the apply launch
    (fd_step_top_opt) form the fused DSGD step's gradient, bit for bit."""
    import learner.finite_differences as fdm
    a, worker, _ = make_learner(24)
    batch = worker.evaluate(N_DIRS, antithetic=True, seed=1000)
    a.step(batch, PR, 0.0, 0.0)
    g = a.gradient_memory.cpu().numpy().copy()
    b, _, _ = make_learner(24)
    saved = fdm.FUSED_STEP_MAX_P
    fdm.FUSED_STEP_MAX_P = 16
    try:
        b.step(batch, PR, 0.0, 0.0)
    finally:
        fdm.FUSED_STEP_MAX_P = saved
    assert b.gradient_memory.cpu().numpy().tobytes() == g.tobytes() and b.epoch == 1
    np.testing.assert_allclose(b.policy.flat.cpu().numpy(), a.policy.flat.cpu().numpy(), rtol=0, atol=1e-6)
    c, _, _ = make_learner(24, opt="adam")
    assert c.opt_route.route == "device" and c.step(batch, PR, 0.0, 0.0) > 0
    assert c.gradient_memory.cpu().numpy().tobytes() == g.tobytes()


def test_learner_list_routes(eng):
    """A list of FDReturn: current returns (every return a direction of its own, lanes_per_dir = 1), then the same
    returns one epoch old through the drift route (fd_lambda_norms, top_dir_weights / n2, fd_grad_lambda), against
    learner_ref.lambda_rows."""
    top = 40
    learner, worker, table = make_learner(top)
    P = learner.policy.num_params
    batch = worker.evaluate(N_DIRS, antithetic=True, seed=1001)
    rets = batch.to_returns()
    n = len(rets)
    r = np.array([x.reward for x in rets])
    idx = np.array([int(x.encoded_noise) for x in rets], np.int64)
    sign = np.array([x.sign for x in rets], np.int8)
    n2 = batch.norm2.cpu().numpy()
    theta0 = learner.policy.flat.cpu().numpy().copy()
    for x in rets:
        x.epoch = learner.epoch
    assert learner.step(rets, PR, 0.0, 0.0) > 0
    w, keep = tref.weights(r, PR, 1, top)
    assert keep.sum() == top
    k_cur = tref.coef_condition(r, PR, 1, top, 0, sign, n2, SIGMA)
    e_cur = ref.rel_l2(learner.gradient_memory.cpu().numpy(),
                       ref.grad(table._table, P, idx, ref.coef_d(w, sign, n2, 1, SIGMA)))
    theta1 = learner.policy.flat.cpu().numpy().copy()
    for x in rets:      # one epoch old: lambda_i = fl32(sign fl32(sigma eps_i) + (theta_0 - theta_1))
        x.epoch = learner.epoch - 1
        x.norm2 = None
    assert learner.step(rets, PR, 0.0, 0.0) > 0
    lam = ref.lambda_rows(table._table, P, idx, sign, np.zeros(n, np.int32), SIGMA, (theta0 - theta1)[None]).astype(LD)
    coef = w / (lam * lam).sum(1)
    e_stale = ref.rel_l2(learner.gradient_memory.cpu().numpy(), (coef[:, None] * lam).sum(0))
    print("learner top_directions list route: current %.2e (kappa %.1f), one epoch old %.2e (tolerance %.0e)"
          % (e_cur, k_cur, e_stale, TOL))
    assert max(e_cur, e_stale) <= TOL


def test_learner_value_errors(eng):
    with pytest.raises(ValueError, match="top_directions"):
        make_learner(None)
    for bad in (0, -1, 0.0, 1.5, "4", True):
        with pytest.raises(ValueError, match="top_directions"):
            make_learner(bad)
    with pytest.raises(ValueError, match="top_directions"):
        make_learner(8, weighting="zscore")
    with pytest.raises(ValueError, match="not built"):
        make_learner(8, objective="mixed")
    with pytest.raises(ValueError, match="weighting"):
        make_learner(None, weighting="best")


# ---- 7. the runner -----------------------------------------------------------------------------------------------
def test_runner_top_directions(eng):
    from run_sequential import SequentialRunner
    r = SequentialRunner(env_id="CartPole-v1", physics=True, antithetic=True, batch_size=64, weighting="top_directions",
                         top_directions=0.25, noise_table_size=1 << 20, verbose=False)
    assert r.learner.weighting == "top_directions" and r.learner.top_directions == 0.25
    theta0 = r.policy.get_trainable_flat().copy()
    r.train(3)
    assert len(r.history) == 3
    assert all(h["Update Magnitude"] > 0 for h in r.history)
    assert r.policy.get_trainable_flat().tobytes() != theta0.tobytes()
    c = SequentialRunner(env_id="CartPole-v1", physics=True, antithetic=True, batch_size=64, weighting="centred_rank",
                         noise_table_size=1 << 20, verbose=False)
    assert c.learner.weighting == "centred_rank"       # reachable from the runner too
    c.train(1)
    assert len(c.history) == 1
