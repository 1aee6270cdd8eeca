"""GPU: run batches -- R independent linear-policy runs per launch (fdr_rollout_runs, fdr_obs_stats_merge_runs,
fdr_fd_step_runs, PopulationRunner).

1. rollout_runs: run r is bit for bit the fdr_rollout_episodes call of the definition (include/fdr.h), in all eight
   output arrays, nothing written behind R * L; one case directly against linear_ref.
2. Permuting the runs permutes the outputs; a run alone (R = 1) gives the same bits.
3. obs_stats_merge_runs equals R obs_stats_merge calls.
4. fd_step_runs against the longdouble restatement (tests/runs_ref.py composes learner_ref and top_dirs_ref per run):
   g at the project's rel-L2 1e-12, theta and (||d theta||, ||grad||) against learner_ref.dsgd_mirror of the kernel's
   own g, poisoned runs leave their neighbours alone, b == D is the NULL form, permutation.
5. PopulationRunner: a run's theta and history do not depend on the population; per-run hyperparameters are honoured.
6. train() makes no host synchronisation.
7. It learns: the README's ARS-V2 CartPole settings, 8 seeds, next to the solo SequentialRunner.
"""
import numpy as np
import pytest
import torch

import learner_ref as ref
import linear_cases as lc
import runs_ref as rr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SENT = -7.0
TOL = 1e-12
NAN = float("nan")
ENV_SHAPE = {"cartpole": (4, 2), "pendulum": (3, 1), "acrobot": (6, 3), "mountaincar": (2, 3), "mountaincar_cont": (2, 1)}


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from fdr import engine
    return engine


def _env(name, T):
    import envs
    return {"cartpole": envs.CartPoleEnv, "pendulum": envs.PendulumEnv, "acrobot": envs.AcrobotEnv,
            "mountaincar": envs.MountainCarEnv, "mountaincar_cont": envs.MountainCarContinuousEnv}[name](T)


# ---- 1. the rollout ------------------------------------------------------------------------------------------------
class RolloutCase(object):
    """R runs x L lanes of one env: per-run theta, sigma (one run with sigma = 0), lane offsets and obs statistics;
    per-lane offsets into lc.table() with both table edges, signs from {+1, -1, 0}, one out-of-range offset."""

    def __init__(self, env, R, L, K, stats, norm, T, seed):
        self.env, self.R, self.L, self.K, self.stats, self.norm, self.T, self.seed = env, R, L, K, stats, norm, T, seed
        self.n_in, self.n_act = ENV_SHAPE[env]
        P = self.P = self.n_in * self.n_act
        rs = np.random.RandomState(1000 * R + L + seed)
        self.table = lc.table()
        self.theta = rs.randn(R, P).astype(np.float32)
        self.sigma = (0.3 + 0.2 * np.arange(R)).astype(np.float32)
        self.sigma[R // 2] = 0.0 if R > 1 else self.sigma[0]
        self.offsets = (rs.permutation(R) * 1000 + rs.randint(0, 7, R) * 2).astype(np.int64)   # even: pairs align
        n = R * L
        self.idx = rs.randint(0, lc.TABLE_SIZE - P + 1, size=n).astype(np.int64)
        self.idx[0] = 0
        self.idx[n - 1] = lc.TABLE_SIZE - P
        self.sign = rs.choice(np.array([1, -1, 0], np.int8), n, p=[0.45, 0.45, 0.1])
        self.bad = n // 2
        self.idx[self.bad] = lc.TABLE_SIZE - P + 1 if seed % 2 else -1
        self.sign[self.bad] = 1
        self.obs_mean = (rs.randn(R, self.n_in) * 0.1).astype(np.float32) if norm else None
        self.obs_std = (0.5 + rs.rand(R, self.n_in)).astype(np.float32) if norm else None
        self.ids = np.concatenate([rr.pair_stream_ids(o, L, K) for o in self.offsets]) if K > 1 else None
        self.chance = 0.3 if stats else None

    def outputs(self, n, pad=0):
        from fdr import engine
        m = n + pad
        buf = torch.full((4, m), SENT, dtype=torch.float64, device=DEV)
        out = engine.RolloutResult(buf[0], buf[1], torch.full((m,), int(SENT), dtype=torch.int32, device=DEV), buf[2])
        out.reward_sq = buf[3]
        if self.stats:
            out.obs_mean = torch.full((m, self.n_in), SENT, dtype=torch.float32, device=DEV)
            out.obs_m2 = torch.full((m, self.n_in), SENT, dtype=torch.float32, device=DEV)
            out.obs_count = torch.full((m,), int(SENT), dtype=torch.int32, device=DEV)
        return out

    @staticmethod
    def host(out, stats):
        keys = ["reward", "reward_sq", "entropy", "timesteps", "norm2"] + (["obs_mean", "obs_m2", "obs_count"] if stats else [])
        return {k: getattr(out, k).cpu().numpy() for k in keys}

    def runs(self, eng, order=None, pad=0):
        """One fdr_rollout_runs launch over the runs in `order` -> host arrays [len(order) * L (+ pad), ...]."""
        order = list(range(self.R)) if order is None else list(order)
        L, K = self.L, self.K
        lanes = np.concatenate([np.arange(r * L, (r + 1) * L) for r in order])
        out = self.outputs(len(lanes), pad)
        spec = eng.PolicySpec("linear", self.n_in, self.n_act, self.P)
        view = eng.RolloutResult(out.reward[:len(lanes)], out.entropy[:len(lanes)], out.timesteps[:len(lanes)],
                                 out.norm2[:len(lanes)])
        view.reward_sq = out.reward_sq[:len(lanes)]
        if self.stats:
            view.obs_mean, view.obs_m2, view.obs_count = (out.obs_mean[:len(lanes)], out.obs_m2[:len(lanes)],
                                                          out.obs_count[:len(lanes)])
        eng.rollout_runs(spec, _env(self.env, self.T), _dev(self.theta[order]), _dev(self.sigma[order]),
                         _dev(self.offsets[order]), L, self.seed, table=_dev(self.table), idx=_dev(self.idx[lanes]),
                         sign=_dev(self.sign[lanes]), n_episodes=K,
                         episode_ids=None if self.ids is None else _dev(self.ids[lanes]), jiggle=True,
                         obs_mean_runs=None if not self.norm else _dev(self.obs_mean[order]),
                         obs_std_runs=None if not self.norm else _dev(self.obs_std[order]), obs_stats=self.chance,
                         ret_sq=True, out=view)
        torch.cuda.synchronize()
        return self.host(out, self.stats)

    def solo(self, eng, r):
        """The fdr_rollout_episodes call of the definition for run r."""
        L, K = self.L, self.K
        sl = slice(r * L, (r + 1) * L)
        out = self.outputs(L)
        spec = eng.PolicySpec("linear", self.n_in, self.n_act, self.P)
        lanes = eng.lanes_desc(_dev(self.theta[r]), 0, _dev(self.table), _dev(self.idx[sl]), _dev(self.sign[sl]),
                               float(self.sigma[r]), lane_offset=int(self.offsets[r]))
        eng.rollout_episodes(spec, _env(self.env, self.T), lanes, L, self.seed, K,
                             episode_ids=None if self.ids is None else _dev(self.ids[sl]), jiggle=True,
                             obs_mean=None if not self.norm else _dev(self.obs_mean[r]),
                             obs_std=None if not self.norm else _dev(self.obs_std[r]), obs_stats=self.chance, ret_sq=True,
                             out=out)
        torch.cuda.synchronize()
        return self.host(out, self.stats)


# (R, L): run boundaries inside a wave, at a wave's edge, across workgroups.  Every env, K in {1, 3}, statistics and
# normalisation on and off over the seven shapes.
ROLLOUT_CASES = [("cartpole", 1, 1, 1, False, False, 64), ("acrobot", 1, 257, 3, True, True, 48),
                 ("pendulum", 5, 3, 3, False, True, 16), ("mountaincar", 3, 64, 1, True, False, 120),
                 ("mountaincar_cont", 2, 65, 3, True, True, 120), ("cartpole", 100, 3, 1, True, True, 64),
                 ("acrobot", 2, 256, 1, False, False, 48)]
_CASES = {}


def _case(spec):
    if spec not in _CASES:
        env, R, L, K, stats, norm, T = spec
        _CASES[spec] = RolloutCase(env, R, L, K, stats, norm, T, seed=11 + R)
    return _CASES[spec]


def _same(a, b, what):
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), "%s: %s differs in %d places" % (what, k, (a[k] != b[k]).sum())


@pytest.mark.parametrize("spec", ROLLOUT_CASES, ids=lambda s: "%s-R%d-L%d-K%d" % s[:4])
def test_rollout_runs_is_the_solo_kernel_per_run(eng, spec):
    c = _case(spec)
    n = c.R * c.L
    g = c.runs(eng, pad=5)
    for k, a in g.items():
        assert np.all(a[n:] == SENT), "%s was written behind R * L" % k
    g = {k: a[:n] for k, a in g.items()}
    assert np.all(g["entropy"] == 0.0)
    nan = np.isnan(g["norm2"])
    assert nan[c.bad] and nan.sum() == 1, "only the lane with the out-of-range offset has norm2 NaN"
    z = c.R // 2
    if c.R > 1:     # the sigma = 0 run: every norm2 0 (but the bad lane's NaN)
        assert np.all(g["norm2"][z * c.L:(z + 1) * c.L][~nan[z * c.L:(z + 1) * c.L]] == 0.0)
    assert g["timesteps"].min() >= c.K and g["timesteps"].max() <= c.K * c.T
    for r in range(c.R):
        s = c.solo(eng, r)
        _same({k: a[r * c.L:(r + 1) * c.L] for k, a in g.items()}, s, "run %d" % r)
    print("%s R %d L %d K %d: 8 arrays bit-equal to %d solo launches; steps %d .. %d"
          % (c.env, c.R, c.L, c.K, c.R, g["timesteps"].min(), g["timesteps"].max()))


def test_rollout_runs_against_linear_ref(eng):
    """linear_cases' pinned CartPole case cut into two runs of 32 lanes (the same theta and sigma, lane offsets 0 and
    32: the case's own global ids): steps and +-1 returns of every lane that is not borderline, bit for bit."""
    c = lc.case("cartpole")
    R, L = 2, 32
    spec = eng.PolicySpec("linear", c.n_in, c.n_act, c.P)
    res = eng.rollout_runs(spec, _env("cartpole", c.T), _dev(np.stack([c.theta, c.theta])),
                           _dev(np.full(R, c.sigma, np.float32)), _dev(np.array([0, L], np.int64) + c.lane_offset), L,
                           c.seed, table=_dev(c.table), idx=_dev(c.idx), sign=_dev(c.sign), jiggle=False)
    o = c.run(np.float32, 0)
    keep = ~o["borderline"]
    assert (~keep).sum() <= 2
    np.testing.assert_array_equal(res.timesteps.cpu().numpy()[keep], o["steps"][keep])
    np.testing.assert_array_equal(res.reward.cpu().numpy()[keep], o["ret"][keep])
    _, n2 = c.thetas()
    np.testing.assert_allclose(res.norm2.cpu().numpy(), n2, rtol=1e-12, atol=0)


# ---- 2. independence -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", [ROLLOUT_CASES[2], ROLLOUT_CASES[4]], ids=lambda s: "%s-R%d-L%d" % s[:3])
def test_rollout_runs_permutation_and_alone(eng, spec):
    c = _case(spec)
    g = c.runs(eng)
    order = list(np.random.RandomState(3).permutation(c.R)) if c.R > 2 else [1, 0]
    p = c.runs(eng, order)
    for k, r in enumerate(order):
        _same({key: a[k * c.L:(k + 1) * c.L] for key, a in p.items()},
              {key: a[r * c.L:(r + 1) * c.L] for key, a in g.items()}, "run %d at place %d" % (r, k))
    for r in range(c.R):
        _same(c.runs(eng, [r]), {key: a[r * c.L:(r + 1) * c.L] for key, a in g.items()}, "run %d alone" % r)


# ---- 3. the merge --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,L", [(1, 1), (1, 300), (5, 1), (5, 3), (5, 300)])
def test_obs_stats_merge_runs(eng, R, L):
    d = 6
    rs = np.random.RandomState(R * 1000 + L)
    mean = rs.randn(R * L, d).astype(np.float32)
    m2 = (rs.rand(R * L, d) * 5).astype(np.float32)
    cnt = rs.randint(0, 40, R * L).astype(np.int32)
    cnt[rs.rand(R * L) < 0.2] = 0
    if R > 1:
        cnt[L:2 * L] = 0        # run 1: every partial empty -> its accumulator stays as it is
    acc = [rs.randn(R, d).astype(np.float32), (rs.rand(R, d) * 3).astype(np.float32),
           rs.randint(0, 1000, R).astype(np.int64)]
    acc[2][0] = 0               # run 0 starts empty
    got = [_dev(a.copy()) for a in acc]
    eng.obs_stats_merge_runs(_dev(mean), _dev(m2), _dev(cnt), L, *got)
    for r in range(R):
        one = [_dev(acc[0][r].copy()), _dev(acc[1][r].copy()), _dev(acc[2][r:r + 1].copy())]
        sl = slice(r * L, (r + 1) * L)
        eng.obs_stats_merge(_dev(mean[sl]), _dev(m2[sl]), _dev(cnt[sl]), *one)
        for k in range(3):
            assert got[k][r].cpu().numpy().tobytes() == one[k].cpu().numpy().reshape(-1).tobytes(), (r, k)
    if R > 1:
        for k in range(3):
            assert got[k][1].cpu().numpy().tobytes() == acc[k][1].tobytes()


# ---- 4. the learner ------------------------------------------------------------------------------------------------
def _step(eng, table_d, P, pk, top="tensor", g=True):
    """One fdr_fd_step_runs launch over a packed batch -> (g [R, P], theta [R, P], out [R, 2]) on the host."""
    R = len(pk["pr"])
    theta = _dev(pk["theta"].copy())
    gd = torch.full((R, P), 123.0, dtype=torch.float64, device=DEV) if g else None
    out = torch.full((R, 2), 123.0, dtype=torch.float64, device=DEV)
    eng.fd_step_runs(table_d, _dev(pk["idx"]), _dev(pk["sign"]), _dev(pk["n2"]), _dev(pk["r"]), pk["stride"],
                     pk["n_train"], pk["lpd"], _dev(pk["sigma"]), theta, _dev(pk["lr"]), rr.LR_SCALE,
                     policy_reward=_dev(pk["pr"]), top_dirs=_dev(pk["top"]) if top == "tensor" else None, g=gd, out=out)
    torch.cuda.synchronize()
    return (None if gd is None else gd.cpu().numpy()), theta.cpu().numpy(), out.cpu().numpy()


def _table_dev(table):
    import test_gpu_learner_edges as edges
    return edges.dev_table(table)      # NaN-guarded: a read outside the table turns the result NaN


def _packed(shape, order=None):
    table, runs = rr.learner_batch(*shape)
    pk = rr.pack(runs, order)
    pk["lpd"] = shape[1]
    return table, runs, pk


@pytest.mark.parametrize("shape", rr.LEARNER_SHAPES, ids=lambda s: "D%d-lpd%d-P%d-R%d" % s[:4])
def test_fd_step_runs_against_the_restatement(eng, shape):
    D, lpd, P, R, _ = shape
    table, runs, pk = _packed(shape)
    g, theta, out = _step(eng, _table_dev(table), P, pk)
    worst = worst_upd = 0.0
    n_bits = 0
    for i, u in enumerate(runs):
        msg = "run %d (%s, b %r)" % (i, u.kind, u.b)
        if u.kind in rr.POISONED:
            assert np.all(np.isnan(g[i])), msg
            assert theta[i].tobytes() == u.theta.tobytes(), msg
            assert out[i, 0] == 0.0 and np.isnan(out[i, 1]), msg
            continue
        if u.kind == "zero":
            assert np.all(g[i] == 0.0) and theta[i].tobytes() == u.theta.tobytes() and np.all(out[i] == 0.0), msg
            continue
        e = ref.rel_l2(g[i], u.grad(table))
        assert e <= TOL, (msg, e)
        worst = max(worst, e)
        new, upd, norm, ambiguous = ref.dsgd_mirror(u.theta, g[i], u.lr, rr.LR_SCALE)
        assert out[i, 1] == norm or ambiguous, msg
        if not ambiguous:
            assert theta[i].tobytes() == new.tobytes(), msg
            n_bits += 1
            rel = abs(out[i, 0] - upd) / upd if upd > 0 else abs(out[i, 0])
            assert rel <= P * 2.0 ** -52, (msg, out[i, 0], upd)
            worst_upd = max(worst_upd, rel)
    print("fd_step_runs D %d lpd %d P %d R %d: worst g rel-L2 %.2e (tolerance %.0e), theta bit-equal to the mirror in "
          "%d runs, ||d theta|| relative %.2e" % (D, lpd, P, R, worst, TOL, n_bits, worst_upd))


@pytest.mark.parametrize("shape", [(3, 2, 8, 3, 0), (257, 2, 18, 3, 0), (2048, 2, 18, 2, 0)],
                         ids=lambda s: "D%d-P%d" % (s[0], s[2]))
def test_fd_step_runs_all_kept_is_the_null_form(eng, shape):
    """top_dirs[r] == D against top_dirs NULL: g, theta and out bit for bit (kinds zscore, top1 -> b forced to D)."""
    D, lpd, P, R, _ = shape
    table, runs, pk = _packed(shape)
    pk["top"] = np.full(R, D, np.int32)
    td = _table_dev(table)
    a, b = _step(eng, td, P, pk, "tensor"), _step(eng, td, P, pk, None)
    assert np.isfinite(a[0]).all()
    for x, y, what in zip(a, b, ("g", "theta", "out")):
        assert x.tobytes() == y.tobytes(), what


def test_fd_step_runs_permutation_and_alone(eng):
    shape = (257, 2, 18, 130, 0)
    table, runs, pk = _packed(shape)
    td = _table_dev(table)
    g, theta, out = _step(eng, td, 18, pk)
    order = list(np.random.RandomState(5).permutation(130))
    _, _, pp = _packed(shape, tuple(order))
    gp, tp, op = _step(eng, td, 18, pp)
    for k, r in enumerate(order):
        assert gp[k].tobytes() == g[r].tobytes() and tp[k].tobytes() == theta[r].tobytes() \
            and op[k].tobytes() == out[r].tobytes(), (k, r)
    for r in (0, 6, 7, 129):        # a run alone: R and the place do not enter its bits (6: nan, 7: b = 0)
        _, _, p1 = _packed(shape, (r,))
        g1, t1, o1 = _step(eng, td, 18, p1)
        assert g1[0].tobytes() == g[r].tobytes() and t1[0].tobytes() == theta[r].tobytes() \
            and o1[0].tobytes() == out[r].tobytes(), r
    # g is optional
    _, t2, o2 = _step(eng, td, 18, pk, g=False)
    assert t2.tobytes() == theta.tobytes() and o2.tobytes() == out.tobytes()


# ---- 5. the runner -------------------------------------------------------------------------------------------------
def _runner(**kw):
    from run_population import PopulationRunner
    base = dict(env_id="CartPole-v1", batch_size=16, episode_len=100, eval_lanes=4, normalize_obs=True,
                top_directions=8, device=DEV)
    base.update(kw)
    return PopulationRunner(**base)


def test_runner_position_independence(eng):
    a = _runner(seeds=[3, 7, 11]).train(3)
    b = _runner(seeds=[7]).train(3)
    assert a.thetas.shape == (3, 8) and b.thetas.shape == (1, 8)
    assert a.thetas[1].cpu().numpy().tobytes() == b.thetas[0].cpu().numpy().tobytes()
    assert np.any(a.thetas.cpu().numpy()[1] != 0)
    ha, hb = a.history, b.history
    for k in ha:
        assert tuple(ha[k].shape) == (3, 3) and tuple(hb[k].shape) == (3, 1)
        assert ha[k][:, 1].cpu().numpy().tobytes() == hb[k][:, 0].cpu().numpy().tobytes(), k
    assert np.all(ha["update_magnitude"].cpu().numpy() > 0)
    for k in range(3):
        assert a.obs_acc[k][1].cpu().numpy().tobytes() == b.obs_acc[k][0].cpu().numpy().tobytes()
    # the runs differ from each other
    assert a.thetas[0].cpu().numpy().tobytes() != a.thetas[1].cpu().numpy().tobytes()


def test_runner_honours_per_run_hyperparameters(eng):
    # seeds differ by construction (a seed is a run); two populations that differ in one run's learning rate only
    a = _runner(seeds=[5, 6], learning_rate=[0.01, 0.01]).train(1)
    b = _runner(seeds=[5, 6], learning_rate=[0.01, 0.03]).train(1)
    ta, tb = a.thetas.cpu().numpy(), b.thetas.cpu().numpy()
    assert ta[0].tobytes() == tb[0].tobytes() and ta[1].tobytes() != tb[1].tobytes()
    np.testing.assert_allclose(tb[1], 3 * ta[1], rtol=1e-5)      # theta starts at zero: one DSGD step scales with lr
    c = _runner(seeds=[5, 6], noise_std=[0.02, 0.05], top_directions=[8, 2]).train(1)
    tc = c.thetas.cpu().numpy()
    assert tc[0].tobytes() == ta[0].tobytes() and tc[1].tobytes() != ta[1].tobytes()


# ---- 6. no host synchronisation ------------------------------------------------------------------------------------
def _sync_mode_enforced():
    """Whether torch.cuda.set_sync_debug_mode("error") raises on a synchronising call on this build."""
    x = torch.ones(4, device=DEV)
    torch.cuda.synchronize()
    old = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        x.sum().item()
        return False
    except RuntimeError:
        return True
    finally:
        torch.cuda.set_sync_debug_mode(old)


def test_train_makes_no_host_sync(eng):
    if not _sync_mode_enforced():
        pytest.skip("this torch build does not enforce set_sync_debug_mode('error') on ROCm")
    r = _runner(seeds=[1, 2, 3])
    r.train(1)                              # first use: contexts, allocations
    torch.cuda.synchronize()
    old = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        r.train(3)
    finally:
        torch.cuda.set_sync_debug_mode(old)
    assert tuple(r.history["eval_mean"].shape) == (4, 3)
    assert np.isfinite(r.history["eval_mean"].cpu().numpy()).all()


# ---- 7. it learns --------------------------------------------------------------------------------------------------
def test_population_learns_cartpole(eng):
    """8 seeds of the README's ARS-V2 CartPole settings for 30 epochs, next to the solo SequentialRunner example for
    the same epochs: the population's median final eval return is at least half the solo run's (the factor covers
    the spread over seeds).  Measured on an MI355X: DESIGN.md 7."""
    from run_population import PopulationRunner
    from run_sequential import SequentialRunner
    epochs = 30
    pop = PopulationRunner(env_id="CartPole-v1", seeds=list(range(8)), top_directions=0.25, batch_size=256,
                           antithetic=True, normalize_obs=True, device=DEV).train(epochs)
    final = pop.history["eval_mean"][-1].cpu().numpy()
    solo = SequentialRunner(env_id="CartPole-v1", physics=True, policy="linear", normalize_obs=True, antithetic=True,
                            batch_size=256, weighting="top_directions", top_directions=0.25, noise_source="counter",
                            verbose=False)
    solo.train(epochs)
    # the solo run's final policy over 64 deterministic lanes under its own observation statistics (DESIGN.md 3.1.3's
    # measure), through the same kernel
    from run_population import obs_norm_from_stats
    om, osd = obs_norm_from_stats(solo.global_obs[0][None], solo.global_obs[1][None], solo.global_obs[2])
    theta = solo.policy.flat.detach().to(torch.float32).reshape(1, -1).contiguous()
    res = eng.rollout_runs(pop.spec, pop.env, theta, torch.zeros(1, dtype=torch.float32, device=DEV),
                           torch.zeros(1, dtype=torch.int64, device=DEV), 64, 12345, jiggle=False,
                           obs_mean_runs=om.contiguous(), obs_std_runs=osd.contiguous())
    solo_final = float(res.reward.mean().item())
    print("population final eval returns (8 seeds): %s; median %.2f; solo SequentialRunner final policy %.2f"
          % (np.array2string(final, precision=2), float(np.median(final)), solo_final))
    assert np.isfinite(final).all()
    assert float(np.median(final)) >= 0.5 * solo_final
