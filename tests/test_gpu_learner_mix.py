"""The mixed objective (reward / novelty / entropy weights: fd_grad_fused_mix_kernel, fd_weights_mix_kernel, their C
entry points, FiniteDifferences(objective="mixed"), SequentialRunner(objective="mixed")) against the extended-precision
restatement tests/learner_mix.py, on the cases of tests/learner_cases.py with the channels tests/learner_mix.py draws.

Tolerance: the project's rel-L2 1e-12 for f64 kernels against the longdouble reference; bitwise where the same kernel
runs on the same inputs (coefficients (1, 0, 0) against the z-score instance, the runner's step against the step run by
hand).  Device tables are NaN-guarded as in tests/test_gpu_learner_edges.py: a read outside the table turns the result
NaN, a broken guard yields a wrong number inside the allocation, never a fault.

Worst measured on an MI355X (each test prints its own), next to the tolerance:
    fused mix, small grid, lanes_per_dir 1 / 3 / 4 / 5 / 7     1.1e-14 / 2.3e-15 / 2.4e-15 / 9.1e-15 / 4.7e-14   1e-12
    per-channel std == 0                                       2.7e-16                            1e-12
    statistics tail (n_all 1 .. 4608) / beyond the window      3.9e-16 / 2.0e-16                  1e-12
    fd_step_mix g                                              4.2e-16                            1e-12
    fd_weights_mix coefficients / through fd_grad_lambda       2.9e-15 / 2.6e-16                  1e-12
    learner: g / list route / one-epoch-old returns            2.4e-16 / 2.7e-16 / 3.0e-16        1e-12
    sharded, 2 ranks against one process (ranks bitwise equal) 1.5e-8                             1e-6
    (1, 0, 0) with NaN / NULL channels, theta after fd_step_mix, the runner's step    bit-equal
The list route is not bitwise the batch route: a list has no pairing, so its 80 returns are 80 directions of one lane
where the batch has 40 of two, and the column sums run in another order.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import learner_cases as lc
import learner_mix as lm
import learner_ref as ref
from learner_cases import PR, SIGMA
from test_gpu_learner_edges import Dev, _bad_dirs, dev, dev_table, what

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12
NAN = float("nan")
LD = np.longdouble
POL = lm.policy_values()


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from fdr import engine
    return engine


def chan(d, nov, ent):
    """(reward, novelty, entropy) device arrays of a Dev; None stays None (NULL at the C boundary)."""
    return (d.r_all, None if nov is None else dev(nov), None if ent is None else dev(ent))


def run_mix(eng, c, d, coefs, nov, ent, rewards=True):
    ch = chan(d, nov, ent)
    if not rewards:
        ch = (None,) + ch[1:]
    return eng.fd_grad_fused_mix(d.table, d.idx, ch, POL, coefs, c.lane_lo, d.sign, d.n2, c.lpd, SIGMA,
                                 c.P).cpu().numpy()


def mix_error(c, out, coefs, nov, ent, cols=None):
    sel = slice(None) if cols is None else cols
    assert out.size == c.P
    return ref.rel_l2(out[sel], ref.grad(c.table, c.P, c.idx_dirs, lm.mix_coefs(c, coefs, nov, ent), cols))


# ---- 1. the fused kernel over the small grid ---------------------------------------------------------------------
@pytest.mark.parametrize("coefs", lm.COEF_SETS)
@pytest.mark.parametrize("lpd", lc.FUSED_LPD)
def test_fused_mix_small_grid(eng, lpd, coefs):
    """lanes_per_dir 1 (the register path), 3 .. 7 (the path above kMixLpd), lane_lo > 0, sign-0 lanes with n2 = 0,
    all-equal returns, table_size == P, the chunk seams 63 / 64 / 65 / 130."""
    assert lc.fused_plan(65, 1000) == lc.PLAN_TABLE[(65, 1000)] and lc.fused_plan(130, 257) == lc.PLAN_TABLE[(130, 257)]
    worst = 0.0
    for c in lc.grid_cases((lpd,)):
        nov, ent, _, _ = lm.channels(c, coefs)
        e = mix_error(c, run_mix(eng, c, Dev(c), coefs, nov, ent), coefs, nov, ent)
        assert e <= TOL, (what(c), coefs, e)
        worst = max(worst, e)
    print("fused mix %r, lpd %d: worst rel-L2 %.2e (tolerance %.0e)" % (coefs, lpd, worst, TOL))


# ---- 2. reward only is the z-score instance, bit for bit ---------------------------------------------------------
@pytest.mark.parametrize("n_dirs,P,lpd", [(1, 1, 1), (67, 257, 1), (130, 1000, 2), (65, 1000, 3), (67, 257, 5),
                                          (4097, 300, 1), (2304, 1500, 2)])
def test_reward_only_is_bitwise_the_zscore_instance(eng, n_dirs, P, lpd):
    """Coefficients (1, 0, 0): the inactive channels full of NaN, then NULL.  (4097, 300) and (2304, 1500): n_all past
    both kernels' register-held counts (1024 and 4096), so the tails are compared too."""
    c = lc.make_case(n_dirs, P, lpd)
    d = Dev(c)
    want = eng.fd_grad_fused(d.table, d.idx, d.r_all, PR, c.lane_lo, d.sign, d.n2, lpd, SIGMA, P).cpu().numpy()
    assert not np.isnan(want).any()
    nan = np.full(c.n_all, NAN)
    for nov, ent in ((nan, nan), (None, None)):
        got = run_mix(eng, c, d, (1.0, 0.0, 0.0), nov, ent)
        assert got.tobytes() == want.tobytes(), "%d of %d differ" % ((got != want).sum(), P)
    coef = eng.fd_weights_mix(chan(d, None, None), POL, (1.0, 0.0, 0.0), c.lane_lo, d.sign, d.n2, lpd, SIGMA)
    staged = eng.fd_weights(d.r_all, PR, c.lane_lo, d.sign, d.n2, lpd, SIGMA)
    assert coef.cpu().numpy().tobytes() == staged.cpu().numpy().tobytes()


# ---- 3. a channel whose std is 0 ---------------------------------------------------------------------------------
@pytest.mark.parametrize("lpd", [1, 2, 3])
def test_constant_channels(eng, lpd):
    worst = 0.0
    coefs = lm.COEF_SETS[0]
    c = lc.make_case(67, 257, lpd)
    nov, ent, _, _ = lm.channels(c, coefs)
    flat = np.full(c.n_all, 0.45)           # novelty all equal: z_n = x_n on every lane
    eq = lc.make_case(67, 257, lpd, returns="equal")
    runs = [(c, coefs, flat, ent, True),
            (eq, coefs, np.full(eq.n_all, 0.45), np.full(eq.n_all, 1.5), True),   # all three channels constant
            (c, (0.0, 1.0, 0.0), nov, None, False)]                               # omega = 1, rewards NULL
    for case, a, nv, en, rewards in runs:
        assert lm.mix_kappa(case, a, nv, en) <= lc.KAPPA_MAX
        e = mix_error(case, run_mix(eng, case, Dev(case), a, nv, en, rewards), a, nv, en)
        assert e <= TOL, (what(case), a, e)
        worst = max(worst, e)
    print("constant channels, lpd %d: worst rel-L2 %.2e (tolerance %.0e)" % (lpd, worst, TOL))


# ---- 4. / 5. the statistics: the tail past the registers, lanes of other ranks -----------------------------------
@pytest.mark.parametrize("n_dirs", [1, 2, 255, 256, 257, 1023, 1024, 1025, 2047, 2049, 4095, 4096, 4097])
def test_statistics_tail(eng, n_dirs):
    """n_all = n_dirs on both sides of every multiple of the workgroup the register-held count could be."""
    coefs = lm.COEF_SETS[0]
    c = lc.make_case(n_dirs, 257, 1)
    assert c.n_all == n_dirs
    nov, ent, _, _ = lm.channels(c, coefs)
    e = mix_error(c, run_mix(eng, c, Dev(c), coefs, nov, ent), coefs, nov, ent)
    print("statistics tail, n_all %d: rel-L2 %.2e (tolerance %.0e)" % (n_dirs, e, TOL))
    assert e <= TOL


def test_statistics_tail_antithetic_4608(eng):
    c = lc.make_case(2304, 1500, 2)
    assert c.n_all == 4608 and lc.fused_plan(2304, 1500) == lc.PLAN_TABLE[(2304, 1500)]
    worst = 0.0
    d = Dev(c)
    for coefs in lm.COEF_SETS:
        nov, ent, _, _ = lm.channels(c, coefs)
        out = run_mix(eng, c, d, coefs, nov, ent)
        np.testing.assert_array_equal(run_mix(eng, c, d, coefs, nov, ent), out)   # the tickets were left at zero
        worst = max(worst, mix_error(c, out, coefs, nov, ent))
    print("statistics tail, n_all 4608 (lpd 2): worst rel-L2 %.2e (tolerance %.0e)" % (worst, TOL))
    assert worst <= TOL


@pytest.mark.parametrize("n_dirs,lpd,lo,n_all", lc.N_ALL_CASES)
def test_statistics_beyond_the_local_window(eng, n_dirs, lpd, lo, n_all):
    c = lc.make_case(n_dirs, 257, lpd, lane_lo=lo, n_all=n_all)
    worst = 0.0
    for coefs in lm.COEF_SETS:
        nov, ent, _, _ = lm.channels(c, coefs)
        worst = max(worst, mix_error(c, run_mix(eng, c, Dev(c), coefs, nov, ent), coefs, nov, ent))
    print("n_all %d, window [%d, +%d): worst rel-L2 %.2e (tolerance %.0e)" % (n_all, lo, n_dirs * lpd, worst, TOL))
    assert worst <= TOL


# ---- 6. out-of-range offsets -------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", ["past", "negative"])
@pytest.mark.parametrize("lpd", [2, 5])
def test_bad_offset_poisons_the_gradient_only(eng, lpd, bad):
    """One bad row among 130 (3 chunks; the bad one in the second): g is NaN everywhere, the table's NaN guard shows
    nothing was read outside it on the clean call that follows on the same workspace."""
    coefs = lm.COEF_SETS[0]
    c = lc.make_case(130, 1000, lpd)
    assert lc.fused_plan(130, 1000)[2] == 3
    nov, ent, _, _ = lm.channels(c, coefs)
    good, poisoned = Dev(c), Dev(c, _bad_dirs(c, 70, bad))
    assert np.all(np.isnan(run_mix(eng, c, poisoned, coefs, nov, ent)))
    assert mix_error(c, run_mix(eng, c, good, coefs, nov, ent), coefs, nov, ent) <= TOL


def test_nan_in_an_active_channel_poisons_g(eng):
    coefs = lm.COEF_SETS[0]
    c = lc.make_case(65, 257, 1)
    nov, ent, _, _ = lm.channels(c, coefs)
    bad = ent.copy()
    bad[c.n_all - 1] = NAN
    assert np.all(np.isnan(run_mix(eng, c, Dev(c), coefs, nov, bad)))


# ---- 7. fd_step_mix ----------------------------------------------------------------------------------------------
def check_step(theta0, g_used, theta_dev, out, hist):
    """theta and theta_hist bit-equal to the mirror fed the kernel's own g, out = (||d theta||, the mirror's norm);
    a norm the mirror calls ambiguous (its f32 rounding depends on the summation order) is not compared."""
    P = theta0.size
    new, upd, norm, ambiguous = ref.dsgd_mirror(theta0, g_used, lc.DSGD_LR, lc.DSGD_SCALE)
    got = theta_dev.cpu().numpy()
    assert hist.cpu().numpy().tobytes() == got.tobytes()
    if ambiguous:
        print("norm ambiguous at P %d: theta and out[1] not compared" % P)
        return
    assert out[1] == norm
    assert got.tobytes() == new.tobytes(), "theta differs from the mirror in %d of %d" % ((got != new).sum(), P)
    assert abs(out[0] - upd) <= P * 2.0 ** -52 * upd


@pytest.mark.parametrize("n_dirs,P", [(3, 1), (3, 257), (3, 1000), (1600, 40000)])
def test_fd_step_mix(eng, n_dirs, P):
    """(1600, 40000): rows_per_chunk 320, further directions per thread.  Two steps on the same workspace."""
    coefs = lm.COEF_SETS[0]
    c = lc.make_case(n_dirs, P, 2)
    assert c.lane_lo == 0 and c.n_all == c.n_local
    if P == 40000:
        assert lc.fused_plan(n_dirs, P) == lc.PLAN_TABLE[(n_dirs, P)] and lc.fused_plan(n_dirs, P)[1] > 256
    nov, ent, _, _ = lm.channels(c, coefs)
    d = Dev(c)
    cols = None if n_dirs * P <= (1 << 22) else lc.big_cols(P)
    g_ref = ref.grad(c.table, P, c.idx_dirs, lm.mix_coefs(c, coefs, nov, ent), cols)
    theta = lc.dsgd_inputs(P)[0]
    t = dev(theta)
    for _ in range(2):
        g = torch.full((P,), NAN, dtype=torch.float64, device="cuda")
        hist = torch.full((P,), NAN, dtype=torch.float32, device="cuda")
        out = eng.fd_step_mix(d.table, d.idx, chan(d, nov, ent), POL, coefs, d.sign, d.n2, 2, SIGMA, t, lc.DSGD_LR,
                              lc.DSGD_SCALE, g=g, theta_hist=hist).cpu().numpy()
        gd = g.cpu().numpy()
        e = ref.rel_l2(gd if cols is None else gd[cols], g_ref)
        assert e <= TOL, e
        check_step(theta, gd, t, out, hist)
        theta = t.cpu().numpy()
    print("fd_step_mix (%d, %d): g rel-L2 %.2e (tolerance %.0e)" % (n_dirs, P, e, TOL))


# ---- 8. the staged weighting -------------------------------------------------------------------------------------
@pytest.mark.parametrize("coefs", lm.COEF_SETS)
@pytest.mark.parametrize("lpd", lc.STAGED_LPD)
def test_fd_weights_mix_small_grid(eng, lpd, coefs):
    worst = 0.0
    for c in lc.grid_cases((lpd,)):
        nov, ent, _, _ = lm.channels(c, coefs)
        d = Dev(c)
        coef = eng.fd_weights_mix(chan(d, nov, ent), POL, coefs, c.lane_lo, d.sign, d.n2, c.lpd, SIGMA).cpu().numpy()
        e = ref.rel_l2(coef, lm.mix_coefs(c, coefs, nov, ent))
        assert e <= TOL, (what(c), coefs, e)
        worst = max(worst, e)
    print("fd_weights_mix %r, lpd %d: worst rel-L2 %.2e (tolerance %.0e)" % (coefs, lpd, worst, TOL))


def test_fd_weights_mix_through_grad_lambda(eng):
    """The delayed-return route: coefficients of fd_weights_mix (sign 1, sigma 1, one lane per direction) into
    fd_grad_lambda with drift slots, against lambda_rows and the reference weights."""
    n, P = 67, 257
    coefs = lm.COEF_SETS[0]
    table, idx, sign, slot, drift, r = lc.lambda_case(n, P)
    rs = np.random.RandomState(991)
    nov, ent = 0.3 * np.abs(rs.randn(n)), 1.4 + 0.05 * rs.randn(n)
    tab, di, ds, dl, dd = dev_table(table), dev(idx), dev(sign), dev(slot), dev(drift)
    n2 = eng.fd_lambda_norms(tab, di, ds, dl, SIGMA, dd, P)
    n2h = n2.cpu().numpy()
    case = lc.Case(n_dirs=n, P=P, lpd=1, lane_lo=0, n_all=n, r_all=r, sign=np.ones(n, np.int8), n2=n2h)
    assert lm.mix_kappa(case, coefs, nov, ent) <= lc.KAPPA_MAX
    ones = torch.ones(n, dtype=torch.int8, device="cuda")
    coef = eng.fd_weights_mix((dev(r), dev(nov), dev(ent)), POL, coefs, 0, ones, n2, 1, 1.0)
    g = eng.fd_grad_lambda(tab, di, ds, dl, coef, SIGMA, dd, P).cpu().numpy()
    w = lm.mix_weights_arrays((r, nov, ent), POL, coefs) / n2h.astype(LD)
    lam = ref.lambda_rows(table, P, idx, sign, slot, SIGMA, drift).astype(LD)
    e = max(ref.rel_l2(coef.cpu().numpy(), w), ref.rel_l2(g, (w[:, None] * lam).sum(0)))
    print("fd_weights_mix -> fd_grad_lambda: rel-L2 %.2e (tolerance %.0e)" % (e, TOL))
    assert e <= TOL


# ---- 9. refusals -------------------------------------------------------------------------------------------------
def test_refusals(eng):
    from fdr._lib import FDRError
    c = lc.make_case(3, 257, 2)
    nov, ent, _, _ = lm.channels(c, lm.COEF_SETS[0])
    d = Dev(c)
    ch = chan(d, nov, ent)
    theta = dev(lc.dsgd_inputs(257)[0])

    def fused(channels, coefs):
        return eng.fd_grad_fused_mix(d.table, d.idx, channels, POL, coefs, 0, d.sign, d.n2, 2, SIGMA, c.P)

    def step(channels, coefs, sign=d.sign, n2=d.n2, idx=d.idx):
        return eng.fd_step_mix(d.table, idx, channels, POL, coefs, sign, n2, 2, SIGMA, theta, 0.01, 0.5)

    def weights(channels, coefs):
        return eng.fd_weights_mix(channels, POL, coefs, 0, d.sign, d.n2, 2, SIGMA)

    for call in (fused, step, weights):
        with pytest.raises(FDRError, match="all three coefficients"):
            call(ch, (0.0, 0.0, 0.0))
        with pytest.raises(FDRError, match="not finite"):
            call(ch, (0.6, NAN, 0.05))
        with pytest.raises(FDRError, match="not finite"):
            call(ch, (float("inf"), 0.4, 0.05))
        with pytest.raises(FDRError, match="active channel's array is NULL"):
            call((ch[0], None, ch[2]), (0.6, 0.4, 0.05))
        with pytest.raises(FDRError, match="active channel's array is NULL"):
            call((None, ch[1], None), (0.6, 0.4, 0.0))
    with pytest.raises(FDRError, match="fdr_fd_grad_fused_mix / fdr_fd_step_mix"):
        eng.fd_grad_fused(d.table, d.idx, d.r_all, PR, 0, d.sign, d.n2, 2, SIGMA, c.P, mode="zscore_mix")
    with pytest.raises(FDRError, match="fdr_fd_grad_fused_mix / fdr_fd_step_mix"):
        eng.fd_step(d.table, d.idx, d.r_all, PR, d.sign, d.n2, 2, SIGMA, theta, 0.01, 0.5, mode="zscore_mix")
    with pytest.raises(FDRError, match="single-process"):       # n_all (6) != n_local (4)
        step(ch, lm.COEF_SETS[0], sign=d.sign[:4], n2=d.n2[:4], idx=d.idx[:4])
    assert theta.cpu().numpy().tobytes() == lc.dsgd_inputs(257)[0].tobytes()     # no refused call moved theta
    assert mix_error(c, fused(ch, lm.COEF_SETS[0]).cpu().numpy(), lm.COEF_SETS[0], nov, ent) <= TOL


# ---- 10. the learner ---------------------------------------------------------------------------------------------
LEARNER_P_SEED = 124


def make_learner(objective, omega=0.0, ent_coef=0.0, weighting="zscore"):
    from dsgd import DSGD
    from learner import FiniteDifferences
    from policies import MujocoPolicy
    from utils import AdaptiveOmega, SharedNoiseTable
    torch.manual_seed(LEARNER_P_SEED)   # the policy's default-init draws (the biases) come from torch's generator
    policy = MujocoPolicy(17, 6, seed=LEARNER_P_SEED, device=torch.device("cuda", 0))
    table = SharedNoiseTable(1 << 16, policy.num_params, random_seed=3)
    om = AdaptiveOmega(default_value=omega, min_value=omega, max_value=omega)
    return FiniteDifferences(policy, DSGD(policy.parameters(), lr=0.01), om, table, noise_std=SIGMA, ent_coef=ent_coef,
                             objective=objective, weighting=weighting)


def learner_case(P, step, n_dirs=40):
    """An antithetic batch on the learner's own table shape (every lane used), with its channels."""
    rs = np.random.RandomState(5000 + 17 * step)
    room = (1 << 16) - P
    idx_dirs = rs.randint(0, room + 1, size=n_dirs).astype(np.int64)
    r = rs.randn(2 * n_dirs) * 3 + 1
    nov, ent = 0.3 * np.abs(rs.randn(2 * n_dirs)), 1.4 + 0.05 * rs.randn(2 * n_dirs)
    return lc.Case(n_dirs=n_dirs, P=P, lpd=2, lane_lo=0, n_all=2 * n_dirs, idx_dirs=idx_dirs, idx=np.repeat(idx_dirs, 2),
                   sign=np.tile(np.array([1, -1], np.int8), n_dirs), r_all=r, nov=nov, ent=ent, max_idx=room)


def learner_batch(learner, c):
    from learner import FDBatch
    table = learner.noise_source._table
    if not hasattr(c, "n2"):
        c.table = table
        c.n2 = np.repeat(ref.norms(table, c.P, c.idx_dirs, SIGMA), 2)
    return FDBatch(dev(c.r_all), dev(c.ent), torch.zeros(c.n_all, dtype=torch.int32, device="cuda"), dev(c.n2),
                   dev(c.idx), dev(c.sign), c.idx, c.sign, learner.epoch, lanes_per_dir=2, novelty=dev(c.nov))


def test_learner_mixed_with_zero_omega_is_the_reward_step(eng):
    a, b = make_learner("reward"), make_learner("mixed")
    assert a.policy.flat.cpu().numpy().tobytes() == b.policy.flat.cpu().numpy().tobytes()
    P = a.policy.num_params
    for step in range(3):
        c = learner_case(P, step)
        ua = a.step(learner_batch(a, c), PR, 0.2, 1.3)
        ub = b.step(learner_batch(b, c), PR, 0.2, 1.3)
        assert ua == ub and ua > 0 and b.last_mix == (1.0, 0.0, 0.0)
    assert a.policy.flat.cpu().numpy().tobytes() == b.policy.flat.cpu().numpy().tobytes()
    assert a.epoch == b.epoch == 3


def test_learner_mixed_gradient_and_routes(eng):
    """omega 0.4, ent_coef 0.05: g against the reference; the list-of-FDReturn route against the FDBatch route; then
    the same returns again one epoch old (the drift route: fd_lambda_norms, fd_weights_mix, fd_grad_lambda)."""
    a, b = make_learner("mixed", 0.4, 0.05), make_learner("mixed", 0.4, 0.05)
    P = a.policy.num_params
    c = learner_case(P, 0)
    coefs = (1.0 - 0.4, 0.4, 0.05)
    batch = learner_batch(a, c)
    assert lm.mix_kappa(c, coefs, c.nov, c.ent) <= lc.KAPPA_MAX
    theta0 = a.policy.flat.cpu().numpy().copy()
    assert a.step(batch, *POL) > 0 and a.last_mix == coefs
    g_ref = ref.grad(c.table, P, c.idx_dirs, lm.mix_coefs(c, coefs, c.nov, c.ent))
    e_g = ref.rel_l2(a.gradient_memory.cpu().numpy(), g_ref)
    rets = learner_batch(b, c).to_returns()
    for r in rets:
        r.epoch = b.epoch
    assert b.step(rets, *POL) > 0
    e_list = ref.rel_l2(b.gradient_memory.cpu().numpy(), a.gradient_memory.cpu().numpy())
    assert a.policy.flat.cpu().numpy().tobytes() == b.policy.flat.cpu().numpy().tobytes()
    # one epoch old: lambda_i = fl32(sign fl32(sigma eps_i) + (theta_0 - theta_1))
    theta1 = b.policy.flat.cpu().numpy().copy()
    for r in rets:
        r.epoch = b.epoch - 1
        r.norm2 = None
    assert b.step(rets, *POL) > 0
    n = c.n_all
    lam = ref.lambda_rows(c.table, P, c.idx, c.sign, np.zeros(n, np.int32), SIGMA, (theta0 - theta1)[None]).astype(LD)
    w = lm.mix_weights_arrays((c.r_all, c.nov, c.ent), POL, coefs) / (lam * lam).sum(1)
    e_stale = ref.rel_l2(b.gradient_memory.cpu().numpy(), (w[:, None] * lam).sum(0))
    print("learner mixed: g rel-L2 %.2e, list route vs batch route %.2e, one-epoch-old returns %.2e (tolerance %.0e)"
          % (e_g, e_list, e_stale, TOL))
    assert max(e_g, e_list, e_stale) <= TOL


def test_learner_refuses_what_is_not_built(eng):
    with pytest.raises(ValueError, match="centred_rank"):
        make_learner("mixed", weighting="centred_rank")
    with pytest.raises(ValueError, match="objective"):
        make_learner("novelty")
    a = make_learner("mixed", 0.4)
    batch = learner_batch(a, learner_case(a.policy.num_params, 0))
    batch.novelty = None
    theta = a.policy.flat.cpu().numpy().copy()
    with pytest.raises(ValueError, match="novelty"):
        a.step(batch, *POL)
    assert a.policy.flat.cpu().numpy().tobytes() == theta.tobytes() and a.epoch == 0


# ---- 11. sharded -------------------------------------------------------------------------------------------------
def test_two_ranks_equal_one_process(tmp_path):
    script = os.path.join(ROOT, "tools", "dist_check_mix.py")
    out = str(tmp_path)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    limit = ["timeout", "-k", "10", "150"]      # each child under its own limit
    p = subprocess.run(limit + [sys.executable, script, "single", out], cwd=ROOT, env=env, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    p = subprocess.run(limit + [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                                "--master-addr", "127.0.0.1", "--master-port", "29561", script, "multi", out],
                       cwd=ROOT, env=env, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import dist_check_mix
    finally:
        sys.path.pop(0)
    err = dist_check_mix.compare(out)       # asserts the ranks bitwise equal
    assert err <= 1e-6, err
    u1, u0 = np.load(os.path.join(out, "upd_single.npy")), np.load(os.path.join(out, "upd_rank0.npy"))
    np.testing.assert_array_equal(u0, np.load(os.path.join(out, "upd_rank1.npy")))
    np.testing.assert_allclose(u0, u1, rtol=1e-6)
    assert np.all(u0 > 0)


# ---- 12. the runner ----------------------------------------------------------------------------------------------
RUNNER_ENVS = [("SimpleTrapEnv-v0", False), ("CartPole-v1", True)]


def make_runner(env_id, physics, objective, **kw):
    from run_sequential import SequentialRunner
    return SequentialRunner(env_id=env_id, physics=physics, objective=objective, batch_size=8, episode_len=20,
                            noise_table_size=1 << 16, eval_prob=0.3, verbose=False, **kw)


@pytest.mark.parametrize("env_id,physics", RUNNER_ENVS)
def test_runner_mixed_defaults_are_the_reward_run(eng, env_id, physics):
    """omega 0 and ent_coef 0: coefficients (1, 0, 0), theta bit-equal after 3 epochs.  omega starts at 0 by default
    but AdaptiveOmega (default maximum 1) raises it by 1 / steps_to_max at the first eval episode that shows no
    improvement, so "omega 0" is held by omega_max_value = 0; with the literal defaults the recorded coefficients
    follow the epoch's omega."""
    a, b = make_runner(env_id, physics, "reward", omega_max_value=0), make_runner(env_id, physics, "mixed",
                                                                                   omega_max_value=0)
    a.train(3)
    b.train(3)
    assert len(a.history) == len(b.history) == 3
    assert all(h["coefs"] == (1.0, 0.0, 0.0) for h in b.history) and "coefs" not in a.history[0]
    assert a.policy.get_trainable_flat().tobytes() == b.policy.get_trainable_flat().tobytes()
    d = make_runner(env_id, physics, "mixed")
    d.train(3)
    assert len(d.history) == 3
    assert all(h["coefs"] == (1.0 - h["Omega"], h["Omega"], 0.0) for h in d.history)


@pytest.mark.parametrize("env_id,physics", RUNNER_ENVS)
def test_runner_mixed_step_is_fd_step_mix_on_the_recorded_channels(eng, env_id, physics, monkeypatch):
    """omega pinned at 0.5, ent_coef 0.01: the first epoch's theta is bit-equal to engine.fd_step_mix run by hand on a
    copy of the initial theta from the epoch's recorded idx, rewards, novelties, entropies and coefficients (the same
    kernel on the same inputs: the wiring, no tolerance), and differs from the reward-only run's."""
    kw = dict(omega_default_value=0.5, omega_min_value=0.5, omega_max_value=0.5, ent_coef=0.01)
    r = make_runner(env_id, physics, "mixed", **kw)
    theta0 = r.policy.flat.detach().clone()
    seen = {}
    real = eng.fd_step_mix

    def spy(table, idx_local, channels, policy_values, coefs, sign_local, norm2_local, lanes_per_dir, sigma, theta, lr,
            lr_scale, **kwargs):
        if not seen:    # what the history does not record: ||lambda||^2 from the rollout, and the learning rate
            seen.update(n2=norm2_local.clone(), lr=lr, lr_scale=lr_scale, lpd=lanes_per_dir, sigma=sigma,
                        on_device=all(c.is_cuda for c in channels))
        return real(table, idx_local, channels, policy_values, coefs, sign_local, norm2_local, lanes_per_dir, sigma,
                    theta, lr, lr_scale, **kwargs)

    monkeypatch.setattr(eng, "fd_step_mix", spy)
    r.train(1)
    assert len(r.history) == 1 and seen["on_device"] and seen["lpd"] == 1
    h = r.history[0]
    assert h["coefs"] == (0.5, 0.5, 0.01) and h["Omega"] == 0.5
    n = len(h["rewards"])
    assert n == 8 and len(h["novelties"]) == len(h["entropies"]) == len(h["idx"]) == n
    theta = theta0.clone()
    real(r.noise_source.device_table(theta.device), dev(np.asarray(h["idx"], np.int64)),
         (dev(h["rewards"]), dev(h["novelties"]), dev(h["entropies"])), h["policy_values"], h["coefs"],
         torch.ones(n, dtype=torch.int8, device="cuda"), seen["n2"], 1, seen["sigma"], theta, seen["lr"],
         seen["lr_scale"])
    got = r.policy.flat.cpu().numpy()
    assert got.tobytes() == theta.cpu().numpy().tobytes()
    assert got.tobytes() != theta0.cpu().numpy().tobytes()
    q = make_runner(env_id, physics, "reward", **kw)
    q.train(1)
    assert np.array_equal(q.history[0]["rewards"], h["rewards"])      # the same rollouts ...
    assert q.policy.flat.cpu().numpy().tobytes() != got.tobytes()     # ... weighted differently
