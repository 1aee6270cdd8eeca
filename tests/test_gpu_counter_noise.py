"""GPU: the counter-based noise source (fdr_noise_fill, utils.noise_sources.CounterNoiseSource) through every layer.

Kernel against the numpy restatement (tests/philox_ref.py, f64): for every element
    |eps_dev - eps_ref| <= 8 * 2^-24 * max(r_ref, 2^-24),      r_ref the element's Box-Muller radius.
Budget: logf <= 1 ulp (so -2 logf(u1) is off by <= 2^-23 relative away from u1 = 1, and sqrtf halves that), sqrtf
and the two multiplies correctly rounded (2^-24 each), sincospif <= 2 ulp on the exact argument 2 u2: at most
4 * 2^-24 * r in all; the test allows twice that.  A wrong Philox word changes an element completely, so the same
comparison pins the integer stream, the 32-bit carry of the row id and the key halves.  The measured maximum is
printed in units of 2^-24 r (DESIGN.md 7 records it).

Above the kernel: purity (a row alone = that row of a larger fill = the same id through `ids`), the device rows'
moments, Worker.evaluate bit for bit the fast path over the same buffer as a plain table, sharding, the learner (batch,
regenerated from ids, one epoch stale) against tests/learner_ref.py at the project's bounds (g rel-L2 1e-5, theta 1e-6
abs), the runner, and the reference interface."""
import numpy as np
import pytest
import torch

import learner_ref as LR
import philox_ref
from philox_ref import MOMENT_FIRST, MOMENT_P, MOMENT_ROWS, MOMENT_SEED

pytestmark = pytest.mark.gpu

SEEDS = (0, 123, 2 ** 63 + 5)
SHAPES = ((1, 1), (3, 3), (5, 5), (3, 1021), (2, 6092), (70000, 5))   # the last: more rows than a grid dimension holds
EXPLICIT_IDS = (0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 64 - 1, 7)
BOUND = 8.0            # in units of 2^-24 max(r_ref, 2^-24)
ULP = 2.0 ** -24
SIGMA = 0.02


def _dev():
    return torch.device("cuda", 0)


def _fill(seed, n_rows, P, stride=None, first_id=0, ids=None):
    from fdr import engine
    ids_d = None
    if ids is not None:
        ids_d = torch.from_numpy(np.array(ids, np.uint64).view(np.int64)).to(_dev())
    stride = (P + 3) // 4 * 4 if stride is None else stride
    out = engine.noise_fill(seed, n_rows, P, stride, ids=ids_d, first_id=first_id, device=_dev())
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(n_rows, stride)


def _err_units(dev_rows, seed, ids, stride):
    """max over the elements of |dev - ref| / (2^-24 max(r_ref, 2^-24))."""
    ref, r = philox_ref.rows(seed, ids, stride)
    assert np.isfinite(dev_rows).all()
    return float((np.abs(dev_rows.astype(np.float64) - ref) / (ULP * np.maximum(r, ULP))).max())


@pytest.mark.parametrize("first_id", [0, 2 ** 32 - 2])
@pytest.mark.parametrize("n_rows,P", SHAPES)
def test_kernel_matches_restatement(n_rows, P, first_id):
    stride = (P + 3) // 4 * 4
    ids = [first_id + k for k in range(n_rows)]
    worst = 0.0
    for seed in SEEDS:
        worst = max(worst, _err_units(_fill(seed, n_rows, P, first_id=first_id), seed, ids, stride))
    print("noise_fill %d x %d from id %d: max error %.3f x 2^-24 r" % (n_rows, P, first_id, worst))
    assert worst <= BOUND


@pytest.mark.parametrize("P", [5, 1021])
def test_kernel_matches_restatement_explicit_ids(P):
    stride = (P + 3) // 4 * 4
    worst = 0.0
    for seed in SEEDS:
        worst = max(worst, _err_units(_fill(seed, len(EXPLICIT_IDS), P, ids=EXPLICIT_IDS), seed, EXPLICIT_IDS, stride))
    print("noise_fill explicit ids x %d: max error %.3f x 2^-24 r" % (P, worst))
    assert worst <= BOUND


def test_row_stride_above_the_minimum_is_written_through():
    """include/fdr.h: every element of the stride is written and continues the row's stream."""
    wide = _fill(123, 3, 5, stride=16, first_id=2 ** 32 - 2)
    ids = [2 ** 32 - 2 + k for k in range(3)]
    assert _err_units(wide, 123, ids, 16) <= BOUND
    np.testing.assert_array_equal(wide[:, :8], _fill(123, 3, 5, first_id=2 ** 32 - 2))


def test_rows_are_pure_functions_of_seed_and_id():
    P, big = 1021, 40
    block = _fill(123, big, P, first_id=2 ** 32 - 20)
    for k in (0, 19, 20, 39):                       # both sides of the 32-bit carry
        d = 2 ** 32 - 20 + k
        np.testing.assert_array_equal(_fill(123, 1, P, first_id=d)[0], block[k])
    pick = [39, 0, 20, 19, 20]
    got = _fill(123, len(pick), P, ids=[2 ** 32 - 20 + k for k in pick])
    np.testing.assert_array_equal(got, block[pick])
    assert not np.array_equal(_fill(124, 1, P, first_id=2 ** 32 - 20)[0], block[0])


def test_device_rows_have_normal_moments():
    rows = _fill(MOMENT_SEED, MOMENT_ROWS, MOMENT_P, first_id=MOMENT_FIRST)
    assert rows.size == 1047824
    zm, zv, z4 = philox_ref.moments_z(rows)
    print("device moments (sigma units): mean %.2f  var %.2f  m4 %.2f" % (zm, zv, z4))
    assert abs(zm) <= 5 and abs(zv) <= 5 and abs(z4) <= 5


# ---- worker ---------------------------------------------------------------------------------------------------------
class _PlainTable(object):
    """A table source over a given device buffer (the SharedNoiseTable interface the Worker's fast path asks for)."""

    def __init__(self, buf):
        self.buf = buf

    def device_table(self, device=None):
        return self.buf

    def sample_batch(self, n):
        raise AssertionError("the test passes explicit lanes")


def _worker(kind, source, T=20):
    from envs import SyntheticEnv
    from policies import DiscretePolicy, MujocoPolicy
    from worker import Agent, Worker
    torch.manual_seed(124)
    pol = DiscretePolicy(4, 2, seed=124) if kind == "discrete" else MujocoPolicy(17, 6, seed=124)
    n_in, n_act = (4, 2) if kind == "discrete" else (17, 6)
    env = SyntheticEnv(n_in, n_act, kind == "discrete", T, env_seed=0, device=_dev())
    src = source(pol.num_params) if callable(source) else source
    w = Worker(pol, Agent(pol, env, random_seed=11), src, None, sigma=SIGMA, eval_prob=0.0, random_seed=3)
    w.epoch = 0
    return w, pol


def _counter(P, seed=123):
    from utils.noise_sources import CounterNoiseSource
    return CounterNoiseSource(P, random_seed=seed)


def _host(res_or_batch):
    torch.cuda.synchronize()
    b = res_or_batch
    return [t.cpu().numpy() for t in (b.reward, b.entropy, b.timesteps, b.norm2)]


@pytest.mark.parametrize("kind", ["mujoco", "discrete"])
def test_evaluate_is_the_fast_path_over_the_filled_rows(kind):
    """Worker.evaluate with a CounterNoiseSource = Worker.launch on a plain table source whose table is the same
    filled buffer, idx = row * row_stride: rewards, entropies, steps, norm2 bit for bit; so is a launch that adds an
    eval lane (idx 0, sign 0) through the `table=` route."""
    w, pol = _worker(kind, _counter)
    src = w.noise_source
    b = w.evaluate(8, antithetic=True, seed=5)
    assert b.noise_table.numel() == 8 * src.row_stride and src.next_id == 8
    assert b.encoded == [str(d) for d in range(8) for _ in range(2)]
    np.testing.assert_array_equal(b.idx_host, np.repeat(np.arange(8) * src.row_stride, 2))
    buf = src.rows(0, 8, _dev())
    assert torch.equal(buf, b.noise_table)
    wt, _ = _worker(kind, _PlainTable(buf))
    sign = np.tile(np.array([1, -1], np.int8), 8)
    res, _, _ = wt.launch(b.idx_host, sign, np.zeros(16, np.int8), seed=5, pairs=True)
    for got, want in zip(_host(b), _host(res)):
        np.testing.assert_array_equal(got, want)
    # 8 antithetic directions + 1 eval lane
    idx17 = np.concatenate([b.idx_host, [0]])
    sign17 = np.concatenate([sign, [0]]).astype(np.int8)
    det17 = (sign17 == 0).astype(np.int8)
    r_c, _, _ = w.launch(idx17, sign17, det17, seed=5, table=b.noise_table)
    r_t, _, _ = wt.launch(idx17, sign17, det17, seed=5)
    for got, want in zip(_host(r_c), _host(r_t)):
        np.testing.assert_array_equal(got, want)
    assert _host(r_c)[3][16] == 0.0


def test_evaluate_prefetch_and_repeat_calls():
    """prefetch=True has nothing to do and does not fail; a second call takes fresh ids and fresh rows, and the first
    batch's rows stay what they were."""
    w, _ = _worker("mujoco", _counter)
    b0 = w.evaluate(4, antithetic=True, seed=5, prefetch=True)
    keep = b0.noise_table.clone()
    b1 = w.evaluate(4, antithetic=True, seed=5, prefetch=True)
    assert b1.encoded[0] == "4" and w.noise_source.next_id == 8
    assert torch.equal(b0.noise_table, keep) and not torch.equal(b1.noise_table, keep)
    assert b0.idx.data_ptr() == b1.idx.data_ptr()          # the descriptors are uploaded once


def test_sharded_evaluate_concatenates_to_the_full_one():
    full_w, _ = _worker("mujoco", _counter)
    full = full_w.evaluate(8, antithetic=True, seed=5)
    rew, n2 = [], []
    for rng in ((0, 8), (8, 16)):
        w, _ = _worker("mujoco", _counter)
        b = w.evaluate(8, antithetic=True, seed=5, lane_range=rng)
        assert w.noise_source.next_id == 8 and len(b) == 8
        assert b.encoded == [str(d) for d in range(rng[0] // 2, rng[1] // 2) for _ in range(2)]
        h = _host(b)
        rew.append(h[0])
        n2.append(h[3])
    assert full_w.noise_source.next_id == 8
    fh = _host(full)
    np.testing.assert_array_equal(np.concatenate(rew), fh[0])
    np.testing.assert_array_equal(np.concatenate(n2), fh[3])


def test_collect_returns_encodes_ids_and_keeps_eval_lanes_unperturbed():
    w, _ = _worker("mujoco", _counter)
    w.eval_prob = 0.4
    rets = w.collect_returns(10)
    train = [r for r in rets if not r.is_eval]
    assert 0 < len(train) < 10
    assert [r.encoded_noise for r in train] == [str(k) for k in range(len(train))]
    assert all(r.encoded_noise == "0" and r.norm2 == 0.0 for r in rets if r.is_eval)
    assert w.noise_source.next_id == len(train)
    eps = w.noise_source.decode("0").astype(np.float32)
    z = (np.float32(SIGMA) * eps).astype(np.float32).astype(np.float64)
    assert abs(train[0].norm2 - float(np.dot(z, z))) <= 1e-9 * train[0].norm2


# ---- learner --------------------------------------------------------------------------------------------------------
def _learner(pol, src):
    from dsgd import DSGD
    from learner import FiniteDifferences
    from utils import AdaptiveOmega
    return FiniteDifferences(pol, DSGD(pol.parameters(), lr=0.01), AdaptiveOmega(), src, noise_std=SIGMA, batch_size=8,
                             max_delayed_return=10)


def _check_step(learner, pol, theta0, g_ref, what):
    opt = learner.gradient_optimizer
    g = learner.gradient_memory.cpu().numpy()
    rel = LR.rel_l2(g, g_ref)
    theta_ref = LR.dsgd_mirror(theta0, np.asarray(g_ref, np.float64), opt.lr, opt.lr_scale)[0]
    dth = float(np.abs(pol.get_trainable_flat().astype(np.float64) - theta_ref).max())
    print("%s: g rel-L2 %.2e, max |theta - ref| %.2e" % (what, rel, dth))
    assert rel <= 1e-5
    assert dth <= 1e-6


def test_learner_steps_from_batch_from_ids_and_one_epoch_stale():
    w, pol_a = _worker("mujoco", _counter)
    P = pol_a.num_params
    stride = w.noise_source.row_stride
    theta0 = pol_a.get_trainable_flat().copy()
    b = w.evaluate(8, antithetic=True, seed=5)
    rets = b.to_returns()
    torch.cuda.synchronize()
    table = b.noise_table.cpu().numpy()                 # the eps rows the kernels read
    rew, n2 = b.reward.cpu().numpy(), b.norm2.cpu().numpy()
    wz = LR.weights(rew, 0.0, "zscore")
    g_ref = LR.grad(table, P, np.arange(8) * stride, LR.coef_d(wz, b.sign_host, n2, 2, SIGMA))

    la = _learner(pol_a, w.noise_source)
    assert la.step(b, 0, 0, 0) > 0
    _check_step(la, pol_a, theta0, g_ref, "FDBatch")

    # a fresh same-seed learner, the rows regenerated from the returns' ids
    _, pol_b = _worker("mujoco", _counter)
    np.testing.assert_array_equal(pol_b.get_trainable_flat(), theta0)
    lb = _learner(pol_b, _counter(P))
    assert [r.encoded_noise for r in rets] == [str(d) for d in range(8) for _ in range(2)]
    assert lb.step(rets, 0, 0, 0) > 0
    _check_step(lb, pol_b, theta0, g_ref, "list[FDReturn]")
    # ... and an FDBatch that arrives with its ids and without its rows
    _, pol_c = _worker("mujoco", _counter)
    lc = _learner(pol_c, _counter(P))
    b.noise_table = None
    assert lc.step(b, 0, 0, 0) > 0
    _check_step(lc, pol_c, theta0, g_ref, "FDBatch without rows")

    # one epoch stale: the same returns again, now against theta_1 (lambda = fl32(+-fl32(sigma eps) + theta_0 - theta_1))
    theta1 = pol_b.get_trainable_flat().copy()
    drift = (theta0 - theta1).astype(np.float32)[None]
    assert lb.epoch == 1 and all(r.epoch == 0 for r in rets)
    idx = np.repeat(np.arange(8) * stride, 2)
    lam = LR.lambda_rows(table, P, idx, b.sign_host, np.zeros(16, np.int64), SIGMA, drift).astype(LR.LD)
    coef = wz / (lam * lam).sum(1)
    g_stale = (coef[:, None] * lam).sum(0)
    assert lb.step(rets, 0, 0, 0) > 0
    _check_step(lb, pol_b, theta1, g_stale, "one epoch stale")


# ---- runner, reference interface ----------------------------------------------------------------------------------------
def _run(seed, **kw):
    from run_sequential import SequentialRunner
    args = dict(env_id="CartPole-v1", noise_source="counter", antithetic=True, batch_size=8, episode_len=20,
                verbose=False, random_seed=seed)
    args.update(kw)
    run = SequentialRunner(**args)
    return run


def test_runner_trains_with_counter_noise():
    run = _run(123)
    run.train(3)
    assert len(run.history) == 3
    ids = np.concatenate([np.asarray(h["idx"]) for h in run.history])
    np.testing.assert_array_equal(ids, np.arange(24, dtype=np.uint64))
    theta = run.policy.get_trainable_flat().copy()
    again = _run(123)
    again.train(3)
    np.testing.assert_array_equal(again.policy.get_trainable_flat(), theta)
    other = _run(124)
    other.train(3)
    assert not np.array_equal(other.policy.get_trainable_flat(), theta)


def test_runner_mixed_objective_with_counter_noise():
    run = _run(123, env_id="SimpleTrapEnv-v0", objective="mixed", episode_len=None)
    run.train(2)
    assert len(run.history) == 2
    for h in run.history:
        assert np.isfinite(h["novelties"]).all() and np.isfinite(h["Noisy Novelty"])
        assert np.isfinite(h["Update Magnitude"]) and h["Update Magnitude"] > 0


def test_unknown_noise_source_names_the_choices():
    from run_sequential import SequentialRunner
    with pytest.raises(ValueError, match="counter"):
        SequentialRunner(env_id="CartPole-v1", noise_source="nope", verbose=False)


def test_sample_equals_decode_bit_for_bit():
    src = _counter(1021)
    src.next_id = 2 ** 32 - 1                         # then 2^32: the id's high word
    for want in (2 ** 32 - 1, 2 ** 32):
        enc, vec = src.sample()
        assert enc == str(want) and vec.dtype == np.float64 and vec.shape == (1021,)
        np.testing.assert_array_equal(vec, src.decode(enc))
        np.testing.assert_array_equal(vec.astype(np.float32), _fill(123, 1, 1021, first_id=want)[0, :1021])
