"""rollout_pair_kernel's step loop against the oracle and the one-lane kernel, at the episode lengths where the
draw batches (5 steps of 6 dims for the cheetah shape) and the work placed in the two LDS hand-off waits can go
wrong: no full batch, exactly one, one plus a remainder, several with remainders 0 / 1 / 3 -- and, with the next
batch drawn one batch ahead, a draw that runs past T in every case.  Odd L leaves a wave with an idle half.

Tolerances are those of test_gpu_kernels.py::test_rollout_pair_and_single_kernels_agree (DESIGN.md "Parity").
"""
import numpy as np
import pytest
import torch

from oracle import agent as oagent
from oracle import envs as oenvs
from oracle import noise as onoise
from oracle import policies as opol

pytestmark = pytest.mark.gpu

DEV = "cuda"
SHAPES = {"cartpole": ("discrete", 4, 2), "cheetah": ("mujoco", 17, 6), "hopper": ("mujoco", 11, 3)}
T_SET = [1, 4, 5, 6, 10, 11, 23]


@pytest.fixture(scope="module")
def eng():
    from fdr import engine
    return engine


def dev(a, dtype=None):
    t = torch.as_tensor(np.asarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.to(DEV).contiguous()


_SETUP = {}


def setup(name):
    """(kind, n_in, n_act, theta, host noise table, device noise table), built once per shape"""
    if name not in _SETUP:
        kind, n_in, n_act = SHAPES[name]
        torch.manual_seed(124)
        theta = opol.TorchPolicy(kind, n_in, n_act, seed=124).get_flat()
        t = onoise.NoiseTable(2 ** 22, theta.size, 124)
        _SETUP[name] = (kind, n_in, n_act, theta, t, dev(t.table))
    return _SETUP[name]


def lane_set(t, L):
    """L perturbed sampling lanes, but lane 0 deterministic and the last lane unperturbed (sign 0)"""
    idx = np.random.RandomState(100 + L).randint(0, t.max_idx, size=L).astype(np.int64)
    sign = np.where(np.arange(L) % 2 == 0, 1, -1).astype(np.int8)
    sign[-1] = 0
    dflag = np.zeros(L, np.int8)
    dflag[0] = 1
    return idx, sign, dflag


def run(eng, name, impl, L, T, seed, idx, sign, dflag, **kw):
    from envs import SyntheticEnv
    kind, n_in, n_act, theta, t, tab = setup(name)
    spec = eng.PolicySpec(kind, n_in, n_act, theta.size)
    lanes = eng.lanes_desc(dev(theta), 0, tab, dev(idx, torch.int64), dev(sign), 0.02, dev(dflag))
    env = SyntheticEnv(n_in, n_act, kind == "discrete", T, env_seed=0)
    try:
        eng.context().set_rollout_impl(impl)
        res = eng.rollout(spec, env, lanes, L, seed, **kw)
        torch.cuda.synchronize()
    finally:
        eng.context().set_rollout_impl("auto")
    return res


def oracle(name, L, T, seed, idx, sign, dflag, **kw):
    kind, n_in, n_act, theta, t, _ = setup(name)
    oenv = oenvs.BatchedSyntheticEnv(n_in, n_act, kind == "discrete", T, L, env_seed=0)
    return oagent.evaluate_lanes(kind, n_in, n_act, theta, t.table, idx, sign, 0.02, oenv, seed,
                                 deterministic=dflag.astype(bool), **kw)


def check_vs_oracle(res, ref, L):
    assert res.reward.numel() == L
    np.testing.assert_allclose(res.reward.cpu().numpy(), ref[0], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(res.entropy.cpu().numpy(), ref[1], rtol=1e-5, atol=1e-5)
    assert np.array_equal(res.timesteps.cpu().numpy(), ref[2])
    np.testing.assert_allclose(res.norm2.cpu().numpy(), ref[3], rtol=1e-9, atol=0)


@pytest.mark.parametrize("T", T_SET)
@pytest.mark.parametrize("L", [2, 3, 9])
def test_pair_kernel_batch_boundaries_vs_oracle_and_single(eng, L, T):
    idx, sign, dflag = lane_set(setup("cheetah")[4], L)
    ref = oracle("cheetah", L, T, 7, idx, sign, dflag)
    pair = run(eng, "cheetah", "pair", L, T, 7, idx, sign, dflag)
    single = run(eng, "cheetah", "single", L, T, 7, idx, sign, dflag)
    check_vs_oracle(pair, ref, L)
    np.testing.assert_allclose(pair.reward.cpu().numpy(), single.reward.cpu().numpy(), rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("T", T_SET)
@pytest.mark.parametrize("norm,rec", [(True, False), (False, True)])
def test_pair_kernel_obs_norm_and_states_vs_oracle(eng, T, norm, rec):
    """the instances whose env state is not the policy input: M s reads s from the slot h1 later overwrites"""
    L, n_in = 3, 17
    idx, sign, dflag = lane_set(setup("cheetah")[4], L)
    om = np.linspace(-0.2, 0.2, n_in).astype(np.float32)
    osd = np.linspace(0.5, 1.5, n_in).astype(np.float32)
    okw = dict(obs_mean=om, obs_std=osd) if norm else {}
    ref = oracle("cheetah", L, T, 5, idx, sign, dflag, record_states=True, **okw)
    states = torch.empty((L, T, n_in), dtype=torch.float32, device=DEV) if rec else None
    res = run(eng, "cheetah", "pair", L, T, 5, idx, sign, dflag, obs_mean=dev(om) if norm else None,
              obs_std=dev(osd) if norm else None, states=states)
    check_vs_oracle(res, ref, L)
    if rec:
        np.testing.assert_allclose(states.cpu().numpy(), ref[-1], atol=1e-4)


def test_pair_kernel_discrete_vs_oracle(eng):
    L, T = 3, 33
    idx, sign, dflag = lane_set(setup("cartpole")[4], L)
    check_vs_oracle(run(eng, "cartpole", "pair", L, T, 7, idx, sign, dflag),
                    oracle("cartpole", L, T, 7, idx, sign, dflag), L)


@pytest.mark.parametrize("T", [10, 23])
def test_pair_kernel_longer_batch_vs_oracle(eng, T):
    """3 action dims: a draw batch spans 10 steps, so the batch drawn ahead must not replace the running one early"""
    L = 3
    idx, sign, dflag = lane_set(setup("hopper")[4], L)
    check_vs_oracle(run(eng, "hopper", "pair", L, T, 7, idx, sign, dflag),
                    oracle("hopper", L, T, 7, idx, sign, dflag), L)


def test_pair_kernel_reproducible(eng):
    L, T = 9, 23
    idx, sign, dflag = lane_set(setup("cheetah")[4], L)
    a = run(eng, "cheetah", "pair", L, T, 7, idx, sign, dflag)
    b = run(eng, "cheetah", "pair", L, T, 7, idx, sign, dflag)
    assert np.array_equal(a.reward.cpu().numpy(), b.reward.cpu().numpy())
