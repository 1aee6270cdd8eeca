"""rollout_pair_kernel with the 12-output reduce-scatter head (MlpPair::kHeadRS: continuous, 6 actions -- the cheetah
shape), forced onto the pair kernel, against the oracle and the one-lane kernel.

The head leaves the 6 means in row threads 0, 1, 2, 4, 5, 6 and the std pre-activations 8 threads up; the draws, the
std read, K a, the entropy sum and the recorded states all follow that placement, so a wrong lane shows in reward,
entropy or states.  L = 1 / 2 / 3: a wave with an idle half, a full wave, a second wave with an idle half; T = 1 / 5 /
6 / 11: below, at and past the 5-step draw batch, with the remainder loop.  Lane 0 is deterministic, the last lane
unperturbed, the others sample.

Tolerances are those of tests/test_gpu_pair_handoff.py (DESIGN.md "Parity"): the head's 64-term sum is in another
order than the oracle's and the one-lane kernel's, nothing else differs.
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
KIND, N_IN, N_ACT = "mujoco", 17, 6
SEED = 7


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


def setup():
    if not _SETUP:
        torch.manual_seed(124)
        theta = opol.TorchPolicy(KIND, N_IN, N_ACT, seed=124).get_flat()
        t = onoise.NoiseTable(2 ** 22, theta.size, 124)
        _SETUP["v"] = (theta, t, dev(t.table))
    return _SETUP["v"]


def lane_set(t, L):
    """L perturbed sampling lanes, but lane 0 deterministic and the last lane unperturbed (sign 0)"""
    idx = np.random.RandomState(100 + L).randint(0, t.max_idx, size=L).astype(np.int64)
    sign = np.where(np.arange(L) % 2 == 0, 1, -1).astype(np.int8)
    sign[-1] = 0
    dflag = np.zeros(L, np.int8)
    dflag[0] = 1
    return idx, sign, dflag


def run(eng, impl, L, T, idx, sign, dflag, **kw):
    from envs import SyntheticEnv
    theta, t, tab = setup()
    spec = eng.PolicySpec(KIND, N_IN, N_ACT, theta.size)
    lanes = eng.lanes_desc(dev(theta), 0, tab, dev(idx, torch.int64), dev(sign), 0.02, dev(dflag))
    env = SyntheticEnv(N_IN, N_ACT, False, T, env_seed=0)
    try:
        eng.context().set_rollout_impl(impl)
        res = eng.rollout(spec, env, lanes, L, SEED, **kw)
        torch.cuda.synchronize()
    finally:
        eng.context().set_rollout_impl("auto")
    return res


def oracle(L, T, idx, sign, dflag, **kw):
    theta, t, _ = setup()
    oenv = oenvs.BatchedSyntheticEnv(N_IN, N_ACT, False, T, L, env_seed=0)
    return oagent.evaluate_lanes(KIND, N_IN, N_ACT, theta, t.table, idx, sign, 0.02, oenv, SEED,
                                 deterministic=dflag.astype(bool), **kw)


def check_vs_oracle(res, ref, L):
    assert res.reward.numel() == L
    np.testing.assert_allclose(res.reward.cpu().numpy(), ref[0], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(res.entropy.cpu().numpy(), ref[1], rtol=1e-5, atol=1e-5)
    assert np.array_equal(res.timesteps.cpu().numpy(), ref[2])
    np.testing.assert_allclose(res.norm2.cpu().numpy(), ref[3], rtol=1e-9, atol=0)


@pytest.mark.parametrize("T", [1, 5, 6, 11])
@pytest.mark.parametrize("L", [1, 2, 3])
def test_rs12_head_vs_oracle_and_single(eng, L, T):
    idx, sign, dflag = lane_set(setup()[1], L)
    ref = oracle(L, T, idx, sign, dflag)
    pair = run(eng, "pair", L, T, idx, sign, dflag)
    single = run(eng, "single", L, T, idx, sign, dflag)
    check_vs_oracle(pair, ref, L)
    np.testing.assert_allclose(pair.reward.cpu().numpy(), single.reward.cpu().numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(pair.entropy.cpu().numpy(), single.entropy.cpu().numpy(), rtol=1e-5, atol=1e-5)
    assert torch.equal(pair.timesteps, single.timesteps)


def test_rs12_head_recorded_states_vs_oracle(eng):
    """every state dim of every step: the remapped action lanes feed K a of the right dims"""
    L, T = 3, 11
    idx, sign, dflag = lane_set(setup()[1], L)
    ref = oracle(L, T, idx, sign, dflag, record_states=True)
    states = torch.empty((L, T, N_IN), dtype=torch.float32, device=DEV)
    res = run(eng, "pair", L, T, idx, sign, dflag, states=states)
    check_vs_oracle(res, ref, L)
    np.testing.assert_allclose(states.cpu().numpy(), ref[-1], atol=1e-4)
