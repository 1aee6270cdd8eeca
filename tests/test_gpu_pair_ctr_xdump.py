"""rollout_pair_kernel<17,6> with the x hand-off written without its select (FDR_PAIR_X_DUMP) and -- in a build with
-DFDR_PAIR_CTR_ADD=1 -- the draw batch's counter word carried by addition, forced onto the pair kernel, against the
oracle and the one-lane kernel (which forms every word with hash_ctr and has no x hand-off).  The cases hold for either
setting of either macro.

L = 1 / 2 / 3: a wave with an idle half, a full wave, a second wave with an idle half (an odd lane count).  T = 1 / 4:
the remainder loop alone, on batch 0's draws (draw(0), hash_ctr); T = 5: exactly one batch; T = 6 / 11: one / two
batches and a remainder that reads the batch drawn ahead -- the first words the recurrence forms.  A wrong word moves
every sampled action of its batch by O(std), far past the tolerances; a constant column of x that the loop disturbs
(the 1 of the folded bias, the zeros) moves layer 1 of every step.

Tolerances are those of tests/test_gpu_pair_head_rs12.py (DESIGN.md "Parity"): the pair kernel's head sums its 64 terms
in another order than the oracle and the one-lane kernel, so reward and entropy agree to rounding; the step counts are
integers and equal.  Bitwise: a launch of lanes [k:] at lane_offset = k is the tail of the whole launch -- the same
instructions on the same words, whichever half of a wave a lane rides in.
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
BIG_OFFSET = 70000  # global lane ids past 2^16


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


def lane_set(L, det=None):
    """L perturbed sampling lanes; det: the deterministic flags (default: lane 0 deterministic when L > 1, so that a
    deterministic lane shares its wave with a sampling one)"""
    t = setup()[1]
    idx = np.random.RandomState(200 + L).randint(0, t.max_idx, size=L).astype(np.int64)
    sign = np.where(np.arange(L) % 2 == 0, 1, -1).astype(np.int8)
    dflag = np.zeros(L, np.int8)
    if det is None:
        dflag[0] = 1 if L > 1 else 0
    else:
        dflag[:] = det
    return idx, sign, dflag


def run(eng, impl, T, idx, sign, dflag, lane_offset=0):
    from envs import SyntheticEnv
    theta, t, tab = setup()
    L = len(idx)
    spec = eng.PolicySpec(KIND, N_IN, N_ACT, theta.size)
    lanes = eng.lanes_desc(dev(theta), 0, tab, dev(idx, torch.int64), dev(sign), 0.02, dev(dflag),
                           lane_offset=lane_offset)
    env = SyntheticEnv(N_IN, N_ACT, False, T, env_seed=0)
    try:
        eng.context().set_rollout_impl(impl)
        res = eng.rollout(spec, env, lanes, L, SEED)
        torch.cuda.synchronize()
    finally:
        eng.context().set_rollout_impl("auto")
    return res


def oracle(T, idx, sign, dflag, lane_offset=0):
    theta, t, _ = setup()
    L = len(idx)
    oenv = oenvs.BatchedSyntheticEnv(N_IN, N_ACT, False, T, L, env_seed=0)
    return oagent.evaluate_lanes(KIND, N_IN, N_ACT, theta, t.table, idx, sign, 0.02, oenv, SEED,
                                 deterministic=dflag.astype(bool), lane_ids=lane_offset + np.arange(L))


def report(tag, res, other_reward, other_entropy):
    print("%s: max |reward diff| %.3e  max |entropy diff| %.3e" % (
        tag, float(np.abs(res.reward.cpu().numpy() - other_reward).max()),
        float(np.abs(res.entropy.cpu().numpy() - other_entropy).max())))


def check_vs_oracle(res, ref, L):
    assert res.reward.numel() == L
    report("pair vs oracle", res, ref[0], ref[1])
    np.testing.assert_allclose(res.reward.cpu().numpy(), ref[0], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(res.entropy.cpu().numpy(), ref[1], rtol=1e-5, atol=1e-5)
    assert np.array_equal(res.timesteps.cpu().numpy(), ref[2])
    np.testing.assert_allclose(res.norm2.cpu().numpy(), ref[3], rtol=1e-9, atol=0)


def check_vs_single(pair, single):
    report("pair vs one-lane", pair, single.reward.cpu().numpy(), single.entropy.cpu().numpy())
    np.testing.assert_allclose(pair.reward.cpu().numpy(), single.reward.cpu().numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(pair.entropy.cpu().numpy(), single.entropy.cpu().numpy(), rtol=1e-5, atol=1e-5)
    assert torch.equal(pair.timesteps, single.timesteps)
    # each kernel is held to the oracle's norm at rtol 1e-9 (the f64 sum in another order): to each other at twice that
    np.testing.assert_allclose(pair.norm2.cpu().numpy(), single.norm2.cpu().numpy(), rtol=2e-9, atol=0)


@pytest.mark.parametrize("T", [1, 4, 5, 6, 11])
@pytest.mark.parametrize("L", [1, 2, 3])
def test_pair_vs_oracle_and_single(eng, L, T):
    idx, sign, dflag = lane_set(L)
    pair = run(eng, "pair", T, idx, sign, dflag)
    check_vs_oracle(pair, oracle(T, idx, sign, dflag), L)
    check_vs_single(pair, run(eng, "single", T, idx, sign, dflag))


def test_global_lane_ids_past_2_16(eng):
    """the lane id sits in the high half of the counter word: the base word formed once must carry all of it"""
    L, T = 3, 11
    idx, sign, dflag = lane_set(L, det=0)
    pair = run(eng, "pair", T, idx, sign, dflag, lane_offset=BIG_OFFSET)
    check_vs_oracle(pair, oracle(T, idx, sign, dflag, lane_offset=BIG_OFFSET), L)
    check_vs_single(pair, run(eng, "single", T, idx, sign, dflag, lane_offset=BIG_OFFSET))
    # and the draws do depend on it
    zero = run(eng, "pair", T, idx, sign, dflag)
    assert not np.allclose(zero.reward.cpu().numpy(), pair.reward.cpu().numpy(), rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("det", [(1, 0), (0, 1)])
def test_deterministic_lane_beside_a_sampling_one(eng, det):
    """one wave: the deterministic half ignores the draws its threads still compute, the other half takes its own"""
    L, T = 2, 11
    idx, sign, dflag = lane_set(L, det=det)
    pair = run(eng, "pair", T, idx, sign, dflag)
    check_vs_oracle(pair, oracle(T, idx, sign, dflag), L)
    check_vs_single(pair, run(eng, "single", T, idx, sign, dflag))


def test_tail_launch_is_bitwise_the_tail_of_the_whole(eng):
    """lanes [1:] at lane_offset = 1: lane 1 moves from half 1 of wave 0 to half 0, lane 2 from half 0 of wave 1 to
    half 1 -- same words, same bits"""
    L, T = 3, 11
    idx, sign, dflag = lane_set(L, det=0)
    whole = run(eng, "pair", T, idx, sign, dflag)
    part = run(eng, "pair", T, idx[1:], sign[1:], dflag[1:], lane_offset=1)
    for name in ("reward", "entropy", "timesteps", "norm2"):
        assert torch.equal(getattr(part, name), getattr(whole, name)[1:]), name
