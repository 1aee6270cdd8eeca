"""GPU: the Welford obs statistics at their edges -- fdr_obs_stats_merge (csrc/fdr_rollout.hip) and the rollouts'
per-lane update (csrc/fdr_rollout_kernel.h, fdr_rollout_dyn.hip; ObsWelford of fdr_rollout_parts.h) -- bit for bit
against oracle.obs_stats.Welford (utils/math_helpers.py:29-38, :68-87; f32, the reference's operation order, G10).

Merge: mean, m2 and count bit-equal to Welford.merge in lane order, over dim 1 / 63 / 64 / 65 / 1024 (1025 refused),
n 0 / 1 / 5 / 300, accumulators that start at count 0, 7, 2^24 + 1 and 2^31 + 5 (where (float)c rounds; the int64
path), partial means spanning 1e-3 .. 1e4, zero counts (all; first, middle and last lane), and the same partials in
reversed lane order -- which must differ from lane order in at least one bit, so an order-blind merge cannot pass.

Per-lane update: the launch records the raw states it visited (states=) next to the statistics (obs_stats=); the
lane's Welford is recomputed on the CPU from those very states and the coins of oracle.obs_stats.lane_coins, so the
env arithmetic drops out and mean / m2 must be BIT-EQUAL (test_gpu_obs_stats.py holds them to 1e-4 against the
oracle's own env states and stays as it is).  T 1 / 63 / 64 / 65 / 130 (the coins come in batches of 64 steps),
chance 0 / 0.3 / 1, L 1 / 5, lane_offset 0 / 1000, with and without obs normalisation (the raw obs enters either
way), in five kernel families: rollout_kernel, its WIDE form, rollout_dyn_kernel at a shape that is no compiled
instance, CartPole (physics, terminating) and a terminating synthetic env.
"""
import numpy as np
import pytest
import torch

import aux_cases as ac
import aux_ref as ar
from oracle import noise as onoise
from oracle import obs_stats as oo
from oracle import policies as opol

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SIGMA = 0.02
SEED = 77
TABLE_SIZE = 1 << 20
THETA_ROW = 4242
NAN = float("nan")

# family -> (policy shape, rollout impl or None = the dispatcher's choice)
FAMILIES = {
    "single": (("mujoco", 17, 6), "single"),
    "wide": (("mujoco", 17, 6), "wide"),
    "dyn": (("mujoco", 13, 5), None),            # no compiled instance: the runtime-shaped kernel
    "cartpole": (("discrete", 4, 2), None),      # physics env, terminating
    "synth_term": (("mujoco", 11, 3), "single"),   # |s'[1]| > 0.5 ends the episode: CPU oracle steps 80, 130, 130, 93, 37
}
TERM_THRESHOLD, TERM_DIM = 0.5, 1
TS = (1, 63, 64, 65, 130)


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from fdr import engine
    return engine


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- merge ------------------------------------------------------------------------------------------------------
def merge_on_device(eng, acc, mean, m2, count):
    am, av = dev(acc[0]), dev(acc[1])
    cnt = torch.tensor([acc[2]], dtype=torch.int64, device=DEV)
    eng.obs_stats_merge(dev(mean), dev(m2), dev(count), am, av, cnt)
    torch.cuda.synchronize()
    return am.cpu().numpy(), av.cpu().numpy(), int(cnt.item())


def check_merge(eng, acc, mean, m2, count, what):
    gm, gv, gc = merge_on_device(eng, acc, mean, m2, count)
    w = ar.welford_ref(len(acc[0]), acc, zip(mean, m2, count))
    assert gc == w.count, what
    np.testing.assert_array_equal(bits(gm), bits(w.mean_), err_msg=what)
    np.testing.assert_array_equal(bits(gv), bits(w.m2), err_msg=what)
    return gm, gv, gc


@pytest.mark.parametrize("dim", ac.MERGE_DIMS)
def test_merge_bit_equal(eng, dim):
    for n in ac.MERGE_NS:
        for start in ac.MERGE_STARTS:
            acc, mean, m2, count = ac.merge_case(dim, n, start)
            what = "dim %d n %d start %d" % (dim, n, start)
            gm, gv, gc = check_merge(eng, acc, mean, m2, count, what)
            if n == 0:          # nothing to fold: the accumulator is bit-unchanged
                assert gc == start
                np.testing.assert_array_equal(bits(gm), bits(acc[0]))
                np.testing.assert_array_equal(bits(gv), bits(acc[1]))
            else:
                assert gc == start + int(count.sum())


@pytest.mark.parametrize("dim,n,start", [(65, 5, 7), (1, 300, 2 ** 24 + 1), (1024, 5, 0), (63, 300, 2 ** 31 + 5)])
def test_merge_zero_counts(eng, dim, n, start):
    """Lanes that sampled nothing are skipped (math_helpers.py:68-87 returns at count 0): all of them, and the first,
    a middle and the last one."""
    acc, mean, m2, count = ac.merge_case(dim, n, start, "all")
    gm, gv, gc = check_merge(eng, acc, mean, m2, count, "all zero")
    assert gc == start
    np.testing.assert_array_equal(bits(gm), bits(acc[0]))
    np.testing.assert_array_equal(bits(gv), bits(acc[1]))
    acc, mean, m2, count = ac.merge_case(dim, n, start, "ends")
    assert count[0] == 0 and count[n // 2] == 0 and count[-1] == 0
    check_merge(eng, acc, mean, m2, count, "zeros at the ends")


def test_merge_depends_on_lane_order(eng):
    o = ac.ORDER_CASE
    acc, mean, m2, count = ac.merge_case(o["dim"], o["n"], o["start"], o["zeros"])
    fm, fv, fc = check_merge(eng, acc, mean, m2, count, "lane order")
    rm, rv, rc = check_merge(eng, acc, mean[::-1].copy(), m2[::-1].copy(), count[::-1].copy(), "reversed")
    assert fc == rc
    assert np.any(bits(fm) != bits(rm)) or np.any(bits(fv) != bits(rv))


def test_merge_refuses_dim_1025(eng):
    acc, mean, m2, count = ac.merge_case(1025, 5, 7)
    am, av = dev(acc[0]), dev(acc[1])
    cnt = torch.tensor([7], dtype=torch.int64, device=DEV)
    with pytest.raises(eng._lib.FDRError, match="obs_dim > 1024"):
        eng.obs_stats_merge(dev(mean), dev(m2), dev(count), am, av, cnt)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(bits(am.cpu().numpy()), bits(acc[0]))
    np.testing.assert_array_equal(bits(av.cpu().numpy()), bits(acc[1]))
    assert int(cnt.item()) == 7


# ---- per-lane update --------------------------------------------------------------------------------------------
_CACHE = {}


def base(shape):
    """(theta, table) on the host and the device: theta = fl32(0.1 * a table row) (test_gpu_dyn_shapes.py's base)."""
    if shape not in _CACHE:
        P = opol.num_params(*shape)
        tab = onoise.NoiseTable(TABLE_SIZE, P, 124)
        theta = (tab.decode(THETA_ROW) * np.float32(0.1)).astype(np.float32)
        _CACHE[shape] = (theta, tab, dev(theta), dev(tab.table))
    return _CACHE[shape]


def lanes_of(shape, L):
    """+, -, unperturbed deterministic, +, - (the first L of them)."""
    _, tab, _, _ = base(shape)
    idx = np.random.RandomState(5).randint(0, tab.max_idx, size=5).astype(np.int64)[:L]
    sign = np.array([1, -1, 0, 1, -1], np.int8)[:L]
    return idx, sign, (sign == 0).astype(np.int8)


def make_env(family, shape, T):
    from envs import CartPoleEnv, SyntheticEnv
    kind, n_in, n_act = shape
    if family == "cartpole":
        return CartPoleEnv(T)
    if family == "synth_term":
        return SyntheticEnv(n_in, n_act, kind == "discrete", T, env_seed=0, device=DEV, done_threshold=TERM_THRESHOLD,
                            done_dim=TERM_DIM)
    return SyntheticEnv(n_in, n_act, kind == "discrete", T, env_seed=0, device=DEV)


def launch(eng, family, T, L, chance, lane_offset, norm):
    shape, impl = FAMILIES[family]
    kind, n_in, n_act = shape
    theta, tab, theta_d, tab_d = base(shape)
    idx, sign, det = lanes_of(shape, L)
    ld = eng.lanes_desc(theta_d, 0, tab_d, dev(idx), dev(sign), SIGMA, dev(det), lane_offset=lane_offset)
    states = torch.full((L, T, n_in), NAN, dtype=torch.float32, device=DEV)
    om = dev(np.linspace(-0.2, 0.2, n_in).astype(np.float32)) if norm else None
    osd = dev(np.linspace(0.5, 1.5, n_in).astype(np.float32)) if norm else None
    try:
        if impl is not None:
            eng.context().set_rollout_impl(impl)
        res = eng.rollout(eng.PolicySpec(kind, n_in, n_act, theta.size), make_env(family, shape, T), ld, L, SEED,
                          jiggle=False, obs_mean=om, obs_std=osd, states=states, obs_stats=chance)
        torch.cuda.synchronize()
    finally:
        if impl is not None:
            eng.context().set_rollout_impl("auto")
    return (states.cpu().numpy(), res.timesteps.cpu().numpy(), res.obs_mean.cpu().numpy(), res.obs_m2.cpu().numpy(),
            res.obs_count.cpu().numpy())


def coins(T, L, chance, lane_offset):
    key = ("coins", T, L, chance, lane_offset)
    if key not in _CACHE:
        lanes = np.arange(L, dtype=np.uint64) + np.uint64(lane_offset)
        _CACHE[key] = np.stack([oo.lane_coins(SEED, lanes, t, chance) for t in range(T)], axis=1)
    return _CACHE[key]


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_lane_welford_bit_equal(eng, family, T):
    n_in = FAMILIES[family][0][1]
    ended_early = sampled = 0
    for L in (1, 5):
        for lane_offset in (0, 1000):
            for norm in (False, True):
                for chance in (0.0, 0.3, 1.0):
                    what = "%s T %d L %d offset %d norm %d chance %g" % (family, T, L, lane_offset, norm, chance)
                    S, steps, gm, gv, gc = launch(eng, family, T, L, chance, lane_offset, norm)
                    assert np.all((steps >= 1) & (steps <= T)), what
                    if family not in ("cartpole", "synth_term"):
                        assert np.all(steps == T), what
                    cn = coins(T, L, chance, lane_offset)
                    for l in range(L):
                        n = int(steps[l])
                        assert np.all(np.isfinite(S[l, :n])) and np.all(np.isnan(S[l, n:])), what
                        w = ar.welford_lane(S[l, :n], cn[l, :n])
                        assert gc[l] == w.count, (what, l, gc[l], w.count)
                        np.testing.assert_array_equal(bits(gm[l]), bits(w.mean_), err_msg="%s lane %d mean" % (what, l))
                        np.testing.assert_array_equal(bits(gv[l]), bits(w.m2), err_msg="%s lane %d m2" % (what, l))
                        ended_early += n < T
                        sampled += w.count
                    assert np.all(gc <= steps), what          # only visited states enter
                    if chance == 0.0:
                        assert not gc.any() and not bits(gm).any() and not bits(gv).any(), what
                    if chance == 1.0:
                        np.testing.assert_array_equal(gc, steps, err_msg=what)
    assert sampled > 0
    if family in ("cartpole", "synth_term") and T == 130:
        assert ended_early > 0, "no lane of %s ended before T = 130: the terminating path was not run" % family
    print("%s T %d: %d states sampled, %d lane episodes ended early" % (family, T, sampled, ended_early))
