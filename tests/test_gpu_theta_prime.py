"""theta' = fl32(theta +/- fl32(sigma * eps)) as the ROLLOUTS form it, bit for bit, at the noise table's edges.

fdr_perturb's kernel (test_gpu_kernels.py, G2) is not what a rollout runs: the rollouts gather theta' themselves
(LanesArgs::src -> ParamSrc -> MlpLane::load / MlpPair::load; prep_kernel / prep_transpose_kernel for the conv policies).

  1  fdr_diag_theta_prime: the two MLP loaders over a recording source -- every value they are given, how often each
     element is read and how often it enters norm2 -- against oracle.noise.perturb, bitwise.
  2  the same table edges through the real kernels, against the oracle at the suite's tolerances; an out-of-range
     lane runs unperturbed and poisons only its own norm2.
  3  table path == host-rows path, bit for bit, in the hot kernels (MLP and conv policies): the rows are numpy's
     theta', so equal outputs mean the table path formed the same bits -- with a single-rounding control showing
     the comparison can tell (continuous MLP shapes).  A discrete policy's outputs cannot: on the CPU oracle (64
     lanes, sigma 0.02, T 12) the single-rounding theta' moves 540-740 elements per lane by 1 ulp and changes the
     return or entropy of 62 continuous (cheetah) lanes but of 1 cartpole and 19 trap lanes, and one 1-ulp element
     changes no discrete lane at all.  Part 1 carries the discrete shapes' pin.
  4  every lane against the oracle at lane counts where lane placement can go wrong (pair kernel: three launch
     rounds with a ragged last one; the wide kernel at 1024 lanes).

The table is a view into a larger device buffer with P floats of a loud sentinel on each side: a gather that runs
past either end shows as a wrong value and never leaves owned memory.
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
SIGMA = 0.02
SENTINEL = 1e30
TABLE_SIZE = 1 << 16
SHAPES = {"trap": ("discrete", 2, 9), "cartpole": ("discrete", 4, 2), "lunar": ("discrete", 8, 4),
          "hopper": ("mujoco", 11, 3), "cheetah": ("mujoco", 17, 6)}
IMPLS = ("pair", "single", "wide")
T = 12          # two full 5-step draw batches of the pair kernel plus a remainder
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


_CASES = {}


class Case(object):
    """One policy shape: theta, the noise table on the host and guard-allocated on the device."""

    def __init__(self, name):
        self.kind, self.n_in, self.n_act = SHAPES[name]
        torch.manual_seed(124)
        self.theta = opol.TorchPolicy(self.kind, self.n_in, self.n_act, seed=124).get_flat()
        self.P = P = self.theta.size
        self.noise = onoise.NoiseTable(TABLE_SIZE, P, 124)
        self.table = self.noise.table
        self.max_idx = self.noise.max_idx
        self.mid = (self.max_idx // 2) | 1        # an odd offset
        self.buf = torch.full((TABLE_SIZE + 2 * P,), SENTINEL, dtype=torch.float32, device=DEV)
        self.buf[P:P + TABLE_SIZE] = dev(self.table)
        self.tab_d = self.buf[P:P + TABLE_SIZE]   # the table: a view with P sentinels on each side
        self.theta_d = dev(self.theta)

    def guards_intact(self):
        P = self.P
        return bool((self.buf[:P] == SENTINEL).all()) and bool((self.buf[P + TABLE_SIZE:] == SENTINEL).all())

    def in_range(self, idx):
        idx = np.asarray(idx)
        return (idx >= 0) & (idx <= self.max_idx)

    def legal(self, idx, sign):
        """The lanes as the oracle can run them: an out-of-range lane is an unperturbed one."""
        ok = self.in_range(idx)
        return np.where(ok, idx, 0).astype(np.int64), np.where(ok, sign, 0).astype(np.int8)

    def thetas(self, idx, sign):
        return onoise.perturb(self.theta, self.table, *self.legal(idx, sign), SIGMA)

    def norm2(self, idx, sign):
        """f64 sum of fl32(sigma eps)^2 (oracle/agent.py evaluate_lanes); 0 unperturbed, NaN out of range."""
        s32, P = np.float32(SIGMA), self.P
        out = []
        for i, sg, ok in zip(idx, sign, self.in_range(idx)):
            if not ok:
                out.append(np.nan)
            elif sg == 0:
                out.append(0.0)
            else:
                st = (self.table[int(i):int(i) + P] * s32).astype(np.float64)
                out.append(float(np.dot(st, st)))
        return np.array(out)

    def spec(self, eng):
        return eng.PolicySpec(self.kind, self.n_in, self.n_act, self.P)

    def lanes(self, eng, idx, sign):
        return eng.lanes_desc(self.theta_d, 0, self.tab_d, dev(idx, torch.int64),
                              None if sign is None else dev(sign, torch.int8), SIGMA)

    def env(self, T_=T):
        from envs import SyntheticEnv
        return SyntheticEnv(self.n_in, self.n_act, self.kind == "discrete", T_, env_seed=0)

    def oracle(self, idx, sign, seed=SEED, T_=T, record_states=False):
        idx, sign = self.legal(idx, sign)
        oenv = oenvs.BatchedSyntheticEnv(self.n_in, self.n_act, self.kind == "discrete", T_, len(idx), env_seed=0)
        return oagent.evaluate_lanes(self.kind, self.n_in, self.n_act, self.theta, self.table, idx, sign, SIGMA, oenv,
                                     seed, record_states=record_states)


def case(name):
    if name not in _CASES:
        _CASES[name] = Case(name)
    return _CASES[name]


def edge_lanes(c, partners=False):
    """(sign, idx) of the eight edge lanes; partners: + their antithetic partners (12 lanes)."""
    sign = [1, -1, 0, 1, -1, 1, 1, 1]
    idx = [0, 0, c.mid, c.max_idx, c.max_idx, c.max_idx + 1, -1, c.mid]
    if partners:
        sign += [-1, -1, -1, 0]
        idx += [c.mid, c.max_idx + 1, -1, c.mid]
    return np.array(sign, np.int8), np.array(idx, np.int64)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- 1. the loaders' own theta' ---------------------------------------------------------------------------------
@pytest.mark.parametrize("loader", ["lane", "pair"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_loader_theta_prime_bit_exact_at_table_edges(eng, name, loader):
    c = case(name)
    sign, idx = edge_lanes(c)
    L = len(idx)
    ok = c.in_range(idx)
    assert list(np.nonzero(~ok)[0]) == [5, 6]
    ref = c.thetas(idx, sign)
    out, reads, counted, n2 = [t.cpu().numpy() for t in eng.theta_prime(c.spec(eng), c.lanes(eng, idx, sign), L,
                                                                          loader)]
    assert np.array_equal(bits(out), bits(ref)), np.argwhere(bits(out) != bits(ref))[:8]
    assert np.array_equal(bits(out[~ok]), bits(np.broadcast_to(c.theta, (2, c.P))))   # out of range: theta itself
    assert reads.min() >= 1                      # every element is loaded ...
    assert np.all(counted == 1)                  # ... and enters norm2 exactly once
    ref_n2 = c.norm2(idx, sign)
    assert np.all(np.isnan(n2[~ok]))
    np.testing.assert_allclose(n2[ok], ref_n2[ok], rtol=1e-9, atol=0)
    assert np.all(n2[sign == 0] == 0.0)
    # sign = NULL is +1 on every lane: lane 7's row again, and the oracle's all-plus rows
    out1, _, counted1, n21 = [t.cpu().numpy() for t in eng.theta_prime(c.spec(eng), c.lanes(eng, idx, None), L,
                                                                         loader)]
    assert np.array_equal(bits(out1[7]), bits(out[7])) and n21[7] == n2[7]
    assert np.array_equal(bits(out1), bits(c.thetas(idx, np.ones(L, np.int8)))) and np.all(counted1 == 1)
    # the rows form: base_stride = P, no table
    rows = dev(ref)
    outr, readsr, countedr, n2r = [t.cpu().numpy() for t in eng.theta_prime(c.spec(eng), eng.lanes_desc(rows, c.P),
                                                                             L, loader)]
    assert np.array_equal(bits(outr), bits(ref))
    assert readsr.min() >= 1 and np.all(countedr == 1) and np.all(n2r == 0.0)
    # an odd lane count: the pair loader's idle half records nothing and leaves its partner's counts alone
    outo, _, countedo, n2o = [t.cpu().numpy() for t in eng.theta_prime(c.spec(eng), c.lanes(eng, idx, sign), L - 1,
                                                                         loader)]
    assert np.array_equal(bits(outo), bits(ref[:L - 1])) and np.all(countedo == 1)
    assert np.array_equal(n2o, n2[:L - 1], equal_nan=True)
    assert c.guards_intact()


# ---- 2. the same edges through the real kernels -----------------------------------------------------------------
def _roll(eng, c, lanes, L, states=None):
    res = eng.rollout(c.spec(eng), c.env(), lanes, L, SEED, states=states)
    torch.cuda.synchronize()
    return res


@pytest.mark.parametrize("L", [12, 11])
@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("name", ["cheetah", "cartpole"])
def test_rollout_kernels_at_table_edges(eng, name, impl, L):
    c = case(name)
    sign, idx = edge_lanes(c, partners=True)
    sign, idx = sign[:L], idx[:L]
    ok = c.in_range(idx)
    # second launch: the out-of-range lanes as plain unperturbed lanes (same lane ids, hence the same draws)
    idx2, sign2 = c.legal(idx, sign)
    idx2[~ok] = c.mid
    try:
        eng.context().set_rollout_impl(impl)
        a = _roll(eng, c, c.lanes(eng, idx, sign), L)
        b = _roll(eng, c, c.lanes(eng, idx2, sign2), L)
    finally:
        eng.context().set_rollout_impl("auto")
    r_ret, r_ent, r_steps, _ = c.oracle(idx, sign)
    r_n2 = c.norm2(idx, sign)
    ret, ent, steps, n2 = (a.reward.cpu().numpy(), a.entropy.cpu().numpy(), a.timesteps.cpu().numpy(),
                           a.norm2.cpu().numpy())
    np.testing.assert_allclose(ret[ok], r_ret[ok], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(ent[ok], r_ent[ok], rtol=1e-5, atol=1e-5)
    assert np.array_equal(steps, r_steps)
    np.testing.assert_allclose(n2[ok], r_n2[ok], rtol=1e-9, atol=0)
    assert np.all(np.isnan(n2[~ok])) and (~ok).sum() == 4
    okt = torch.as_tensor(ok, device=DEV)
    for f in ("reward", "entropy", "timesteps"):       # every lane, the out-of-range ones included: bit-equal
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    assert torch.equal(a.norm2[okt], b.norm2[okt])
    assert torch.all(b.norm2[~okt] == 0.0)
    assert c.guards_intact()


# ---- 3. table path == host-rows path in the hot kernels ---------------------------------------------------------
def _lanes64(c):
    L = 64
    rs = np.random.RandomState(5)
    base = rs.randint(0, c.max_idx + 1, size=L // 2).astype(np.int64)
    base[0], base[1] = 0, c.max_idx
    idx = np.repeat(base, 2)
    sign = np.tile(np.array([1, -1], np.int8), L // 2)
    sign[-2:] = 0
    return idx, sign


def _table_vs_rows(eng, c, impl, rows_np, idx, sign):
    L = len(idx)
    out = []
    try:
        eng.context().set_rollout_impl(impl)
        for lanes in (c.lanes(eng, idx, sign), eng.lanes_desc(dev(rows_np), c.P)):
            st = torch.full((L, T, c.n_in), float("nan"), dtype=torch.float32, device=DEV)
            out.append((_roll(eng, c, lanes, L, states=st), st))
    finally:
        eng.context().set_rollout_impl("auto")
    return out


def _single_rounding_rows(c, idx, sign):
    """theta' as one rounding of the exact theta + sign * fl32(sigma) * eps (what an FMA contraction would form)."""
    eps = np.stack([c.table[int(i):int(i) + c.P] for i in idx]).astype(np.float64)
    s = np.float64(np.float32(SIGMA))
    return (c.theta.astype(np.float64)[None, :] + sign.astype(np.float64)[:, None] * s * eps).astype(np.float32)


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("name", ["cheetah", "hopper", "cartpole", "lunar"])
def test_rollout_table_path_equals_rows_path_bitwise(eng, name, impl):
    """reward, entropy, timesteps and every visited state, table descriptor vs numpy's theta' as host rows.

    Control (continuous shapes): rows formed with ONE rounding instead of two must not give the same bits -- a
    differing return or state in at least 16 of the 62 perturbed lanes (the CPU oracle gives 57 by return alone at
    this size).  Measured on an MI355X: cheetah 59 (pair) / 61 (single) / 61 (wide), hopper 48 / 55 / 55 of 62.
    The discrete shapes assert the equality only: their outputs cannot see a 1-ulp theta' (module docstring), the
    loader read-back above carries their pin."""
    c = case(name)
    idx, sign = _lanes64(c)
    rows = c.thetas(idx, sign)
    (a, sa), (b, sb) = _table_vs_rows(eng, c, impl, rows, idx, sign)
    for f in ("reward", "entropy", "timesteps"):
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    assert torch.equal(sa, sb) and not torch.isnan(sa).any()
    assert torch.all(b.norm2 == 0.0)
    np.testing.assert_allclose(a.norm2.cpu().numpy(), c.norm2(idx, sign), rtol=1e-9, atol=0)
    if c.kind == "mujoco":
        rows1 = _single_rounding_rows(c, idx, sign)
        moved = (bits(rows1) != bits(rows)).sum(axis=1)
        assert moved[:62].min() > 0 and np.all(moved[62:] == 0)
        (_, _), (d, sd) = _table_vs_rows(eng, c, impl, rows1, idx, sign)
        differs = (d.reward != a.reward) | (sd != sa).flatten(1).any(dim=1)
        n = int(differs[:62].sum())
        print("single-rounding control %s/%s: %d of 62 perturbed lanes differ" % (name, impl, n))
        assert n >= 16, n
        assert not bool(differs[62:].any())
    assert c.guards_intact()


# conv policies (fdr_impala_* / fdr_atari_*: prep_kernel / prep_transpose_kernel gather theta'); rows force the
# per-lane core, so pairs = False is the like-for-like form
CONV_SIGN = np.array([1, -1, 0, 1], np.int8)


class ConvCase(object):
    def __init__(self, theta, table_size):
        self.theta, self.P = theta, theta.size
        P = self.P
        self.table = np.random.RandomState(124).randn(table_size).astype(np.float32)
        self.max_idx = table_size - P
        self.idx = np.array([0, 0, (self.max_idx // 2) | 1, self.max_idx], np.int64)
        self.buf = torch.full((table_size + 2 * P,), SENTINEL, dtype=torch.float32, device=DEV)
        self.buf[P:P + table_size] = dev(self.table)
        self.tab_d = self.buf[P:P + table_size]
        self.rows = onoise.perturb(theta, self.table, self.idx, CONV_SIGN, SIGMA)
        s32 = np.float32(SIGMA)
        st = [(self.table[int(i):int(i) + P] * s32).astype(np.float64) for i in self.idx]
        self.norm2 = np.array([float(np.dot(x, x)) if sg != 0 else 0.0 for x, sg in zip(st, CONV_SIGN)])

    def table_lanes(self, eng):
        return eng.lanes_desc(dev(self.theta), 0, self.tab_d, dev(self.idx), dev(CONV_SIGN), SIGMA)

    def rows_lanes(self, eng, rows=None):
        return eng.lanes_desc(dev(self.rows if rows is None else rows), self.P)

    def single_rounding_rows(self):
        eps = np.stack([self.table[int(i):int(i) + self.P] for i in self.idx]).astype(np.float64)
        s = np.float64(np.float32(SIGMA))
        return (self.theta.astype(np.float64)[None, :] + CONV_SIGN.astype(np.float64)[:, None] * s * eps).astype(
            np.float32)

    def guards_intact(self):
        n = self.buf.numel()
        return bool((self.buf[:self.P] == SENTINEL).all()) and bool((self.buf[n - self.P:] == SENTINEL).all())


def conv_case(kind):
    if kind not in _CASES:
        if kind == "impala":
            from test_gpu_impala import _theta
            _CASES[kind] = ConvCase(_theta(6), 1 << 22)
        else:
            from oracle import atari as oa
            _CASES[kind] = ConvCase(oa.init_theta(6, 124), 1 << 21)
    return _CASES[kind]


def _conv_rollouts_equal(a, b, c):
    torch.cuda.synchronize()
    for f in ("reward", "entropy", "timesteps", "actions", "probs"):
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    np.testing.assert_allclose(a.norm2.cpu().numpy(), c.norm2, rtol=1e-9)      # one value per lane (not per env)
    assert a.norm2.numel() == 4 and torch.all(b.norm2 == 0.0)
    assert c.guards_intact()


@pytest.mark.parametrize("fp16", [False, True])
def test_impala_rollout_table_path_equals_rows_path_bitwise(eng, fp16):
    """reward, entropy, timesteps, actions and probs of fdr_impala_rollout, table descriptor vs host rows.

    Control (f32): rows formed with one rounding instead of two move ~301 k of the 1.16 M elements of each
    perturbed lane by 1 ulp, and on an MI355X the recorded probs of all three perturbed lanes then differ from the
    table run's (the unperturbed lane's do not) -- asserted."""
    c = conv_case("impala")
    spec = eng.ImpalaSpec(6, 2, 3, env_seed=5, fp16=fp16, pairs=False)
    a = eng.impala_rollout(spec, c.table_lanes(eng), 4, 11, record=True)
    b = eng.impala_rollout(spec, c.rows_lanes(eng), 4, 11, record=True)
    _conv_rollouts_equal(a, b, c)
    if not fp16:
        rows1 = c.single_rounding_rows()
        moved = (bits(rows1) != bits(c.rows)).sum(axis=1)
        d = eng.impala_rollout(spec, c.rows_lanes(eng, rows1), 4, 11, record=True)
        torch.cuda.synchronize()
        differs = (d.probs != a.probs).reshape(4, -1).any(dim=1).cpu().numpy()
        print("impala single-rounding control: theta' elements moved per lane %s, lanes whose probs differ %s"
              % (moved.tolist(), differs.tolist()))
        assert np.all(moved[CONV_SIGN != 0] > 0) and differs.tolist() == [True, True, False, True]


def test_impala_strategies_table_path_equals_rows_path_bitwise(eng):
    c = conv_case("impala")
    rs = np.random.RandomState(9)
    frames = dev(rs.randint(0, 256, size=(3, 3, 64, 64)).astype(np.float32))
    reward = dev(rs.choice([-1.0, 0.0, 1.0, 2.0], size=3).astype(np.float32))
    for fp16 in (False, True):
        spec = eng.ImpalaSpec(6, fp16=fp16, pairs=False)
        a = eng.impala_strategies(spec, c.table_lanes(eng), 4, frames, reward)
        b = eng.impala_strategies(spec, c.rows_lanes(eng), 4, frames, reward)
        torch.cuda.synchronize()
        assert tuple(a.shape) == (4, 3, 6) and torch.equal(a, b), fp16
        assert not torch.equal(a[0], a[1])          # the +eps and -eps lanes of offset 0 are different policies
    assert c.guards_intact()


def test_atari_rollout_and_strategies_table_path_equals_rows_path_bitwise(eng):
    c = conv_case("atari")
    spec = eng.AtariSpec(6, 2, 3, env_seed=9)
    a = eng.atari_rollout(spec, c.table_lanes(eng), 4, 21, record=True)
    b = eng.atari_rollout(spec, c.rows_lanes(eng), 4, 21, record=True)
    _conv_rollouts_equal(a, b, c)
    frames = eng.atari_env_frames(5, 0, 0, 3)
    sa = eng.atari_strategies(eng.AtariSpec(6), c.table_lanes(eng), 4, frames)
    sb = eng.atari_strategies(eng.AtariSpec(6), c.rows_lanes(eng), 4, frames)
    torch.cuda.synchronize()
    assert tuple(sa.shape) == (4, 3, 6) and torch.equal(sa, sb)
    assert not torch.equal(sa[0], sa[1])
    assert c.guards_intact()


# ---- 4. every lane against the oracle where lane placement can go wrong -----------------------------------------
def _all_lanes_vs_oracle(eng, c, L, impl):
    rs = np.random.RandomState(L)
    idx = rs.randint(0, c.max_idx + 1, size=L).astype(np.int64)
    sign = np.tile(np.array([1, -1, 1, -1, 0], np.int8), L // 5 + 1)[:L]
    try:
        eng.context().set_rollout_impl(impl)
        res = _roll(eng, c, c.lanes(eng, idx, sign), L)
    finally:
        eng.context().set_rollout_impl("auto")
    r_ret, r_ent, r_steps, r_n2 = c.oracle(idx, sign)
    np.testing.assert_allclose(res.reward.cpu().numpy(), r_ret, rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(res.entropy.cpu().numpy(), r_ent, rtol=1e-5, atol=1e-5)
    assert np.array_equal(res.timesteps.cpu().numpy(), r_steps)
    np.testing.assert_allclose(res.norm2.cpu().numpy(), r_n2, rtol=1e-9, atol=0)


def test_pair_kernel_three_launch_rounds_every_lane_vs_oracle(eng):
    """L = 2 x (16 lanes per CU) x CUs + 11: three launch rounds of the pair kernel -- every workgroup slot, every
    round's lane_base, the ragged last round and an idle half wave."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    _all_lanes_vs_oracle(eng, case("cheetah"), 2 * 16 * cus + 11, "pair")


def test_wide_kernel_1024_lanes_every_lane_vs_oracle(eng):
    """The wide one-lane kernel at the discrete benchmark configuration's lane count (auto selects it)."""
    _all_lanes_vs_oracle(eng, case("cartpole"), 1024, "auto")
