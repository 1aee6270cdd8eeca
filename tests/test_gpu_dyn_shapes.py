"""GPU: the runtime-shaped kernel family (csrc/fdr_rollout_dyn.hip) -- MLP policies at shapes that are no compiled
instance, and FDR_ROLLOUT_GENERIC at shapes that are.

Everything is pinned against the CPU oracle (oracle.agent.evaluate_lanes, oracle.policies.lanes_forward,
oracle.noise.perturb) at test_gpu_kernels.py's tolerances: returns rtol = atol = 1e-4, entropy 1e-5, steps equal,
norm2 rtol 1e-9, forward 1e-5 abs, theta' bit for bit.

Base theta: fl32(0.1 * a noise-table row) (as test_policy_forward_vs_reference), not the fresh normc init, whose
unperturbed deterministic lanes sit at an argmax near-tie on every step (top-two gap 7e-9 .. 3e-6 on the oracle).

Action margins.  A discrete lane's action is only determined where the oracle's own margin exceeds the forward
tolerance 1e-5: |cumsum_i - u tot| over the partition boundaries i < n_act - 1 for a sampled lane, the top-two gap for
a deterministic one.  Every discrete case asserts its oracle's minimum margin over the episode >= 1e-5 before it
compares (margin()).  Measured on the CPU oracle with the index seeds below (min over all lanes and steps):
  episodes T = 70   (5, 3)d sampled 2.07e-4, deterministic 4.28e-2; (64, 16)d sampled 2.42e-4 (index seed 4: seed 1
                    gives 1.42e-5, seed 2 1.35e-5 -- above the tolerance, but by less than half of it), deterministic
                    1.87e-4
  episodes T = 1    (5, 3)d sampled 6.6e-2, deterministic 4.28e-2; (64, 16)d sampled 1.08e-3, deterministic 2.01e-4
  features (5, 3)d  obs-norm 1.85e-4, Welford 2.07e-4, u_inject 1.45e-4, terminating (threshold 0.60) 2.12e-3
  (4, 2)d generic / single, T = 123: L = 13 2.88e-4, L = 64 1.36e-4
  (1, 1)d has one action: no boundary, margin inf.
"""
import re

import numpy as np
import pytest
import torch

from oracle import agent as oagent
from oracle import envs as oenvs
from oracle import noise as onoise
from oracle import policies as opol
from oracle import rng as crng

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SIGMA = 0.02
TABLE_SIZE = 1 << 20
THETA_ROW = 4242            # the table row the base theta is cut from
TOL = 1e-5                  # the forward tolerance: the least action margin a compared discrete episode may have

EDGE = {"d1x1": ("discrete", 1, 1), "d5x3": ("discrete", 5, 3), "d64x16": ("discrete", 64, 16),
        "c1x1": ("mujoco", 1, 1), "c13x5": ("mujoco", 13, 5), "c4x7": ("mujoco", 4, 7), "c64x8": ("mujoco", 64, 8)}
FEATURE = {"d5x3": EDGE["d5x3"], "c13x5": EDGE["c13x5"]}
COMPILED = {"c17x6": ("mujoco", 17, 6), "d4x2": ("discrete", 4, 2)}
# index seeds: 1, except where the module docstring names another (name, T, det)
IDX_SEED = 1
IDX_SEED_OF = {("d64x16", 70, False): 4}
SEED = 7


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


# ---- cases (pure numpy) -----------------------------------------------------------------------------------------
_CACHE = {}


def base(shape):
    """(theta, NoiseTable) of a (kind, n_in, n_act): theta = fl32(0.1 * table row)."""
    if shape not in _CACHE:
        P = opol.num_params(*shape)
        tab = onoise.NoiseTable(TABLE_SIZE, P, 124)
        _CACHE[shape] = ((tab.decode(THETA_ROW) * np.float32(0.1)).astype(np.float32), tab)
    return _CACHE[shape]


def lanes10(shape, det, idx_seed=IDX_SEED, L=10):
    """Antithetic pairs plus two deterministic eval lanes of theta itself."""
    _, tab = base(shape)
    n_pairs = (L - 2) // 2
    idx = np.random.RandomState(idx_seed).randint(0, tab.max_idx, size=n_pairs + (L - 2) % 2).astype(np.int64)
    idx = np.concatenate([np.repeat(idx, 2)[:L - 2], np.zeros(2, np.int64)])
    sign = np.concatenate([np.tile(np.array([1, -1], np.int8), n_pairs + 1)[:L - 2], np.zeros(2, np.int8)])
    dflag = np.concatenate([np.full(L - 2, 1 if det else 0, np.int8), np.ones(2, np.int8)])
    return idx, sign, dflag


def oracle(shape, lanes, T, seed=SEED, lane_ids=None, done=(0.0, 0), **kw):
    """evaluate_lanes on the synthetic env (jiggle off, states recorded) -> dict; cached."""
    idx, sign, dflag = lanes
    key = ("oracle", shape, idx.tobytes(), sign.tobytes(), dflag.tobytes(), T, seed, done,
           None if lane_ids is None else tuple(lane_ids), tuple(sorted((k, np.asarray(v).tobytes()) for k, v in kw.items())))
    if key not in _CACHE:
        kind, n_in, n_act = shape
        theta, tab = base(shape)
        env = oenvs.BatchedSyntheticEnv(n_in, n_act, kind == "discrete", T, len(idx), env_seed=0,
                                        done_threshold=done[0], done_dim=done[1])
        out = oagent.evaluate_lanes(kind, n_in, n_act, theta, tab.table, idx, sign, SIGMA, env, seed,
                                    deterministic=dflag.astype(bool), jiggle=False, record_states=True,
                                    lane_ids=lane_ids, **kw)
        res = dict(ret=out[0], ent=out[1], steps=out[2], norm2=out[3], states=out[-1])
        if kw.get("obs_chance") is not None:
            res["stats"] = out[4]
        _CACHE[key] = res
    return _CACHE[key]


def margin(shape, lanes, o, seed=SEED, lane_ids=None, obs_mean=None, obs_std=None):
    """The oracle's least action margin over the episodes it ran (discrete; inf for one action / continuous)."""
    kind, n_in, n_act = shape
    if kind != "discrete" or n_act == 1:
        return np.inf
    idx, sign, dflag = lanes
    theta, tab = base(shape)
    thetas = onoise.perturb(theta, tab.table, idx, sign, SIGMA)
    ids = np.arange(len(idx), dtype=np.uint64) if lane_ids is None else np.asarray(lane_ids, np.uint64)
    worst = np.inf
    for t in range(int(o["steps"].max())):
        alive = o["steps"] > t
        x = o["states"][:, t]
        if obs_mean is not None:
            x = np.clip((x - obs_mean) / obs_std, -10, 10).astype(np.float32)
        p = opol.lanes_forward(kind, n_in, n_act, thetas, x)
        u = crng.uniform(seed, ids, t, 0)
        for l in np.nonzero(alive)[0]:
            if dflag[l]:
                top = np.sort(p[l])[-2:]
                m = float(top[1] - top[0])
            else:
                c = np.cumsum(p[l], dtype=np.float32)
                m = float(np.abs(c[:-1] - np.float32(u[l]) * c[-1]).min())
            worst = min(worst, m)
    return worst


# ---- GPU launches -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    from fdr import engine
    return engine


def _device_base(shape):
    key = ("dev", shape)
    if key not in _CACHE:
        theta, tab = base(shape)
        _CACHE[key] = (_dev(theta), _dev(tab.table))
    return _CACHE[key]


def _spec(eng, shape):
    return eng.PolicySpec(shape[0], shape[1], shape[2], opol.num_params(*shape))


def _launch(eng, shape, lanes, T, seed=SEED, lane_offset=0, impl=None, record=True, done=(0.0, 0), **kw):
    from envs import SyntheticEnv
    kind, n_in, n_act = shape
    idx, sign, dflag = lanes
    L = len(idx)
    theta_d, tab_d = _device_base(shape)
    ld = eng.lanes_desc(theta_d, 0, tab_d, _dev(idx), _dev(sign), SIGMA, _dev(dflag), lane_offset=lane_offset)
    env = SyntheticEnv(n_in, n_act, kind == "discrete", T, env_seed=0, device=DEV, done_threshold=done[0],
                       done_dim=done[1])
    states = torch.full((L, T, n_in), float("nan"), dtype=torch.float32, device=DEV) if record else None
    try:
        if impl is not None:
            eng.context().set_rollout_impl(impl)
        res = eng.rollout(_spec(eng, shape), env, ld, L, seed, jiggle=False, states=states, **kw)
        torch.cuda.synchronize()
    finally:
        if impl is not None:
            eng.context().set_rollout_impl("auto")
    return dict(ret=res.reward.cpu().numpy(), ent=res.entropy.cpu().numpy(), steps=res.timesteps.cpu().numpy(),
                norm2=res.norm2.cpu().numpy(), states=None if states is None else states.cpu().numpy(), res=res)


def _check_episodes(g, o):
    np.testing.assert_array_equal(g["steps"], o["steps"])
    np.testing.assert_allclose(g["ret"], o["ret"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(g["ent"], o["ent"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(g["norm2"], o["norm2"], rtol=1e-9, atol=0)


# ---- 1. theta' bitwise ------------------------------------------------------------------------------------------
DENORMAL = np.float32(1e-40)
EPS_DENORMAL_STEP = np.float32(1e-37)     # fl32(0.02 * 1e-37) is denormal


@pytest.mark.parametrize("name", sorted(EDGE) + ["c3x1_generic"])
def test_theta_prime_bitwise(eng, name):
    """The dyn loader's theta' over sign +, -, 0, idx == max_idx and idx == max_idx + 1, with -0.0, +0.0 and
    denormals planted in theta and under them in the table rows (test_gpu_theta_prime_signs.py's plants)."""
    generic = name.endswith("_generic")
    shape = ("mujoco", 3, 1) if generic else EDGE[name]
    theta, tab = base(shape)
    theta, table = theta.copy(), tab.table.copy()
    P = theta.size
    idx = np.array([tab.max_idx // 2, 17, 64, tab.max_idx, tab.max_idx + 1], np.int64)
    sign = np.array([1, -1, 0, 1, 1], np.int8)
    plants = (1, P // 2, P - 4)                     # first layer, second layer, head
    for p0 in plants:
        theta[p0:p0 + 3] = [-0.0, 0.0, DENORMAL]
    for off in idx[:4]:
        for p0 in plants:
            table[off + p0:off + p0 + 3] = [0.0, -0.0, EPS_DENORMAL_STEP]
        table[off + 8:off + 11] = [-0.0, 0.0, -EPS_DENORMAL_STEP]
    ok = idx <= tab.max_idx
    want = onoise.perturb(theta, table, np.where(ok, idx, 0), np.where(ok, sign, 0), SIGMA)
    lanes = eng.lanes_desc(_dev(theta), 0, _dev(table), _dev(idx), _dev(sign), SIGMA)
    try:
        if generic:
            eng.context().set_rollout_impl("generic")
        out, reads, counted, n2 = [t.cpu().numpy() for t in eng.theta_prime(_spec(eng, shape), lanes, 5, "dyn")]
    finally:
        eng.context().set_rollout_impl("auto")
    diff = np.argwhere(out.view(np.uint32) != want.view(np.uint32))
    assert len(diff) == 0, diff[:8]
    assert reads.min() >= 1 and np.all(counted == 1)
    for i in (2, 4):                                # unperturbed / out of range: theta itself, -0.0 kept
        assert np.array_equal(out[i].view(np.uint32), theta.view(np.uint32))
    assert np.isnan(n2[4]) and n2[2] == 0.0
    s32 = np.float32(SIGMA)
    ref_n2 = [float(np.sum(((s32 * table[i:i + P]).astype(np.float32).astype(np.float64)) ** 2)) for i in idx[:4]]
    np.testing.assert_allclose(n2[[0, 1, 3]], np.array(ref_n2)[[0, 1, 3]], rtol=1e-9, atol=0)


# ---- 2. forward -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(EDGE))
def test_policy_forward(eng, name):
    """7 lanes (not a multiple of the 4 lanes per workgroup) against lanes_forward; discrete also with BN statistics."""
    shape = EDGE[name]
    kind, n_in, n_act = shape
    theta, tab = base(shape)
    L = 7
    rs = np.random.RandomState(3)
    idx = rs.randint(0, tab.max_idx, size=L).astype(np.int64)
    sign = np.array([1, -1, 0, 1, -1, 1, 0], np.int8)
    x = rs.randn(L, n_in).astype(np.float32)
    theta_d, tab_d = _device_base(shape)
    lanes = eng.lanes_desc(theta_d, 0, tab_d, _dev(idx), _dev(sign), SIGMA)
    thetas = onoise.perturb(theta, tab.table, idx, sign, SIGMA)
    got = eng.policy_forward(_spec(eng, shape), lanes, L, _dev(x))
    want = opol.lanes_forward(kind, n_in, n_act, thetas, x)
    if kind == "discrete":
        np.testing.assert_allclose(got.cpu().numpy(), want, rtol=0, atol=1e-5)
        np.testing.assert_allclose(got.sum(-1).cpu().numpy(), 1.0, rtol=0, atol=1e-5)
        stats = [(rs.randn(n).astype(np.float32) * np.float32(0.3), rs.uniform(0.5, 2.0, n).astype(np.float32))
                 for n in (n_in, 64, 64)]
        bm, bv = _dev(np.concatenate([s[0] for s in stats])), _dev(np.concatenate([s[1] for s in stats]))
        got = eng.policy_forward(_spec(eng, shape), lanes, L, _dev(x), bm, bv)
        want = opol.lanes_forward(kind, n_in, n_act, thetas, x, bn_stats=stats)
        np.testing.assert_allclose(got.cpu().numpy(), want, rtol=0, atol=1e-5)
    else:
        np.testing.assert_allclose(got[0].cpu().numpy(), want[0], rtol=0, atol=1e-5)
        np.testing.assert_allclose(got[1].cpu().numpy(), want[1], rtol=0, atol=1e-5)


# ---- 3. whole episodes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("T", [70, 1])
@pytest.mark.parametrize("name", sorted(EDGE))
def test_episodes_vs_oracle(eng, name, T, det):
    """10 lanes (antithetic pairs + two eval lanes); T = 70 crosses the 64-draw batch of a discrete lane and several
    batches of a continuous one (64 // n_act steps each); T = 1."""
    shape = EDGE[name]
    lanes = lanes10(shape, det, idx_seed=IDX_SEED_OF.get((name, T, det), IDX_SEED))
    o = oracle(shape, lanes, T)
    m = margin(shape, lanes, o)
    print("%s T=%d det=%d: oracle action margin %.3g" % (name, T, det, m))
    assert m >= TOL
    g = _launch(eng, shape, lanes, T)
    _check_episodes(g, o)
    np.testing.assert_allclose(g["states"], o["states"], rtol=0, atol=1e-4)
    if name == "d1x1":
        np.testing.assert_allclose(g["ent"], 0.0, rtol=0, atol=1e-12)      # a one-way softmax


# ---- 4. features ------------------------------------------------------------------------------------------------
def _obs_norm(n_in):
    return np.linspace(-0.2, 0.2, n_in).astype(np.float32), np.linspace(0.5, 1.5, n_in).astype(np.float32)


@pytest.mark.parametrize("name", sorted(FEATURE))
def test_states_and_obs_normalisation(eng, name):
    shape, T = FEATURE[name], 70
    lanes = lanes10(shape, False)
    om, osd = _obs_norm(shape[1])
    o = oracle(shape, lanes, T, obs_mean=om, obs_std=osd)
    m = margin(shape, lanes, o, obs_mean=om, obs_std=osd)
    print("%s obs-norm: oracle action margin %.3g" % (name, m))
    assert m >= TOL
    g = _launch(eng, shape, lanes, T, obs_mean=_dev(om), obs_std=_dev(osd))
    _check_episodes(g, o)
    np.testing.assert_allclose(g["states"], o["states"], rtol=0, atol=1e-4)     # the raw observations


@pytest.mark.parametrize("name", sorted(FEATURE))
def test_welford_statistics(eng, name):
    shape, T = FEATURE[name], 70
    lanes = lanes10(shape, False)
    o = oracle(shape, lanes, T, obs_chance=0.5)
    m = margin(shape, lanes, o)
    print("%s welford: oracle action margin %.3g" % (name, m))
    assert m >= TOL
    g = _launch(eng, shape, lanes, T, record=False, obs_stats=0.5)
    _check_episodes(g, o)
    res = g["res"]
    cnt = res.obs_count.cpu().numpy()
    np.testing.assert_array_equal(cnt, [s.count for s in o["stats"]])
    assert cnt.sum() > 0.3 * o["steps"].sum()
    gm, g2 = res.obs_mean.cpu().numpy(), res.obs_m2.cpu().numpy()
    for l, s in enumerate(o["stats"]):
        if s.count:
            np.testing.assert_allclose(gm[l], s.mean_, rtol=1e-5, atol=1e-5)
            np.testing.assert_allclose(g2[l], s.m2, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("name", sorted(FEATURE))
def test_u_inject_replays_the_oracles_draws(eng, name):
    """The oracle's own draws of another seed, injected: the launch's seed no longer matters."""
    shape, T, L, seed_act = FEATURE[name], 70, 10, 1234
    kind, n_in, n_act = shape
    lanes = lanes10(shape, False)
    o = oracle(shape, lanes, T, seed=seed_act)
    m = margin(shape, lanes, o, seed=seed_act)
    print("%s u_inject: oracle action margin %.3g" % (name, m))
    assert m >= TOL
    ids = np.arange(L, dtype=np.uint64)
    if kind == "discrete":
        u = np.stack([crng.uniform(seed_act, ids, t, 0) for t in range(T)], axis=1).reshape(L, T, 1)
    else:
        ks = np.arange(n_act, dtype=np.uint64)[None, :]
        u = np.stack([crng.normal(seed_act, ids[:, None], t, ks) for t in range(T)], axis=1)
    g = _launch(eng, shape, lanes, T, seed=99, u_inject=_dev(u.astype(np.float32)))
    _check_episodes(g, o)
    np.testing.assert_allclose(g["states"], o["states"], rtol=0, atol=1e-4)


# done_threshold on dimension n_in - 1, chosen on the CPU oracle: at least three lanes end early, at least one
# reaches T, and on the free-running episodes no |s[done_dim]| of any lane and step lies within 1e-4 of it (the
# states' tolerance; measured gaps 4.0e-3 and 2.3e-3)
DONE_THR = {"d5x3": 0.60, "c13x5": 0.62}


@pytest.mark.parametrize("name", sorted(FEATURE))
def test_terminating_env(eng, name):
    shape, T = FEATURE[name], 70
    done = (DONE_THR[name], shape[1] - 1)
    lanes = lanes10(shape, False)
    o = oracle(shape, lanes, T, done=done)
    m = margin(shape, lanes, o)
    print("%s terminating: steps %s, oracle action margin %.3g" % (name, o["steps"].tolist(), m))
    assert m >= TOL
    assert (o["steps"] < T).sum() >= 3 and (o["steps"] == T).sum() >= 1
    free = np.abs(oracle(shape, lanes, T)["states"][:, 1:, done[1]])
    assert np.abs(free - np.float32(done[0])).min() > 1e-4
    g = _launch(eng, shape, lanes, T, done=done)
    _check_episodes(g, o)
    for l, n in enumerate(g["steps"]):
        assert np.all(np.isnan(g["states"][l, n:])), "lane %d wrote a state after its last step" % l
        np.testing.assert_allclose(g["states"][l, :n], o["states"][l, :n], rtol=0, atol=1e-4)


def _code(excinfo):
    return int(re.search(r"\(code (\d+)\)", str(excinfo.value)).group(1))


def test_u_inject_with_statistics_is_still_refused(eng):
    from fdr import _lib
    shape = FEATURE["d5x3"]
    with pytest.raises(_lib.FDRError) as ei:
        _launch(eng, shape, lanes10(shape, False), 20, record=False, obs_stats=0.5,
                u_inject=torch.zeros((10, 20, 1), dtype=torch.float32, device=DEV))
    assert _code(ei) == _lib.FDR_ERR_UNSUPPORTED


# ---- 5. same shape, two kernels ---------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [13, 64])
@pytest.mark.parametrize("name", sorted(COMPILED))
def test_generic_and_single_kernels_agree(eng, name, L):
    shape, T = COMPILED[name], 123
    lanes = lanes10(shape, False, idx_seed=L, L=L)
    o = oracle(shape, lanes, T)
    m = margin(shape, lanes, o)
    print("%s L=%d: oracle action margin %.3g" % (name, L, m))
    assert m >= TOL
    a = _launch(eng, shape, lanes, T, impl="single", record=False)
    b = _launch(eng, shape, lanes, T, impl="generic", record=False)
    _check_episodes(b, o)
    np.testing.assert_array_equal(a["steps"], b["steps"])
    np.testing.assert_allclose(b["ret"], a["ret"], rtol=1e-5, atol=0)
    np.testing.assert_allclose(b["ent"], a["ent"], rtol=0, atol=1e-5)
    np.testing.assert_allclose(b["norm2"], a["norm2"], rtol=1e-12, atol=0)


# ---- 6. shard invariance ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(FEATURE))
def test_shard_invariance(eng, name):
    """Lanes [k:] launched with lane_offset = k are bitwise the tail of the whole launch (k = 3: other wave slots)."""
    shape, T, k = FEATURE[name], 70, 3
    lanes = lanes10(shape, False)
    whole = _launch(eng, shape, lanes, T)
    part = _launch(eng, shape, tuple(a[k:] for a in lanes), T, lane_offset=k)
    np.testing.assert_array_equal(part["steps"], whole["steps"][k:])
    np.testing.assert_array_equal(part["ret"], whole["ret"][k:])
    np.testing.assert_array_equal(part["states"].view(np.uint32), whole["states"][k:].view(np.uint32))
    assert len(np.unique(whole["ret"][:8])) == 8           # every sampled lane its own episode


# ---- 7. refusals ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,text", [(("discrete", 65, 2), "n_in must be in 1..64"),
                                        (("mujoco", 65, 2), "n_in must be in 1..64"),
                                        (("discrete", 4, 17), "n_act must be in 1..16"),
                                        (("mujoco", 4, 9), "n_act must be in 1..8")])
def test_refusals(eng, shape, text):
    """Outside the limits: FDR_ERR_UNSUPPORTED naming the limit, nothing launched (the outputs keep their fill)."""
    from envs import SyntheticEnv
    from fdr import _lib
    kind, n_in, n_act = shape
    P = opol.num_params(kind, n_in, n_act)
    base_t = torch.zeros(P, dtype=torch.float32, device=DEV)
    buf = torch.full((4, 8), -7.0, dtype=torch.float64, device=DEV)
    out = eng.RolloutResult(buf[0], buf[1], torch.full((8,), -7, dtype=torch.int32, device=DEV), buf[2])
    env = SyntheticEnv(n_in, n_act, kind == "discrete", 10, device=DEV)
    for impl in ("auto", "generic"):
        try:
            eng.context().set_rollout_impl(impl)
            with pytest.raises(_lib.FDRError) as ei:
                eng.rollout(eng.PolicySpec(kind, n_in, n_act, P), env, eng.lanes_desc(base_t, 0), 8, 1, out=out)
        finally:
            eng.context().set_rollout_impl("auto")
        torch.cuda.synchronize()
        assert _code(ei) == _lib.FDR_ERR_UNSUPPORTED and text in str(ei.value)
        assert torch.all(buf == -7.0) and torch.all(out.timesteps == -7), "a refused call launched"
    x = torch.zeros((8, n_in), dtype=torch.float32, device=DEV)
    with pytest.raises(_lib.FDRError) as ei:
        eng.policy_forward(eng.PolicySpec(kind, n_in, n_act, P), eng.lanes_desc(base_t, 0), 8, x)
    assert _code(ei) == _lib.FDR_ERR_UNSUPPORTED and text in str(ei.value)
    with pytest.raises(_lib.FDRError) as ei:
        eng.theta_prime(eng.PolicySpec(kind, n_in, n_act, P), eng.lanes_desc(base_t, 0), 8, "dyn")
    assert _code(ei) == _lib.FDR_ERR_UNSUPPORTED and text in str(ei.value)


def test_n_params_is_checked_against_the_runtime_layout(eng):
    from envs import SyntheticEnv
    from fdr import _lib
    P = opol.num_params("mujoco", 24, 4)
    base_t = torch.zeros(P + 1, dtype=torch.float32, device=DEV)
    with pytest.raises(_lib.FDRError) as ei:
        eng.rollout(eng.PolicySpec("mujoco", 24, 4, P + 1), SyntheticEnv(24, 4, False, 10, device=DEV),
                    eng.lanes_desc(base_t, 0), 8, 1)
    assert _code(ei) == _lib.FDR_ERR_INVALID


_ENV_VAR_CHILD = """
import torch
import envs
from fdr import engine
P = 4546
spec = engine.PolicySpec("mujoco", 3, 1, P)
env = envs.SyntheticEnv(3, 1, False, 5, device="cuda:0")
base = torch.zeros(P, dtype=torch.float32, device="cuda:0")
res = engine.rollout(spec, env, engine.lanes_desc(base, 0), 4, 1)
torch.cuda.synchronize()
assert res.timesteps.tolist() == [5, 5, 5, 5]
print("generic-ok")
"""


def test_environment_variable_selects_generic():
    """FDR_ROLLOUT=generic in a fresh process: a physics env's shape on the synthetic env runs (it is refused under
    every other selection: test_gpu_physics_envs.py::test_refusals)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.pathsep.join([root, os.path.join(root, "dfd-starter_amd")] +
                           [p for p in os.environ.get("PYTHONPATH", "").split(os.pathsep) if p])
    r = subprocess.run([sys.executable, "-c", _ENV_VAR_CHILD], env=dict(os.environ, FDR_ROLLOUT="generic",
                                                                         PYTHONPATH=path),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "generic-ok" in r.stdout, r.stderr[-2000:]


# ---- 8. runner --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env_shape,kw", [((24, 4, False), {}),
                                          ((5, 3, True), dict(normalize_obs=True, vbn_buffer_size=16))])
def test_runner_trains_at_a_runtime_shape(env_shape, kw):
    from envs import SyntheticEnv
    from run_sequential import SequentialRunner
    r = SequentialRunner(env_shape=env_shape, episode_len=30, batch_size=8, antithetic=True,
                         noise_table_size=2 ** 20, verbose=False, **kw)
    assert isinstance(r.env, SyntheticEnv)
    assert (r.env.obs_dim, r.env.act_dim, r.env.discrete, r.env.episode_len) == env_shape + (30,)
    before = r.policy.get_trainable_flat().copy()
    r.train(2)
    torch.cuda.synchronize()
    after = r.policy.get_trainable_flat()
    assert len(r.history) == 2
    assert np.all(np.isfinite(after)) and not np.array_equal(before, after)
    for h in r.history:
        assert np.isfinite(h["Policy Novelty"])                 # fdr_policy_forward at the new shape
        assert all(np.all(np.isfinite(np.asarray(v, dtype=np.float64))) for k, v in h.items()
                   if isinstance(v, (int, float, np.floating, np.ndarray)) and k != "idx")
