"""GPU parity of the Impala path (fdr_impala_forward / fdr_impala_rollout) against the oracle and the
reference's own outputs (tests/golden/g8_impala.npz).  Tolerances: features/probs/state 1e-5 abs (f32,
MFMA vs torch-CPU summation order); sampled actions and integer rewards exact; norm2 rel 1e-9."""
import numpy as np
import pytest
import torch

from oracle import impala as oi

pytestmark = pytest.mark.gpu

ATOL = 1e-5


@pytest.fixture(scope="module")
def engine():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from fdr import engine
    return engine


@pytest.fixture(scope="module")
def g8(golden):
    return golden("g8_impala.npz")


@pytest.fixture(scope="module")
def table():
    return np.random.RandomState(124).randn(2 ** 22).astype(np.float32)


def test_forward_matches_reference_golden(engine, g8):
    A, P = int(g8["A"]), int(g8["P"])
    tab = np.random.RandomState(int(g8["table_seed"])).randn(2 ** 22).astype(np.float32)
    off = int(g8["param_offset"])
    theta = torch.tensor((tab[off:off + P] * np.float32(0.1)).astype(np.float32), device="cuda")
    rm = torch.tensor(g8["rm"], device="cuda")
    rv = torch.tensor(g8["rv"], device="cuda")
    spec = engine.ImpalaSpec(A)
    nq, T = g8["frames"].shape[:2]
    h = torch.zeros(nq, 256, device="cuda")
    c = torch.zeros(nq, 256, device="cuda")
    for t in range(T):
        fr = torch.tensor(g8["frames"][:, t].astype(np.float32), device="cuda")
        rw = torch.tensor(g8["rewards"][:, t], device="cuda")
        nd = torch.tensor(1.0 - g8["dones"][:, t].astype(np.float32), device="cuda")
        probs, feat = engine.impala_forward(spec, theta, fr, h, c, reward=rw, notdone=nd, bn_mean=rm, bn_var=rv,
                                            feat=True)
        torch.cuda.synchronize()
        np.testing.assert_allclose(feat.cpu().numpy(), g8["feat"][:, t], atol=ATOL)
        np.testing.assert_allclose(h.cpu().numpy(), g8["h"][:, t], atol=ATOL)
        np.testing.assert_allclose(c.cpu().numpy(), g8["c"][:, t], atol=ATOL)
        np.testing.assert_allclose(probs.cpu().numpy(), g8["probs"][:, t], atol=ATOL)


def _theta(A, seed=124):
    """A trained-looking theta: torch default init of the reference layout (ImpalaCNN has no normc)."""
    torch.manual_seed(seed)
    parts = []
    for name, shape in oi.layout(A):
        if name.endswith("bn.w") or ".bn" in name and name.endswith(".w"):
            parts.append(torch.ones(shape).reshape(-1))
        elif ".bn" in name or name.startswith("fc.bn") or name.startswith("head.bn"):
            parts.append(torch.zeros(shape).reshape(-1))
        else:
            fan_in = int(np.prod(shape[1:])) if len(shape) > 1 else shape[0]
            bound = 1.0 / np.sqrt(fan_in)
            parts.append(torch.empty(shape).uniform_(-bound, bound).reshape(-1))
    return torch.cat(parts).numpy().astype(np.float32)


def _run(engine, table, A, E, T, idx, sign, det, seed=11, env_seed=5, entropy=True, lane_offset=0, rm=None, rv=None):
    theta = _theta(A)
    L = len(idx)
    dev = "cuda"
    tt = torch.tensor(table, device=dev)
    th = torch.tensor(theta, device=dev)
    idx_t = torch.tensor(np.asarray(idx, np.int64), device=dev)
    sg_t = torch.tensor(np.asarray(sign, np.int8), device=dev)
    det_t = torch.tensor(np.asarray(det, np.int8), device=dev)
    lanes = engine.lanes_desc(th, 0, tt, idx_t, sg_t, 0.02, det_t, lane_offset=lane_offset)
    spec = engine.ImpalaSpec(A, E, T, entropy=entropy, env_seed=env_seed)
    rm_t = None if rm is None else torch.tensor(rm, device=dev)
    rv_t = None if rv is None else torch.tensor(rv, device=dev)
    out = engine.impala_rollout(spec, lanes, L, seed, jiggle=True, bn_mean=rm_t, bn_var=rv_t, record=True)
    torch.cuda.synchronize()
    nb = oi.num_bn()
    ref = oi.evaluate_lanes(theta, table, np.asarray(idx), np.asarray(sign), 0.02, A, E, T, seed, env_seed,
                            np.zeros(nb, np.float32) if rm is None else rm,
                            np.ones(nb, np.float32) if rv is None else rv,
                            deterministic=np.asarray(det, bool), lane_offset=lane_offset, record=True)
    return out, ref


def _compare(out, ref, L, E, T, A, entropy=True):
    probs = out.probs.cpu().numpy().reshape(L, E, T, A)
    np.testing.assert_allclose(probs, ref["probs"], atol=ATOL)
    acts = out.actions.cpu().numpy().reshape(L, E, T)
    assert (acts == ref["actions"]).mean() == 1.0, np.argwhere(acts != ref["actions"])
    np.testing.assert_array_equal(out.reward.cpu().numpy().reshape(L, E), ref["ret"])
    np.testing.assert_array_equal(out.timesteps.cpu().numpy().reshape(L, E), ref["steps"])
    if entropy:
        np.testing.assert_allclose(out.entropy.cpu().numpy().reshape(L, E), ref["ent"], atol=ATOL)
    np.testing.assert_allclose(out.norm2.cpu().numpy(), ref["norm2"], rtol=1e-9)


def test_rollout_antithetic_stochastic(engine, table):
    A, E, T = 6, 2, 4
    idx = [1234, 1234]
    out, ref = _run(engine, table, A, E, T, idx, [1, -1], [0, 0])
    _compare(out, ref, 2, E, T, A)


def test_rollout_deterministic_with_bn_stats_and_lane_offset(engine, table):
    A, E, T = 4, 1, 3
    rs = np.random.RandomState(3)
    nb = oi.num_bn()
    rm = (0.1 * rs.randn(nb)).astype(np.float32)
    rv = (1.0 + 0.5 * np.abs(rs.randn(nb))).astype(np.float32)
    idx = [77, 2_000_000, 3_000_000]
    out, ref = _run(engine, table, A, E, T, idx, [1, 0, -1], [1, 1, 0], lane_offset=5, rm=rm, rv=rv)
    _compare(out, ref, 3, E, T, A)


def test_rollout_four_envs_ragged_lanes(engine, table):
    """E = 4 (BASELINE config 4's envs per perturbation) with a lane count that is not a multiple of
    the 8-XCD workgroup grouping."""
    A, E, T = 6, 4, 2
    idx = [10, 20, 30]
    out, ref = _run(engine, table, A, E, T, idx, [1, 1, -1], [0, 0, 0], entropy=False)
    _compare(out, ref, 3, E, T, A, entropy=False)
    assert np.all(out.entropy.cpu().numpy() == 0.0)


def test_bad_offset_poisons_norm_without_fault(engine, table):
    A = 6
    th = torch.tensor(_theta(A), device="cuda")
    tt = torch.tensor(table, device="cuda")
    idx = torch.tensor([0, len(table)], dtype=torch.int64, device="cuda")      # second is out of range
    sg = torch.tensor([1, 1], dtype=torch.int8, device="cuda")
    lanes = engine.lanes_desc(th, 0, tt, idx, sg, 0.02)
    out = engine.impala_rollout(engine.ImpalaSpec(A, 1, 1, entropy=False), lanes, 2, 3)
    torch.cuda.synchronize()
    n2 = out.norm2.cpu().numpy()
    assert np.isfinite(n2[0]) and np.isnan(n2[1])


def test_policy_api_matches_reference_golden(engine, g8):
    """ImpalaPolicy.forward on the reference's obs dicts (utils/impala_env_wrapper.py:25-28)."""
    from policies import ImpalaPolicy
    A, P = int(g8["A"]), int(g8["P"])
    pol = ImpalaPolicy((64, 64, 3), A, seed=124)
    tab = np.random.RandomState(int(g8["table_seed"])).randn(2 ** 22).astype(np.float32)
    off = int(g8["param_offset"])
    pol.set_trainable_flat((tab[off:off + P] * np.float32(0.1)).astype(np.float32))
    o = 0
    for m in pol.model.bn_layers():
        n = m.num_features
        m.running_mean.copy_(torch.as_tensor(g8["rm"][o:o + n]))
        m.running_var.copy_(torch.as_tensor(g8["rv"][o:o + n]))
        o += n
    for q in range(g8["frames"].shape[0]):
        pol.reset()
        for t in range(g8["frames"].shape[1]):
            obs = {"frame": torch.as_tensor(g8["frames"][q, t].astype(np.float32)).view(1, 1, 3, 64, 64),
                   "reward": torch.as_tensor(g8["rewards"][q, t]).view(1, 1),
                   "done": torch.as_tensor(bool(g8["dones"][q, t])).view(1, 1)}
            probs = pol.forward(obs)
            assert tuple(probs.shape) == (1, 1, A)
            np.testing.assert_allclose(probs.view(-1).cpu().numpy(), g8["probs"][q, t], atol=ATOL)
            np.testing.assert_allclose(pol.state[0].view(-1).cpu().numpy(), g8["h"][q, t], atol=ATOL)


def test_worker_and_learner_fd_step(engine):
    """Worker.evaluate (E = 2 envs per perturbation, antithetic) -> FiniteDifferences.step: the rollout
    returns match the oracle and the update follows the oracle's FD gradient over the per-env returns."""
    from dsgd import DSGD
    from envs import FrameEnv
    from learner import FiniteDifferences
    from policies import ImpalaPolicy
    from utils import AdaptiveOmega, SharedNoiseTable
    from worker import Agent, Worker
    from oracle import learner as ol
    torch.manual_seed(124)
    pol = ImpalaPolicy((64, 64, 3), 6, seed=124)
    P = pol.num_params
    nt = SharedNoiseTable(2 ** 22, P, random_seed=124)
    env = FrameEnv(6, episode_len=2, envs_per_lane=2, env_seed=5)
    worker = Worker(pol, Agent(pol, env, random_seed=3), nt, None, sigma=0.02)
    learner = FiniteDifferences(pol, DSGD(pol.parameters(), lr=0.01), AdaptiveOmega(), nt, noise_std=0.02)
    theta0 = pol.get_trainable_flat().copy()
    batch = worker.evaluate(2, antithetic=True, seed=77)
    assert len(batch) == 8 and batch.lanes_per_dir == 4
    rew = batch.reward.cpu().numpy()
    lanes_idx, lanes_sign = batch.idx_host[::2], batch.sign_host[::2]
    nb = oi.num_bn()
    ref = oi.evaluate_lanes(theta0, nt._table, lanes_idx, lanes_sign, 0.02, 6, 2, 2, 77, 5,
                            np.zeros(nb, np.float32), np.ones(nb, np.float32))
    np.testing.assert_array_equal(rew.reshape(4, 2), ref["ret"])
    np.testing.assert_allclose(batch.norm2.cpu().numpy(), np.repeat(ref["norm2"], 2), rtol=1e-9)
    upd = learner.step(batch, 0.0, 0.0, 0.0)
    g, _ = ol.fd_gradient(nt._table, P, batch.idx_host, batch.sign_host, rew, 0.0, 0.02)
    d = pol.get_trainable_flat().astype(np.float64) - theta0
    np.testing.assert_allclose(np.linalg.norm(d), upd, rtol=1e-5)
    cos = float(np.dot(d, g) / (np.linalg.norm(d) * np.linalg.norm(g)))   # DSGD ascends g
    assert cos > 1 - 1e-6, cos


# ---- fp16 mode (BASELINE config 5): parity against the f32 reference within the fp16 tolerance ------
F16_RTOL = 2e-2   # "fp16 mode <= 2e-2 relative"


def test_fp16_forward_vs_reference_golden(engine, g8):
    A, P = int(g8["A"]), int(g8["P"])
    tab = np.random.RandomState(int(g8["table_seed"])).randn(2 ** 22).astype(np.float32)
    off = int(g8["param_offset"])
    theta = torch.tensor((tab[off:off + P] * np.float32(0.1)).astype(np.float32), device="cuda")
    rm = torch.tensor(g8["rm"], device="cuda")
    rv = torch.tensor(g8["rv"], device="cuda")
    spec = engine.ImpalaSpec(A, fp16=True)
    nq, T = g8["frames"].shape[:2]
    h = torch.zeros(nq, 256, device="cuda")
    c = torch.zeros(nq, 256, device="cuda")
    for t in range(T):
        fr = torch.tensor(g8["frames"][:, t].astype(np.float32), device="cuda")
        rw = torch.tensor(g8["rewards"][:, t], device="cuda")
        nd = torch.tensor(1.0 - g8["dones"][:, t].astype(np.float32), device="cuda")
        probs, feat = engine.impala_forward(spec, theta, fr, h, c, reward=rw, notdone=nd, bn_mean=rm, bn_var=rv,
                                            feat=True)
        torch.cuda.synchronize()
        f = feat.cpu().numpy()
        scale = np.abs(g8["feat"][:, t]).max()
        assert np.abs(f - g8["feat"][:, t]).max() <= F16_RTOL * scale
        np.testing.assert_allclose(h.cpu().numpy(), g8["h"][:, t], atol=F16_RTOL * np.abs(g8["h"][:, t]).max())
        np.testing.assert_allclose(probs.cpu().numpy(), g8["probs"][:, t], rtol=F16_RTOL)


def test_fp16_rollout_first_step_vs_oracle(engine, table):
    """Step 0 sees identical inputs in both precisions: probabilities within the fp16 tolerance, the
    theta' norms identical to the f32 path (they come from the same f32 perturbation)."""
    A, E, T = 6, 2, 3
    theta = _theta(A)
    idx = [77, 2_000_000, 3_000_000]
    sign = [1, -1, 1]
    dev = "cuda"
    lanes = engine.lanes_desc(torch.tensor(theta, device=dev), 0, torch.tensor(table, device=dev),
                              torch.tensor(np.asarray(idx, np.int64), device=dev),
                              torch.tensor(np.asarray(sign, np.int8), device=dev), 0.02)
    out16 = engine.impala_rollout(engine.ImpalaSpec(A, E, T, env_seed=5, fp16=True), lanes, 3, 11, record=True)
    out32 = engine.impala_rollout(engine.ImpalaSpec(A, E, T, env_seed=5), lanes, 3, 11, record=True)
    torch.cuda.synchronize()
    p16 = out16.probs.cpu().numpy()[:, 0]
    p32 = out32.probs.cpu().numpy()[:, 0]
    np.testing.assert_allclose(p16, p32, rtol=F16_RTOL)
    np.testing.assert_array_equal(out16.norm2.cpu().numpy(), out32.norm2.cpu().numpy())
    assert np.all(np.isfinite(out16.reward.cpu().numpy())) and np.all(np.isfinite(out16.entropy.cpu().numpy()))
    np.testing.assert_allclose(out16.entropy.cpu().numpy(), out32.entropy.cpu().numpy(), rtol=F16_RTOL)


@pytest.mark.parametrize("fp16", [False, True])
def test_replay_input_projection_gemm_bit_identical(engine, table, fp16):
    """Entropy replay with the x W_ih^T half of the gates as one MFMA GEMM per 64-step chunk
    (lstm_xproj_kernel) against the per-step streaming form: identical fma chains, so the entropies are
    bit-identical; T = 70 spans two chunks (64 + 6) and E = 4 makes partial row blocks."""
    from fdr._lib import check, lib
    A, E, T, L = 6, 4, 70, 3
    theta = _theta(A)
    tt = torch.tensor(table, device="cuda")
    lanes = engine.lanes_desc(torch.tensor(theta, device="cuda"), 0, tt,
                              torch.tensor([10, 2000, 30000], dtype=torch.int64, device="cuda"),
                              torch.tensor([1, -1, 1], dtype=torch.int8, device="cuda"), 0.02)
    spec = engine.ImpalaSpec(A, E, T, entropy=True, env_seed=5, fp16=fp16)
    outs = []
    try:
        for on in (1, 0):
            engine.context().set_replay_gemm(on)
            out = engine.impala_rollout(spec, lanes, L, 11)
            torch.cuda.synchronize()
            outs.append(out.entropy.cpu().numpy().copy())
    finally:
        engine.context().set_replay_gemm(True)
    assert np.all(np.isfinite(outs[0])) and np.any(outs[0] != 0)
    np.testing.assert_array_equal(outs[0], outs[1])


def test_rollout_long_horizon_vs_oracle(engine, table):
    """f32 rollout over T = 130 steps (three 64-step chunks of the entropy replay's input-projection GEMM,
    the last partial) against the oracle: actions / integer returns exact, per-step probabilities and the
    replayed entropy within 1e-5."""
    A, E, T = 6, 2, 130
    out, ref = _run(engine, table, A, E, T, [4321, 4321], [1, -1], [0, 0])
    _compare(out, ref, 2, E, T, A)


def test_fp16_multistep_drift_bound_vs_f32_oracle(engine, table):
    """fp16 rollouts (config 5, A = 4, 4 envs) over 60 steps: the oracle (f32) is driven with the fp16 kernel's
    own actions, so both see identical frames / rewards; every step's probabilities stay within the fp16
    tolerance of f32 -- a bound on the drift of the fp16 LSTM state over the episode."""
    A, E, T = 4, 4, 60
    theta = _theta(A)
    dev = "cuda"
    lanes = engine.lanes_desc(torch.tensor(theta, device=dev), 0, torch.tensor(table, device=dev),
                              torch.tensor([555], dtype=torch.int64, device=dev),
                              torch.tensor([1], dtype=torch.int8, device=dev), 0.02)
    out = engine.impala_rollout(engine.ImpalaSpec(A, E, T, entropy=False, env_seed=5, fp16=True), lanes, 1, 11,
                                record=True)
    torch.cuda.synchronize()
    probs = out.probs.cpu().numpy().reshape(E, T, A)
    acts = out.actions.cpu().numpy().reshape(E, T)
    from oracle.noise import perturb
    p = oi.unflatten(perturb(theta, table, [555], [1], 0.02)[0], A)
    nb = oi.num_bn()
    bn = oi.split_bn(np.zeros(nb, np.float32), np.ones(nb, np.float32))
    envs = np.arange(E, dtype=np.uint64)
    h, c, r_prev = torch.zeros(E, oi.HID), torch.zeros(E, oi.HID), np.zeros(E, np.float32)
    worst = 0.0
    for t in range(T):
        pr, h, c, _, _ = oi.forward(p, bn, oi.frames(5, envs, t).astype(np.float32), r_prev, h, c)
        worst = max(worst, float(np.abs(pr.numpy() - probs[:, t]).max()))
        r_prev = oi.rewards(5, envs, t, acts[:, t], A)
    assert worst <= F16_RTOL, worst
    ret = sum(oi.rewards(5, envs, t, acts[:, t], A) for t in range(T)).astype(np.float64)
    np.testing.assert_allclose(out.reward.cpu().numpy() - ret, 0.0, atol=2e-12)   # +- jiggle only


def test_fp16_pair_core_matches_per_lane_core(engine, table):
    """fdr_impala_desc.pairs (config 5's antithetic pairs): the core step computes W_l x = theta x + s_l (E x) on MFMA
    from theta's and the pairs' sigma-eps fragment images (core_kernel_hpm2) instead of streaming each lane's
    f16(theta + s sigma eps).  Step 0 sees identical conv features in both forms: probabilities within the fp16
    tolerance of the per-lane form and of the f32 path; norms identical; whole episodes finite; the replayed
    entropies within the fp16 tolerance of f32."""
    A, E, T = 4, 4, 5
    theta = _theta(A)
    idx = np.repeat(np.array([77, 2_000_000, 3_000_000, 4_500_000], np.int64), 2)
    sign = np.tile(np.array([1, -1], np.int8), 4)
    dev = "cuda"
    lanes = engine.lanes_desc(torch.tensor(theta, device=dev), 0, torch.tensor(table, device=dev),
                              torch.tensor(idx, device=dev), torch.tensor(sign, device=dev), 0.02)
    outs = {}
    for name, fp16, pairs in (("lane", True, False), ("pair", True, True), ("f32", False, False)):
        outs[name] = engine.impala_rollout(engine.ImpalaSpec(A, E, T, env_seed=5, fp16=fp16, pairs=pairs), lanes,
                                           len(idx), 11, record=True)
    torch.cuda.synchronize()
    p_pair = outs["pair"].probs.cpu().numpy()[:, 0]
    np.testing.assert_allclose(p_pair, outs["lane"].probs.cpu().numpy()[:, 0], rtol=F16_RTOL / 4)
    np.testing.assert_allclose(p_pair, outs["f32"].probs.cpu().numpy()[:, 0], rtol=F16_RTOL)
    np.testing.assert_array_equal(outs["pair"].norm2.cpu().numpy(), outs["lane"].norm2.cpu().numpy())
    for t in (outs["pair"].reward, outs["pair"].entropy):
        assert np.all(np.isfinite(t.cpu().numpy()))
    np.testing.assert_allclose(outs["pair"].entropy.cpu().numpy(), outs["f32"].entropy.cpu().numpy(), rtol=F16_RTOL)


@pytest.mark.parametrize("E,n_pairs", [(4, 4), (4, 3), (1, 6), (2, 2)])
def test_fp16_pair_form_episodes_vs_f32_oracle(engine, table, E, n_pairs):
    """VERDICT r5 item 4 (the HIP-vs-HIP bitwise tests re-pointed at the oracle): the fp16 pair form (core_kernel_hpm2:
    two pairs per 8-wave workgroup, three MFMAs per tile and k-step; the replay as replay_chunk_hpm2 after
    xproj_pair_kernel) over whole recorded episodes with the entropy replay, T = 70 = two replay chunks, against the f32
    oracle along the kernel's own actions: probabilities and replayed entropies within the fp16 tolerance, returns
    exact up to the jiggle, sampled actions the reference's outside the rounding margin.  3 pairs (6 lanes, n_lanes %
    4 == 2) have no two-pair workgroup: they run the per-lane form, bitwise a pairs = False launch."""
    A, T, seed = 5, 70, 11
    theta = _theta(A)
    offs = np.array([77, 2_000_000, 3_000_000, 1_500_000, 1_111_111, 999], np.int64)[:n_pairs]  # < 2^22 - P
    idx = np.repeat(offs, 2)
    sign = np.tile(np.array([1, -1], np.int8), n_pairs)
    L = len(idx)
    dev = "cuda"
    lanes = engine.lanes_desc(torch.tensor(theta, device=dev), 0, torch.tensor(table, device=dev),
                              torch.tensor(idx, device=dev), torch.tensor(sign, device=dev), 0.02)
    out = engine.impala_rollout(engine.ImpalaSpec(A, E, T, entropy=True, env_seed=5, fp16=True, pairs=True), lanes, L,
                                seed, record=True)
    torch.cuda.synchronize()
    if L % 4:
        lane = engine.impala_rollout(engine.ImpalaSpec(A, E, T, entropy=True, env_seed=5, fp16=True), lanes, L, seed,
                                     record=True)
        torch.cuda.synchronize()
        for f in ("actions", "probs", "reward", "entropy", "norm2"):
            np.testing.assert_array_equal(getattr(out, f).cpu().numpy(), getattr(lane, f).cpu().numpy(), err_msg=f)
    acts = out.actions.cpu().numpy().reshape(L, E, T)
    nb = oi.num_bn()
    ref = oi.follow_lanes(theta, table, idx, sign, 0.02, A, E, T, 5, np.zeros(nb, np.float32), np.ones(nb, np.float32),
                          acts)
    from oracle import rng as crng
    jig = np.stack([crng.jiggle(seed, np.uint64(l) * np.uint64(E) + np.arange(E, dtype=np.uint64)) for l in range(L)])
    _, _, amb = _check_vs_followed_oracle(out.probs.cpu().numpy().reshape(L, E, T, A), acts,
                                          out.reward.cpu().numpy().reshape(L, E) - jig,
                                          out.entropy.cpu().numpy().reshape(L, E), ref, seed, range(L), E, F16_RTOL)
    assert amb <= 0.01 * L * E * T
    np.testing.assert_array_equal(out.norm2.cpu().numpy()[0::2], out.norm2.cpu().numpy()[1::2])


def test_fp16_pair_core_sign_zero_lanes(engine, table):
    """fdr_impala_desc.pairs allows signs +-1 or 0 in any combination (include/fdr.h): an unperturbed (sign-0) lane
    of a pair sees theta alone.  The MFMA pair form zeroes its S X column (E adds exact zeros), so a sign-0 lane's
    recorded episode (with the entropy replay) is BITWISE the same whatever its pair's table
    offset, and a +-1 lane's the same whatever its partner's sign.  Step 0's probabilities agree with the per-lane
    form (f16(theta') per lane) within the fp16 tolerance, and the norms are the per-lane ones (0 for sign 0)."""
    A, T, E = 5, 40, 4
    theta = _theta(A)
    offs = np.array([77, 2_000_001, 999_999, 5], np.int64)
    signs = np.array([1, -1, 0, 0, 1, 0, 0, -1], np.int8)
    dev = "cuda"

    def run(offs_, signs_, pairs=True):
        idx = np.repeat(offs_, 2)
        lanes = engine.lanes_desc(torch.tensor(theta, device=dev), 0, torch.tensor(table, device=dev),
                                  torch.tensor(idx, device=dev), torch.tensor(signs_, device=dev), 0.02)
        spec = engine.ImpalaSpec(A, E, T, entropy=True, env_seed=5, fp16=True, pairs=pairs)
        o = engine.impala_rollout(spec, lanes, len(idx), 11, record=True)
        torch.cuda.synchronize()
        return {f: getattr(o, f).cpu().numpy() for f in ("actions", "probs", "reward", "entropy", "norm2")}

    a = run(offs, signs)
    b = run(offs[::-1].copy(), signs)                 # every pair at another table offset
    c = run(offs, np.array([1, -1] * 4, np.int8))     # every lane perturbed
    per_lane = run(offs, signs, pairs=False)

    def envs(x, lanes):
        return np.concatenate([x[l * E:(l + 1) * E] for l in lanes])
    for f in ("actions", "probs", "reward", "entropy"):
        np.testing.assert_array_equal(envs(a[f], [2, 3, 5, 6]), envs(b[f], [2, 3, 5, 6]), err_msg=f)
        np.testing.assert_array_equal(envs(a[f], [0, 1, 4, 7]), envs(c[f], [0, 1, 4, 7]), err_msg=f)
    np.testing.assert_array_equal(a["norm2"], per_lane["norm2"])
    assert np.all(a["norm2"][[2, 3, 5, 6]] == 0)
    np.testing.assert_allclose(a["probs"][:, 0], per_lane["probs"][:, 0], atol=2e-2)


@pytest.mark.parametrize("fp16", [False, True])
def test_pair_with_mismatched_offsets_poisons_its_norms(engine, table, fp16):
    """fdr_impala_desc.pairs requires both lanes of a pair on one table offset; a pair that breaks it gets NaN norms
    on both lanes (the FD step is poisoned visibly, as for an out-of-range offset) and no fault, and the other pairs'
    episodes are bitwise those of a batch without the violation."""
    A, T, E = 5, 20, 4
    theta = _theta(A)
    dev = "cuda"
    spec = engine.ImpalaSpec(A, E, T, entropy=True, env_seed=5, fp16=fp16, pairs=True)
    sign = torch.tensor(np.array([1, -1] * 4, np.int8), device=dev)

    def run(idx):
        lanes = engine.lanes_desc(torch.tensor(theta, device=dev), 0, torch.tensor(table, device=dev),
                                  torch.tensor(np.array(idx, np.int64), device=dev), sign, 0.02)
        o = engine.impala_rollout(spec, lanes, len(idx), 11, record=True)
        torch.cuda.synchronize()
        return {f: getattr(o, f).cpu().numpy() for f in ("actions", "probs", "reward", "entropy", "norm2")}
    bad = run([77, 77, 100, 200, 5, 5, 9, 9])
    good = run([77, 77, 100, 100, 5, 5, 9, 9])
    assert np.isnan(bad["norm2"][2]) and np.isnan(bad["norm2"][3])
    keep = [0, 1, 4, 5, 6, 7]
    assert np.all(np.isfinite(bad["norm2"][keep]))
    np.testing.assert_array_equal(bad["norm2"][keep], good["norm2"][keep])
    envs = np.concatenate([np.arange(l * E, (l + 1) * E) for l in keep])
    for f in ("actions", "probs", "reward", "entropy"):
        np.testing.assert_array_equal(bad[f][envs], good[f][envs], err_msg=f)


def test_strategies_pair_with_mismatched_offsets_poisons_its_probs(engine, table):
    """fdr_impala_strategies in the fp16 pair form with a pair whose two lanes carry different offsets
    returns NaN probabilities on both lanes (it would otherwise score lane 2p + 1 with lane 2p's noise); the other
    pairs' strategies are bitwise those of a batch without the violation."""
    A, Z = 5, 6
    theta = _theta(A)
    dev = "cuda"
    spec = engine.ImpalaSpec(A, fp16=True, pairs=True)
    sign = torch.tensor(np.array([1, -1] * 4, np.int8), device=dev)
    frames = torch.tensor(np.random.RandomState(3).randint(0, 256, size=(Z, 3, 64, 64)).astype(np.float32), device=dev)

    def run(idx):
        lanes = engine.lanes_desc(torch.tensor(theta, device=dev), 0, torch.tensor(table, device=dev),
                                  torch.tensor(np.array(idx, np.int64), device=dev), sign, 0.02)
        pr = engine.impala_strategies(spec, lanes, len(idx), frames)
        torch.cuda.synchronize()
        return pr.cpu().numpy()
    bad = run([77, 77, 100, 200, 5, 5, 9, 9])
    good = run([77, 77, 100, 100, 5, 5, 9, 9])
    assert np.all(np.isnan(bad[2:4]))
    assert np.all(np.isfinite(good))
    np.testing.assert_array_equal(bad[[0, 1, 4, 5, 6, 7]], good[[0, 1, 4, 5, 6, 7]])


@pytest.mark.parametrize("E,n_pairs", [(4, 3), (4, 4), (1, 6), (2, 2)])
def test_f32_pair_core_bit_identical(engine, table, E, n_pairs):
    """f32 pair form (fdr_impala_desc.pairs): w = fl32(theta + s fl32(sigma eps)) formed in registers is the
    per-lane pack's value bit for bit, and every env keeps core_kernel's fma chains -- whole episodes with the
    entropy replay are bitwise identical to the per-lane form (actions, probabilities, returns, entropies)."""
    A, T = 6, 40
    theta = _theta(A)
    offs = np.array([77, 2_000_000, 3_000_000, 4_500_000, 1_111_111, 999], np.int64)[:n_pairs]
    idx = np.repeat(offs, 2)
    sign = np.tile(np.array([1, -1], np.int8), n_pairs)
    dev = "cuda"
    lanes = engine.lanes_desc(torch.tensor(theta, device=dev), 0, torch.tensor(table, device=dev),
                              torch.tensor(idx, device=dev), torch.tensor(sign, device=dev), 0.02)
    o = [engine.impala_rollout(engine.ImpalaSpec(A, E, T, env_seed=5, pairs=pr), lanes, len(idx), 11, record=True)
         for pr in (False, True)]
    torch.cuda.synchronize()
    for f in ("actions", "probs", "reward", "entropy", "norm2"):
        np.testing.assert_array_equal(getattr(o[0], f).cpu().numpy(), getattr(o[1], f).cpu().numpy())


def _check_vs_followed_oracle(out_probs, out_acts, out_ret, out_ent, ref, seed, lane_ids, E, tol):
    """A kernel's recorded trajectories [L, E, T] against oi.follow_lanes along the same actions: every step's
    probabilities within tol (abs), the replayed entropy within tol (rel), returns equal up to the +-1e-12
    jiggle, and every sampled action equal to the inverse CDF of the REFERENCE probabilities at the step's
    counter uniform -- except where u * sum(p) lies closer to a partition boundary than the two probability
    vectors' largest cumulative difference (then the kernel's own, slightly different, probabilities may
    legitimately pick the neighbour; such a flip is explained, and counted).
    Returns (worst prob diff, worst rel entropy diff, explained flips)."""
    from oracle import rng as crng
    from oracle.policies import categorical_inverse_cdf
    T = out_acts.shape[2]
    dp = np.abs(out_probs - ref["probs"]).max()
    assert dp <= tol, dp
    de = np.abs(out_ent - ref["ent"]) / np.abs(ref["ent"])
    assert de.max() <= tol, de.max()
    np.testing.assert_allclose(out_ret - ref["ret"], 0.0, rtol=0, atol=2e-12)
    flips = 0
    for li, l in enumerate(lane_ids):
        envs = np.uint64(l) * np.uint64(E) + np.arange(E, dtype=np.uint64)
        for t in range(T):
            u = crng.uniform(seed, envs, t, 0)
            pr, pk = ref["probs"][li, :, t], out_probs[li, :, t]
            margin = oi.sample_margin(pr, u)
            dcs = np.abs(np.cumsum(pk.astype(np.float64), -1) - np.cumsum(pr.astype(np.float64), -1)).max(-1)
            for e in range(E):
                if out_acts[li, e, t] == categorical_inverse_cdf(pr[e], u[e]):
                    continue
                assert margin[e] <= dcs[e] + 1e-6, (l, e, t, out_acts[li, e, t], margin[e], dcs[e])
                flips += 1
    return dp, de.max(), flips


def test_fp16_pair_default_path_whole_episode_vs_f32_oracle(engine, table):
    """the kernels config 5 actually runs -- Worker.evaluate(antithetic) sets pairs, and the
    fp16 pair core is core_kernel_hpm2 (MFMA step: theta x + s (E x) on f16 fragment images) with the replay's
    input projection on xproj_pair_kernel and the chunked replay_chunk_hpm2.  2 antithetic pairs, A = 4, E = 4, T = 130 (the
    replay crosses two 64-step chunk boundaries), stochastic actions; the f32 oracle follows the kernel's own
    actions (policies/impala.py:136-186, worker/agent.py:20-71): per-step probabilities within 2e-2, replayed
    entropies within 2e-2, returns exact up to the jiggle, sampled actions consistent with the reference."""
    A, E, T, L, seed = 4, 4, 130, 4, 11
    theta = _theta(A)
    idx = np.repeat(np.array([555, 1_234_567], np.int64), 2)
    sign = np.tile(np.array([1, -1], np.int8), 2)
    dev = "cuda"
    lanes = engine.lanes_desc(torch.tensor(theta, device=dev), 0, torch.tensor(table, device=dev),
                              torch.tensor(idx, device=dev), torch.tensor(sign, device=dev), 0.02)
    spec = engine.ImpalaSpec(A, E, T, entropy=True, env_seed=5, fp16=True, pairs=True)
    out = engine.impala_rollout(spec, lanes, L, seed, record=True)
    torch.cuda.synchronize()
    acts = out.actions.cpu().numpy().reshape(L, E, T)
    nb = oi.num_bn()
    ref = oi.follow_lanes(theta, table, idx, sign, 0.02, A, E, T, 5, np.zeros(nb, np.float32),
                          np.ones(nb, np.float32), acts)
    from oracle import rng as crng
    jig = np.stack([crng.jiggle(seed, np.uint64(l) * np.uint64(E) + np.arange(E, dtype=np.uint64)) for l in range(L)])
    dp, de, amb = _check_vs_followed_oracle(out.probs.cpu().numpy().reshape(L, E, T, A), acts,
                                            out.reward.cpu().numpy().reshape(L, E) - jig,
                                            out.entropy.cpu().numpy().reshape(L, E), ref, seed, range(L), E, F16_RTOL)
    print("fp16 pair core: max |dp| %.3g, max rel d(ent) %.3g, %d / %d explained action flips" % (dp, de, amb, L * E * T))
    assert amb <= 0.01 * L * E * T


def test_fp16_conv_stack_forward_and_strategies_vs_oracle(engine, table):
    """VERDICT r5 item 4 (the conv-mode bitwise test re-pointed at the oracle): the fp16 conv stack (conv_kernel_h2,
    the only conv form) in the forward API -- 13 envs, ragged over the 8 XCD slots, non-trivial BN statistics, three
    steps of carried LSTM state -- and in fdr_impala_strategies (8 perturbed lanes in the pair form, 5 probe frames),
    against the f32 oracle: features, LSTM state and probabilities within the fp16 tolerance."""
    A = 4
    theta_np = _theta(A)
    theta = torch.tensor(theta_np, device="cuda")
    spec = engine.ImpalaSpec(A, fp16=True)
    g = torch.Generator().manual_seed(3)
    n = 13
    frames = (torch.rand(n, 3, 64, 64, generator=g) * 255).floor()
    reward = torch.randn(n, generator=g)
    nb = oi.num_bn()
    rm = torch.randn(nb, generator=g).mul(0.1)
    rv = torch.rand(nb, generator=g).add(0.5)
    p = oi.unflatten(theta_np, A)
    bn = oi.split_bn(rm.numpy(), rv.numpy())
    h = torch.zeros(n, 256, device="cuda")
    c = torch.zeros(n, 256, device="cuda")
    hr, cr = torch.zeros(n, oi.HID), torch.zeros(n, oi.HID)
    for t in range(3):
        fr = frames.roll(t, 0)
        probs, feat = engine.impala_forward(spec, theta, fr.cuda(), h, c, reward=reward.cuda(), bn_mean=rm.cuda(),
                                            bn_var=rv.cuda(), feat=True)
        torch.cuda.synchronize()
        pr, hr, cr, fe, _ = oi.forward(p, bn, fr.numpy(), reward.numpy(), hr, cr)
        for got, want in ((feat, fe), (h, hr), (c, cr)):
            w = want.numpy()
            assert np.abs(got.cpu().numpy() - w).max() <= F16_RTOL * max(1.0, np.abs(w).max())
        np.testing.assert_allclose(probs.cpu().numpy(), pr.numpy(), atol=F16_RTOL)
    idx = np.repeat(np.array([77, 2_000_000, 3_000_000, 999], np.int64), 2)
    sign = np.tile(np.array([1, -1], np.int8), 4)
    lanes = engine.lanes_desc(theta, 0, torch.tensor(table, device="cuda"), torch.tensor(idx, device="cuda"),
                              torch.tensor(sign, device="cuda"), 0.02)
    st = engine.impala_strategies(engine.ImpalaSpec(A, fp16=True, pairs=True), lanes, len(idx), frames[:5].cuda(),
                                  reward=reward[:5].cuda(), bn_mean=rm.cuda(), bn_var=rv.cuda())
    torch.cuda.synchronize()
    ref = oi.lane_strategies(theta_np, table, idx, sign, 0.02, A, frames[:5].numpy(), reward[:5].numpy(), rm.numpy(),
                             rv.numpy())
    np.testing.assert_allclose(st.cpu().numpy(), ref, atol=F16_RTOL)


# ---- the step plan: the rows no test above reaches, at the smallest shape that reaches them ----
_FIELDS = ("actions", "probs", "reward", "entropy", "norm2")


def _pair_batch(engine, table, theta, n_pairs):
    idx = np.repeat(np.array([77, 2_000_000, 3_000_000], np.int64)[:n_pairs], 2)
    sign = np.tile(np.array([1, -1], np.int8), n_pairs)
    lanes = engine.lanes_desc(torch.tensor(theta, device="cuda"), 0, torch.tensor(table, device="cuda"),
                              torch.tensor(idx, device="cuda"), torch.tensor(sign, device="cuda"), 0.02)
    return lanes, idx, sign


def _episode(engine, spec, lanes, L, seed=11):
    o = engine.impala_rollout(spec, lanes, L, seed, record=True)
    torch.cuda.synchronize()
    return {f: getattr(o, f).cpu().numpy().copy() for f in _FIELDS}


def _fp16_pair_episode_vs_f32_oracle(out, theta, table, idx, sign, A, E, T, seed=11, entropy=True):
    """The bounds of test_fp16_pair_form_episodes_vs_f32_oracle on one recorded batch."""
    from oracle import rng as crng
    L = len(idx)
    acts = out["actions"].reshape(L, E, T)
    nb = oi.num_bn()
    ref = oi.follow_lanes(theta, table, idx, sign, 0.02, A, E, T, 5, np.zeros(nb, np.float32), np.ones(nb, np.float32),
                          acts)
    jig = np.stack([crng.jiggle(seed, np.uint64(l) * np.uint64(E) + np.arange(E, dtype=np.uint64)) for l in range(L)])
    ent = out["entropy"].reshape(L, E)
    if not entropy:  # no replay ran: the entropy is reported as 0 and there is nothing to bound
        assert np.all(ent == 0.0)
        ent = ref["ent"]
    _, _, amb = _check_vs_followed_oracle(out["probs"].reshape(L, E, T, A), acts, out["reward"].reshape(L, E) - jig, ent,
                                          ref, seed, range(L), E, F16_RTOL)
    assert amb <= 0.01 * L * E * T
    np.testing.assert_array_equal(out["norm2"][0::2], out["norm2"][1::2])


@pytest.mark.parametrize("fp16,pairs", [(False, False), (False, True), (True, False), (True, True)])
def test_replay_chunk_tail_with_and_without_gemm(engine, table, fp16, pairs):
    """T = 65: the entropy replay crosses the 64-step chunk boundary with a one-step tail; 4 lanes x 1 env (one
    core_kernel_hpm2 workgroup).  With the input-projection GEMM on and off (fdr_ctx_set_replay_gemm) the f32 forms and
    the fp16 per-lane form run the same fma chains: whole recorded episodes bitwise identical, and the f32 pair form
    (core_kernel_p, then core_kernel_pr with the GEMM / core_kernel<kReplay> without) bitwise the per-lane form.  The
    fp16 pair form replays on replay_chunk_hpm2 with the GEMM and per lane (core_kernel_h<kReplay>) without: each within
    the pair form's bounds of the f32 oracle."""
    A, E, T, n_pairs = 5, 1, 65, 2
    theta = _theta(A)
    lanes, idx, sign = _pair_batch(engine, table, theta, n_pairs)
    L = len(idx)
    spec = engine.ImpalaSpec(A, E, T, entropy=True, env_seed=5, fp16=fp16, pairs=pairs)
    runs = {}
    try:
        for on in (1, 0):
            engine.context().set_replay_gemm(on)
            runs[on] = _episode(engine, spec, lanes, L)
    finally:
        engine.context().set_replay_gemm(True)
    if fp16 and pairs:
        for on in (1, 0):
            _fp16_pair_episode_vs_f32_oracle(runs[on], theta, table, idx, sign, A, E, T)
        return
    assert np.all(np.isfinite(runs[1]["entropy"])) and np.all(runs[1]["entropy"] != 0)
    for f in _FIELDS:
        np.testing.assert_array_equal(runs[1][f], runs[0][f], err_msg=f)
    if pairs:
        lane = _episode(engine, engine.ImpalaSpec(A, E, T, entropy=True, env_seed=5), lanes, L)
        for f in _FIELDS:
            np.testing.assert_array_equal(runs[1][f], lane[f], err_msg=f)


@pytest.mark.parametrize("fp16", [False, True])
def test_pair_form_without_entropy(engine, table, fp16):
    """The pair forms of the rollout step alone (entropy off: no projection, no replay), T = 3, 4 lanes x 1 env: f32
    bitwise the per-lane form, fp16 within the pair form's bounds of the f32 oracle."""
    A, E, T = 5, 1, 3
    theta = _theta(A)
    lanes, idx, sign = _pair_batch(engine, table, theta, 2)
    out = _episode(engine, engine.ImpalaSpec(A, E, T, entropy=False, env_seed=5, fp16=fp16, pairs=True), lanes, 4)
    if fp16:
        _fp16_pair_episode_vs_f32_oracle(out, theta, table, idx, sign, A, E, T, entropy=False)
        return
    lane = _episode(engine, engine.ImpalaSpec(A, E, T, entropy=False, env_seed=5), lanes, 4)
    for f in _FIELDS:
        np.testing.assert_array_equal(out[f], lane[f], err_msg=f)
    assert np.all(out["entropy"] == 0.0)


@pytest.mark.parametrize("fp16", [False, True])
def test_eight_envs_run_per_lane_under_pairs(engine, table, fp16):
    """E = 8 has no pair form: with fdr_impala_desc.pairs set the call runs the per-lane kernels, bitwise a pairs = False
    launch (T = 3 with the entropy replay, 4 lanes); the f32 episodes are the oracle's."""
    A, E, T = 5, 8, 3
    theta = _theta(A)
    lanes, idx, sign = _pair_batch(engine, table, theta, 2)
    o = [_episode(engine, engine.ImpalaSpec(A, E, T, entropy=True, env_seed=5, fp16=fp16, pairs=pr), lanes, 4)
         for pr in (False, True)]
    assert np.all(np.isfinite(o[1]["entropy"])) and np.all(o[1]["entropy"] > 0)
    for f in _FIELDS:
        np.testing.assert_array_equal(o[0][f], o[1][f], err_msg=f)
    if not fp16:
        out, ref = _run(engine, table, A, E, T, idx, sign, [0] * 4)
        _compare(out, ref, 4, E, T, A)
        np.testing.assert_array_equal(out.probs.cpu().numpy(), o[1]["probs"])


@pytest.mark.parametrize("fp16,pairs", [(False, False), (False, True), (True, False), (True, True)])
def test_full_size_rollout_properties(engine, fp16, pairs):
    """BASELINE configs 4/5 at full size (1024 lanes x 4 envs x T = 1000, A = 6 / 4): bitwise reproducible (a
    second launch that also records per-step probabilities / actions), antithetic lanes have identical
    ||lambda||^2, returns integer (+- jiggle) within [-T, T], entropies finite in (0, ln A] -- and (VERDICT r2
    item 2) sampled lanes {0, 1, 511, 1023} of the full launch, all 4 envs, whole 1000-step episodes, against the
    f32 oracle along the kernel's trajectories (worker/agent.py:20-71): f32 every step's probabilities and the
    entropies within 1e-5 and every sampled action the reference's (outside a 1e-5 boundary margin); fp16 the
    drift bound of config 5 (2e-2); returns exact up to the jiggle in both."""
    A = 4 if fp16 else 6
    L, E, T, seed = 1024, 4, 1000, 123
    theta = _theta(A)
    P = theta.size
    dev = "cuda"
    tab = torch.randn(25_000_000, generator=torch.Generator().manual_seed(124))
    idx_h = np.repeat(np.random.RandomState(4).randint(0, 25_000_000 - P, size=L // 2), 2)
    sign_h = np.tile(np.array([1, -1], np.int8), L // 2)
    lanes = engine.lanes_desc(torch.tensor(theta, device=dev), 0, tab.to(dev), torch.as_tensor(idx_h, device=dev),
                              torch.as_tensor(sign_h, device=dev), 0.02)
    spec = engine.ImpalaSpec(A, E, T, entropy=True, env_seed=5, fp16=fp16, pairs=pairs)
    outs = []
    for rec in (False, True):
        o = engine.impala_rollout(spec, lanes, L, seed, record=rec)
        torch.cuda.synchronize()
        outs.append([t.cpu().numpy().copy() for t in (o.reward, o.entropy, o.timesteps, o.norm2)])
    for a, b in zip(*outs):
        np.testing.assert_array_equal(a, b)
    ret, ent, steps, n2 = outs[0]
    assert np.all(steps == T)
    assert np.all(np.isfinite(ret)) and np.all(np.abs(ret) <= T + 1e-9)
    np.testing.assert_allclose(ret, np.round(ret), rtol=0, atol=2e-12)
    assert np.all(np.isfinite(ent)) and np.all(ent > 0) and np.all(ent <= np.log(A) + 1e-6)
    np.testing.assert_array_equal(n2[0::2], n2[1::2])
    assert np.all(n2 > 0)
    # sampled lanes against the oracle (each lane evaluated with its own global lane id)
    from oracle import rng as crng
    sample = [0, 1, 511, 1023]
    probs = o.probs.view(L, E, T, A)[sample].cpu().numpy()
    acts = o.actions.view(L, E, T)[sample].cpu().numpy()
    del o
    nb = oi.num_bn()
    table = tab.numpy()
    ref = {"probs": [], "ret": [], "ent": []}
    for k, l in enumerate(sample):
        r = oi.follow_lanes(theta, table, idx_h[l:l + 1], sign_h[l:l + 1], 0.02, A, E, T, 5,
                            np.zeros(nb, np.float32), np.ones(nb, np.float32), acts[k:k + 1], lane_offset=l)
        for key in ref:
            ref[key].append(r[key][0])
    ref = {k: np.stack(v) for k, v in ref.items()}
    jig = np.stack([crng.jiggle(seed, np.uint64(l) * np.uint64(E) + np.arange(E, dtype=np.uint64)) for l in sample])
    tol = F16_RTOL if fp16 else ATOL
    dp, de, amb = _check_vs_followed_oracle(probs, acts, ret.reshape(L, E)[sample] - jig, ent.reshape(L, E)[sample],
                                            ref, seed, sample, E, tol)
    print("full size fp16=%s pairs=%s: max |dp| %.3g, max rel d(ent) %.3g, %d / %d explained action flips"
          % (fp16, pairs, dp, de, amb, len(sample) * E * T))
    assert amb <= (0.01 if fp16 else 0.001) * len(sample) * E * T

