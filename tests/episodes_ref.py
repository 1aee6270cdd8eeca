"""CPU reference of fdr_rollout_episodes (K episodes per lane, caller-chosen random streams).

Episode e of lane l is the episode the one-lane kernel runs for global lane id id(l, e), so the reference is K calls of
oracle.agent.evaluate_lanes (through test_gpu_physics_envs.cartpole_oracle, which adds the borderline flags) with
lane_ids = id(:, e), folded by the entry's formulas:

  ret   = (((R_0 + R_1) + ...) + R_{K-1}) / K        ret_sq = sum_e R_e^2
  steps = sum_e n_e                                  ent    = (sum_e S_e) / steps,  S_e = ent_e * n_e

expected_ids is the id rule of worker.episode_stream_ids written out lane by lane.
"""
import functools

import numpy as np

CASE_LANES = 62           # case_short(62): 31 sampled +- pairs
CASE_K = 3
# (mode, seed) of the oracle comparisons and the borderline lanes each has on the CPU restatement
ORACLE_CASES = (("pair", 71, 0), ("pair", 72, 0), ("pair", 74, 0), (False, 71, 1), ("batch", 72, 0))


def expected_ids(mode, sign, lane_offset, K, lanes_per_dir):
    """[n, K] int64 stream ids; for mode False the kernel's default rule (what it computes without an array)."""
    out = np.zeros((len(sign), K), np.int64)
    for l in range(len(sign)):
        g = lane_offset + l
        for e in range(K):
            if mode == "batch":
                out[l, e] = e
            elif mode == "pair" and sign[l] != 0:
                out[l, e] = (g - g % lanes_per_dir) * K + e
            else:
                out[l, e] = g * K + e
    return out


def fold(episodes):
    """Per-episode dicts (ret, ent, steps, norm2, borderline[, stats]) -> the entry's per-lane outputs."""
    K = len(episodes)
    rsum = np.zeros_like(episodes[0]["ret"])
    rsq = np.zeros_like(rsum)
    esum = np.zeros_like(rsum)
    steps = np.zeros(len(rsum), np.int64)
    border = np.zeros(len(rsum), bool)
    for ep in episodes:
        r = np.asarray(ep["ret"], np.float64)
        rsum = rsum + r
        rsq = rsq + r * r
        esum = esum + np.asarray(ep["ent"], np.float64) * ep["steps"]
        steps += ep["steps"]
        border |= ep.get("borderline", False)
    return dict(ret=rsum / float(K), ret_sq=rsq, steps=steps.astype(np.int32), ent=esum / steps,
                norm2=episodes[0]["norm2"], borderline=border)


@functools.lru_cache(maxsize=None)
def cartpole_case(mode, seed, K=CASE_K, L=CASE_LANES, T=500):
    """The CartPole comparison of one (mode, seed): case_short(L) lanes, ids by expected_ids at lane_offset 0 with
    +- pairs -> (lanes, ids, folded reference).  Computed once per process."""
    from test_gpu_physics_envs import cartpole_oracle, case_short
    idx, sign, det = case_short(L)
    ids = expected_ids(mode, sign, 0, K, 2)
    eps = [cartpole_oracle(idx, sign, det, seed, T=T, lane_ids=ids[:, e]) for e in range(K)]
    return (idx, sign, det), ids, fold(eps)
