"""Evaluation noise of a +-pair difference on CartPole-v1, on the CPU restatement (DESIGN.md 3.1's variance table).

A random-init DiscretePolicy(4, 2), 32 sampled +eps / -eps pairs at sigma = 0.02, T = 500: the variance over the 32
pairs of R+ - R- when each lane plays under its own random stream or the partners share one, for 1 episode and for the
mean of K.  The episodes are oracle.agent.evaluate_lanes on tests/physics_ref.BatchedCartPole with lane_ids = the
stream ids of worker.episode_stream_ids -- what fdr_rollout_episodes runs on the device.  No GPU.

    python tools/crn_variance.py [--seeds 71 72 74] [--episodes 3]
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "dfd-starter_amd"), os.path.join(REPO, "tests")):
    sys.path.insert(0, p)

import physics_ref as ref  # noqa: E402
from oracle import agent as oagent  # noqa: E402
from oracle import noise as onoise  # noqa: E402
from oracle import policies as opol  # noqa: E402

N_PAIRS, SIGMA, T = 32, 0.02, 500


def pair_ids(mode, L, K):
    """The id rule of worker.episode_stream_ids (restated here: the worker module loads the device library)."""
    g = np.arange(L, dtype=np.int64)
    first = g - g % 2 if mode == "pair" else g
    return first[:, None] * K + np.arange(K, dtype=np.int64)[None, :]


def mean_returns(theta, tab, idx, sign, seed, mode, K):
    L = len(idx)
    ids = pair_ids(mode, L, K)
    total = np.zeros(L)
    for e in range(K):
        lanes = ids[:, e].astype(np.uint64)
        env = ref.BatchedCartPole(L, seed, lanes, T)
        total = total + oagent.evaluate_lanes("discrete", 4, 2, theta, tab.table, idx, sign, SIGMA, env, seed,
                                              jiggle=False, lane_ids=lanes)[0]
    return total / K


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, nargs="*", default=[71, 72, 74])
    ap.add_argument("--episodes", type=int, default=3)
    a = ap.parse_args()
    theta = opol.TorchPolicy("discrete", 4, 2, seed=124).get_flat()
    tab = onoise.NoiseTable(1 << 20, theta.size, 124)
    idx = np.repeat(np.random.RandomState(6).randint(0, tab.max_idx, size=N_PAIRS).astype(np.int64), 2)
    sign = np.tile(np.array([1, -1], np.int8), N_PAIRS)
    rows = (("own stream per lane, 1 episode", False, 1), ("partners share one stream, 1 episode", "pair", 1),
            ("own streams, mean of %d episodes" % a.episodes, False, a.episodes),
            ("partners share streams, mean of %d episodes" % a.episodes, "pair", a.episodes))
    print("| evaluation | variance of (R+ - R-) over the %d pairs, seeds %s | pairs with R+ = R- |"
          % (N_PAIRS, " / ".join(map(str, a.seeds))))
    print("|---|---|---|")
    for label, mode, K in rows:
        var, same = [], []
        for seed in a.seeds:
            r = mean_returns(theta, tab, idx, sign, seed, mode, K)
            d = r[0::2] - r[1::2]
            var.append(float(np.var(d)))
            same.append(int((d == 0).sum()))
        print("| %s | %s | %s |" % (label, " / ".join("%.3g" % v for v in var), " / ".join(map(str, same))),
              flush=True)


if __name__ == "__main__":
    main()
