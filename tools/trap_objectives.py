"""The deceptive trap gridworld under the two learner objectives (a measurement, no bar): the same
SequentialRunner(env_id="SimpleTrapEnv-v0") from the same seed for --epochs epochs, once with objective="reward" (the
reference's step) and once with objective="mixed" (adaptive omega with the runner's defaults, --ent-coef).  A row every
--every epochs: the eval EMA of the policy's reward and novelty, the mean training return of the 10 epochs before the
row, omega.

    python tools/trap_objectives.py [--epochs 300] [--batch-size 64] [--seed 123]
"""
import argparse
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "dfd-starter_amd")):
    sys.path.insert(0, p)

from run_sequential import SequentialRunner  # noqa: E402


def run(objective, a):
    r = SequentialRunner(env_id="SimpleTrapEnv-v0", objective=objective, batch_size=a.batch_size, random_seed=a.seed,
                         eval_prob=a.eval_prob, ent_coef=a.ent_coef if objective == "mixed" else 0.0,
                         noise_table_size=1 << 22, verbose=False)
    t0 = time.perf_counter()
    r.train(a.epochs)
    wall = time.perf_counter() - t0
    h = r.history
    rows = []
    for k in list(range(a.every - 1, len(h), a.every)) or [len(h) - 1]:
        rows.append((h[k]["Epoch"], h[k]["Policy Reward"], float(np.mean([e["Noisy Reward"] for e in h[max(0, k - 9):k + 1]])),
                     h[k]["Policy Novelty"], h[k]["Omega"]))
    return rows, wall, max(e["Noisy Reward"] for e in h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=300)
    ap.add_argument("--every", type=int, default=50)
    ap.add_argument("--batch-size", type=int, default=64)
    ap.add_argument("--eval-prob", type=float, default=0.05)
    ap.add_argument("--ent-coef", type=float, default=0.01)
    ap.add_argument("--seed", type=int, default=123)
    a = ap.parse_args()
    res = {o: run(o, a) for o in ("reward", "mixed")}
    print("SimpleTrapEnv-v0, %d epochs, batch %d, seed %d: wall %.1f s (reward) / %.1f s (mixed); best epoch mean return "
          "%.3f / %.3f" % (a.epochs, a.batch_size, a.seed, res["reward"][1], res["mixed"][1], res["reward"][2],
                           res["mixed"][2]))
    print("| epoch | reward: policy / train | mixed: policy / train | mixed: policy novelty | mixed: omega |")
    print("|---|---|---|---|---|")
    for x, m in zip(res["reward"][0], res["mixed"][0]):
        print("| %d | %.3f / %.3f | %.3f / %.3f | %.4f | %.3f |" % (x[0], x[1], x[2], m[1], m[2], m[3], m[4]), flush=True)


if __name__ == "__main__":
    main()
