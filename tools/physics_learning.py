"""Learning measurement on the physics envs (DESIGN.md 7's tables; a measurement, no bar): SequentialRunner(physics=True,
batch_size=2048, antithetic=True) with the reference's hyperparameters for 300 epochs, once per weighting.  "train" is
the mean return of the epoch's sampled training lanes averaged over the 10 epochs before the row, "eval" the mean return
over 64 deterministic lanes of theta from 64 different resets, "done" the share of those 64 that reached the goal.
--episodes K / --crn {none,pair,batch}: the runner's episodes_per_lane and common_random_numbers -- every lane, the 64
eval lanes too, then returns the mean of K episodes, and "done" is the share of eval lanes with an episode that ended
before the time limit.
--weightings: the learner weightings to run, each "zscore", "centred_rank" or "top_directions:<b>" (b an int, or a
fraction of the directions such as 0.25).

    python tools/physics_learning.py [env_id ...] [--epochs 300] [--episodes K] [--crn none|pair|batch]
                                     [--weightings zscore centred_rank top_directions:0.25]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "dfd-starter_amd")):
    sys.path.insert(0, p)

from learner.finite_differences import parse_weighting  # noqa: E402
from run_sequential import SequentialRunner  # noqa: E402

IDS = ["Acrobot-v1", "MountainCar-v0", "MountainCarContinuous-v0"]
LABELS = {"zscore": "z-score", "centred_rank": "centred rank"}     # the tables' column names


def run(env_id, weighting, epochs, every, episodes=1, crn=False):
    weighting, top = parse_weighting(weighting)
    r = SequentialRunner(env_id=env_id, physics=True, batch_size=2048, antithetic=True, verbose=False,
                         episodes_per_lane=episodes, common_random_numbers=crn, weighting=weighting,
                         top_directions=top)
    launch = r.worker.launch
    train, rows = [], []

    def evaluate(epoch):
        n = 64
        res = launch(np.zeros(n, np.int64), np.zeros(n, np.int8), np.ones(n, np.int8), seed=100000 + epoch,
                     jiggle=False)[0]
        ret, steps = res.reward.cpu().numpy(), res.timesteps.cpu().numpy()
        recent = np.mean(train[-10:]) if train else float("nan")
        rows.append((epoch, recent, float(ret.mean()), float((steps < episodes * r.env.episode_len).mean())))

    def spy(idx, sign, det, **kw):
        if len(train) % every == 0:
            evaluate(len(train))
        out = launch(idx, sign, det, **kw)
        train.append(float(out[0].reward[torch.as_tensor(sign != 0, device=out[0].reward.device)].mean().item()))
        return out
    r.worker.launch = spy
    t0 = time.perf_counter()
    r.train(epochs)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    evaluate(epochs)
    return rows, wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("env_ids", nargs="*", default=IDS)
    ap.add_argument("--epochs", type=int, default=300)
    ap.add_argument("--every", type=int, default=50)
    ap.add_argument("--episodes", type=int, default=1)
    ap.add_argument("--crn", choices=("none", "pair", "batch"), default="none")
    ap.add_argument("--weightings", nargs="+", default=["zscore", "centred_rank"])
    a = ap.parse_args()
    crn = False if a.crn == "none" else a.crn
    for env_id in a.env_ids:
        res = [run(env_id, w, a.epochs, a.every, a.episodes, crn) for w in a.weightings]
        names = [LABELS.get(w, w) for w in a.weightings]
        print("%s, K = %d, crn %s: %d epochs, wall %s"
              % (env_id, a.episodes, a.crn, a.epochs,
                 " / ".join("%.1f s (%s)" % (r[1], w) for w, r in zip(names, res))))
        print("| epoch | " + " | ".join("%s: train | %s: eval (done)" % (w, w) for w in names) + " |")
        print("|---|" + "---|---|" * len(a.weightings))
        for rows in zip(*(r[0] for r in res)):
            print("| %d | " % rows[0][0] + " | ".join("%.1f | %.1f (%.0f %%)" % (x[1], x[2], 100 * x[3]) for x in rows)
                  + " |", flush=True)


if __name__ == "__main__":
    main()
