"""Speed of the thread-per-lane linear rollout against the wave-per-lane MLP rollout, CartPole physics, T = 500.

One process, one GPU.  After one warm-up launch of each, ROUNDS rounds alternate between
    linear   rollout_linear_kernel<cartpole> at 65,536 and at 1,048,576 lanes, theta = N(0, 1), sigma = 1 (64 different
             controllers per wave: episodes end between ~8 and 500 steps)
    mlp      rollout_kernel<cartpole> (DiscretePolicy(4, 2), sampled actions, sigma = 0.02) at 65,536 lanes
each timed with device events around the one launch, then a synchronise.  Reported per launch: milliseconds, env
steps/s from the summed `steps`, lanes/s; then the medians and the spread, and whether the linear launch at 65,536
lanes took less time than the MLP launch in every round (the one condition set for this kernel: it does at least 30
times less arithmetic per lane-step and runs 64 lanes per wave).  One JSON line at the end.

Usage: python tools/bench_linear.py [--rounds 3] [--steps 500]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "dfd-starter_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from envs import CartPoleEnv  # noqa: E402
from fdr import engine  # noqa: E402
from policies import DiscretePolicy  # noqa: E402

DEV = torch.device("cuda", 0)
TABLE = 1 << 22


def make_lanes(theta, table, n, sigma, seed):
    rs = np.random.RandomState(seed)
    idx = torch.as_tensor(rs.randint(0, TABLE - theta.numel() + 1, size=n).astype(np.int64), device=DEV)
    sign = torch.as_tensor(np.where(np.arange(n) % 2 == 0, 1, -1).astype(np.int8), device=DEV)
    return engine.lanes_desc(theta, 0, table, idx, sign, sigma)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    res = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), int(res.timesteps.sum(dtype=torch.int64).item())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=500)
    args = ap.parse_args()
    env = CartPoleEnv(args.steps)
    table = torch.as_tensor(np.random.RandomState(1).randn(TABLE).astype(np.float32), device=DEV)
    lin_theta = torch.as_tensor(np.random.RandomState(2).randn(8).astype(np.float32), device=DEV)
    lin_spec = engine.PolicySpec("linear", 4, 2, 8)
    mlp = DiscretePolicy(4, 2, seed=124, device=DEV)
    bm, bv = mlp.bn_stats()
    configs = {
        "linear_65536": (65536, lambda lanes, n: engine.rollout(lin_spec, env, lanes, n, 7, device=DEV),
                         make_lanes(lin_theta, table, 65536, 1.0, 3)),
        "linear_1048576": (1 << 20, lambda lanes, n: engine.rollout(lin_spec, env, lanes, n, 7, device=DEV),
                           make_lanes(lin_theta, table, 1 << 20, 1.0, 4)),
        "mlp_65536": (65536, lambda lanes, n: engine.rollout(mlp.spec, env, lanes, n, 7, bn_mean=bm, bn_var=bv,
                                                             device=DEV),
                      make_lanes(mlp.flat, table, 65536, 0.02, 5)),
    }
    for name, (n, fn, lanes) in configs.items():      # warm-up
        timed(lambda: fn(lanes, n))
    rows = {k: [] for k in configs}
    for r in range(args.rounds):
        for name, (n, fn, lanes) in configs.items():
            ms, steps = timed(lambda: fn(lanes, n))
            rows[name].append((ms, steps))
            print("round %d %-15s %9.3f ms  %12d env steps  %.4g steps/s  %.4g lanes/s"
                  % (r, name, ms, steps, steps / (ms * 1e-3), n / (ms * 1e-3)))
    out = {"metric": "linear_rollout_cartpole", "rounds": args.rounds, "T": args.steps}
    for name, (n, _, _) in configs.items():
        ms = np.array([x[0] for x in rows[name]])
        steps = rows[name][0][1]
        out[name] = {"lanes": n, "ms_median": float(np.median(ms)), "ms_min": float(ms.min()), "ms_max": float(ms.max()),
                     "env_steps": steps, "steps_per_s": steps / (float(np.median(ms)) * 1e-3),
                     "lanes_per_s": n / (float(np.median(ms)) * 1e-3)}
    faster = [a[0] < b[0] for a, b in zip(rows["linear_65536"], rows["mlp_65536"])]
    out["linear_faster_than_mlp_every_round"] = bool(all(faster))
    print(json.dumps(out))
    return 0 if all(faster) else 1


if __name__ == "__main__":
    sys.exit(main())
