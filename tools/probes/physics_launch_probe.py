"""Launch time of the physics-env rollouts (DESIGN.md 3.1's table): 4096 antithetic lanes of a random-init policy with
sampled actions, HIP events around the launch, median of 40 after 3 warm-ups.

    python tools/probes/physics_launch_probe.py [env ...]      (default: all five)
    python tools/probes/physics_launch_probe.py --episodes 8 cartpole pendulum
        one K-episode launch of rollout_episodes_kernel against K one-episode launches of rollout_kernel (lane_offset
        = e * L, so both play the same number of fresh episodes), same process, same medians
"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (REPO, os.path.join(REPO, "dfd-starter_amd")):
    sys.path.insert(0, p)

import envs  # noqa: E402
from fdr import engine  # noqa: E402
from oracle import noise as onoise  # noqa: E402
from oracle import policies as opol  # noqa: E402

ENVS = {"cartpole": ("discrete", envs.CartPoleEnv), "pendulum": ("mujoco", envs.PendulumEnv),
        "acrobot": ("discrete", envs.AcrobotEnv), "mountaincar": ("discrete", envs.MountainCarEnv),
        "mountaincar_cont": ("mujoco", envs.MountainCarContinuousEnv)}
L, WARM, REPS, SIGMA = 4096, 3, 40, 0.02


def timed(fn):
    ms = []
    for i in range(WARM + REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(i)
        b.record()
        b.synchronize()
        if i >= WARM:
            ms.append(a.elapsed_time(b))
    return float(np.median(ms)), min(ms), max(ms)


def episodes(names, K):
    dev = torch.device("cuda", 0)
    for name in names:
        kind, cls = ENVS[name]
        env = cls()
        theta = opol.TorchPolicy(kind, env.obs_dim, env.act_dim, seed=124).get_flat()
        tab = onoise.NoiseTable(1 << 22, theta.size, 124)
        idx = np.repeat(tab.sample_indices(L // 2), 2)
        sign = np.tile(np.array([1, -1], np.int8), L // 2)
        spec = engine.PolicySpec(kind, env.obs_dim, env.act_dim, theta.size)
        dv = [torch.from_numpy(a).to(dev) for a in (theta, tab.table, idx, sign)]
        lanes = [engine.lanes_desc(dv[0], 0, dv[1], dv[2], dv[3], SIGMA, lane_offset=e * L) for e in range(K)]
        out = engine.rollout(spec, env, lanes[0], L, 11)
        out_k = engine.rollout_episodes(spec, env, lanes[0], L, 11, K)

        def parent(i):
            for e in range(K):
                engine.rollout(spec, env, lanes[e], L, 11 + i, out=out)

        one = timed(lambda i: engine.rollout(spec, env, lanes[0], L, 11 + i, out=out))
        many = timed(parent)
        new = timed(lambda i: engine.rollout_episodes(spec, env, lanes[0], L, 11 + i, K, out=out_k))
        steps = out_k.timesteps.cpu().numpy()
        print("%-17s T %4d  K %d  rollout x1 %.3f ms  rollout x%d %.3f ms (%.3f-%.3f)  rollout_episodes %.3f ms "
              "(%.3f-%.3f)  ratio %.3f  steps per lane mean %.1f"
              % (name, env.episode_len, K, one[0], K, many[0], many[1], many[2], new[0], new[1], new[2],
                 new[0] / many[0], steps.mean()), flush=True)


def main(names):
    dev = torch.device("cuda", 0)
    for name in names:
        kind, cls = ENVS[name]
        env = cls()
        theta = opol.TorchPolicy(kind, env.obs_dim, env.act_dim, seed=124).get_flat()
        tab = onoise.NoiseTable(1 << 22, theta.size, 124)
        idx = np.repeat(tab.sample_indices(L // 2), 2)
        sign = np.tile(np.array([1, -1], np.int8), L // 2)
        spec = engine.PolicySpec(kind, env.obs_dim, env.act_dim, theta.size)
        lanes = engine.lanes_desc(torch.from_numpy(theta).to(dev), 0, torch.from_numpy(tab.table).to(dev),
                                  torch.from_numpy(idx).to(dev), torch.from_numpy(sign).to(dev), SIGMA)
        out = engine.rollout(spec, env, lanes, L, 11)
        ms = []
        for i in range(WARM + REPS):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            engine.rollout(spec, env, lanes, L, 11 + i, out=out)
            b.record()
            b.synchronize()
            if i >= WARM:
                ms.append(a.elapsed_time(b))
        steps = out.timesteps.cpu().numpy()
        med = float(np.median(ms))
        print("%-17s T %4d  launch %.3f ms (%.3f-%.3f)  steps per lane mean %.1f max %d  per lane-step %.3f ns"
              % (name, env.episode_len, med, min(ms), max(ms), steps.mean(), steps.max(),
                 1e6 * med / float(steps.sum())), flush=True)


if __name__ == "__main__":
    args = sys.argv[1:]
    if "--episodes" in args:
        k = args.index("--episodes")
        n_ep = int(args[k + 1])
        del args[k:k + 2]
        episodes(args or list(ENVS), n_ep)
    else:
        main(args or list(ENVS))
