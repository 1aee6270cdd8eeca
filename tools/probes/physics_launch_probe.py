"""Launch time of the physics-env rollouts (DESIGN.md 3.1's table): 4096 antithetic lanes of a random-init policy with
sampled actions, HIP events around the launch, median of 40 after 3 warm-ups.

    python tools/probes/physics_launch_probe.py [env ...]      (default: all five)
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
    main(sys.argv[1:] or list(ENVS))
