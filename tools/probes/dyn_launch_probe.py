"""Launch time of the runtime-shaped rollout kernel against the compiled ones (DESIGN.md 3.1's table): antithetic lanes
of a random-init policy with sampled actions on the synthetic env, HIP events around the launch, median of 40 after 3
warm-ups; one process, one build.

    python tools/probes/dyn_launch_probe.py

"generic" against "single" (the yardstick: the compiled one-lane kernel) and "auto" at (17, 6) with 4096 lanes, T =
1000 and (4, 2) with 1024 lanes, T = 500; "generic" alone at (24, 4) and (64, 8) with 4096 lanes, T = 1000.
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

# (kind, n_in, n_act, lanes, T, impls)
CASES = [("mujoco", 17, 6, 4096, 1000, ("single", "auto", "generic")),
         ("discrete", 4, 2, 1024, 500, ("single", "auto", "generic")),
         ("mujoco", 24, 4, 4096, 1000, ("generic",)),
         ("mujoco", 64, 8, 4096, 1000, ("generic",))]
WARM, REPS, SIGMA = 3, 40, 0.02


def main():
    dev = torch.device("cuda", 0)
    ctx = engine.context(dev)
    for kind, n_in, n_act, L, T, impls in CASES:
        env = envs.SyntheticEnv(n_in, n_act, kind == "discrete", T, device=dev)
        theta = opol.TorchPolicy(kind, n_in, n_act, seed=124).get_flat()
        tab = onoise.NoiseTable(1 << 22, theta.size, 124)
        idx = np.repeat(tab.sample_indices(L // 2), 2)
        sign = np.tile(np.array([1, -1], np.int8), L // 2)
        spec = engine.PolicySpec(kind, n_in, n_act, theta.size)
        lanes = engine.lanes_desc(torch.from_numpy(theta).to(dev), 0, torch.from_numpy(tab.table).to(dev),
                                  torch.from_numpy(idx).to(dev), torch.from_numpy(sign).to(dev), SIGMA)
        base = None
        for impl in impls:
            ctx.set_rollout_impl(impl)
            try:
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
            finally:
                ctx.set_rollout_impl("auto")
            med = float(np.median(ms))
            if impl == "single":
                base = med
            ratio = "" if base is None else "  x%.2f of single" % (med / base)
            print("(%2d, %2d)%s %5d lanes T %4d  %-7s launch %.3f ms (%.3f-%.3f)  per lane-step %.3f ns%s"
                  % (n_in, n_act, "d" if kind == "discrete" else "c", L, T, impl, med, min(ms), max(ms),
                     1e6 * med / (L * T), ratio), flush=True)


if __name__ == "__main__":
    main()
