"""The sharded mixed-objective FD step against the single process, on ONE GPU (2 gloo ranks share cuda:0).

    python tools/dist_check_mix.py single <out_dir>       # 1 process -> <out_dir>/theta_single.npy
    python -m torch.distributed.run --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29561 \
        tools/dist_check_mix.py multi <out_dir>           # 2 ranks   -> <out_dir>/theta_rank{r}.npy
    python tools/dist_check_mix.py compare <out_dir>

The same seeded synthetic batches (no rollout: table offsets, rewards, novelties and entropies drawn from a seed,
||lambda||^2 from fdr_fd_lambda_norms) go through FiniteDifferences(objective="mixed").step with omega = 0.4 and
ent_coef = 0.05; each rank holds its lane_range slice.  Step 0: an FDBatch whose split every rank knows
(rank_lanes); step 1: an FDBatch without it (the counts are exchanged first); step 2: lists of FDReturn, split
30 % / 70 % (fdr_fd_weights_mix + fdr_fd_grad_lambda).  Every step is one all-gather of the three channels stacked
and one all-reduce of g.  tests/test_gpu_learner_mix.py drives it: the ranks end bitwise equal, and within 1e-6 of
the single process (the all-reduce only changes the summation order)."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "dfd-starter_amd")]
N_DIRS, LPD, STEPS = 48, 2, 3
OMEGA, ENT_COEF, SIGMA = 0.4, 0.05, 0.02
POLICY = (0.25, 0.2, 1.3)


def run(mode, out):
    import numpy as np
    import torch
    import torch.distributed as dist
    rank, world = int(os.environ.get("RANK", "0")), 1
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if mode == "multi":
        dist.init_process_group("gloo")
        world = dist.get_world_size()
    from dsgd import DSGD
    from fdr import dist as fdist
    from fdr import engine
    from learner import FDBatch, FiniteDifferences
    from policies import MujocoPolicy
    from utils import AdaptiveOmega, SharedNoiseTable
    torch.manual_seed(124)
    policy = MujocoPolicy(17, 6, seed=124, device=dev)
    P = policy.num_params
    table = SharedNoiseTable(1 << 22, P, random_seed=124)
    omega = AdaptiveOmega(default_value=OMEGA, min_value=OMEGA, max_value=OMEGA)
    learner = FiniteDifferences(policy, DSGD(policy.parameters(), lr=0.01), omega, table, noise_std=SIGMA,
                                ent_coef=ENT_COEF, objective="mixed")
    tab_d = table.device_table(dev)
    n = N_DIRS * LPD
    upd = []
    for step in range(STEPS):
        rs = np.random.RandomState(4000 + step)
        idx = np.repeat(rs.randint(0, (1 << 22) - P, size=N_DIRS).astype(np.int64), LPD)
        sign = np.tile(np.array([1, -1], np.int8), N_DIRS)
        rew = rs.randn(n) * 3 + 1
        nov = 0.3 * np.abs(rs.randn(n))
        ent = 1.4 + 0.05 * rs.randn(n)
        if step < 2:
            lo, hi = fdist.lane_range(N_DIRS, LPD, world, rank)
        else:   # the list route: any split of the returns will do
            cut = (3 * n) // 10
            lo, hi = (0, n) if world == 1 else ((0, cut) if rank == 0 else (cut, n))
        idx_d, sign_d = torch.as_tensor(idx[lo:hi], device=dev), torch.as_tensor(sign[lo:hi], device=dev)
        n2 = engine.fd_lambda_norms(tab_d, idx_d, sign_d, None, SIGMA, None, P)
        b = FDBatch(torch.as_tensor(rew[lo:hi], device=dev), torch.as_tensor(ent[lo:hi], device=dev), None, n2, idx_d,
                    sign_d, idx[lo:hi], sign[lo:hi], learner.epoch, lanes_per_dir=LPD,
                    novelty=torch.as_tensor(nov[lo:hi], device=dev))
        if step == 0 and world > 1:
            b.rank_lanes = [b - a for a, b in (fdist.lane_range(N_DIRS, LPD, world, r) for r in range(world))]
        if step == 2:
            b.timesteps = torch.zeros(hi - lo, dtype=torch.int32, device=dev)
            rets = b.to_returns()
            for r in rets:
                r.epoch = learner.epoch
            upd.append(learner.step(rets, *POLICY))
        else:
            upd.append(learner.step(b, *POLICY))
    os.makedirs(out, exist_ok=True)
    name = "single" if mode == "single" else "rank%d" % rank
    np.save(os.path.join(out, "theta_%s.npy" % name), policy.get_trainable_flat())
    np.save(os.path.join(out, "upd_%s.npy" % name), np.asarray(upd))
    if mode == "multi":
        dist.destroy_process_group()


def compare(out, world=2):
    """-> max |theta_2rank - theta_1rank|; raises if the ranks differ."""
    import numpy as np
    single = np.load(os.path.join(out, "theta_single.npy"))
    ranks = [np.load(os.path.join(out, "theta_rank%d.npy" % r)) for r in range(world)]
    for r in ranks[1:]:
        assert r.tobytes() == ranks[0].tobytes(), "ranks diverged"
    err = float(np.abs(ranks[0] - single).max())
    print("mixed objective: max |theta_%drank - theta_1rank| = %.3e" % (world, err))
    return err


if __name__ == "__main__":
    if sys.argv[1] == "compare":
        assert compare(sys.argv[2]) <= 1e-6
        print("dist_check_mix ok")
    else:
        run(sys.argv[1], sys.argv[2])
