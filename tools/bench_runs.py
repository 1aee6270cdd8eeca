"""Run batches against R solo sequences: CartPole-v1, T = 500, D = 256 antithetic directions, b = 64, observation
normalisation on (the README's ARS-V2 example), for R in {1, 16, 128, 1024}.

    population   PopulationRunner.train: one epoch of all R runs in a fixed number of launches
    solo         the same engine-level epoch issued R times in sequence -- noise_fill, rollout_episodes,
                 obs_stats_merge, fd_step_top per run -- without host syncs, from the same theta (zero); its
                 policy_reward stays the host constant 0 (fd_step_top takes a host scalar; an EMA would need a sync)

After 5 warm-up epochs each, 20 epochs are timed between two device events with one synchronise at the end; the two
alternate for three rounds in one process.  Prints one JSON line per R: ms per epoch and run-epochs per second of
both, and solo / population per round.  At R >= 16 the population must be the faster one in every round (exit 1
otherwise); R = 1 is reported only.

    python tools/bench_runs.py [--runs 1,16,128,1024] [--epochs 20] [--warmup 5] [--rounds 3]
"""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "dfd-starter_amd"))

from fdr import engine  # noqa: E402
import run_population as rp  # noqa: E402

D, B, T, EVAL = 256, 64, 500, 8


class SoloSequences(object):
    """R solo runs stepped one after another with the existing single-run entries, all state on the device."""

    def __init__(self, pop):
        self.pop = pop
        dev = pop.device
        R, L, P = pop.n_runs, pop.lanes_per_run, pop.n_params
        self.theta = [torch.zeros(P, dtype=torch.float32, device=dev) for _ in range(R)]
        self.rows = torch.empty(D * pop.row_stride, dtype=torch.float32, device=dev)
        self.idx = pop._idx[:L].clone()          # run 0's lanes: offsets into one run's rows
        self.sign = pop._sign[:L].clone()
        self.acc = [(torch.zeros(pop.spec.n_in, dtype=torch.float32, device=dev),
                     torch.zeros(pop.spec.n_in, dtype=torch.float32, device=dev),
                     torch.zeros(1, dtype=torch.int64, device=dev)) for _ in range(R)]
        self.norm = [rp.obs_norm_from_stats(a[0][None], a[1][None], a[2]) for a in self.acc]
        self.res = engine._rollout_outputs(L, dev)
        self.g = torch.empty(P, dtype=torch.float64, device=dev)
        self.out = torch.empty(2, dtype=torch.float64, device=dev)
        self.epoch = 0

    def train(self, n_epochs):
        pop = self.pop
        L, n_train, lpd = pop.lanes_per_run, pop.n_train, pop.lanes_per_dir
        for _ in range(n_epochs):
            e = self.epoch
            for r in range(pop.n_runs):
                seed = int(pop.seeds[r])
                engine.noise_fill(pop.launch_seed, D, pop.n_params, pop.row_stride, first_id=(seed << 32) + e * D,
                                  out=self.rows)
                lanes = engine.lanes_desc(self.theta[r], 0, self.rows, self.idx, self.sign, float(pop.noise_std[r]),
                                          lane_offset=seed * L)
                om, osd = self.norm[r]
                res = engine.rollout_episodes(pop.spec, pop.env, lanes, L, rp.launch_key(pop.launch_seed, e), 1,
                                              jiggle=True, obs_mean=om[0], obs_std=osd[0],
                                              obs_stats=rp.OBS_STATS_CHANCE, out=self.res, device=pop.device)
                engine.obs_stats_merge(res.obs_mean, res.obs_m2, res.obs_count, *self.acc[r])
                self.norm[r] = rp.obs_norm_from_stats(self.acc[r][0][None], self.acc[r][1][None], self.acc[r][2])
                engine.fd_step_top(self.rows, self.idx[:n_train], res.reward[:n_train], 0.0, self.sign[:n_train],
                                   res.norm2[:n_train], lpd, float(pop.noise_std[r]), self.theta[r],
                                   float(pop.learning_rate[r]), 1.0, B, g=self.g, out=self.out)
            self.epoch += 1


def timed(obj, epochs):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    obj.train(epochs)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / epochs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", default="1,16,128,1024")
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    ok = True
    for R in [int(x) for x in a.runs.split(",")]:
        pop = rp.PopulationRunner(env_id="CartPole-v1", n_runs=R, top_directions=B, batch_size=D, antithetic=True,
                                  normalize_obs=True, eval_lanes=EVAL, episode_len=T)
        solo = SoloSequences(pop)
        pop.train(a.warmup)
        solo.train(a.warmup)
        torch.cuda.synchronize()
        pm, sm = [], []
        for _ in range(a.rounds):
            pm.append(timed(pop, a.epochs))
            sm.append(timed(solo, a.epochs))
        ratio = [s / p for s, p in zip(sm, pm)]
        faster = all(p < s for p, s in zip(pm, sm))
        if R >= 16 and not faster:
            ok = False
        print(json.dumps({"bench": "runs", "env": "CartPole-v1", "T": T, "n_dirs": D, "top_dirs": B, "R": R,
                          "lanes_per_run": pop.lanes_per_run, "epochs": a.epochs,
                          "population_ms_per_epoch": [round(x, 4) for x in pm],
                          "solo_ms_per_epoch": [round(x, 4) for x in sm],
                          "population_run_epochs_per_s": [round(1e3 * R / x, 1) for x in pm],
                          "solo_run_epochs_per_s": [round(1e3 * R / x, 1) for x in sm],
                          "solo_over_population": [round(x, 2) for x in ratio],
                          "population_faster_every_round": faster}), flush=True)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
