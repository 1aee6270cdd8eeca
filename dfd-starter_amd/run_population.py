"""PopulationRunner -- R independent linear-policy ARS runs advanced together (a build extension).

ARS results are reported over many seeds and over grids of learning rate, noise std, directions and top-b.  One
run's rollout is a few hundred lanes on a device built for hundreds of thousands, and its FD step is three launches
of fixed cost, so R solo runs cost R times a launch that is nearly empty.  Here every run has its own theta, sigma,
learning rate, b, observation statistics and random streams, and one epoch of ALL runs is a fixed number of launches
that does not depend on R:

    1. ids of the epoch's directions (one add), engine.noise_fill: the R * D noise rows
    2. engine.rollout_runs: R x (lpd * D training lanes + eval_lanes sign-0 lanes), one lane per thread
    3. engine.obs_stats_merge_runs and the next epoch's obs_mean / obs_std (WelfordRunningStat.mean / .std's rules)
    4. the eval mean -> the 0.9 / 0.1 EMA policy_reward; engine.fd_step_runs: selection, gradient and DSGD per run
    5. one row per run into the preallocated history tensors

Nothing crosses to the host inside ``train``: it only enqueues.  Reading ``history`` or ``thetas`` is what
synchronises.

A run's whole trajectory is a function of its seed and its hyperparameters, not of R or of its place in the
population:
    direction id of run r, epoch e, direction d     (seeds[r] << 32) + e * D + d          (the counter noise source)
    global id of run r's lane 0                     seeds[r] * L                          (streams, jiggle)
    launch key of epoch e                           a function of (launch_seed, e) alone
and every device reduction here runs in an order fixed by the run's own shape.
"""
import numpy as np
import torch

from fdr import engine
from learner.finite_differences import resolve_top_directions
from run_sequential import make_physics_env
from worker.worker import episode_stream_ids

OBS_STATS_CHANCE = 0.01   # Agent's obs_stats_update_chance


# ---- the id layout: pure numpy, no GPU -----------------------------------------------------------------------------
def check_seeds(seeds, lanes_per_run, episodes_per_lane):
    """Seeds a population can hold: distinct ints >= 0, small enough that every direction id stays a non-negative
    int64 (seed < 2^31) and every stream id stays below 2^32 ((seed + 1) * L * K <= 2^32)."""
    s = [int(x) for x in seeds]
    if len(s) < 1:
        raise ValueError("a population needs at least one seed")
    if len(set(s)) != len(s):
        raise ValueError("seeds must be distinct: equal seeds would be the same run twice")
    L, K = int(lanes_per_run), int(episodes_per_lane)
    for x in s:
        if x < 0 or x >= (1 << 31):
            raise ValueError("seed %d outside [0, 2^31)" % x)
        if (x + 1) * L * K > (1 << 32):
            raise ValueError("seed %d too large: stream ids (seed + 1) * %d lanes * %d episodes must stay within 2^32"
                             % (x, L, K))
    return np.asarray(s, np.int64)


def direction_ids(seeds, epoch, n_dirs):
    """int64 [R, D]: (seed << 32) + epoch * D + d; refuses an epoch whose ids would leave the seed's 2^32 block."""
    e, D = int(epoch), int(n_dirs)
    if e < 0 or (e + 1) * D > (1 << 32):
        raise ValueError("epoch %d: direction ids (epoch + 1) * %d must stay within 2^32" % (e, D))
    return (np.asarray(seeds, np.int64)[:, None] << 32) + (e * D + np.arange(D, dtype=np.int64))[None, :]


def run_lane_offsets(seeds, lanes_per_run):
    """int64 [R]: the global id of each run's lane 0, seed * L."""
    return np.asarray(seeds, np.int64) * int(lanes_per_run)


def lane_signs(n_dirs, lanes_per_dir, eval_lanes):
    """int8 [L] of one run: +1 / -1 pairs (or +1 alone) per direction, then the sign-0 eval lanes."""
    tr = np.tile(np.array([1, -1], np.int8), n_dirs) if lanes_per_dir == 2 else np.ones(n_dirs, np.int8)
    return np.concatenate([tr, np.zeros(int(eval_lanes), np.int8)])


def stream_ids(seeds, n_dirs, lanes_per_dir, eval_lanes, episodes_per_lane, common_random_numbers=False):
    """int64 [R * L, K] episode stream ids, run after run (worker.episode_stream_ids per run at the run's lane
    offset), or None without common random numbers: the kernel's default (offset + l) * K + e is then the same ids."""
    sign = lane_signs(n_dirs, lanes_per_dir, eval_lanes)
    offs = run_lane_offsets(seeds, len(sign))
    if not common_random_numbers:
        for o in offs:
            episode_stream_ids(False, sign, int(o), episodes_per_lane, 1)   # the range check alone
        return None
    return np.concatenate([episode_stream_ids(common_random_numbers, sign, int(o), episodes_per_lane, lanes_per_dir)
                           for o in offs])


def launch_key(launch_seed, epoch):
    """The rollout launch's key: a function of (launch_seed, epoch) alone (Agent.next_seed's mixing)."""
    return (int(launch_seed) * 1000003 + int(epoch)) & ((1 << 63) - 1)


# ---- observation statistics -> (mean, std): WelfordRunningStat.mean / .std as f32 torch operations -------------------
def obs_norm_from_stats(acc_mean, acc_m2, acc_count):
    """acc_mean / acc_m2 [R, n_in] f32, acc_count [R] i64 -> (obs_mean, obs_std) [R, n_in] f32 by the rules of
    utils.math_helpers.WelfordRunningStat: count < 2 gives 0 / 1; var = m2 / (count - 1); a zero variance gives 1."""
    few = (acc_count < 2)[:, None]
    denom = (acc_count - 1).clamp(min=1).to(torch.float32)[:, None]
    var = acc_m2 / denom
    std = torch.sqrt(torch.where(var == 0, torch.ones_like(var), var))
    return (torch.where(few, torch.zeros_like(acc_mean), acc_mean), torch.where(few, torch.ones_like(std), std))


def row_sums(x):
    """[R, n] -> [R]: each row's sum by halving -- columns [0, h) plus columns [h, 2h), an odd last column carried --
    in elementwise operations only, so a row's bits depend on n alone, not on R or on the row's place."""
    while x.shape[1] > 1:
        n = x.shape[1]
        h = n // 2
        s = x[:, :h] + x[:, h:2 * h]
        x = torch.cat([s, x[:, 2 * h:]], 1) if n % 2 else s
    return x[:, 0]


def _per_run(value, n, what, dtype):
    a = np.asarray(value, dtype)
    if a.ndim == 0:
        a = np.full(n, a, dtype)
    if a.shape != (n,):
        raise ValueError("%s: a scalar or one value per run (%d)" % (what, n))
    return a


HISTORY_KEYS = ("eval_mean", "train_mean", "update_magnitude", "grad_norm", "env_steps")


class PopulationRunner(object):
    def __init__(self, env_id="CartPole-v1", n_runs=128, seeds=None, learning_rate=0.01, noise_std=0.02,
                 top_directions=None, batch_size=256, antithetic=True, normalize_obs=True, episodes_per_lane=1,
                 common_random_numbers=False, eval_lanes=8, episode_len=None, device=None, launch_seed=0):
        """seeds: one per run (default range(n_runs); given, they decide the number of runs).  learning_rate,
        noise_std, top_directions: a scalar or one per run; top_directions None is the z-score over all lanes, an int b
        or a float fraction of batch_size keeps the b best directions (FiniteDifferences' rule).  batch_size = D
        directions per run and epoch, two lanes each when antithetic; eval_lanes unperturbed lanes per run feed the
        run's policy_reward EMA.  launch_seed keys the noise rows and, with the epoch, every rollout launch."""
        self.env = make_physics_env(env_id, episode_len)    # ValueError for any other env id
        D, lpd, E, K = int(batch_size), 2 if antithetic else 1, int(eval_lanes), int(episodes_per_lane)
        if D < 1 or E < 1 or not 1 <= K <= 1024:
            raise ValueError("batch_size and eval_lanes must be >= 1, episodes_per_lane in 1 .. 1024")
        self.n_dirs, self.lanes_per_dir, self.eval_lanes, self.episodes_per_lane = D, lpd, E, K
        self.n_train, self.lanes_per_run = D * lpd, D * lpd + E
        L = self.lanes_per_run
        if common_random_numbers and L % lpd:
            raise ValueError("common_random_numbers: eval_lanes must be a multiple of the lanes per direction")
        # seeds given: they are the population, n_runs is not consulted
        self.seeds = check_seeds(range(int(n_runs)) if seeds is None else seeds, L, K)
        R = self.n_runs = len(self.seeds)
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        dev = self.device
        n_in, n_act = self.env.obs_dim, self.env.act_dim
        P = self.n_params = n_in * n_act
        self.spec = engine.PolicySpec("linear", n_in, n_act, P)
        self.launch_seed = int(launch_seed)
        self.normalize_obs = bool(normalize_obs)
        self.learning_rate = _per_run(learning_rate, R, "learning_rate", np.float64)
        self.noise_std = _per_run(noise_std, R, "noise_std", np.float32)
        tops = top_directions if isinstance(top_directions, (list, tuple, np.ndarray)) else [top_directions] * R
        if len(tops) != R:
            raise ValueError("top_directions: a scalar or one value per run (%d)" % R)
        self.top_dirs = None if all(t is None for t in tops) else \
            np.asarray([D if t is None else resolve_top_directions(t, D) for t in tops], np.int32)

        def to_dev(a):
            return torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.thetas = torch.zeros((R, P), dtype=torch.float32, device=dev)       # ARS starts at zero
        self._sigma = to_dev(self.noise_std)
        self._lr = to_dev(self.learning_rate)
        self._top = None if self.top_dirs is None else to_dev(self.top_dirs)
        self._offsets = to_dev(run_lane_offsets(self.seeds, L))
        self._ids0 = to_dev(direction_ids(self.seeds, 0, D).reshape(-1))          # epoch e: + e * D
        self._ids = torch.empty_like(self._ids0)
        self.row_stride = (P + 3) // 4 * 4
        self._rows = torch.empty(R * D * self.row_stride, dtype=torch.float32, device=dev)
        sign = lane_signs(D, lpd, E)
        lane_idx = np.zeros((R, L), np.int64)
        lane_idx[:, :D * lpd] = np.repeat((np.arange(R * D, dtype=np.int64) * self.row_stride).reshape(R, D), lpd, 1)
        self._idx = to_dev(lane_idx.reshape(-1))
        self._sign = to_dev(np.tile(sign, R))
        ids = stream_ids(self.seeds, D, lpd, E, K, common_random_numbers)
        self._episode_ids = None if ids is None else to_dev(ids)
        self._res = engine._rollout_outputs(R * L, dev)
        if self.normalize_obs:
            engine._obs_stat_outputs(self._res, R * L, n_in, dev)
            self.obs_acc = (torch.zeros((R, n_in), dtype=torch.float32, device=dev),
                            torch.zeros((R, n_in), dtype=torch.float32, device=dev),
                            torch.zeros(R, dtype=torch.int64, device=dev))
            self.obs_mean, self.obs_std = obs_norm_from_stats(*self.obs_acc)
        else:
            self.obs_acc = self.obs_mean = self.obs_std = None
        self.policy_reward = torch.zeros(R, dtype=torch.float64, device=dev)
        self._step_out = torch.empty((R, 2), dtype=torch.float64, device=dev)
        self.epoch = 0
        self._blocks = []      # per train() call: {key: [n_epochs, R] device tensor}

    @property
    def history(self):
        """{key: [epochs, R] device tensor} for HISTORY_KEYS; reading the values is what synchronises."""
        if not self._blocks:
            return {k: torch.empty((0, self.n_runs), device=self.device) for k in HISTORY_KEYS}
        return {k: torch.cat([b[k] for b in self._blocks]) for k in HISTORY_KEYS}

    @torch.no_grad()
    def train(self, n_epochs):
        """Enqueue n_epochs epochs of every run.  No host synchronisation: no .item(), no host copy."""
        n_epochs = int(n_epochs)
        R, L, D, n_train = self.n_runs, self.lanes_per_run, self.n_dirs, self.n_train
        direction_ids(self.seeds[:1], self.epoch + max(n_epochs, 1) - 1, D)      # the id range, checked on the host
        dev = self.device
        block = {k: torch.empty((n_epochs, R), dtype=torch.int64 if k == "env_steps" else torch.float64, device=dev)
                 for k in HISTORY_KEYS}
        res = self._res
        for i in range(n_epochs):
            e = self.epoch
            torch.add(self._ids0, e * D, out=self._ids)
            engine.noise_fill(self.launch_seed, R * D, self.n_params, self.row_stride, ids=self._ids, out=self._rows)
            engine.rollout_runs(self.spec, self.env, self.thetas, self._sigma, self._offsets, L,
                                launch_key(self.launch_seed, e), table=self._rows, idx=self._idx, sign=self._sign,
                                n_episodes=self.episodes_per_lane, episode_ids=self._episode_ids, jiggle=True,
                                obs_mean_runs=self.obs_mean, obs_std_runs=self.obs_std,
                                obs_stats=OBS_STATS_CHANCE if self.normalize_obs else None, out=res)
            if self.normalize_obs:
                engine.obs_stats_merge_runs(res.obs_mean, res.obs_m2, res.obs_count, L, *self.obs_acc)
                self.obs_mean, self.obs_std = obs_norm_from_stats(*self.obs_acc)
            rew = res.reward.view(R, L)
            ev = row_sums(rew[:, n_train:]) / float(self.eval_lanes)
            self.policy_reward = self.policy_reward * 0.9 + ev * 0.1
            engine.fd_step_runs(self._rows, self._idx, self._sign, res.norm2, res.reward, L, n_train,
                                self.lanes_per_dir, self._sigma, self.thetas, self._lr, 1.0,
                                policy_reward=self.policy_reward, top_dirs=self._top, out=self._step_out)
            block["eval_mean"][i] = ev
            block["train_mean"][i] = row_sums(rew[:, :n_train]) / float(n_train)
            block["update_magnitude"][i] = self._step_out[:, 0]
            block["grad_norm"][i] = self._step_out[:, 1]
            block["env_steps"][i] = res.timesteps.view(R, L).sum(1)
            self.epoch += 1
        if n_epochs > 0:
            self._blocks.append(block)
        return self
