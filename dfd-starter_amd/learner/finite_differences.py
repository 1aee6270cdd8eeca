"""FiniteDifferences -- the reference learner's API (learner/finite_differences.py:6-114) on the GPU.

``step(batch, policy_reward, policy_novelty, policy_entropy)`` accepts either the reference's
list of FDReturn or an FDBatch (device SoA from Worker.evaluate) and runs, all on the device:

    fdr_fd_grad_fused  ONE launch: z = standardize(r - r_pol) over the batch, coef_d = sum_i z_i s_i sigma /
                       ||lambda_i||^2, g = sum_d coef_d * table[idx_d : idx_d + P] (f64, fixed order, chunk
                       partials combined in-launch)
    fdr_dsgd_step      ONE launch (P <= 65536): theta <- theta - lr*sqrt(P)*lr_scale * fl32(-g) / ||fl32(-g)||

Sharded over ranks (DESIGN.md "Multi-GPU") the z-score step needs ONE collective: every rank reduces its lanes
to the moments [A | B | n | r' slots] (A = sum r'_i v_i, B = sum v_i; its r' at its global lanes, 0 elsewhere),
one RCCL all-reduce sums them, and DSGD forms m, sd in two passes over all r' and g = (A - m B) / sd on the fly
(equal to the z-weighted sum in real arithmetic, B = 0 exactly for antithetic pairs).  One-sided
batches, and batches whose lane split is not known on every rank (a list of FDReturn), all-gather the returns
instead.
``weighting="centred_rank"`` (build extension named by the north star; the reference's weighting is the
z-score) ranks all returns, so it keeps the all-gather of the per-lane returns + the all-reduce of g.

``weighting="top_directions"`` with ``top_directions=b`` (build extension: the selection of Augmented Random Search)
keeps the b best directions, ranked by the maximum of their lanes' returns, and z-scores the kept lanes' returns over
themselves; every other lane weighs 0 (fdr_fd_step_top / fdr_fd_grad_fused_top, fdr_top_dir_weights on the list route,
where every return is a direction of its own).  An int b >= 1 is clipped to the step's direction count D, a float f in
(0, 1] means ceil(f D).  It ranks all returns like the centred rank, and takes the same routes.

``objective="mixed"`` (build extension; the reference carries the combination at finite_differences.py:40-48, switched
off) weights lane i by (1 - omega) z(r_i - r_pol) + omega z(nov_i - nov_pol) + ent_coef z(ent_i - ent_pol), every
channel standardised over all lanes, with omega read from ``self.omega`` at the step: fdr_fd_step_mix /
fdr_fd_grad_fused_mix in place of the two calls above, fdr_fd_weights_mix on the delayed-return route.  Sharded it
takes the gather form (one all-gather of the three channels stacked, one all-reduce of g).  ``objective="reward"``,
the default, is the reference's step; "mixed" with omega = 0 and ent_coef = 0 equals it bit for bit.

``gradient_optimizer`` is honoured as the reference honours it (finite_differences.py:51-59: any torch.optim
optimizer steps on ``policy.set_grad_from_flat(-g)``).  describe_optimizer() sorts it once into one of three routes:
"dsgd" (the two calls above, unchanged); "device" -- torch.optim.Adam / AdamW / SGD over exactly the policy's
parameters in one group, float lr, no amsgrad / maximize / capturable / differentiable: the optimizer's own
single-tensor step runs in the apply launch (fdr_fd_step_opt / fdr_fd_step_mix_opt, or fdr_opt_step after a reduced
gradient / moments), the hyperparameters read from ``param_groups[0]`` at every step (an LR scheduler works), its
state two flat f32 [P] rows owned by the learner and published into ``gradient_optimizer.state`` as per-parameter
views under torch's keys (state_dict() reports them; a load_state_dict is copied in before the next step); "generic" --
anything else: g on the device, then literally zero_grad(), set_grad_from_flat(-g), optimizer.step() (slow, correct for
any optimizer).

Returns carry a current epoch in the synchronous engine; returns from an older epoch (the
reference's async server mode) add the parameter drift theta_epoch - theta_now to lambda
(finite_differences.py:66-92) -- fdr_fd_lambda_norms / fdr_fd_grad_lambda, single-process or sharded
(a list of FDReturn on every rank: counts + rewards all-gathered, one all-reduce of g).

With a CounterNoiseSource the table of every route above is the batch's own rows (FDBatch.noise_table, idx = row *
row_stride); returns or batches that carry only their encoded direction ids have the distinct ids' rows filled again
on the device (fdr_noise_fill with an ids array), bit for bit what the rollout gathered from.
"""
import numpy as np
import torch

from dsgd import DSGD
from fdr import dist as fdist
from fdr import engine
from utils import math_helpers
from utils.noise_sources import HostNoiseRows, is_counter_noise, is_host_noise, require_noise_source

from .fd_return import FDBatch

FUSED_STEP_MAX_P = 1 << 16   # fdr_fd_step fuses DSGD into the gradient launch up to this many parameters


class OptimizerRoute(object):
    """How the learner applies its gradient_optimizer: route "dsgd" | "device" | "generic"; kind "adam" | "adamw" |
    "sgd" on the device route; why: what sent an Adam / AdamW / SGD to the generic route (None otherwise)."""

    def __init__(self, route, kind=None, why=None):
        self.route, self.kind, self.why = route, kind, why

    def __repr__(self):
        return "OptimizerRoute(%r, %r, %r)" % (self.route, self.kind, self.why)


def _tiles_flat(params, flat):
    """Do the parameters, in order, tile the policy's flat f32 buffer exactly?"""
    off = 0
    for p in params:
        d = p.data
        if d.dtype != torch.float32 or d.device != flat.device or not d.is_contiguous() \
                or d.data_ptr() != flat.data_ptr() + 4 * off:
            return False
        off += d.numel()
    return off == flat.numel()


def describe_optimizer(policy, opt):
    """Sort a gradient optimizer into the learner's routes (see the module docstring).  Exact classes only: a subclass
    may override step()."""
    if isinstance(opt, DSGD):
        return OptimizerRoute("dsgd")
    if type(opt) not in (torch.optim.Adam, torch.optim.AdamW, torch.optim.SGD):
        return OptimizerRoute("generic")
    if len(opt.param_groups) != 1:
        return OptimizerRoute("generic", why="%d param groups" % len(opt.param_groups))
    gr = opt.param_groups[0]
    if not _tiles_flat(gr["params"], policy.flat):
        return OptimizerRoute("generic", why="parameters other than the policy's")
    for flag in ("amsgrad", "maximize", "capturable", "differentiable"):
        if gr.get(flag):
            return OptimizerRoute("generic", why=flag)
    scalars = [gr["lr"], gr["weight_decay"]] + (list(gr["betas"]) + [gr["eps"]] if "betas" in gr else
                                                [gr["momentum"], gr["dampening"]])
    if any(torch.is_tensor(x) for x in scalars):
        return OptimizerRoute("generic", why="tensor hyperparameter")
    if type(opt) is torch.optim.SGD:
        return OptimizerRoute("device", "sgd")
    return OptimizerRoute("device", "adamw" if gr.get("decoupled_weight_decay") else "adam")


def _check_top_directions(b):
    """top_directions: an int b >= 1 (directions kept) or a float fraction in (0, 1]."""
    if b is None:
        raise ValueError("weighting='top_directions' needs top_directions: an int b >= 1 or a float fraction in (0, 1]")
    if isinstance(b, bool) or not isinstance(b, (int, float, np.integer, np.floating)):
        raise ValueError("top_directions is an int b >= 1 or a float fraction in (0, 1], not %r" % (b,))
    if isinstance(b, (int, np.integer)):
        if b < 1:
            raise ValueError("top_directions as an int is the number of directions kept: >= 1, not %d" % b)
    elif not (0.0 < b <= 1.0):
        raise ValueError("top_directions as a float is the fraction of directions kept: in (0, 1], not %r" % (b,))


def resolve_top_directions(b, n_dirs):
    """The directions a step over n_dirs directions keeps: an int clipped to n_dirs (the list route can deliver fewer
    returns than expected), a float f -> ceil(f n_dirs).  The product is the f64 one, so a fraction that is not a
    binary number can land just above an integer: 0.07 * 100 = 7.000000000000001 keeps 8 directions, not 7.  Pass an
    int where the count matters."""
    _check_top_directions(b)
    if isinstance(b, (int, np.integer)):
        return max(1, min(int(b), int(n_dirs)))
    return max(1, min(int(np.ceil(float(b) * n_dirs)), int(n_dirs)))


def parse_weighting(spec):
    """A command-line weighting -> (weighting, top_directions): "zscore" | "centred_rank" | "top_directions:<b>", b an
    int (directions kept: "512") or, where it does not read as an int, a float fraction of them ("0.25", "1e-1")."""
    name, _, b = spec.partition(":")
    if name != "top_directions":
        if b:
            raise ValueError("only top_directions takes a parameter, not %r" % (spec,))
        return name, None
    try:
        top = int(b)
    except ValueError:
        top = float(b)      # ValueError for anything that is no number
    _check_top_directions(top)
    return name, top


class FiniteDifferences(object):
    def __init__(self, policy, gradient_optimizer, omega, noise_source, noise_std=0.1, batch_size=100,
                 ent_coef=0.0, max_delayed_return=10, process_group=None, weighting="zscore", one_collective=True,
                 objective="reward", top_directions=None):
        if weighting not in ("zscore", "centred_rank", "top_directions"):
            raise ValueError("weighting must be 'zscore' (the reference), 'centred_rank' or 'top_directions'")
        if objective not in ("reward", "mixed"):
            raise ValueError("objective must be 'reward' (the reference's step) or 'mixed'")
        if objective == "mixed" and weighting != "zscore":
            raise ValueError("objective='mixed' standardises each channel: weighting=%r is not built for it" % weighting)
        if weighting == "top_directions":
            _check_top_directions(top_directions)
        elif top_directions is not None:
            raise ValueError("top_directions goes with weighting='top_directions'")
        self.weighting = weighting
        self.top_directions = top_directions
        self.objective = objective
        self.last_mix = None    # objective="mixed": the (reward, novelty, entropy) coefficients of the latest step
        self._policy_values = (0.0, 0.0, 0.0)   # ... and the policy's own reward, novelty, entropy it subtracted
        self.one_collective = one_collective
        self.max_delayed_return = max_delayed_return
        self.ent_coef = ent_coef
        self.noise_std = noise_std
        self.policy = policy
        self.gradient_optimizer = gradient_optimizer
        require_noise_source(noise_source, "FiniteDifferences")
        self.noise_source = noise_source
        self._host_noise = is_host_noise(noise_source)
        self._counter_noise = is_counter_noise(noise_source)
        self.omega = omega
        self.batch_size = batch_size
        self.process_group = process_group
        self.epoch = 0
        self.discarded_returns = 0
        self.policy_history = [(policy.flat.detach().clone(), 0)]
        self.dist_map = {0: None}
        self.using_dsgd = isinstance(gradient_optimizer, DSGD)
        self.opt_route = describe_optimizer(policy, gradient_optimizer)
        self._opt_rows = None   # device route: the optimizer state, f32 [2, P] (exp_avg | exp_avg_sq; momentum_buffer)
        self._opt_t = 0         # ... and the steps it has taken (torch's state["step"])
        P = policy.num_params
        self.gradient_memory = torch.zeros(P, dtype=torch.float64, device=policy.flat.device)
        self._out = torch.zeros(2, dtype=torch.float64, device=policy.flat.device)
        # policy_history entries written by the DSGD launch itself (no per-step copy): a ring one longer than
        # the history, so a slot is rewritten only after its entry left the history
        self._hist_ring = None
        self._hist_next = 0

    # ------------------------------------------------------------------------------------------
    def _distributed(self):
        return fdist.active(self.process_group)

    def step(self, batch, policy_reward, policy_novelty, policy_entropy):
        """Reference signature; returns the update magnitude ||d theta|| as a float."""
        out = self.step_async(batch, policy_reward, policy_novelty, policy_entropy)
        if out is None:
            return 0
        upd, gnorm = out.tolist()
        if self.using_dsgd:
            assert gnorm > 0, "DSGD ENCOUNTERED GRADIENT WITH NORM OF ZERO"   # dynamic_sgd.py:28
        return upd

    def step_async(self, batch, policy_reward, policy_novelty, policy_entropy):
        """Same as step() but leaves (||d theta||, ||grad||) on the device: no host sync."""
        if policy_reward is None:
            policy_reward = 0
        if self.objective == "mixed":
            self._policy_values = (float(policy_reward), float(policy_novelty or 0), float(policy_entropy or 0))
        if isinstance(batch, FDBatch):
            return self._step_batch(batch, float(policy_reward))
        return self._step_returns(list(batch), float(policy_reward))

    # ------------------------------------------------------------------------------------------
    def _table(self, b=None):
        """What lambda is gathered from: a host-noise or counter-noise batch's own rows, else the shared table.  A
        counter-noise batch that arrives without its rows has them regenerated from its encoded ids."""
        t = getattr(b, "noise_table", None) if b is not None else None
        if t is not None:
            return t
        if self._counter_noise:
            if b is None or getattr(b, "encoded", None) is None:
                raise ValueError("a counter noise source's FDBatch carries its rows (noise_table) or its ids (encoded)")
            lpd = b.lanes_per_dir
            table, idx = self._counter_rows(b.encoded[::lpd])
            b.idx_host = np.repeat(idx, lpd)
            b.idx = torch.as_tensor(b.idx_host, device=self.policy.flat.device)
            b.noise_table = table
            return table
        if self._host_noise:
            raise ValueError("a host noise source's FDBatch carries its noise rows (Worker.evaluate sets noise_table)")
        return self.noise_source.device_table(self.policy.flat.device)

    def _counter_rows(self, encoded):
        """Device rows of the directions a counter noise source encoded (ids as strings, any order, repeats allowed --
        antithetic partners share one): -> (table [n_unique * row_stride], idx_host [len(encoded)] offsets into it).
        One fdr_noise_fill over the distinct ids; bit for bit the rows the rollout gathered from."""
        src = self.noise_source
        ids = np.array([int(e) for e in encoded], dtype=np.uint64)
        uniq, inv = np.unique(ids, return_inverse=True)
        table = src.rows(uniq, len(uniq), self.policy.flat.device)
        return table, inv.reshape(-1).astype(np.int64) * src.row_stride

    def _mix_coefs(self):
        """(1 - omega, omega, ent_coef) at this step (NSRA-ES; the reference's finite_differences.py:40-48)."""
        w = float(self.omega.omega)
        self.last_mix = (1.0 - w, w, float(self.ent_coef))
        return self.last_mix

    def _mix_local(self, reward, novelty, entropy, coefs):
        """The batch's channels as device f64, None where the coefficient is 0 (such a channel is never read)."""
        dev = self.policy.flat.device
        out = []
        for name, t, a in zip(("reward", "novelty", "entropy"), (reward, novelty, entropy), coefs):
            if a == 0.0:
                out.append(None)
                continue
            if t is None:
                raise ValueError("objective='mixed' with a non-zero %s coefficient needs the batch's %s (a Worker "
                                 "without a strategy handler computes no novelty)" % (name, name))
            t = t if torch.is_tensor(t) else torch.as_tensor(np.asarray(t, np.float64))
            out.append(t.to(device=dev, dtype=torch.float64).contiguous())
        return out

    def _step_batch_mixed(self, b, table):
        """objective="mixed": fd_step_mix (one process, P <= 65536), else fd_grad_fused_mix + DSGD; sharded, one
        all-gather of the three channels stacked, fd_grad_fused_mix on this rank's lanes, one all-reduce of g (the
        one-collective moments form is not extended to three channels)."""
        P = self.policy.num_params
        coefs = self._mix_coefs()
        ch = self._mix_local(b.reward, b.novelty, b.entropy, coefs)
        if not self._distributed():
            if P <= FUSED_STEP_MAX_P and self.opt_route.route == "device":
                slot = self._hist_slot()
                engine.fd_step_mix_opt(table, b.idx, ch, self._policy_values, coefs, b.sign, b.norm2, b.lanes_per_dir,
                                       self.noise_std, self.policy.flat, self._opt_spec(), g=self.gradient_memory,
                                       out=self._out, theta_hist=slot)
                return self._after_opt(slot)
            if P <= FUSED_STEP_MAX_P and self.using_dsgd:
                lr, lr_scale = self._lr()
                slot = self._hist_slot()
                engine.fd_step_mix(table, b.idx, ch, self._policy_values, coefs, b.sign, b.norm2, b.lanes_per_dir,
                                   self.noise_std, self.policy.flat, lr, lr_scale, g=self.gradient_memory, out=self._out,
                                   theta_hist=slot)
                return self._after_update(slot)
            g = engine.fd_grad_fused_mix(table, b.idx, ch, self._policy_values, coefs, 0, b.sign, b.norm2,
                                         b.lanes_per_dir, self.noise_std, P, out=self.gradient_memory)
            return self._apply(g)
        ch_all, lane_lo = self._gather_channels(ch, b.reward.numel(), getattr(b, "rank_lanes", None))
        g = engine.fd_grad_fused_mix(table, b.idx, ch_all, self._policy_values, coefs, lane_lo, b.sign, b.norm2,
                                     b.lanes_per_dir, self.noise_std, P, out=self.gradient_memory)
        fdist.allreduce_grad(g, self.process_group)
        return self._apply(g)

    def _gather_channels(self, ch, n, sizes):
        """One all-gather of the active channels stacked [n, k] -> (each channel over all lanes, this rank's offset)."""
        dev = self.policy.flat.device
        active = [c for c in ch if c is not None]
        stacked = torch.stack(active, dim=1).contiguous() if n else torch.zeros((0, len(active)), dtype=torch.float64,
                                                                                  device=dev)
        if sizes is None:
            sizes = fdist.exchange_counts(n, dev, self.process_group)
        k = len(active)
        flat_all, lo = fdist.gather_rewards(stacked.reshape(-1), self.process_group, [int(s) * k for s in sizes])
        cols = flat_all.reshape(-1, k)
        it = iter(range(k))
        return [None if c is None else cols[:, next(it)].contiguous() for c in ch], lo // k

    def _step_batch(self, b, policy_reward):
        table = self._table(b)
        if not np.all(b.sign_host != 0):
            raise ValueError("FDBatch for the learner must not contain eval lanes (sign 0)")
        if self.objective == "mixed":
            return self._step_batch_mixed(b, table)
        P = self.policy.num_params
        if self.weighting == "top_directions":
            return self._step_batch_top(b, table, policy_reward)
        if not self._distributed():
            if P <= FUSED_STEP_MAX_P and self.opt_route.route == "device":   # the same two launches, the apply swapped
                slot = self._hist_slot()
                engine.fd_step_opt(table, b.idx, b.reward, policy_reward, b.sign, b.norm2, b.lanes_per_dir,
                                   self.noise_std, self.policy.flat, self._opt_spec(), mode=self.weighting,
                                   g=self.gradient_memory, out=self._out, theta_hist=slot)
                return self._after_opt(slot)
            if P <= FUSED_STEP_MAX_P and self.using_dsgd:   # the whole step in one launch: weights + gradient + DSGD
                lr, lr_scale = self._lr()
                slot = self._hist_slot()
                engine.fd_step(table, b.idx, b.reward, policy_reward, b.sign, b.norm2, b.lanes_per_dir, self.noise_std,
                               self.policy.flat, lr, lr_scale, mode=self.weighting, g=self.gradient_memory, out=self._out,
                               theta_hist=slot)
                return self._after_update(slot)
            g = engine.fd_grad_fused(table, b.idx, b.reward, policy_reward, 0, b.sign, b.norm2, b.lanes_per_dir,
                                     self.noise_std, P, mode=self.weighting, out=self.gradient_memory)
            return self._apply(g)
        sizes = getattr(b, "rank_lanes", None)
        if self.weighting == "zscore" and self.one_collective and sizes is not None and b.lanes_per_dir == 2 \
                and self.opt_route.route != "generic":   # the generic route takes g itself: the gather form below
            # the split is known on every rank (Worker.evaluate's lane_range): [A | B | n | r' slots], ONE all-reduce.
            # Antithetic only: there B = 0 exactly, so A - m B carries no cancellation; one-sided batches with
            # near-constant returns (|m| >> sd) would lose digits in it, and take the exact gather path below.
            ws, rank = fdist.world_rank(self.process_group)
            if len(sizes) != ws or int(sizes[rank]) != b.reward.numel():
                # the slots of [A | B | n | r'] would overlap or leave gaps: m, sd and g silently wrong
                raise ValueError("FDBatch.rank_lanes %s does not match the learner's process group (world %d, rank "
                                 "%d, %d local lanes)" % (list(sizes), ws, rank, b.reward.numel()))
            mom = engine.fd_grad_fused(table, b.idx, b.reward, policy_reward, int(sum(sizes[:rank])), b.sign, b.norm2,
                                       b.lanes_per_dir, self.noise_std, P, mode="moments", n_all=int(sum(sizes)))
            fdist.allreduce_grad(mom, self.process_group)            # the step's one collective
            return self._apply(mom, moments=True)
        rewards_all, lane_lo = fdist.gather_rewards(b.reward, self.process_group, getattr(b, "rank_lanes", None))
        g = engine.fd_grad_fused(table, b.idx, rewards_all, policy_reward, lane_lo, b.sign, b.norm2,
                                 b.lanes_per_dir, self.noise_std, P, mode=self.weighting, out=self.gradient_memory)
        fdist.allreduce_grad(g, self.process_group)
        return self._apply(g)

    def _step_batch_top(self, b, table, policy_reward):
        """weighting="top_directions": the routes of centred rank -- fd_step_top_opt / fd_step_top (one process,
        P <= 65536), else fd_grad_fused_top + the apply; sharded, the gather form (the selection ranks the
        directions of all ranks): one all-gather of the returns, one all-reduce of g."""
        P = self.policy.num_params
        lpd = b.lanes_per_dir
        if not self._distributed():
            top = resolve_top_directions(self.top_directions, b.reward.numel() // lpd)
            if P <= FUSED_STEP_MAX_P and self.opt_route.route == "device":
                slot = self._hist_slot()
                engine.fd_step_top_opt(table, b.idx, b.reward, policy_reward, b.sign, b.norm2, lpd, self.noise_std,
                                       self.policy.flat, self._opt_spec(), top, g=self.gradient_memory, out=self._out,
                                       theta_hist=slot)
                return self._after_opt(slot)
            if P <= FUSED_STEP_MAX_P and self.using_dsgd:
                lr, lr_scale = self._lr()
                slot = self._hist_slot()
                engine.fd_step_top(table, b.idx, b.reward, policy_reward, b.sign, b.norm2, lpd, self.noise_std,
                                   self.policy.flat, lr, lr_scale, top, g=self.gradient_memory, out=self._out,
                                   theta_hist=slot)
                return self._after_update(slot)
            g = engine.fd_grad_fused_top(table, b.idx, b.reward, policy_reward, 0, b.sign, b.norm2, lpd, self.noise_std,
                                         P, top, out=self.gradient_memory)
            return self._apply(g)
        rewards_all, lane_lo = fdist.gather_rewards(b.reward, self.process_group, getattr(b, "rank_lanes", None))
        top = resolve_top_directions(self.top_directions, rewards_all.numel() // lpd)
        g = engine.fd_grad_fused_top(table, b.idx, rewards_all, policy_reward, lane_lo, b.sign, b.norm2, lpd,
                                     self.noise_std, P, top, out=self.gradient_memory)
        fdist.allreduce_grad(g, self.process_group)
        return self._apply(g)

    def _lr(self):
        """DSGD's (lr, lr_scale); adjust_lr is DSGD's alone (finite_differences.py:51-52)."""
        self.gradient_optimizer.adjust_lr(self.omega)
        return self.gradient_optimizer.lr, self.gradient_optimizer.lr_scale

    # ---- the device route's optimizer state --------------------------------------------------------------------
    def _opt_keys(self):
        if self.opt_route.kind == "sgd":
            return ("momentum_buffer",) if self.gradient_optimizer.param_groups[0]["momentum"] != 0 else ()
        return ("exp_avg", "exp_avg_sq")

    def _sync_opt_state(self, keys):
        """The learner's rows and gradient_optimizer.state agree before a step: state tensors that are not views of
        the rows (a load_state_dict, a step the caller ran) are copied in and the step count taken from them; keys
        that went missing after publication (state cleared) restart from zero, as torch would; then fresh views."""
        opt = self.gradient_optimizer
        flat = self.policy.flat
        first = self._opt_rows is None
        if first:
            self._opt_rows = torch.zeros((2, flat.numel()), dtype=torch.float32, device=flat.device)
        rows = self._opt_rows
        params = opt.param_groups[0]["params"]
        foreign = missing = False
        off = 0
        for p in params:
            st = opt.state[p] if p in opt.state else {}
            n = p.numel()
            for r, k in enumerate(keys):
                t = st.get(k)
                if t is None:
                    missing = True
                elif t.data_ptr() != rows[r].data_ptr() + 4 * off or t.dtype != torch.float32 or t.device != flat.device:
                    rows[r, off:off + n].copy_(t.detach().reshape(-1).to(device=flat.device, dtype=torch.float32))
                    foreign = True
            off += n
        if not (first or foreign or missing):
            return
        if foreign:
            steps = [opt.state[p]["step"] for p in params if p in opt.state and "step" in opt.state[p]]
            self._opt_t = int(float(steps[0])) if steps else max(self._opt_t, 1)
        elif missing:
            if not first:
                rows.zero_()
            self._opt_t = 0
        off = 0
        for p in params:
            st = opt.state[p]
            n = p.numel()
            for r, k in enumerate(keys):
                st[k] = rows[r, off:off + n].view_as(p)
            if self.opt_route.kind != "sgd":
                st["step"] = torch.tensor(float(self._opt_t))
            off += n

    def _opt_spec(self):
        """This step's OptSpec: the hyperparameters as param_groups[0] holds them now, the step count, the rows."""
        keys = self._opt_keys()
        if keys:
            self._sync_opt_state(keys)
        gr = self.gradient_optimizer.param_groups[0]
        rows = self._opt_rows
        if self.opt_route.kind == "sgd":
            return engine.OptSpec("sgd", gr["lr"], self._opt_t + 1, rows[0] if keys else None, None,
                                  weight_decay=gr["weight_decay"], momentum=gr["momentum"], dampening=gr["dampening"],
                                  nesterov=gr["nesterov"])
        return engine.OptSpec(self.opt_route.kind, gr["lr"], self._opt_t + 1, rows[0], rows[1], betas=gr["betas"],
                              eps=gr["eps"], weight_decay=gr["weight_decay"])

    def _after_opt(self, hist=None):
        self._opt_t += 1
        if self.opt_route.kind != "sgd":
            for p in self.gradient_optimizer.param_groups[0]["params"]:
                self.gradient_optimizer.state[p]["step"].fill_(self._opt_t)
        return self._after_update(hist)

    def _apply_generic(self, g):
        """The reference's literal sequence (finite_differences.py:51-59) on device tensors, for any optimizer."""
        flat = self.policy.flat
        old = flat.detach().clone()
        self.gradient_optimizer.zero_grad()
        neg = -g
        self.policy.set_grad_from_flat(neg)
        self.gradient_optimizer.step()
        self._out[0] = torch.linalg.vector_norm((old - flat.detach()).double())
        self._out[1] = torch.linalg.vector_norm(neg.float().double())
        return self._after_update()

    def _hist_slot(self):
        if self._hist_ring is None:
            n = max(1, self.max_delayed_return) + 1
            self._hist_ring = torch.empty((n, self.policy.num_params), dtype=torch.float32, device=self.policy.flat.device)
        slot = self._hist_ring[self._hist_next]
        self._hist_next = (self._hist_next + 1) % self._hist_ring.shape[0]
        return slot

    def _after_update(self, hist=None):
        self.gradient_optimizer.steps = getattr(self.gradient_optimizer, "steps", 0) + 1
        self.epoch += 1
        self._build_distance_map()
        self._update_policy_history(hist)
        return self._out

    def _apply(self, src, moments=False):
        if self.opt_route.route == "device":
            slot = self._hist_slot()
            engine.opt_step(self.policy.flat, src, moments, self._opt_spec(),
                            g_out=self.gradient_memory if moments else None, out=self._out, theta_hist=slot)
            return self._after_opt(slot)
        if self.opt_route.route == "generic":
            return self._apply_generic(src)
        lr, lr_scale = self._lr()
        engine.dsgd_step_ex(self.policy.flat, src, moments, lr, lr_scale, g_out=self.gradient_memory if moments else None,
                            out=self._out)
        return self._after_update()

    def _build_distance_map(self):
        # finite_differences.py:66-73: dist_map[ep] = theta_ep - theta_now for the recent epochs.  The
        # differences are formed on first use (only stale returns read them), not eagerly every step.
        self.dist_map = _LazyDistMap(self.epoch, self.policy_history, self.policy.flat.detach())

    def _update_policy_history(self, hist=None):
        # finite_differences.py:75-78; hist: theta already copied by the DSGD launch (fdr_fd_step theta_hist)
        self.policy_history.append((self.policy.flat.detach().clone() if hist is None else hist, self.epoch))
        while len(self.policy_history) > self.max_delayed_return:
            self.policy_history.pop(0)

    # ------------------------------------------------------------------------------------------
    def _step_returns(self, rets, policy_reward):
        """list[FDReturn] path (finite_differences.py:24-64, 80-114)."""
        keep = []
        for r in rets:
            if r.epoch not in self.dist_map:
                print("FINITE DIFFERENCE LEARNER RECEIVED RETURN THAT WAS TOO OLD")
                print("RECEIVED EPOCH:", r.epoch, "ACCEPTABLE EPOCHS:", list(self.dist_map.keys()))
                self.discarded_returns += 1
                continue
            keep.append(r)
        if self._distributed():
            # every rank joins the exchange, even with no (kept) returns of its own
            return self._step_returns_lambda(keep, policy_reward)
        if not keep:
            return None
        dev = self.policy.flat.device
        P = self.policy.num_params
        if self._host_noise:
            # finite_differences.py:94: decode() regenerates each return's noise vector on the host (f64); the device
            # gathers lambda_i = sign fl32(sigma fl32(noise_i)) (+ drift) from those rows
            return self._step_returns_lambda(keep, policy_reward)
        current = [r for r in keep if self.dist_map[r.epoch] is None]
        stale = [r for r in keep if self.dist_map[r.epoch] is not None]
        if stale:
            # finite_differences.py:88-114: lambda_i = sigma * eps_i + dist_map[epoch_i], v_i = lambda_i / ||lambda_i||^2
            return self._step_returns_lambda(keep, policy_reward)
        rewards = torch.as_tensor([r.reward for r in current], dtype=torch.float64, device=dev)
        if self._counter_noise:   # the encoded ids' rows, regenerated on the device; idx = row offsets into them
            table, idx = self._counter_rows([r.encoded_noise for r in current])
        else:
            table = self.noise_source.device_table(dev)
            idx = np.array([int(r.encoded_noise) for r in current], dtype=np.int64)
        sign = np.array([int(getattr(r, "sign", 1) or 1) for r in current], dtype=np.int8)
        idx_d = torch.as_tensor(idx, device=dev)
        sign_d = torch.as_tensor(sign, device=dev)
        if all(getattr(r, "norm2", None) is not None for r in current):
            n2 = torch.as_tensor([r.norm2 for r in current], dtype=torch.float64, device=dev)
        else:
            n2 = engine.fd_lambda_norms(table, idx_d, sign_d, None, self.noise_std, None, P)
        b = FDBatch(rewards, None, None, n2, idx_d, sign_d, idx, sign, self.epoch)
        if self._counter_noise:
            b.noise_table = table
        if self.objective == "mixed":
            b.novelty = torch.as_tensor([float(r.novelty) for r in current], dtype=torch.float64, device=dev)
            b.entropy = torch.as_tensor([float(r.entropy) for r in current], dtype=torch.float64, device=dev)
        return self._step_batch(b, policy_reward)


    def _step_returns_lambda(self, keep, policy_reward):
        """list[FDReturn] with the lambda kernels: delayed returns single-process, and every sharded list step (finite_differences.py:24-64, 80-114; the
        reference's server accepts returns up to max_delayed_return epochs old, networking/server.py:83-89).
        Sharded, each rank holds its own returns; the policy history -- hence dist_map -- is replicated (every rank applies
        the same DSGD step), so each rank forms its lambda_i = sign_i fl32(sigma eps_i) + dist_map[epoch_i] alone.
        Exchange: the per-rank return counts + an all-gather of the rewards (the z-score is global), then ONE
        all-reduce of g.  Every rank takes this path for every list step, stale returns or not, so the ranks'
        collectives always match."""
        dev = self.policy.flat.device
        P = self.policy.num_params
        n = len(keep)
        if self._host_noise:
            noises = np.stack([self.noise_source.decode(r.encoded_noise) for r in keep]) if n else np.zeros((0, P))
            rows = HostNoiseRows(np.zeros(P, np.float32), noises, np.arange(n), np.ones(n, np.int8), self.noise_std,
                                 dev, with_theta=False)
            table, idx_host = rows.table, rows.idx_host
        elif self._counter_noise:
            table, idx_host = self._counter_rows([r.encoded_noise for r in keep])
        else:
            table = self.noise_source.device_table(dev)
            idx_host = np.array([int(r.encoded_noise) for r in keep], np.int64)
        sizes = fdist.exchange_counts(n, dev, self.process_group)
        if sum(sizes) == 0:
            return None
        epochs = sorted({r.epoch for r in keep if self.dist_map[r.epoch] is not None})
        drift = torch.stack([self.dist_map[e] for e in epochs]).contiguous() if epochs else None
        slot_of = {e: k for k, e in enumerate(epochs)}
        rewards = torch.as_tensor([r.reward for r in keep], dtype=torch.float64, device=dev)
        if self.objective == "mixed":
            coefs = self._mix_coefs()
            ch = self._mix_local(rewards, torch.as_tensor([float(r.novelty) for r in keep], dtype=torch.float64),
                                 torch.as_tensor([float(r.entropy) for r in keep], dtype=torch.float64), coefs)
            ch_all, lane_lo = self._gather_channels(ch, n, sizes) if self._distributed() else (ch, 0)
        else:
            rewards_all, lane_lo = fdist.gather_rewards(rewards, self.process_group, sizes)
        g = self.gradient_memory
        if n:
            idx_d = torch.as_tensor(idx_host, device=dev)
            sign_d = torch.as_tensor(np.array([int(getattr(r, "sign", 1) or 1) for r in keep], np.int8), device=dev)
            slot_d = torch.as_tensor(np.array([slot_of.get(r.epoch, -1) for r in keep], np.int32), device=dev)
            n2 = engine.fd_lambda_norms(table, idx_d, sign_d, slot_d, self.noise_std, drift, P)
            if self.objective == "mixed":
                ones = torch.ones(n, dtype=torch.int8, device=dev)
                coef = engine.fd_weights_mix(ch_all, self._policy_values, coefs, lane_lo, ones, n2, 1, 1.0)
            elif self.weighting == "centred_rank":   # ranks over all returns, v_i = lambda_i / ||lambda_i||^2
                coef = engine.rank_weights(rewards_all, lane_lo, n) / n2
            elif self.weighting == "top_directions":   # every return a direction of its own (lanes_per_dir = 1)
                top = resolve_top_directions(self.top_directions, rewards_all.numel())
                coef = engine.top_dir_weights(rewards_all, policy_reward, 1, top, lane_lo, n) / n2
            else:
                ones = torch.ones(n, dtype=torch.int8, device=dev)
                coef = engine.fd_weights(rewards_all, policy_reward, lane_lo, ones, n2, 1, 1.0)
            g = engine.fd_grad_lambda(table, idx_d, sign_d, slot_d, coef, self.noise_std, drift, P, g)
        else:
            g.zero_()
        fdist.allreduce_grad(g, self.process_group)
        return self._apply(g)


class _LazyDistMap(object):
    """The learner's epoch -> drift map (finite_differences.py:66-73) with the same keys and values as the
    reference's eager dict: None for the current epoch, theta_ep - theta_now (device f32) for the epochs
    in the policy history.  A difference is computed on first access and cached; theta_now is the
    learner's parameter tensor, which only changes in the next step, when the map is rebuilt."""

    def __init__(self, epoch, history, flat):
        self._cur = epoch
        self._hist = {ep: params for params, ep in history}
        self._flat = flat
        self._cache = {}

    def __contains__(self, ep):
        return ep == self._cur or ep in self._hist

    def __getitem__(self, ep):
        if ep in self._hist:
            if ep not in self._cache:
                self._cache[ep] = self._hist[ep] - self._flat
            return self._cache[ep]
        if ep == self._cur:
            return None
        raise KeyError(ep)

    def keys(self):
        return [self._cur] + [ep for ep in self._hist if ep != self._cur]

    def __len__(self):
        return len(self.keys())

