"""Device-level operations of the FD engine: thin torch-tensor wrappers over the C ABI.

PyTorch-ROCm is plumbing here (device memory, streams, torch.distributed); every computation
runs in libfdr.so.  All calls are asynchronous on the current HIP stream.
"""
import ctypes

import torch

from . import _lib
from ._lib import check, lib


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream(device=None):
    """The current HIP stream of `device` as a C pointer (torch's raw-stream accessor: a few us cheaper per call
    than building the Stream object)."""
    if _RAW_STREAM is not None:
        if isinstance(device, torch.device) and device.index is not None:
            idx = device.index
        elif isinstance(device, int):
            idx = device
        else:
            idx = torch.cuda.current_device() if device is None else torch.device(device).index
            idx = torch.cuda.current_device() if idx is None else idx
        return ctypes.c_void_p(_RAW_STREAM(idx))
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class Context(object):
    """One fdr_ctx (include/fdr.h): the engine state of one device -- rollout kernel selection, Impala phase
    profiling, replay GEMM switch, debug clocks.  engine.context(device) holds the default one per device;
    further contexts are independent (e.g. two rollout selections side by side in one process)."""

    def __init__(self, device=None):
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        h = ctypes.c_void_p()
        check(lib.fdr_ctx_create(int(dev.index), ctypes.byref(h)), "fdr_ctx_create")
        self.handle = h

    def set_rollout_impl(self, impl):
        """"pair" | "single" | "wide" | "auto" | "generic" (FDR_ROLLOUT_*; "generic": the runtime-shaped kernels
        for every synthetic-env rollout and policy forward of this context)."""
        code = {"pair": _lib.FDR_ROLLOUT_PAIR, "single": _lib.FDR_ROLLOUT_SINGLE, "auto": _lib.FDR_ROLLOUT_AUTO,
                "wide": _lib.FDR_ROLLOUT_WIDE, "generic": _lib.FDR_ROLLOUT_GENERIC}[impl]
        check(lib.fdr_ctx_set_rollout_impl(self.handle, code), "fdr_ctx_set_rollout_impl")

    def set_replay_gemm(self, on):
        """Diagnostics (include/fdr_diag.h): the entropy replay's input projection as a GEMM per chunk (default) or
        streamed per step -- bit-identical gates."""
        check(lib.fdr_ctx_set_replay_gemm(self.handle, 1 if on else 0), "fdr_ctx_set_replay_gemm")

    def impala_profile(self, enable):
        check(lib.fdr_ctx_impala_profile(self.handle, 1 if enable else 0), "fdr_ctx_impala_profile")

    def impala_profile_read(self):
        out = (ctypes.c_double * 3)()
        check(lib.fdr_ctx_impala_profile_read(self.handle, ctypes.cast(out, ctypes.c_void_p)),
              "fdr_ctx_impala_profile_read")
        return tuple(out)

    def impala_debug_clock(self, buf):
        check(lib.fdr_ctx_impala_debug_clock(self.handle, None if buf is None else ctypes.c_void_p(buf.data_ptr())),
              "fdr_ctx_impala_debug_clock")

    def __del__(self):
        try:
            lib.fdr_ctx_destroy(self.handle)
        except Exception:
            pass


_CTX = {}


def context(device=None):
    """The engine's context of `device` (created on first use)."""
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    c = _CTX.get(dev)
    if c is None:
        c = _CTX[dev] = Context(dev)
    return c


def _c(device=None, ctx=None):
    return (ctx if ctx is not None else context(device)).handle


class PolicySpec(object):
    """Shape of a policy family (policies/discrete.py:34-48, policies/mujoco.py:32-41)."""

    def __init__(self, kind, n_in, n_act, n_params):
        assert kind in ("discrete", "mujoco", "linear")
        self.kind, self.n_in, self.n_act, self.n_params = kind, int(n_in), int(n_act), int(n_params)

    def desc(self, bn_mean=None, bn_var=None):
        if self.kind == "linear":  # W [n_act, n_in] alone: hidden 0, no BN statistics
            return _lib.PolicyDesc(_lib.FDR_POLICY_LINEAR, self.n_in, self.n_act, 0, self.n_params, None, None)
        return _lib.PolicyDesc(_lib.FDR_POLICY_DISCRETE if self.kind == "discrete" else _lib.FDR_POLICY_MUJOCO,
                               self.n_in, self.n_act, 64, self.n_params,
                               None if bn_mean is None else bn_mean.data_ptr(),
                               None if bn_var is None else bn_var.data_ptr())


def _check_dev(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise ValueError("fdr: tensors must live on the GPU (got %s)" % t.device)


def lanes_desc(base, base_stride, table=None, idx=None, sign=None, sigma=0.0, deterministic=None, lane_offset=0):
    _check_dev(base, table, idx, sign, deterministic)
    if base.dtype != torch.float32 or not base.is_contiguous():
        raise ValueError("base must be contiguous float32")
    if idx is not None and idx.dtype != torch.int64:
        raise ValueError("idx must be int64")
    if sign is not None and sign.dtype != torch.int8:
        raise ValueError("sign must be int8")
    if deterministic is not None and deterministic.dtype != torch.int8:
        raise ValueError("deterministic must be int8")
    d = _lib.LanesDesc(base.data_ptr(), int(base_stride),
                       None if table is None else table.data_ptr(),
                       0 if table is None else table.numel(),
                       None if idx is None else idx.data_ptr(),
                       None if sign is None else sign.data_ptr(),
                       float(sigma),
                       None if deterministic is None else deterministic.data_ptr(),
                       int(lane_offset))
    # the descriptor holds raw device pointers: keep the tensors alive as long as it lives, or the
    # caching allocator may hand their blocks to the next allocation before the kernel runs
    d._refs = (base, table, idx, sign, deterministic)
    return d


def perturb(theta, table, idx, sign, sigma):
    """theta' = theta + sign * fl32(sigma * table[idx:idx+P]) -> [n, P] (worker/worker.py:28)."""
    _check_dev(theta, table, idx, sign)
    n, P = idx.numel(), theta.numel()
    out = torch.empty((n, P), dtype=torch.float32, device=theta.device)
    check(lib.fdr_perturb(_c(theta.device), _p(theta), P, _p(table), table.numel(), _p(idx), _p(sign), n,
                          float(sigma), _p(out), _stream(theta.device)), "fdr_perturb")
    return out


def policy_forward(spec, lanes, n_lanes, x, bn_mean=None, bn_var=None, ctx=None):
    """One observation per lane.  discrete -> probs [n, A]; mujoco -> (mean, std) [n, A]; linear -> y [n, A]."""
    _check_dev(x, bn_mean, bn_var)
    x = x.to(torch.float32).contiguous()
    dev = x.device
    out0 = torch.empty((n_lanes, spec.n_act), dtype=torch.float32, device=dev)
    out1 = None if spec.kind in ("discrete", "linear") else torch.empty_like(out0)
    pd = spec.desc(bn_mean, bn_var)
    check(lib.fdr_policy_forward(_c(dev, ctx), ctypes.byref(pd), ctypes.byref(lanes), n_lanes, _p(x), _p(out0),
                                 _p(out1), _stream(dev)), "fdr_policy_forward")
    return out0 if out1 is None else (out0, out1)


def theta_prime(spec, lanes, n_lanes, loader, bn_mean=None, bn_var=None, device=None, ctx=None):
    """Diagnostics (include/fdr_diag.h, fdr_diag_theta_prime): the weights one of the MLP rollouts' loaders forms,
    read back.  loader "lane" | "pair" | "dyn" (the runtime-shaped kernels').  -> (out f32, reads i32, counted i32)
    [n_lanes, P], n2 f64 [n_lanes]."""
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    _check_dev(bn_mean, bn_var)
    code = {"lane": _lib.FDR_LOADER_LANE, "pair": _lib.FDR_LOADER_PAIR, "dyn": _lib.FDR_LOADER_DYN}[loader]
    out = torch.full((n_lanes, spec.n_params), float("nan"), dtype=torch.float32, device=dev)
    reads = torch.zeros((n_lanes, spec.n_params), dtype=torch.int32, device=dev)
    counted = torch.zeros_like(reads)
    n2 = torch.full((n_lanes,), -1.0, dtype=torch.float64, device=dev)
    pd = spec.desc(bn_mean, bn_var)
    check(lib.fdr_diag_theta_prime(_c(dev, ctx), ctypes.byref(pd), ctypes.byref(lanes), n_lanes, code, _p(out), _p(reads),
                                   _p(counted), _p(n2), _stream(dev)), "fdr_diag_theta_prime")
    return out, reads, counted, n2


class RolloutResult(object):
    """SoA result of one batched rollout (the FDReturn fields, learner/fd_return.py:5-16)."""

    def __init__(self, ret, ent, steps, norm2):
        self.reward, self.entropy, self.timesteps, self.norm2 = ret, ent, steps, norm2


def _rollout_outputs(n_lanes, dev):
    """A RolloutResult whose four outputs share one allocation (one caching-allocator call per rollout)."""
    buf = torch.empty(28 * n_lanes, dtype=torch.uint8, device=dev)
    return RolloutResult(buf[:8 * n_lanes].view(torch.float64), buf[8 * n_lanes:16 * n_lanes].view(torch.float64),
                         buf[24 * n_lanes:].view(torch.int32), buf[16 * n_lanes:24 * n_lanes].view(torch.float64))


def _obs_stat_outputs(out, n_lanes, n_in, dev):
    """The per-lane Welford obs statistics as out.obs_mean / obs_m2 / obs_count; -> the three tensors."""
    out.obs_mean = torch.empty((n_lanes, n_in), dtype=torch.float32, device=dev)
    out.obs_m2 = torch.empty_like(out.obs_mean)
    out.obs_count = torch.empty(n_lanes, dtype=torch.int32, device=dev)
    return out.obs_mean, out.obs_m2, out.obs_count


def rollout(spec, env, lanes, n_lanes, seed, jiggle=True, obs_mean=None, obs_std=None,
            bn_mean=None, bn_var=None, out=None, device=None, states=None, obs_stats=None, ctx=None,
            u_inject=None):
    """fdr_rollout; fdr_rollout_ex when states (f32 [n_lanes, T, n_in] device tensor) is given,
    obs_stats = the per-step sampling chance (-> out.obs_mean / obs_m2 / obs_count per lane), or u_inject =
    host-injected draws (f32 [n_lanes, T, k] device tensor: k = 1 uniform per step for a discrete policy, n_act
    normals for a continuous one) replacing the counter stream."""
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    _check_dev(obs_mean, obs_std, bn_mean, bn_var)
    if out is None:
        out = _rollout_outputs(n_lanes, dev)
    pd = spec.desc(bn_mean, bn_var)
    ed = env.desc()
    if states is not None or obs_stats is not None or u_inject is not None:
        x = _lib.RolloutExtras(None, None, None, None, 0.0, None)
        if u_inject is not None:
            _check_dev(u_inject)
            k = 1 if spec.kind == "discrete" else spec.n_act
            if u_inject.dtype != torch.float32 or not u_inject.is_contiguous() or \
                    u_inject.numel() != n_lanes * env.episode_len * k:
                raise ValueError("u_inject must be contiguous float32 [n_lanes, T, %d]" % k)
            x.u_inject = u_inject.data_ptr()
        if states is not None:
            _check_dev(states)
            if states.dtype != torch.float32 or not states.is_contiguous() or \
                    states.numel() != n_lanes * env.episode_len * spec.n_in:
                raise ValueError("states must be contiguous float32 [n_lanes, T, n_in]")
            x.states = states.data_ptr()
        if obs_stats is not None:
            x.obs_chance = float(obs_stats)
            x.obs_mean, x.obs_m2, x.obs_count = (t.data_ptr() for t in
                                                 _obs_stat_outputs(out, n_lanes, spec.n_in, dev))
        check(lib.fdr_rollout_ex(_c(dev, ctx), ctypes.byref(pd), ctypes.byref(ed), ctypes.byref(lanes), n_lanes,
                                 ctypes.c_uint64(seed & ((1 << 64) - 1)), 1 if jiggle else 0, _p(obs_mean),
                                 _p(obs_std), _p(out.reward), _p(out.entropy), _p(out.timesteps),
                                 _p(out.norm2), ctypes.byref(x), _stream(dev)), "fdr_rollout_ex")
        return out
    check(lib.fdr_rollout(_c(dev, ctx), ctypes.byref(pd), ctypes.byref(ed), ctypes.byref(lanes), n_lanes,
                          ctypes.c_uint64(seed & ((1 << 64) - 1)), 1 if jiggle else 0, _p(obs_mean),
                          _p(obs_std), _p(out.reward), _p(out.entropy), _p(out.timesteps), _p(out.norm2),
                          _stream(dev)), "fdr_rollout")
    return out


def rollout_episodes(spec, env, lanes, n_lanes, seed, n_episodes, episode_ids=None, jiggle=True, obs_mean=None,
                     obs_std=None, bn_mean=None, bn_var=None, obs_stats=None, ret_sq=False, out=None, device=None,
                     ctx=None):
    """fdr_rollout_episodes: n_episodes episodes per lane in one launch (the physics envs), theta' formed once per
    lane.  episode_ids: None (episode e of lane l draws as global lane (lane_offset + l) * K + e) or an int64
    [n_lanes, n_episodes] device tensor of stream ids in [0, 2^32) -- lanes given equal ids share their resets and
    draws.  -> RolloutResult: reward = the mean episode return, timesteps = the summed steps, entropy over all
    visited states; .reward_sq (sum of squared episode returns) with ret_sq=True; obs_stats as rollout()."""
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    _check_dev(obs_mean, obs_std, bn_mean, bn_var, episode_ids)
    K = int(n_episodes)
    if episode_ids is not None:
        if episode_ids.dtype != torch.int64 or not episode_ids.is_contiguous() or \
                episode_ids.numel() != n_lanes * K:
            raise ValueError("episode_ids must be contiguous int64 [n_lanes, n_episodes]")
    if out is None:
        out = _rollout_outputs(n_lanes, dev)
    sq = None
    if ret_sq:
        sq = getattr(out, "reward_sq", None)
        if sq is None:
            sq = out.reward_sq = torch.empty(n_lanes, dtype=torch.float64, device=dev)
    om = m2 = cnt = None
    chance = 0.0
    if obs_stats is not None:
        chance = float(obs_stats)
        om, m2, cnt = _obs_stat_outputs(out, n_lanes, spec.n_in, dev)
    pd =spec.desc(bn_mean, bn_var)
    ed = env.desc()
    check(lib.fdr_rollout_episodes(_c(dev, ctx), ctypes.byref(pd), ctypes.byref(ed), ctypes.byref(lanes), n_lanes,
                                   ctypes.c_uint64(seed & ((1 << 64) - 1)), 1 if jiggle else 0, _p(obs_mean),
                                   _p(obs_std), K, _p(episode_ids), _p(out.reward), _p(sq), _p(out.entropy),
                                   _p(out.timesteps), _p(out.norm2), _p(om), _p(m2), _p(cnt), chance, _stream(dev)),
          "fdr_rollout_episodes")
    return out


def fd_weights(rewards_all, policy_reward, lane_lo, sign_local, norm2_local, lanes_per_dir, sigma, coef=None):
    _check_dev(rewards_all, sign_local, norm2_local)
    n_local = sign_local.numel()
    n_dirs = n_local // lanes_per_dir
    if coef is None:
        coef = torch.empty(n_dirs, dtype=torch.float64, device=rewards_all.device)
    check(lib.fdr_fd_weights(_c(rewards_all.device), _p(rewards_all), rewards_all.numel(), float(policy_reward), int(lane_lo),
                             n_local, _p(sign_local), _p(norm2_local), int(lanes_per_dir), float(sigma),
                             _p(coef), _stream(rewards_all.device)), "fdr_fd_weights")
    return coef


_WS = {}


def _workspace(key, nbytes, device, zeroed=False):
    """Per-(purpose, device) scratch, grown on demand.  zeroed: allocated zero-filled (the in-launch
    counters of fdr_fd_grad_fused must start at zero; every call leaves them zero)."""
    buf = _WS.get((key, device))
    if buf is None or buf.numel() < nbytes:
        n = max(int(nbytes), 16)
        buf = torch.zeros(n, dtype=torch.uint8, device=device) if zeroed else \
            torch.empty(n, dtype=torch.uint8, device=device)
        _WS[(key, device)] = buf
    return buf


_WS_ZERO_PREFIX = {}


_FUSED_SIZES = {}


def _fused_workspace(mode, n_dirs, lanes_per_dir, n_params, device, n_all=None):
    """The fdr_fd_grad_fused / fdr_fd_step workspace with its ticket-counter prefix guaranteed zero (n_all: the
    FDR_WEIGHT_TOP_DIRS query takes it in mode's place -- its mask covers the lanes of all ranks).

    A call leaves exactly its own counter prefix, fdr_fd_grad_fused_counter_bytes(n_dirs, P), at zero; the bytes
    behind it hold that call's slabs / partials.  A later call whose prefix is longer (more column blocks) would
    find non-zero counters there, so the prefix is re-zeroed (on the current stream, ahead of the launch)
    whenever it grows past what is known to be zero."""
    key = ("fused_%d" % mode, device)
    old = _WS.get(key)
    skey = (mode, n_dirs, int(lanes_per_dir), n_params, n_all)
    sizes = _FUSED_SIZES.get(skey)
    if sizes is None:  # the library's size queries, once per shape
        if mode == _lib.FDR_WEIGHT_TOP_DIRS:
            nb = lib.fdr_fd_grad_fused_top_workspace_bytes(n_dirs, int(lanes_per_dir), n_params, int(n_all))
        else:
            nb = lib.fdr_fd_grad_fused_workspace_bytes(n_dirs, int(lanes_per_dir), n_params, mode)
        if nb < 0:
            raise ValueError("fused workspace query: bad n_dirs / lanes_per_dir / P / n_all")
        sizes = _FUSED_SIZES[skey] = (nb, int(lib.fdr_fd_grad_fused_counter_bytes(n_dirs, n_params)))
    nb, cb = sizes
    ws = _workspace(key[0], nb, device, zeroed=True)
    if ws is not old:
        _WS_ZERO_PREFIX[key] = ws.numel()
    if cb > _WS_ZERO_PREFIX.get(key, 0):
        ws[:cb].zero_()
    _WS_ZERO_PREFIX[key] = cb
    return ws


WEIGHT_MODES = {"zscore": _lib.FDR_WEIGHT_ZSCORE, "centred_rank": _lib.FDR_WEIGHT_CENTERED_RANK,
                "moments": _lib.FDR_WEIGHT_MOMENTS, "zscore_mix": _lib.FDR_WEIGHT_ZSCORE_MIX}


def _mix_channels(channels, policy_values, coefs):
    """(reward, novelty, entropy) device f64 arrays (None: not given -- legal where the coefficient is 0), the
    policy's own three values and the three coefficients -> (arrays, device, n_all, 6 floats)."""
    channels = tuple(channels)
    if len(channels) != 3 or len(policy_values) != 3 or len(coefs) != 3:
        raise ValueError("the mixed objective takes three channels: reward, novelty, entropy")
    given = [c for c in channels if c is not None]
    if not given:
        raise ValueError("the mixed objective needs at least one channel array")
    for c in given:
        if c.dtype != torch.float64 or c.numel() != given[0].numel() or not c.is_contiguous():
            raise ValueError("channel arrays are contiguous f64 of one length")
    _check_dev(*given)
    vals = [float(0.0 if v is None else v) for v in policy_values] + [float(a) for a in coefs]
    return channels, given[0].device, given[0].numel(), vals


def fd_grad_fused_mix(table, idx_local, channels, policy_values, coefs, lane_lo, sign_local, norm2_local, lanes_per_dir,
                      sigma, n_params, out=None):
    """fd_grad_fused with the mixed weights (fdr_fd_grad_fused_mix): channels = (rewards_all, novelty_all,
    entropy_all) over all lanes, policy_values and coefs in the same order; a channel whose coefficient is 0 may be
    None and is never read.  -> g f64 [P]."""
    channels, dev, n_all, vals = _mix_channels(channels, policy_values, coefs)
    _check_dev(table, idx_local, sign_local, norm2_local, channels[0], channels[1], channels[2])
    n_dirs = idx_local.numel() // int(lanes_per_dir)
    if out is None:
        out = torch.empty(n_params, dtype=torch.float64, device=dev)
    ws = _fused_workspace(_lib.FDR_WEIGHT_ZSCORE_MIX, n_dirs, lanes_per_dir, n_params, dev)
    check(lib.fdr_fd_grad_fused_mix(_c(dev), _p(table), table.numel(), _p(idx_local), n_dirs, n_params, _p(channels[0]),
                                    _p(channels[1]), _p(channels[2]), n_all, *vals, int(lane_lo), _p(sign_local),
                                    _p(norm2_local), int(lanes_per_dir), float(sigma), _p(out), out.numel(), _p(ws),
                                    ws.numel(), _stream(dev)), "fdr_fd_grad_fused_mix")
    return out


def fd_step_mix(table, idx_local, channels, policy_values, coefs, sign_local, norm2_local, lanes_per_dir, sigma, theta,
                lr, lr_scale, g=None, out=None, theta_hist=None):
    """fd_step with the mixed weights (fdr_fd_step_mix); channels / policy_values / coefs as fd_grad_fused_mix.
    Returns device f64[2] = (||d theta||, ||grad||)."""
    channels, dev, n_all, vals = _mix_channels(channels, policy_values, coefs)
    _check_dev(table, idx_local, sign_local, norm2_local, theta, g, theta_hist, channels[0], channels[1], channels[2])
    P = theta.numel()
    n_dirs = idx_local.numel() // int(lanes_per_dir)
    if g is None:
        g = torch.empty(P, dtype=torch.float64, device=dev)
    if out is None:
        out = torch.empty(2, dtype=torch.float64, device=dev)
    ws = _fused_workspace(_lib.FDR_WEIGHT_ZSCORE_MIX, n_dirs, lanes_per_dir, P, dev)
    check(lib.fdr_fd_step_mix(_c(dev), _p(table), table.numel(), _p(idx_local), n_dirs, P, _p(channels[0]),
                              _p(channels[1]), _p(channels[2]), n_all, *vals, _p(sign_local), _p(norm2_local),
                              int(lanes_per_dir), float(sigma), _p(theta), float(lr), float(lr_scale), _p(g),
                              _p(theta_hist), _p(out), _p(ws), ws.numel(), _stream(dev)), "fdr_fd_step_mix")
    return out


def fd_weights_mix(channels, policy_values, coefs, lane_lo, sign_local, norm2_local, lanes_per_dir, sigma, coef=None):
    """fd_weights with the mixed weights (fdr_fd_weights_mix) -> coef f64 [n_dirs]."""
    channels, dev, n_all, vals = _mix_channels(channels, policy_values, coefs)
    _check_dev(sign_local, norm2_local, channels[0], channels[1], channels[2])
    n_local = sign_local.numel()
    if coef is None:
        coef = torch.empty(n_local // int(lanes_per_dir), dtype=torch.float64, device=dev)
    check(lib.fdr_fd_weights_mix(_c(dev), _p(channels[0]), _p(channels[1]), _p(channels[2]), n_all, *vals, int(lane_lo),
                                 n_local, _p(sign_local), _p(norm2_local), int(lanes_per_dir), float(sigma), _p(coef),
                                 _stream(dev)), "fdr_fd_weights_mix")
    return coef


def fd_grad_fused(table, idx_local, rewards_all, policy_reward, lane_lo, sign_local, norm2_local, lanes_per_dir, sigma,
                  n_params, mode="zscore", out=None, n_all=None):
    """Weights + noise-weighted gradient in one launch (fdr_fd_grad_fused).  idx_local / sign_local / norm2_local:
    one entry per local lane.  mode "zscore" / "centred_rank" -> g f64 [P]; "moments" (rewards_all = the local
    rewards, n_all = the lanes of all ranks, lane_lo = this rank's first global lane) ->
    [A | B | n_local | r' slots [n_all]] f64 [2P + 1 + n_all]."""
    _check_dev(table, idx_local, rewards_all, sign_local, norm2_local)
    dev = table.device
    n_dirs = idx_local.numel() // int(lanes_per_dir)
    m = WEIGHT_MODES[mode]
    if n_all is None:
        n_all = rewards_all.numel() + (int(lane_lo) if mode == "moments" else 0)
    n_out = int(lib.fdr_fd_grad_fused_out_len(m, n_params, int(n_all)))
    if n_out <= 0:
        raise ValueError("fd_grad_fused: bad mode / P / n_all")
    if out is None:
        out = torch.empty(n_out, dtype=torch.float64, device=dev)
    elif out.numel() < n_out:
        raise ValueError("fd_grad_fused: out holds %d doubles, needs %d" % (out.numel(), n_out))
    ws = _fused_workspace(m, n_dirs, lanes_per_dir, n_params, dev)
    check(lib.fdr_fd_grad_fused(_c(dev), _p(table), table.numel(), _p(idx_local), n_dirs, n_params, _p(rewards_all),
                                int(n_all), float(policy_reward), int(lane_lo), _p(sign_local), _p(norm2_local),
                                int(lanes_per_dir), float(sigma), m, _p(out), out.numel(), _p(ws), ws.numel(),
                                _stream(dev)),
          "fdr_fd_grad_fused")
    return out


def fd_step(table, idx_local, rewards, policy_reward, sign_local, norm2_local, lanes_per_dir, sigma, theta, lr,
            lr_scale, mode="zscore", g=None, out=None, theta_hist=None):
    """The single-process FD step (fdr_fd_step): weights + gradient (-> g) in one launch, DSGD on theta in place in
    a second; theta_hist (f32 [P], optional) receives the updated theta.  Returns device f64[2] =
    (||d theta||, ||grad||)."""
    _check_dev(table, idx_local, rewards, sign_local, norm2_local, theta, g, theta_hist)
    dev = table.device
    P = theta.numel()
    n_dirs = idx_local.numel() // int(lanes_per_dir)
    m = WEIGHT_MODES[mode]
    if g is None:
        g = torch.empty(P, dtype=torch.float64, device=dev)
    if out is None:
        out = torch.empty(2, dtype=torch.float64, device=dev)
    ws = _fused_workspace(m, n_dirs, lanes_per_dir, P, dev)
    check(lib.fdr_fd_step(_c(dev), _p(table), table.numel(), _p(idx_local), n_dirs, P, _p(rewards), rewards.numel(),
                          float(policy_reward), _p(sign_local), _p(norm2_local), int(lanes_per_dir), float(sigma), m,
                          _p(theta), float(lr), float(lr_scale), _p(g), _p(theta_hist), _p(out), _p(ws), ws.numel(),
                          _stream(dev)), "fdr_fd_step")
    return out


def rank_weights(rewards_all, lane_lo, n_local):
    """Centred-rank weights of lanes [lane_lo, lane_lo + n_local) over rewards_all (f64 [n_local])."""
    _check_dev(rewards_all)
    w = torch.empty(n_local, dtype=torch.float64, device=rewards_all.device)
    check(lib.fdr_rank_weights(_c(rewards_all.device), _p(rewards_all), rewards_all.numel(), int(lane_lo), int(n_local), _p(w),
                               _stream(rewards_all.device)), "fdr_rank_weights")
    return w


def top_dir_weights(rewards_all, policy_reward, lanes_per_dir, top_dirs, lane_lo, n_local, selected=False):
    """Top-b direction weights (fdr_top_dir_weights) of lanes [lane_lo, lane_lo + n_local): the top_dirs best
    directions by the maximum of their lanes_per_dir returns keep their lanes, z-scored over the kept lanes; 0.0
    elsewhere.  -> w f64 [n_local], or (w, selected int8 [n_local / lanes_per_dir]) with selected=True."""
    _check_dev(rewards_all)
    dev = rewards_all.device
    w = torch.empty(n_local, dtype=torch.float64, device=dev)
    sel = torch.empty(n_local // max(1, int(lanes_per_dir)), dtype=torch.int8, device=dev) if selected else None
    ws = _workspace("top_dirs", max(0, lib.fdr_top_dir_weights_workspace_bytes(rewards_all.numel())), dev)
    check(lib.fdr_top_dir_weights(_c(dev), _p(rewards_all), rewards_all.numel(), float(policy_reward),
                                  int(lanes_per_dir), int(top_dirs), int(lane_lo), int(n_local), _p(w), _p(sel), _p(ws),
                                  ws.numel(), _stream(dev)), "fdr_top_dir_weights")
    return (w, sel) if selected else w


def fd_grad_fused_top(table, idx_local, rewards_all, policy_reward, lane_lo, sign_local, norm2_local, lanes_per_dir,
                      sigma, n_params, top_dirs, out=None):
    """fd_grad_fused with the top-b direction weights (fdr_fd_grad_fused_top): top_dirs of the n_all / lanes_per_dir
    directions of rewards_all (all ranks' lanes) are kept.  -> g f64 [P]."""
    _check_dev(table, idx_local, rewards_all, sign_local, norm2_local)
    dev = table.device
    n_dirs = idx_local.numel() // int(lanes_per_dir)
    if out is None:
        out = torch.empty(n_params, dtype=torch.float64, device=dev)
    ws = _fused_workspace(_lib.FDR_WEIGHT_TOP_DIRS, n_dirs, lanes_per_dir, n_params, dev, n_all=rewards_all.numel())
    check(lib.fdr_fd_grad_fused_top(_c(dev), _p(table), table.numel(), _p(idx_local), n_dirs, n_params,
                                    _p(rewards_all), rewards_all.numel(), float(policy_reward), int(lane_lo),
                                    _p(sign_local), _p(norm2_local), int(lanes_per_dir), float(sigma), int(top_dirs),
                                    _p(out), out.numel(), _p(ws), ws.numel(), _stream(dev)), "fdr_fd_grad_fused_top")
    return out


def fd_step_top(table, idx_local, rewards, policy_reward, sign_local, norm2_local, lanes_per_dir, sigma, theta, lr,
                lr_scale, top_dirs, g=None, out=None, theta_hist=None):
    """fd_step with the top-b direction weights (fdr_fd_step_top).  Returns device f64[2] = (||d theta||, ||grad||)."""
    _check_dev(table, idx_local, rewards, sign_local, norm2_local, theta, g, theta_hist)
    dev = table.device
    P = theta.numel()
    n_dirs = idx_local.numel() // int(lanes_per_dir)
    if g is None:
        g = torch.empty(P, dtype=torch.float64, device=dev)
    if out is None:
        out = torch.empty(2, dtype=torch.float64, device=dev)
    ws = _fused_workspace(_lib.FDR_WEIGHT_TOP_DIRS, n_dirs, lanes_per_dir, P, dev, n_all=rewards.numel())
    check(lib.fdr_fd_step_top(_c(dev), _p(table), table.numel(), _p(idx_local), n_dirs, P, _p(rewards), rewards.numel(),
                              float(policy_reward), _p(sign_local), _p(norm2_local), int(lanes_per_dir), float(sigma),
                              int(top_dirs), _p(theta), float(lr), float(lr_scale), _p(g), _p(theta_hist), _p(out),
                              _p(ws), ws.numel(), _stream(dev)), "fdr_fd_step_top")
    return out


def dsgd_step_ex(theta, src, moments, lr, lr_scale, g_out=None, out=None):
    """DSGD from g (moments=False) or from summed moments (g = (A - m B) / sd written to g_out)."""
    _check_dev(theta, src, g_out)
    dev = theta.device
    if out is None:
        out = torch.empty(2, dtype=torch.float64, device=dev)
    nb = lib.fdr_dsgd_workspace_bytes(theta.numel())
    ws = _workspace("dsgd", nb, dev)
    check(lib.fdr_dsgd_step_ex(_c(dev), _p(theta), _p(src), 1 if moments else 0, theta.numel(), float(lr), float(lr_scale),
                               _p(g_out), _p(out), _p(ws), ws.numel(), _stream(dev)), "fdr_dsgd_step_ex")
    return out


OPT_KINDS = {"adam": _lib.FDR_OPT_ADAM, "adamw": _lib.FDR_OPT_ADAMW, "sgd": _lib.FDR_OPT_SGD}


class OptSpec(object):
    """One torch.optim step for fdr_opt_step / fdr_fd_step_opt: kind "adam" | "adamw" | "sgd", the hyperparameters as
    torch's param group holds them, step = the count including this step, and the f32 [P] state rows (adam / adamw:
    exp_avg, exp_avg_sq; sgd with momentum: momentum_buffer, None)."""

    def __init__(self, kind, lr, step, state0=None, state1=None, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                 momentum=0.0, dampening=0.0, nesterov=False):
        self.kind = OPT_KINDS[kind] if isinstance(kind, str) else int(kind)
        self.lr, self.step, self.state0, self.state1 = float(lr), int(step), state0, state1
        self.betas, self.eps, self.weight_decay = (float(betas[0]), float(betas[1])), float(eps), float(weight_decay)
        self.momentum, self.dampening, self.nesterov = float(momentum), float(dampening), bool(nesterov)

    def args(self):
        """The optimizer block of the C calls, in order."""
        return (self.kind, self.lr, self.betas[0], self.betas[1], self.eps, self.weight_decay, self.momentum,
                self.dampening, 1 if self.nesterov else 0, self.step, _p(self.state0), _p(self.state1))

    def check(self, P, dev):
        for t in (self.state0, self.state1):
            if t is not None and (t.dtype != torch.float32 or t.numel() != P or not t.is_contiguous()
                                  or t.device != dev):
                raise ValueError("optimizer state rows are contiguous f32 [P] on theta's device")


def opt_step(theta, src, moments, opt, g_out=None, out=None, theta_hist=None):
    """An Adam / AdamW / SGD step (fdr_opt_step) from g (moments=False) or from summed moments (g written to g_out);
    any P.  Returns device f64[2] = (||d theta||, ||fl32(-g)||)."""
    _check_dev(theta, src, g_out, theta_hist)
    dev = theta.device
    P = theta.numel()
    opt.check(P, dev)
    if out is None:
        out = torch.empty(2, dtype=torch.float64, device=dev)
    ws = _workspace("opt", lib.fdr_opt_workspace_bytes(P), dev, zeroed=True)   # the ticket counter starts at zero
    check(lib.fdr_opt_step(_c(dev), opt.kind, _p(theta), _p(src), 1 if moments else 0, P, *opt.args()[1:], _p(g_out),
                           _p(theta_hist), _p(out), _p(ws), ws.numel(), _stream(dev)), "fdr_opt_step")
    return out


def fd_step_opt(table, idx_local, rewards, policy_reward, sign_local, norm2_local, lanes_per_dir, sigma, theta, opt,
                mode="zscore", g=None, out=None, theta_hist=None):
    """fd_step with the optimizer's apply launch in DSGD's place (fdr_fd_step_opt): weights + gradient (-> g) in one
    launch, opt (an OptSpec) on theta and its state in place in a second.  Returns device f64[2]."""
    _check_dev(table, idx_local, rewards, sign_local, norm2_local, theta, g, theta_hist)
    dev = table.device
    P = theta.numel()
    opt.check(P, dev)
    n_dirs = idx_local.numel() // int(lanes_per_dir)
    m = WEIGHT_MODES[mode]
    if g is None:
        g = torch.empty(P, dtype=torch.float64, device=dev)
    if out is None:
        out = torch.empty(2, dtype=torch.float64, device=dev)
    ws = _fused_workspace(m, n_dirs, lanes_per_dir, P, dev)
    check(lib.fdr_fd_step_opt(_c(dev), _p(table), table.numel(), _p(idx_local), n_dirs, P, _p(rewards), rewards.numel(),
                              float(policy_reward), _p(sign_local), _p(norm2_local), int(lanes_per_dir), float(sigma), m,
                              _p(theta), *opt.args(), _p(g), _p(theta_hist), _p(out), _p(ws), ws.numel(), _stream(dev)),
          "fdr_fd_step_opt")
    return out


def fd_step_top_opt(table, idx_local, rewards, policy_reward, sign_local, norm2_local, lanes_per_dir, sigma, theta, opt,
                    top_dirs, g=None, out=None, theta_hist=None):
    """fd_step_top with the optimizer's apply launch in DSGD's place (fdr_fd_step_top_opt); opt an OptSpec."""
    _check_dev(table, idx_local, rewards, sign_local, norm2_local, theta, g, theta_hist)
    dev = table.device
    P = theta.numel()
    opt.check(P, dev)
    n_dirs = idx_local.numel() // int(lanes_per_dir)
    if g is None:
        g = torch.empty(P, dtype=torch.float64, device=dev)
    if out is None:
        out = torch.empty(2, dtype=torch.float64, device=dev)
    ws = _fused_workspace(_lib.FDR_WEIGHT_TOP_DIRS, n_dirs, lanes_per_dir, P, dev, n_all=rewards.numel())
    check(lib.fdr_fd_step_top_opt(_c(dev), _p(table), table.numel(), _p(idx_local), n_dirs, P, _p(rewards),
                                  rewards.numel(), float(policy_reward), _p(sign_local), _p(norm2_local),
                                  int(lanes_per_dir), float(sigma), int(top_dirs), _p(theta), *opt.args(), _p(g),
                                  _p(theta_hist), _p(out), _p(ws), ws.numel(), _stream(dev)), "fdr_fd_step_top_opt")
    return out


def fd_step_mix_opt(table, idx_local, channels, policy_values, coefs, sign_local, norm2_local, lanes_per_dir, sigma,
                    theta, opt, g=None, out=None, theta_hist=None):
    """fd_step_mix with the optimizer's apply launch in DSGD's place (fdr_fd_step_mix_opt)."""
    channels, dev, n_all, vals = _mix_channels(channels, policy_values, coefs)
    _check_dev(table, idx_local, sign_local, norm2_local, theta, g, theta_hist, channels[0], channels[1], channels[2])
    P = theta.numel()
    opt.check(P, dev)
    n_dirs = idx_local.numel() // int(lanes_per_dir)
    if g is None:
        g = torch.empty(P, dtype=torch.float64, device=dev)
    if out is None:
        out = torch.empty(2, dtype=torch.float64, device=dev)
    ws = _fused_workspace(_lib.FDR_WEIGHT_ZSCORE_MIX, n_dirs, lanes_per_dir, P, dev)
    check(lib.fdr_fd_step_mix_opt(_c(dev), _p(table), table.numel(), _p(idx_local), n_dirs, P, _p(channels[0]),
                                  _p(channels[1]), _p(channels[2]), n_all, *vals, _p(sign_local), _p(norm2_local),
                                  int(lanes_per_dir), float(sigma), _p(theta), *opt.args(), _p(g), _p(theta_hist),
                                  _p(out), _p(ws), ws.numel(), _stream(dev)), "fdr_fd_step_mix_opt")
    return out


def fd_grad(table, idx_dirs, coef, n_params, g=None):
    _check_dev(table, idx_dirs, coef)
    dev = table.device
    n_dirs = idx_dirs.numel()
    if g is None:
        g = torch.empty(n_params, dtype=torch.float64, device=dev)
    nb = lib.fdr_fd_grad_workspace_bytes(n_dirs, n_params)
    ws = _workspace("grad", nb, dev)
    check(lib.fdr_fd_grad(_c(dev), _p(table), table.numel(), _p(idx_dirs), _p(coef), n_dirs, n_params, _p(g),
                          _p(ws), ws.numel(), _stream(dev)), "fdr_fd_grad")
    return g


def dsgd_step(theta, g, lr, lr_scale, out=None):
    """In-place theta update; returns device f64[2] = (||d theta||, ||grad||)."""
    _check_dev(theta, g)
    dev = theta.device
    if out is None:
        out = torch.empty(2, dtype=torch.float64, device=dev)
    nb = lib.fdr_dsgd_workspace_bytes(theta.numel())
    ws = _workspace("dsgd", nb, dev)
    check(lib.fdr_dsgd_step(_c(dev), _p(theta), _p(g), theta.numel(), float(lr), float(lr_scale), _p(out), _p(ws),
                            ws.numel(), _stream(dev)), "fdr_dsgd_step")
    return out


# ---- ImpalaPolicy (policies/impala.py) --------------------------------------------------------
def impala_num_params(n_act):
    return int(lib.fdr_impala_num_params(int(n_act)))


def impala_num_bn_stats():
    return int(lib.fdr_impala_num_bn_stats())


class ImpalaSpec(object):
    """Shape of an ImpalaPolicy rollout: A actions, E envs per perturbation, T-step episodes."""

    def __init__(self, n_act, envs_per_lane=1, episode_len=1, entropy=True, env_seed=0, fp16=False, pairs=False):
        """pairs: lanes 2p, 2p+1 are antithetic pairs -- the rollout's core step streams each pair's sigma-eps once
        (fdr_impala_desc.pairs; f32: bit-identical to the per-lane form, fp16: within the fp16 tolerance)."""
        self.n_act, self.envs_per_lane, self.episode_len = int(n_act), int(envs_per_lane), int(episode_len)
        self.entropy, self.env_seed, self.fp16 = bool(entropy), int(env_seed), bool(fp16)
        self.pairs = bool(pairs)
        self.n_params = impala_num_params(n_act)
        if self.n_params < 0:
            raise ValueError("n_act out of range")

    def desc(self, bn_mean=None, bn_var=None):
        _check_dev(bn_mean, bn_var)
        for t in (bn_mean, bn_var):
            if t is not None and (t.dtype != torch.float32 or t.numel() != impala_num_bn_stats()):
                raise ValueError("BN stats must be float32[%d]" % impala_num_bn_stats())
        return _lib.ImpalaDesc(self.n_act, self.envs_per_lane, self.episode_len, 1 if self.entropy else 0,
                               self.env_seed & ((1 << 64) - 1), self.n_params,
                               None if bn_mean is None else bn_mean.data_ptr(),
                               None if bn_var is None else bn_var.data_ptr(), 1 if self.fp16 else 0,
                               1 if self.pairs else 0)


def impala_rollout(spec, lanes, n_lanes, seed, jiggle=True, bn_mean=None, bn_var=None, record=False, out=None,
                   device=None, ctx=None):
    """fdr_impala_rollout: returns RolloutResult with per-env [n_lanes*E] fields, norm2 per lane,
    plus .actions [n_lanes*E, T] / .probs [n_lanes*E, T, A] when record=True."""
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    n_env = n_lanes * spec.envs_per_lane
    if out is None:
        out = RolloutResult(torch.empty(n_env, dtype=torch.float64, device=dev),
                            torch.empty(n_env, dtype=torch.float64, device=dev),
                            torch.empty(n_env, dtype=torch.int32, device=dev),
                            torch.empty(n_lanes, dtype=torch.float64, device=dev))
    out.actions = torch.empty((n_env, spec.episode_len), dtype=torch.int32, device=dev) if record else None
    out.probs = torch.empty((n_env, spec.episode_len, spec.n_act), dtype=torch.float32, device=dev) if record \
        else None
    d = spec.desc(bn_mean, bn_var)
    nb = lib.fdr_impala_workspace_bytes(ctypes.byref(d), n_lanes)
    if nb < 0:
        raise ValueError("bad impala spec")
    ws = _workspace("impala", nb, dev)
    check(lib.fdr_impala_rollout(_c(dev, ctx), ctypes.byref(d), ctypes.byref(lanes), n_lanes,
                                 ctypes.c_uint64(seed & ((1 << 64) - 1)), 1 if jiggle else 0, _p(out.reward),
                                 _p(out.entropy), _p(out.timesteps), _p(out.norm2), _p(out.actions), _p(out.probs),
                                 _p(ws), ws.numel(), _stream(dev)), "fdr_impala_rollout")
    return out


def impala_forward(spec, theta, frames, h, c, reward=None, notdone=None, bn_mean=None, bn_var=None, feat=False):
    """One ImpalaCNN step for n envs sharing theta; h, c [n, 256] are updated in place.
    Returns probs [n, A] (and the relu'd conv features [n, 2048] if feat)."""
    _check_dev(theta, frames, h, c, reward, notdone)
    dev = theta.device
    frames = frames.to(torch.float32).reshape(-1, 3 * 64 * 64).contiguous()
    n = frames.shape[0]
    for t in (h, c):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != n * 256:
            raise ValueError("h / c must be contiguous float32 [n, 256]")
    if reward is not None:
        reward = reward.to(torch.float32).reshape(-1).contiguous()
    if notdone is not None:
        notdone = notdone.to(torch.float32).reshape(-1).contiguous()
    probs = torch.empty((n, spec.n_act), dtype=torch.float32, device=dev)
    f = torch.empty((n, 2048), dtype=torch.float32, device=dev) if feat else None
    d = spec.desc(bn_mean, bn_var)
    nb = lib.fdr_impala_forward_workspace_bytes(spec.n_act, n, 1 if spec.fp16 else 0)
    ws = _workspace("impala_fwd", nb, dev)
    check(lib.fdr_impala_forward(_c(dev), ctypes.byref(d), _p(theta), n, _p(frames), _p(reward), _p(notdone), _p(h),
                                 _p(c), _p(probs), _p(f), _p(ws), ws.numel(), _stream(dev)), "fdr_impala_forward")
    return (probs, f) if feat else probs


def impala_strategies(spec, lanes, n_lanes, frames, reward=None, h=None, c=None, bn_mean=None, bn_var=None):
    """get_strategy of n_lanes ImpalaPolicy parameter vectors over the Z shared probe obs: the stacked obs
    run as ONE LSTM sequence per lane (policies/impala.py:24-27) from (h, c) [n_lanes, 256] (updated in
    place) or from the reset state (None).  frames [Z, 3, 64, 64] (0..255), reward [Z] -> probs
    [n_lanes, Z, A] f32."""
    dev = frames.device
    _check_dev(frames, reward, h, c)
    frames = frames.to(torch.float32).reshape(-1, 3 * 64 * 64).contiguous()
    Z = frames.shape[0]
    if reward is not None:
        reward = reward.to(torch.float32).reshape(-1).contiguous()
        if reward.numel() != Z:
            raise ValueError("reward must have one entry per probe frame")
    if (h is None) != (c is None):
        raise ValueError("give both h and c, or neither")
    for t in (h, c):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != n_lanes * 256):
            raise ValueError("h / c must be contiguous float32 [n_lanes, 256]")
    probs = torch.empty((n_lanes, Z, spec.n_act), dtype=torch.float32, device=dev)
    d = spec.desc(bn_mean, bn_var)
    nb = lib.fdr_impala_strategies_workspace_bytes(ctypes.byref(d), n_lanes, Z)
    if nb < 0:
        raise ValueError("bad impala spec")
    ws = _workspace("impala_strat", nb, dev)
    check(lib.fdr_impala_strategies(_c(dev), ctypes.byref(d), ctypes.byref(lanes), n_lanes, Z, _p(frames), _p(reward),
                                    _p(h), _p(c), _p(probs), _p(ws), ws.numel(), _stream(dev)),
          "fdr_impala_strategies")
    return probs


def impala_bn_refresh(spec, theta, frames, bn_mean, bn_var, reward=None, first_done=False, h=None, c=None,
                      momentum=0.1):
    """ImpalaPolicy.compute_vbn on the device (policies/impala.py:12-16): a train-mode pass of the n-obs buffer
    frames [n, 3, 64, 64] (0..255) / reward [n] updates bn_mean / bn_var (modules() order) in place; the LSTM runs
    the n obs as one sequence from (h, c) [256] (zeroed first if first_done; None: zero state) and leaves its end
    state in h / c."""
    _check_dev(theta, frames, bn_mean, bn_var, reward, h, c)
    dev = theta.device
    frames = frames.to(torch.float32).reshape(-1, 3 * 64 * 64).contiguous()
    n = frames.shape[0]
    if reward is not None:
        reward = reward.to(torch.float32).reshape(-1).contiguous()
        if reward.numel() != n:
            raise ValueError("reward must have one entry per buffer frame")
    if (h is None) != (c is None):
        raise ValueError("give both h and c, or neither")
    for t in (h, c, bn_mean, bn_var):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise ValueError("h / c / bn_mean / bn_var must be contiguous float32")
    if h is not None and (h.numel() != 256 or c.numel() != 256):
        raise ValueError("h / c must hold 256 floats")
    if n < 2:
        raise ValueError("Expected more than 1 value per channel when training (compute_vbn needs >= 2 obs)")
    d = spec.desc(None, None)
    ws = _workspace("impala_vbn", lib.fdr_impala_bn_refresh_workspace_bytes(n), dev)
    check(lib.fdr_impala_bn_refresh(_c(dev), ctypes.byref(d), _p(theta), n, _p(frames), _p(reward),
                                    1 if first_done else 0, _p(h), _p(c), float(momentum), _p(bn_mean), _p(bn_var),
                                    _p(ws), ws.numel(), _stream(dev)), "fdr_impala_bn_refresh")


def impala_env_frames(env_seed, n_act, env_id, t0, n, actions=None, device=None):
    """The frame env's observations frame_t (t0 <= t < t0 + n) of global env env_id -> (frames [n, 3, 64, 64]
    f32, rewards [n] f32 returned by the steps given actions [n] (device i32; None -> 0))."""
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if actions is not None:
        _check_dev(actions)
        actions = actions.to(torch.int32).reshape(-1).contiguous()
        if actions.numel() != n:
            raise ValueError("actions must have n entries")
    frames = torch.empty((n, 3, 64, 64), dtype=torch.float32, device=dev)
    reward = torch.empty(n, dtype=torch.float32, device=dev)
    check(lib.fdr_impala_env_frames(ctypes.c_uint64(int(env_seed) & ((1 << 64) - 1)), int(n_act), int(env_id), int(t0),
                                    int(n), _p(actions), _p(frames), _p(reward), _stream(dev)), "fdr_impala_env_frames")
    return frames, reward


def impala_profile(enable, device=None):
    """Phase timing of the device's Impala rollouts (its engine context)."""
    context(device).impala_profile(enable)


def impala_profile_read(device=None):
    """(conv_ms, core_ms, replay_ms) summed over the last profiled fdr_impala_rollout (host sync)."""
    return context(device).impala_profile_read()


# ---- strategy distances / novelty (utils/math_helpers.py:147-222) ---------------------------------
DIST_KINDS = {"l2": _lib.FDR_DIST_L2, "tvd": _lib.FDR_DIST_TVD, "w2": _lib.FDR_DIST_W2}


def strategy_distances(strategies, archive, kind, full=False):
    """strategies [n, Z, D], archive [H, Z, D] (f32 device) -> (min [n] f64, argmin [n] i32[, dists [n, H]])."""
    _check_dev(strategies, archive)
    S = strategies.to(torch.float32).contiguous()
    B = archive.to(torch.float32).contiguous()
    n, Z, D = S.shape
    H = B.shape[0]
    if tuple(B.shape[1:]) != (Z, D):
        raise ValueError("archive shape %s does not match strategies %s" % (tuple(B.shape), tuple(S.shape)))
    dev = S.device
    mn = torch.empty(n, dtype=torch.float64, device=dev)
    am = torch.empty(n, dtype=torch.int32, device=dev)
    dd = torch.empty((n, H), dtype=torch.float64, device=dev) if full else None
    check(lib.fdr_strategy_distances(_c(dev), _p(S), n, _p(B), H, Z, D, DIST_KINDS[kind], _p(dd), _p(mn), _p(am),
                                     _stream(dev)), "fdr_strategy_distances")
    return (mn, am, dd) if full else (mn, am)


def lane_strategies(spec, lanes_fn, n_lanes, zeta, bn_mean=None, bn_var=None):
    """get_strategy (discrete: probs; mujoco: [mean | std]) of n_lanes policies over the Z probe
    states zeta -> f32 [n_lanes, Z, D].  lanes_fn(Z) must return a lanes descriptor of n_lanes * Z
    (policy, state) pairs, policy-major (every lane field repeated Z times)."""
    _check_dev(zeta)
    Z = zeta.shape[0]
    x = zeta.to(torch.float32).reshape(Z, -1).repeat(n_lanes, 1).contiguous()
    out = policy_forward(spec, lanes_fn(Z), n_lanes * Z, x, bn_mean, bn_var)
    if isinstance(out, tuple):
        out = torch.cat(out, dim=-1)
    return out.reshape(n_lanes, Z, -1)


def obs_stats_merge(mean, m2, count, acc_mean, acc_m2, acc_count):
    """Fold per-lane Welford partials into the device accumulator (in place, lane order)."""
    _check_dev(mean, m2, count, acc_mean, acc_m2, acc_count)
    n, d = mean.shape
    check(lib.fdr_obs_stats_merge(_c(mean.device), _p(mean), _p(m2), _p(count), n, d, _p(acc_mean), _p(acc_m2), _p(acc_count),
                                  _stream(mean.device)), "fdr_obs_stats_merge")


# ---- run batches: R independent linear-policy runs per launch (run_population.py) ------------------
def _runs_f32(t, shape, what):
    if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
        raise ValueError("%s must be contiguous float32 %s" % (what, list(shape)))


def rollout_runs(spec, env, theta_runs, sigma_runs, run_lane_offset, lanes_per_run, seed, table=None, idx=None,
                 sign=None, n_episodes=1, episode_ids=None, jiggle=True, obs_mean_runs=None, obs_std_runs=None,
                 obs_stats=None, ret_sq=False, out=None, ctx=None):
    """fdr_rollout_runs: R runs x lanes_per_run lanes of a linear policy in one launch.  theta_runs [R, P], sigma_runs
    [R], obs_mean_runs / obs_std_runs [R, n_in] (both or neither) f32 and run_lane_offset [R] i64 per run; idx / sign
    [R * L] into the shared table and episode_ids [R * L, K] per lane.  Run r's lanes are bit for bit
    rollout_episodes' for run r's slices.  -> RolloutResult over the R * L lanes (entropy 0.0), as rollout_episodes."""
    _check_dev(theta_runs, sigma_runs, run_lane_offset, table, idx, sign, episode_ids, obs_mean_runs, obs_std_runs)
    dev = theta_runs.device
    R, L, K = theta_runs.shape[0], int(lanes_per_run), int(n_episodes)
    n_lanes = R * L
    _runs_f32(theta_runs, (R, spec.n_params), "theta_runs")
    _runs_f32(sigma_runs, (R,), "sigma_runs")
    if run_lane_offset.dtype != torch.int64 or not run_lane_offset.is_contiguous() or run_lane_offset.numel() != R:
        raise ValueError("run_lane_offset must be contiguous int64 [R]")
    if (obs_mean_runs is None) != (obs_std_runs is None):
        raise ValueError("obs_mean_runs and obs_std_runs go together")
    if obs_mean_runs is not None:
        _runs_f32(obs_mean_runs, (R, spec.n_in), "obs_mean_runs")
        _runs_f32(obs_std_runs, (R, spec.n_in), "obs_std_runs")
    if table is not None:
        if idx is None or idx.dtype != torch.int64 or not idx.is_contiguous() or idx.numel() != n_lanes:
            raise ValueError("idx must be contiguous int64 [R * lanes_per_run]")
        if sign is not None and (sign.dtype != torch.int8 or not sign.is_contiguous() or sign.numel() != n_lanes):
            raise ValueError("sign must be contiguous int8 [R * lanes_per_run]")
    if episode_ids is not None and (episode_ids.dtype != torch.int64 or not episode_ids.is_contiguous() or
                                    episode_ids.numel() != n_lanes * K):
        raise ValueError("episode_ids must be contiguous int64 [R * lanes_per_run, n_episodes]")
    if out is None:
        out = _rollout_outputs(n_lanes, dev)
    sq = None
    if ret_sq:
        sq = getattr(out, "reward_sq", None)
        if sq is None:
            sq = out.reward_sq = torch.empty(n_lanes, dtype=torch.float64, device=dev)
    om = m2 = cnt = None
    chance = 0.0
    if obs_stats is not None:
        chance = float(obs_stats)
        om, m2, cnt = (getattr(out, "obs_mean", None), getattr(out, "obs_m2", None), getattr(out, "obs_count", None))
        if om is None:
            om, m2, cnt = _obs_stat_outputs(out, n_lanes, spec.n_in, dev)
    pd = spec.desc()
    ed = env.desc()
    check(lib.fdr_rollout_runs(_c(dev, ctx), ctypes.byref(pd), ctypes.byref(ed), R, L, _p(theta_runs), _p(sigma_runs),
                               _p(obs_mean_runs), _p(obs_std_runs), _p(run_lane_offset), _p(table),
                               0 if table is None else table.numel(), _p(idx), _p(sign),
                               ctypes.c_uint64(seed & ((1 << 64) - 1)), 1 if jiggle else 0, K, _p(episode_ids),
                               _p(out.reward), _p(sq), _p(out.entropy), _p(out.timesteps), _p(out.norm2), _p(om), _p(m2),
                               _p(cnt), chance, _stream(dev)), "fdr_rollout_runs")
    return out


def obs_stats_merge_runs(mean, m2, count, lanes_per_run, acc_mean, acc_m2, acc_count):
    """fdr_obs_stats_merge_runs: run r folds its lanes_per_run partials (mean / m2 [R * L, dim], count [R * L]) into
    accumulator r (acc_mean / acc_m2 [R, dim] f32, acc_count [R] i64) in lane order, in place, one launch."""
    _check_dev(mean, m2, count, acc_mean, acc_m2, acc_count)
    R, d = acc_mean.shape
    L = int(lanes_per_run)
    if mean.shape[0] != R * L or mean.shape[1] != d or count.numel() != R * L or acc_count.numel() != R:
        raise ValueError("obs_stats_merge_runs: shapes do not match [R * L, dim] / [R, dim]")
    check(lib.fdr_obs_stats_merge_runs(_c(mean.device), _p(mean), _p(m2), _p(count), R, L, d, _p(acc_mean), _p(acc_m2),
                                       _p(acc_count), _stream(mean.device)), "fdr_obs_stats_merge_runs")


def fd_step_runs(table, idx, sign, norm2, rewards, run_stride, n_train, lanes_per_dir, sigma_runs, theta_runs, lr,
                 lr_scale, policy_reward=None, top_dirs=None, g=None, out=None):
    """fdr_fd_step_runs: the whole FD step (top-b or z-score weights, gradient, DSGD) of R runs in one launch, one
    workgroup per run.  idx / sign / norm2 / rewards: per lane, run_stride entries per run, the first n_train of them
    the run's training lanes.  sigma_runs f32, lr f64, policy_reward f64 (None: 0), top_dirs i32 (None: z-score over
    all lanes): [R] device tensors.  theta_runs [R, P] is stepped in place.  -> out f64 [R, 2] = (||d theta||, ||grad||);
    g: None or f64 [R, P] receiving the gradients."""
    _check_dev(table, idx, sign, norm2, rewards, sigma_runs, theta_runs, lr, policy_reward, top_dirs, g, out)
    dev = theta_runs.device
    R, P = theta_runs.shape
    for t, dt, what in ((idx, torch.int64, "idx"), (sign, torch.int8, "sign"), (norm2, torch.float64, "norm2"),
                        (rewards, torch.float64, "rewards")):
        if t.dtype != dt or not t.is_contiguous() or t.numel() < (R - 1) * int(run_stride) + int(n_train):
            raise ValueError("%s must be contiguous %s with run_stride entries per run" % (what, dt))
    _runs_f32(theta_runs, (R, P), "theta_runs")
    _runs_f32(sigma_runs, (R,), "sigma_runs")
    for t, dt, what in ((lr, torch.float64, "lr"), (policy_reward, torch.float64, "policy_reward"),
                        (top_dirs, torch.int32, "top_dirs")):
        if t is not None and (t.dtype != dt or not t.is_contiguous() or t.numel() != R):
            raise ValueError("%s must be contiguous %s [R]" % (what, dt))
    if g is not None and (g.dtype != torch.float64 or not g.is_contiguous() or g.numel() != R * P):
        raise ValueError("g must be contiguous float64 [R, P]")
    if out is None:
        out = torch.empty((R, 2), dtype=torch.float64, device=dev)
    elif out.dtype != torch.float64 or not out.is_contiguous() or out.numel() != 2 * R:
        raise ValueError("out must be contiguous float64 [R, 2]")
    check(lib.fdr_fd_step_runs(_c(dev), _p(table), table.numel(), _p(idx), _p(sign), _p(norm2), _p(rewards),
                               int(run_stride), R, int(n_train), int(lanes_per_dir), P, _p(policy_reward),
                               _p(sigma_runs), _p(top_dirs), _p(theta_runs), _p(lr), float(lr_scale), _p(g), _p(out),
                               _stream(dev)), "fdr_fd_step_runs")
    return out


# ---- counter-based noise rows (utils/noise_sources.py CounterNoiseSource) --------------------------
def noise_fill(seed, n_rows, n_params, row_stride=None, ids=None, first_id=0, out=None, device=None):
    """out [n_rows * row_stride] f32: row r = the normals of direction id ids[r] (device int64 / uint64 bits, [n_rows])
    or first_id + r under `seed` (fdr_noise_fill: Philox4x32-10 + Box-Muller, every element of the stride written)."""
    _check_dev(ids, out)
    n_rows, n_params = int(n_rows), int(n_params)
    if row_stride is None:
        row_stride = (n_params + 3) // 4 * 4
    dev = out.device if out is not None else ids.device if ids is not None else \
        torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if ids is not None and (ids.dtype not in (torch.int64, getattr(torch, "uint64", torch.int64)) or ids.numel() != n_rows
                            or not ids.is_contiguous()):
        raise ValueError("ids must be %d contiguous 64-bit integers" % n_rows)
    if out is None:
        out = torch.empty(n_rows * int(row_stride), dtype=torch.float32, device=dev)
    elif out.dtype != torch.float32 or not out.is_contiguous() or out.numel() < n_rows * int(row_stride):
        raise ValueError("out must be contiguous float32 [n_rows * row_stride]")
    if n_rows == 0:
        return out
    mask = (1 << 64) - 1
    check(lib.fdr_noise_fill(_c(dev), int(seed) & mask, _p(ids), int(first_id) & mask, n_rows, n_params, int(row_stride),
                             _p(out), _stream(dev)), "fdr_noise_fill")
    return out


# ---- delayed returns: lambda with policy drift (learner/finite_differences.py:66-114) -------------
def fd_lambda_norms(table, idx, sign, slot, sigma, drift, n_params):
    """||fl32(sign * fl32(sigma * eps_i) + D[slot_i])||^2 per return (f64 [n])."""
    _check_dev(table, idx, sign, slot, drift)
    n = idx.numel()
    n2 = torch.empty(n, dtype=torch.float64, device=table.device)
    ns = 0 if drift is None else drift.shape[0]
    check(lib.fdr_fd_lambda_norms(_c(table.device), _p(table), table.numel(), _p(idx), _p(sign), _p(slot), n, n_params,
                                  float(sigma), _p(drift), ns, _p(n2), _stream(table.device)), "fdr_fd_lambda_norms")
    return n2


def fd_grad_lambda(table, idx, sign, slot, coef, sigma, drift, n_params, g=None):
    """g = sum_i coef_i * lambda_i (f64 [P])."""
    _check_dev(table, idx, sign, slot, coef, drift)
    dev = table.device
    n = idx.numel()
    if g is None:
        g = torch.empty(n_params, dtype=torch.float64, device=dev)
    ns = 0 if drift is None else drift.shape[0]
    nb = lib.fdr_fd_grad_workspace_bytes(n, n_params)
    ws = _workspace("grad", nb, dev)
    check(lib.fdr_fd_grad_lambda(_c(dev), _p(table), table.numel(), _p(idx), _p(sign), _p(slot), _p(coef), n, n_params,
                                 float(sigma), _p(drift), ns, _p(g), _p(ws), ws.numel(), _stream(dev)),
          "fdr_fd_grad_lambda")
    return g


def bn_refresh(spec, theta, x, bn_mean, bn_var, momentum=0.1):
    """compute_vbn on the device: updates bn_mean / bn_var (f32, [n_in | 64 | 64]) in place."""
    _check_dev(theta, x, bn_mean, bn_var)
    x = x.to(torch.float32).reshape(-1, spec.n_in).contiguous()
    n = x.shape[0]
    pd = spec.desc(None, None)
    ws = _workspace("vbn", lib.fdr_bn_refresh_workspace_bytes(n), x.device)
    check(lib.fdr_bn_refresh(_c(x.device), ctypes.byref(pd), _p(theta), _p(x), n, float(momentum), _p(bn_mean), _p(bn_var),
                             _p(ws), ws.numel(), _stream(x.device)), "fdr_bn_refresh")


# ---- AtariPolicy (policies/atari.py) -------------------------------------------------------------------
def atari_num_params(n_act):
    return int(lib.fdr_atari_num_params(int(n_act)))


class AtariSpec(object):
    def __init__(self, n_act, envs_per_lane=1, episode_len=1, env_seed=0):
        self.n_act, self.envs_per_lane, self.episode_len = int(n_act), int(envs_per_lane), int(episode_len)
        self.env_seed = int(env_seed)
        self.n_params = atari_num_params(n_act)
        if self.n_params < 0:
            raise ValueError("n_act out of range")

    def desc(self, bn_mean=None, bn_var=None):
        _check_dev(bn_mean, bn_var)
        for t in (bn_mean, bn_var):
            if t is not None and (t.dtype != torch.float32 or t.numel() != 16 + 32 + 256):
                raise ValueError("BN stats must be float32[304]")
        return _lib.AtariDesc(self.n_act, self.envs_per_lane, self.episode_len, 0, self.env_seed & ((1 << 64) - 1),
                              self.n_params, None if bn_mean is None else bn_mean.data_ptr(),
                              None if bn_var is None else bn_var.data_ptr())


def atari_rollout(spec, lanes, n_lanes, seed, jiggle=True, bn_mean=None, bn_var=None, record=False, device=None):
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    n_env = n_lanes * spec.envs_per_lane
    out = RolloutResult(torch.empty(n_env, dtype=torch.float64, device=dev),
                        torch.empty(n_env, dtype=torch.float64, device=dev),
                        torch.empty(n_env, dtype=torch.int32, device=dev),
                        torch.empty(n_lanes, dtype=torch.float64, device=dev))
    out.actions = torch.empty((n_env, spec.episode_len), dtype=torch.int32, device=dev) if record else None
    out.probs = torch.empty((n_env, spec.episode_len, spec.n_act), dtype=torch.float32, device=dev) if record \
        else None
    d = spec.desc(bn_mean, bn_var)
    nb = lib.fdr_atari_workspace_bytes(ctypes.byref(d), n_lanes)
    ws = _workspace("atari", nb, dev)
    check(lib.fdr_atari_rollout(_c(dev), ctypes.byref(d), ctypes.byref(lanes), n_lanes,
                                ctypes.c_uint64(seed & ((1 << 64) - 1)), 1 if jiggle else 0, _p(out.reward),
                                _p(out.entropy), _p(out.timesteps), _p(out.norm2), _p(out.actions), _p(out.probs),
                                _p(ws), ws.numel(), _stream(dev)), "fdr_atari_rollout")
    return out


def atari_env_frames(env_seed, env_id, t0, n, device=None):
    """The stacked-frame env's observations [n, 4, 84, 84] f32 of global env env_id at steps t0 .. t0 + n - 1
    (fdr_atari_env_frames; independent of the actions)."""
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    out = torch.empty((int(n), 4, 84, 84), dtype=torch.float32, device=dev)
    check(lib.fdr_atari_env_frames(ctypes.c_uint64(int(env_seed) & ((1 << 64) - 1)), int(env_id), int(t0), int(n),
                                   _p(out), _stream(dev)), "fdr_atari_env_frames")
    return out


def atari_forward(spec, theta, frames, bn_mean=None, bn_var=None, feat=False):
    _check_dev(theta, frames)
    frames = frames.to(torch.float32).reshape(-1, 4 * 84 * 84).contiguous()
    n = frames.shape[0]
    dev = theta.device
    probs = torch.empty((n, spec.n_act), dtype=torch.float32, device=dev)
    f = torch.empty((n, 2592), dtype=torch.float32, device=dev) if feat else None
    d = spec.desc(bn_mean, bn_var)
    ws = _workspace("atari_fwd", lib.fdr_atari_forward_workspace_bytes(spec.n_act, n), dev)
    check(lib.fdr_atari_forward(_c(dev), ctypes.byref(d), _p(theta), n, _p(frames), _p(probs), _p(f), _p(ws), ws.numel(),
                                _stream(dev)), "fdr_atari_forward")
    return (probs, f) if feat else probs


def atari_bn_refresh(spec, theta, frames, bn_mean, bn_var, momentum=0.1):
    """AtariPolicy.compute_vbn on the device (policies/policy.py:31-34): a train-mode pass of the n frames
    [n, 4, 84, 84] (0..255) updating the running stats bn_mean / bn_var [16 | 32 | 256] in place (fdr_atari_bn_refresh).
    n >= 2 (torch's train-mode BatchNorm1d raises for one value per channel)."""
    _check_dev(frames)
    dev = frames.device
    frames = frames.to(torch.float32).reshape(-1, 4 * 84 * 84).contiguous()
    n = frames.shape[0]
    if n < 2:
        raise ValueError("Expected more than 1 value per channel when training (compute_vbn needs >= 2 obs)")
    d = spec.desc(None, None)
    ws = _workspace("atari_vbn", lib.fdr_atari_bn_refresh_workspace_bytes(n), dev)
    check(lib.fdr_atari_bn_refresh(_c(dev), ctypes.byref(d), _p(theta), n, _p(frames), float(momentum), _p(bn_mean),
                                   _p(bn_var), _p(ws), ws.numel(), _stream(dev)), "fdr_atari_bn_refresh")


def atari_strategies(spec, lanes, n_lanes, frames, bn_mean=None, bn_var=None):
    """AtariPolicy.get_strategy of n_lanes parameter vectors (lanes descriptor) over the Z shared probe frames
    [Z, 4, 84, 84] (0..255) -> probs [n_lanes, Z, A] f32, batched (fdr_atari_strategies)."""
    _check_dev(frames)
    dev = frames.device
    frames = frames.to(torch.float32).reshape(-1, 4 * 84 * 84).contiguous()
    Z = frames.shape[0]
    probs = torch.empty((n_lanes, Z, spec.n_act), dtype=torch.float32, device=dev)
    d = spec.desc(bn_mean, bn_var)
    nb = lib.fdr_atari_strategies_workspace_bytes(ctypes.byref(d), n_lanes, Z)
    if nb < 0:
        raise ValueError("bad atari spec")
    ws = _workspace("atari_strat", nb, dev)
    check(lib.fdr_atari_strategies(_c(dev), ctypes.byref(d), ctypes.byref(lanes), n_lanes, Z, _p(frames), _p(probs),
                                   _p(ws), ws.numel(), _stream(dev)), "fdr_atari_strategies")
    return probs
