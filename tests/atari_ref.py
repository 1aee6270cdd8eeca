"""Float64 reference of the AtariPolicy path: features, forward, rollout semantics, strategies and compute_vbn.

TEST INFRASTRUCTURE ONLY.  Plain torch-CPU double / numpy; no project kernel.  It restates oracle/atari.py (the f32
torch-CPU oracle, pinned to the reference by G11 / G16) one precision higher, so that the distance of a device result
from THIS can be measured against the distance of the f32 oracle from this (d_oracle) instead of against a fixed
tolerance.

What is double and what is not:
  * theta' is formed exactly as the device forms it -- oracle.noise.perturb: fl32(theta + fl32(sigma * +-eps)) -- and
    only then cast to double; the running stats and the frames are cast likewise.
  * the integer streams (frames, reward targets, action uniforms, jiggle) are the oracle's own functions: they are
    integer hashes, not arithmetic.
  * BN is eval mode with eps 1e-5; entropy is torch's Categorical.entropy definition (renormalise, log clamped at the
    f32 minimum) in double; the action is argmax (deterministic lanes) or the inverse CDF over the reference's own
    probabilities with the oracle's f32 uniform.
evaluate_lanes also returns the decision margin of every (lane, env, step): how far the probabilities may move before
the action can change (stochastic: min_k |cumsum_k - u * total|; deterministic: top-1 minus top-2 probability; +inf
when n_act == 1).
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import atari as oa
from oracle import impala as oi
from oracle import rng as crng
from oracle.noise import perturb

BN_EPS = 1e-5
F32_MIN = float(torch.finfo(torch.float32).min)
STAT_BLOCKS = (("bn1", 0, 16), ("bn2", 16, 48), ("bn3", 48, 304))


def unflatten(flat, n_act):
    """f32 parameter vector -> {name: double tensor} in the reference's parameters() order."""
    flat = torch.as_tensor(np.asarray(flat, np.float32)).double()
    out, off = {}, 0
    for name, shape in oa.layout(n_act):
        n = int(np.prod(shape))
        out[name] = flat[off:off + n].view(shape)
        off += n
    assert off == flat.numel(), (off, flat.numel())
    return out


def split_bn(rm, rv):
    rm = torch.as_tensor(np.asarray(rm, np.float32)).double()
    rv = torch.as_tensor(np.asarray(rv, np.float32)).double()
    return {name: (rm[lo:hi], rv[lo:hi]) for name, lo, hi in STAT_BLOCKS}


def _bn(x, p, bn, name):
    rm, rv = bn[name]
    shape = (1, -1) + (1,) * (x.dim() - 2)
    y = (x - rm.view(shape)) / torch.sqrt(rv.view(shape) + BN_EPS)
    return y * p[name + ".w"].view(shape) + p[name + ".b"].view(shape)


def _frames64(frames):
    return torch.as_tensor(np.asarray(frames, np.float64)).reshape(-1, oa.FRAME_C, oa.FRAME_H, oa.FRAME_W)


@torch.no_grad()
def features(p, bn, frames):
    x = _frames64(frames)
    x = F.relu(_bn(F.conv2d(x, p["c1.w"], p["c1.b"], stride=4), p, bn, "bn1"))
    x = F.relu(_bn(F.conv2d(x, p["c2.w"], p["c2.b"], stride=2), p, bn, "bn2"))
    return x.reshape(x.shape[0], -1)


@torch.no_grad()
def forward(p, bn, frames):
    """-> (probs [n, A], feat [n, 2592]) double tensors."""
    f = features(p, bn, frames)
    h = F.relu(_bn(F.linear(f, p["fc.w"], p["fc.b"]), p, bn, "bn3"))
    return torch.softmax(F.linear(h, p["head.w"], p["head.b"]), dim=-1), f


def entropy(probs):
    p = torch.as_tensor(probs, dtype=torch.float64)
    p = p / p.sum(-1, keepdim=True)
    lg = torch.clamp(torch.log(p), min=F32_MIN)
    return -(p * lg).sum(-1)


def decide(probs, u=None):
    """probs [E, A] double numpy; u [E] f32 uniforms or None (argmax) -> (actions [E], margins [E])."""
    pr = np.asarray(probs, np.float64)
    E, A = pr.shape
    if u is None:
        a = pr.argmax(-1)
        if A == 1:
            return a, np.full(E, np.inf)
        top = np.sort(pr, -1)
        return a, top[:, -1] - top[:, -2]
    cs = np.cumsum(pr, -1)
    target = np.asarray(u, np.float64) * cs[:, -1]
    a = (cs[:, :-1] <= target[:, None]).sum(-1)
    if A == 1:
        return a, np.full(E, np.inf)
    return a, np.abs(cs[:, :-1] - target[:, None]).min(-1)


def norm2(table, idx, sign, sigma, P):
    s32 = np.float32(sigma)
    out = []
    for i, sg in zip(idx, sign):
        if sg == 0:
            out.append(0.0)
            continue
        st = (table[int(i):int(i) + P] * s32).astype(np.float64)
        out.append(float(np.dot(st, st)))
    return np.array(out)


def evaluate_lanes(theta, table, idx, sign, sigma, n_act, envs_per_lane, T, seed, env_seed, rm, rv,
                   deterministic=False, jiggle=True, lane_offset=0):
    """fdr_atari_rollout in double: lane l (theta'_l) drives global envs (lane_offset + l) * E + e for T steps.
    -> dict(ret [L, E], ent [L, E], steps, norm2 [L], actions [L, E, T], probs [L, E, T, A] f64,
    margin [L, E, T], step_ent [L, E, T])."""
    L, E = len(idx), int(envs_per_lane)
    thetas = perturb(theta, table, idx, sign, sigma)
    P = thetas.shape[1]
    bn = split_bn(rm, rv)
    det = np.broadcast_to(np.asarray(deterministic, dtype=bool), (L,))
    ret = np.zeros((L, E), np.float64)
    ent = np.zeros((L, E), np.float64)
    acts = np.zeros((L, E, T), np.int32)
    probs = np.zeros((L, E, T, n_act), np.float64)
    margin = np.zeros((L, E, T), np.float64)
    step_ent = np.zeros((L, E, T), np.float64)
    for l in range(L):
        p = unflatten(thetas[l], n_act)
        envs = np.uint64(lane_offset + l) * np.uint64(E) + np.arange(E, dtype=np.uint64)
        for t in range(T):
            pr, _ = forward(p, bn, oa.frames(env_seed, envs, t))
            pn = pr.numpy()
            probs[l, :, t] = pn
            a, m = decide(pn, None if det[l] else crng.uniform(seed, envs, t, 0))
            acts[l, :, t] = a
            margin[l, :, t] = m
            ret[l] += oi.rewards(env_seed, envs, t, a, n_act)
            step_ent[l, :, t] = entropy(pr).numpy()
        ent[l] = step_ent[l].sum(-1) / T
        if jiggle:
            ret[l] += crng.jiggle(seed, envs)
    return dict(ret=ret, ent=ent, steps=np.full((L, E), T, np.int32), norm2=norm2(table, idx, sign, sigma, P),
                actions=acts, probs=probs, margin=margin, step_ent=step_ent)


def strategies(theta, table, idx, sign, sigma, n_act, frames, rm, rv):
    """get_strategy of every lane's theta' over the shared probe frames -> [L, Z, A] f64."""
    thetas = perturb(theta, table, idx, sign, sigma)
    bn = split_bn(rm, rv)
    return np.stack([forward(unflatten(th, n_act), bn, frames)[0].numpy() for th in thetas])


@torch.no_grad()
def compute_vbn(p, rm, rv, frames, momentum=0.1):
    """AtariPolicy.compute_vbn in double: one train-mode pass of the buffer.  Each BN normalises with its batch mean
    and biased variance and folds the batch mean and the UNBIASED variance into its running stats with `momentum`.
    p: unflatten(...) (double).  -> (rm', rv') f64 numpy [16 | 32 | 256]."""
    rm = np.asarray(rm, np.float32).astype(np.float64)
    rv = np.asarray(rv, np.float32).astype(np.float64)
    m = float(momentum)

    def tbn(x, name, lo, hi):
        dims = [d for d in range(x.dim()) if d != 1]
        n = x.numel() // x.shape[1]
        mean = x.mean(dims, keepdim=True)
        var_sum = ((x - mean) ** 2).sum(dims, keepdim=True)
        rm[lo:hi] = m * mean.reshape(-1).numpy() + (1.0 - m) * rm[lo:hi]
        rv[lo:hi] = m * (var_sum.reshape(-1).numpy() / (n - 1)) + (1.0 - m) * rv[lo:hi]
        shape = (1, -1) + (1,) * (x.dim() - 2)
        y = (x - mean) / torch.sqrt(var_sum / n + BN_EPS)
        return y * p[name + ".w"].view(shape) + p[name + ".b"].view(shape)

    x = _frames64(frames)
    x = F.relu(tbn(F.conv2d(x, p["c1.w"], p["c1.b"], stride=4), "bn1", 0, 16))
    x = F.relu(tbn(F.conv2d(x, p["c2.w"], p["c2.b"], stride=2), "bn2", 16, 48))
    tbn(F.linear(x.reshape(x.shape[0], -1), p["fc.w"], p["fc.b"]), "bn3", 48, 304)
    return rm, rv
