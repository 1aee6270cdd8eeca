"""Float64 reference of the ImpalaPolicy path: features, core input, LSTM + head, forward with notdone, rollout
semantics (evaluate_lanes / follow_lanes), strategies with a carried and returned state, and compute_vbn.

TEST INFRASTRUCTURE ONLY.  Plain torch-CPU double / numpy; no project kernel.  It restates oracle/impala.py (the f32
torch-CPU oracle, pinned to the reference by G8 / G14) one precision higher, so that the distance of a device result
from THIS can be measured against the distance of the f32 oracle from this (d_oracle) instead of a fixed tolerance.

What is double and what is not:
  * theta' is formed exactly as the device forms it -- oracle.noise.perturb: fl32(theta + s * fl32(sigma * eps)) --
    and only then cast to double; the running stats, frames, rewards and carried states are cast likewise.
  * the integer streams (frames, reward targets, action uniforms, jiggle) are the oracle's own functions.
  * BN is eval mode with eps 1e-5; the entropy is the REPLAYED one (worker/agent.py:60-66): the visited core inputs
    run once more as one sequence from the end-of-episode state, mean over T of torch's Categorical.entropy
    (renormalise, log clamped at the f32 minimum) in double.
evaluate_lanes also returns the decision margin of every (lane, env, step): stochastic min_k |cumsum_k - u * total|,
deterministic top-1 minus top-2 probability, +inf when n_act == 1; and the largest |gate pre-activation| per step.

staged = "lane" | "pair" models the ROUNDING POINTS of the fp16 mode (fdr_impala_desc.fp16, DESIGN.md 3.4,
fdr_impala_h.hip) in float64 -- nothing of it runs on or is taken from the device:
  1. weights, lane form: conv, fc and LSTM weight matrices = f16(theta') (theta' formed in f32, rounded once into the
     half pack);
  2. weights, pair form (core_kernel_hpm2 / replay_chunk_hpm2 / xproj_pair_kernel): the convs as in 1.; fc and LSTM
     matrices = f16(theta) + s * f16(fl32(sigma eps)), the sum exact (two MFMAs into one f32 accumulator);
  3. every activation image the conv stack stores in LDS is f16: the BN'd (and ReLU'd) input of each of the 15 convs,
     and each conv's output after its f32 epilogue (bias; max pool of the stage entries; residual add) -- the features
     handed to the core are the ReLU of the last of these;
  4. the B operands of the fc (the BN1d'd features) and of the gates (fc output + clipped reward, and h) are f16;
  5. NOT rounded: BN weights / biases / statistics (folded in f32), conv / fc / LSTM biases, the head (BN, weights,
     bias), the state h / c as carried, sigmoid / tanh / softmax, the accumulators.
The model is not bit-faithful (f32 accumulation, the order of BN folding and the per-lane form's f32 activations in the
core are not modelled); the tolerance rule of tests/impala_cases.py absorbs that.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import impala as oi
from oracle import rng as crng
from oracle.noise import perturb

BN_EPS = 1e-5
F32_MIN = float(torch.finfo(torch.float32).min)
HID = oi.HID
GATE_SAT = 6.0      # a gate pre-activation beyond +-6 counts as saturated: sigmoid / tanh within 2.5e-3 of their limits
F16_WEIGHTS = tuple(n for n, s in oi.layout(1) if len(s) > 1 and not n.startswith("head."))
CORE_WEIGHTS = ("fc.w", "lstm.w_ih", "lstm.w_hh")


def f16(x):
    """round a double tensor to the nearest f16 (values beyond f16's range would become inf: none occur)"""
    return x.to(torch.float16).to(torch.float64)


def _ident(x):
    return x


def layout(n_act):
    return oi.layout(n_act)


def unflatten(flat, n_act):
    """f32 parameter vector -> {name: double tensor} in the reference's parameters() order."""
    flat = torch.as_tensor(np.asarray(flat, np.float32)).double()
    out, off = {}, 0
    for name, shape in oi.layout(n_act):
        n = int(np.prod(shape))
        out[name] = flat[off:off + n].view(shape)
        off += n
    assert off == flat.numel(), (off, flat.numel())
    return out


def staged_params(theta_p, n_act, staged=None, theta=None, noise=None, sign=0):
    """theta_p: the lane's f32 theta'.  staged None: plain double.  "lane": rounding point 1.  "pair": rounding point 2
    (theta: the shared f32 base, noise: fl32(sigma * eps) f32, sign: the lane's)."""
    p = unflatten(theta_p, n_act)
    if staged is None:
        return p
    p = dict(p)
    for name in F16_WEIGHTS:
        p[name] = f16(p[name])
    if staged == "pair":
        base, eps = unflatten(theta, n_act), unflatten(noise, n_act)
        for name in CORE_WEIGHTS:
            p[name] = f16(base[name]) + float(sign) * f16(eps[name])
    else:
        assert staged == "lane", staged
    return p


def split_bn(rm, rv):
    out, off = {}, 0
    rm = torch.as_tensor(np.asarray(rm, np.float32)).double()
    rv = torch.as_tensor(np.asarray(rv, np.float32)).double()
    for name, n in oi.bn_layout():
        out[name] = (rm[off:off + n], rv[off:off + n])
        off += n
    return out


def _bn(x, p, bn, name):
    rm, rv = bn[name]
    shape = (1, -1) + (1,) * (x.dim() - 2)
    y = (x - rm.view(shape)) / torch.sqrt(rv.view(shape) + BN_EPS)
    return y * p[name + ".w"].view(shape) + p[name + ".b"].view(shape)


def _frames64(frames):
    return torch.as_tensor(np.asarray(frames, np.float64)).reshape(-1, oi.FRAME_C, oi.FRAME_H, oi.FRAME_W)


@torch.no_grad()
def features(p, bn, frames, staged=None):
    """frames (N, 3, 64, 64) 0..255 -> relu'd (N, 2048) double.  staged: rounding point 3."""
    r = _ident if staged is None else f16
    x = _frames64(frames) / 255.0
    for i in range(len(oi.STAGES)):
        x = r(_bn(x, p, bn, "feat%d.bn" % i))
        x = F.conv2d(x, p["feat%d.conv.w" % i], p["feat%d.conv.b" % i], padding=1)
        x = r(F.max_pool2d(x, kernel_size=3, stride=2, padding=1))
        for k in (1, 2):
            pre = "res%d_%d" % (k, i)
            y = r(F.relu(_bn(x, p, bn, pre + ".bn0")))
            y = r(F.conv2d(y, p[pre + ".conv0.w"], p[pre + ".conv0.b"], padding=1))
            y = r(F.relu(_bn(y, p, bn, pre + ".bn1")))
            y = F.conv2d(y, p[pre + ".conv1.w"], p[pre + ".conv1.b"], padding=1)
            x = r(y + x)
    return F.relu(x).reshape(x.shape[0], -1)


@torch.no_grad()
def core_input(p, bn, feat, reward, staged=None):
    """fc + ReLU + clipped reward -> (N, 257) double.  staged: the fc's B operand is f16 (rounding point 4)."""
    r = _ident if staged is None else f16
    x = F.relu(F.linear(r(_bn(torch.as_tensor(feat, dtype=torch.float64), p, bn, "fc.bn")), p["fc.w"], p["fc.b"]))
    rw = torch.clamp(torch.as_tensor(np.asarray(reward, np.float64)), -1, 1).view(-1, 1)
    return torch.cat([x, rw], dim=-1)


@torch.no_grad()
def lstm_head(p, bn, core_in, h, c, notdone=None, staged=None):
    """-> probs, h, c, gates (pre-activations, N x 1024) double.  staged: both gate B operands f16 (point 4)."""
    r = _ident if staged is None else f16
    core_in = torch.as_tensor(core_in, dtype=torch.float64)
    h = torch.as_tensor(h, dtype=torch.float64)
    c = torch.as_tensor(c, dtype=torch.float64)
    if notdone is not None:
        nd = torch.as_tensor(np.asarray(notdone, np.float64)).view(-1, 1)
        h, c = nd * h, nd * c
    gates = F.linear(r(core_in), p["lstm.w_ih"], p["lstm.b_ih"]) + F.linear(r(h), p["lstm.w_hh"], p["lstm.b_hh"])
    i, f, g, o = gates.chunk(4, dim=-1)
    c2 = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
    h2 = torch.sigmoid(o) * torch.tanh(c2)
    logits = F.linear(_bn(h2, p, bn, "head.bn"), p["head.w"], p["head.b"])
    return torch.softmax(logits, dim=-1), h2, c2, gates


def forward(p, bn, frames, reward, h, c, notdone=None, staged=None):
    """-> probs, h, c, feat, core_in, gates"""
    feat = features(p, bn, frames, staged)
    ci = core_input(p, bn, feat, reward, staged)
    probs, h2, c2, gates = lstm_head(p, bn, ci, h, c, notdone, staged)
    return probs, h2, c2, feat, ci, gates


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
    a = np.minimum((cs[:, :-1] <= target[:, None]).sum(-1), A - 1)
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


def lane_params(theta, table, idx, sign, sigma, n_act, staged=None):
    """[params of lane l] with theta' formed in f32 as the device forms it (and the staged weights of `staged`)."""
    theta = np.asarray(theta, np.float32)
    thetas = perturb(theta, table, idx, sign, sigma)
    P = theta.size
    out = []
    for l, (i, sg) in enumerate(zip(idx, sign)):
        noise = None
        if staged == "pair":
            noise = (table[int(i):int(i) + P] * np.float32(sigma)).astype(np.float32) if sg != 0 else np.zeros(P, np.float32)
        out.append(staged_params(thetas[l], n_act, staged, theta, noise, int(sg)))
    return out


def evaluate_lanes(theta, table, idx, sign, sigma, n_act, envs_per_lane, T, seed, env_seed, rm, rv,
                   deterministic=False, jiggle=True, lane_offset=0, actions=None, staged=None, entropy_pass=True,
                   feats=None):
    """fdr_impala_rollout in double: lane l (theta'_l) drives global envs (lane_offset + l) * E + e for T steps from the
    reset state.  actions [L, E, T] given: follow them (follow_lanes) instead of deciding.  feats [L, E, T, 2048]: the
    conv features of an earlier call with the same conv weights (the frames do not depend on the actions, and the
    "lane" and "pair" stagings share their conv weights), returned as "feat".
    -> dict(ret [L, E], ent [L, E] (replayed), steps, norm2 [L], actions [L, E, T], own_actions [L, E, T] (the
    decisions of the reference's own probabilities, whatever was followed), probs [L, E, T, A],
    margin [L, E, T], step_ent [L, E, T] (of the visited states), replay_ent [L, E, T], gate_max [L, E, T], gate_sat
    [L, E, T] (the share of the step's 1024 gate pre-activations beyond +-GATE_SAT),
    h, c [L, E, 256] (end of episode), feat [L, E, T, 2048])."""
    L, E = len(idx), int(envs_per_lane)
    P = np.asarray(theta).size
    params = lane_params(theta, table, idx, sign, sigma, n_act, staged)
    bn = split_bn(rm, rv)
    det = np.broadcast_to(np.asarray(deterministic, dtype=bool), (L,))
    ret = np.zeros((L, E), np.float64)
    ent = np.zeros((L, E), np.float64)
    acts = np.zeros((L, E, T), np.int32)
    own = np.zeros((L, E, T), np.int32)
    probs = np.zeros((L, E, T, n_act), np.float64)
    margin = np.zeros((L, E, T), np.float64)
    step_ent = np.zeros((L, E, T), np.float64)
    replay_ent = np.zeros((L, E, T), np.float64)
    gate_max = np.zeros((L, E, T), np.float64)
    gate_sat = np.zeros((L, E, T), np.float64)
    hs, cs = np.zeros((L, E, HID)), np.zeros((L, E, HID))
    feat_out = np.zeros((L, E, T, oi.FEAT), np.float64)
    for l in range(L):
        p = params[l]
        envs = np.uint64(lane_offset + l) * np.uint64(E) + np.arange(E, dtype=np.uint64)
        h = torch.zeros(E, HID, dtype=torch.float64)
        c = torch.zeros(E, HID, dtype=torch.float64)
        r_prev = np.zeros(E, np.float64)
        cis = []
        for t in range(T):
            ft = (features(p, bn, oi.frames(env_seed, envs, t), staged) if feats is None
                  else torch.as_tensor(feats[l, :, t], dtype=torch.float64))
            feat_out[l, :, t] = ft.numpy()
            ci = core_input(p, bn, ft, r_prev, staged)
            pr, h, c, gates = lstm_head(p, bn, ci, h, c, staged=staged)
            cis.append(ci)
            pn = pr.numpy()
            probs[l, :, t] = pn
            a, m = decide(pn, None if det[l] else crng.uniform(seed, envs, t, 0))
            own[l, :, t] = a
            if actions is not None:
                a = np.asarray(actions).reshape(L, E, T)[l, :, t]
            acts[l, :, t] = a
            margin[l, :, t] = m
            step_ent[l, :, t] = entropy(pr).numpy()
            gate_max[l, :, t] = gates.abs().max(-1).values.numpy()
            gate_sat[l, :, t] = (gates.abs() > GATE_SAT).double().mean(-1).numpy()
            rw = oi.rewards(env_seed, envs, t, a, n_act)
            ret[l] += rw
            r_prev = rw.astype(np.float64)
        hs[l], cs[l] = h.numpy(), c.numpy()
        if entropy_pass:
            eh, ec = h, c
            for t in range(T):
                pe, eh, ec, _ = lstm_head(p, bn, cis[t], eh, ec, staged=staged)
                replay_ent[l, :, t] = entropy(pe).numpy()
            ent[l] = replay_ent[l].sum(-1) / T
        if jiggle:
            ret[l] += crng.jiggle(seed, envs)
    return dict(ret=ret, ent=ent, steps=np.full((L, E), T, np.int32), norm2=norm2(table, idx, sign, sigma, P),
                actions=acts, own_actions=own, probs=probs, margin=margin, step_ent=step_ent, replay_ent=replay_ent, gate_max=gate_max, gate_sat=gate_sat,
                h=hs, c=cs, feat=feat_out)


def follow_lanes(theta, table, idx, sign, sigma, n_act, envs_per_lane, T, seed, env_seed, rm, rv, actions, **kw):
    """evaluate_lanes along GIVEN trajectories (a kernel's own actions): identical frames and rewards on both sides."""
    return evaluate_lanes(theta, table, idx, sign, sigma, n_act, envs_per_lane, T, seed, env_seed, rm, rv,
                          actions=actions, **kw)


def strategy(p, bn, frames, rewards=None, h=None, c=None, first_done=False, staged=None, feat=None):
    """ImpalaPolicy.get_strategy: the n stacked obs as ONE LSTM sequence from (h, c) (None: the reset state).
    feat: the conv features of an earlier call.  -> probs (n, A), h (256), c (256), feat (n, 2048) double numpy."""
    n = np.asarray(frames).reshape(-1, oi.FRAME_C * oi.FRAME_H * oi.FRAME_W).shape[0]
    feat = features(p, bn, frames, staged) if feat is None else torch.as_tensor(feat, dtype=torch.float64)
    ci = core_input(p, bn, feat, np.zeros(n) if rewards is None else rewards, staged)
    h = torch.zeros(1, HID, dtype=torch.float64) if h is None else torch.as_tensor(np.asarray(h, np.float64)).view(1, HID)
    c = torch.zeros(1, HID, dtype=torch.float64) if c is None else torch.as_tensor(np.asarray(c, np.float64)).view(1, HID)
    if first_done:
        h, c = h * 0, c * 0
    out = []
    for t in range(n):
        pr, h, c, _ = lstm_head(p, bn, ci[t:t + 1], h, c, staged=staged)
        out.append(pr)
    probs = torch.cat(out).numpy() if out else np.zeros((0, p["head.b"].numel()))
    return probs, h.view(-1).numpy(), c.view(-1).numpy(), feat.numpy()


def lane_strategies(theta, table, idx, sign, sigma, n_act, frames, rewards, rm, rv, h=None, c=None, staged=None,
                    feats=None):
    """strategies of every lane's theta' from its row of h / c [L, 256] (None: reset)
    -> probs [L, Z, A], h, c [L, 256], feats [L, Z, 2048] (reusable: "lane" and "pair" share their conv weights)"""
    bn = split_bn(rm, rv)
    res = [strategy(p, bn, frames, rewards, None if h is None else h[l], None if c is None else c[l], staged=staged,
                    feat=None if feats is None else feats[l])
           for l, p in enumerate(lane_params(theta, table, idx, sign, sigma, n_act, staged))]
    return tuple(np.stack([r[k] for r in res]) for k in range(4))


@torch.no_grad()
def compute_vbn(p, rm, rv, frames, rewards=None, first_done=False, h=None, c=None, momentum=0.1):
    """ImpalaPolicy.compute_vbn in double: one train-mode pass of the n-obs buffer.  Each BN normalises with its batch
    mean and biased variance and folds the batch mean and the UNBIASED variance into its running stats; the LSTM reads
    the n obs as one sequence from (h, c), zeroed first iff first_done.  -> (rm', rv', h', c') f64 numpy."""
    rm = np.asarray(rm, np.float32).astype(np.float64)
    rv = np.asarray(rv, np.float32).astype(np.float64)
    m = float(momentum)
    offs, o = {}, 0
    for name, n in oi.bn_layout():
        offs[name] = (o, o + n)
        o += n

    def tbn(x, name):
        lo, hi = offs[name]
        dims = [d for d in range(x.dim()) if d != 1]
        n = x.numel() // x.shape[1]
        mean = x.mean(dims, keepdim=True)
        var_sum = ((x - mean) ** 2).sum(dims, keepdim=True)
        rm[lo:hi] = m * mean.reshape(-1).numpy() + (1.0 - m) * rm[lo:hi]
        rv[lo:hi] = m * (var_sum.reshape(-1).numpy() / (n - 1)) + (1.0 - m) * rv[lo:hi]
        shape = (1, -1) + (1,) * (x.dim() - 2)
        y = (x - mean) / torch.sqrt(var_sum / n + BN_EPS)
        return y * p[name + ".w"].view(shape) + p[name + ".b"].view(shape)

    x = _frames64(frames) / 255.0
    nobs = x.shape[0]
    for i in range(len(oi.STAGES)):
        x = tbn(x, "feat%d.bn" % i)
        x = F.conv2d(x, p["feat%d.conv.w" % i], p["feat%d.conv.b" % i], padding=1)
        x = F.max_pool2d(x, kernel_size=3, stride=2, padding=1)
        for k in (1, 2):
            pre = "res%d_%d" % (k, i)
            y = F.relu(tbn(x, pre + ".bn0"))
            y = F.conv2d(y, p[pre + ".conv0.w"], p[pre + ".conv0.b"], padding=1)
            y = F.relu(tbn(y, pre + ".bn1"))
            y = F.conv2d(y, p[pre + ".conv1.w"], p[pre + ".conv1.b"], padding=1)
            x = y + x
    x = F.relu(x).reshape(nobs, -1)
    x = F.relu(F.linear(tbn(x, "fc.bn"), p["fc.w"], p["fc.b"]))
    rw = np.zeros(nobs) if rewards is None else np.asarray(rewards, np.float64)
    ci = torch.cat([x, torch.clamp(torch.as_tensor(rw), -1, 1).view(-1, 1)], dim=-1)
    h = torch.zeros(1, HID, dtype=torch.float64) if h is None else torch.as_tensor(np.asarray(h, np.float64)).view(1, HID)
    c = torch.zeros(1, HID, dtype=torch.float64) if c is None else torch.as_tensor(np.asarray(c, np.float64)).view(1, HID)
    if first_done:
        h, c = h * 0, c * 0
    hs = []
    for t in range(nobs):
        gates = F.linear(ci[t:t + 1], p["lstm.w_ih"], p["lstm.b_ih"]) + F.linear(h, p["lstm.w_hh"], p["lstm.b_hh"])
        i_, f_, g_, o_ = gates.chunk(4, dim=-1)
        c = torch.sigmoid(f_) * c + torch.sigmoid(i_) * torch.tanh(g_)
        h = torch.sigmoid(o_) * torch.tanh(c)
        hs.append(h)
    tbn(torch.cat(hs), "head.bn")   # the head's logits feed no statistic
    return rm, rv, h.view(-1).numpy(), c.view(-1).numpy()
