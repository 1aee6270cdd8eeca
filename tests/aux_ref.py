"""High-precision restatements of the three auxiliary device paths: strategy distances / novelty
(fdr_strategy_distances), the Welford obs statistics (fdr_obs_stats_merge, the rollouts' per-lane update) and the
DiscretePolicy's BatchNorm refresh (fdr_bn_refresh).  TEST INFRASTRUCTURE ONLY, in the style of tests/optim_ref.py:
written from the formulas, pinned by tests/test_aux_ref.py, and nothing here was tuned against a kernel.

Distances (utils/math_helpers.py:147-222).  a [Z, D] one strategy, B [H, Z, D] the archive, d[h] = mean_z term:
    l2   math_helpers.py:166-170   term = || b - a ||_2
    tvd  math_helpers.py:216-219   term = sum_d |a - b|                       (no 1/2 factor)
    w2   math_helpers.py:202-213   term = sum_k (m1 - m2)^2 + s1 + s2 - 2 sqrt(s1 s2),  D = 2k = [mean | std]
dist_ref evaluates them in np.longdouble from the exact f32 entries and returns next to d a magnitude `scale`, the
same formula over magnitudes, so that cancellation inside the formula (W2 with near-equal stds: s1 + s2 against
2 sqrt(s1 s2)) does not count as error of an implementation:
    tvd  mean_z sum_d (|a| + |b|)        l2  d itself        w2  mean_z sum_k (dm^2 + s1 + s2 + 2 sqrt(s1 s2))
A correct f64 evaluation lies within k 2^-53 scale of d; k for the kernel's own summation order (dist_f64) is what
tests/test_aux_ref.py measures on the CPU (K_CPU below), and the kernel is allowed K_DEV = 8 K_CPU: its compiler may
contract a multiply-add and its f64 sqrt need not round as numpy's.

Novelty (compute_strategy_novelty, math_helpers.py:147-155) is np.min over the archive: the first minimum, a NaN
propagates, and np.argmin names the first NaN.

Welford (math_helpers.py:7-124): oracle.obs_stats.Welford is already f32 in the reference's operation order and
pinned by G10; welford_ref only drives it, so nothing here can drift from it.

BN refresh (policies/policy.py:31-34 compute_vbn over policies/discrete.py:34-48): one train-mode pass in float64
from the f32 theta and x.  Each BatchNorm1d normalises with the batch mean and the biased variance (eps 1e-5) and
folds new = momentum stat + (1 - momentum) old into its running stats, stat = the batch mean / the unbiased variance
(torch/nn/modules/batchnorm.py).  Next to each new stat: scale = |momentum stat| + |(1 - momentum) old|.
"""
import numpy as np

from oracle import obs_stats as oo
from oracle import policies as opol

LD = np.longdouble
U53 = 2.0 ** -53
U24 = 2.0 ** -24
KINDS = ("tvd", "l2", "w2")
BN_EPS = 1e-5

# Largest k of dist_f64 (the kernel's summation order in numpy float64) against dist_ref over aux_cases.DIST_CASES,
# all kinds; measured by tests/test_aux_ref.py::test_f64_floor_of_the_kernels_order, which asserts the re-measured value
# stays at or below it, and that it stays <= 4 (inputs well conditioned).  The device bound is 8 x this.
K_CPU = 3.0
K_DEV = 8 * K_CPU

# The f32 floor of the hidden-layer BatchNorms: the largest distance, in 2^-24 scale, of the installed torch's CPU f32
# train-mode pass (one thread: split over threads its f32 sums, and with them this floor, change) from vbn_ref over
# aux_cases.VBN_CASES (both passes, mean and var), per BN; measured and asserted by
# tests/test_aux_ref.py::test_torch_f32_floor_of_the_hidden_bns.  The kernel is allowed 4 x (the margin of
# tests/test_gpu_optim.py).  Two groups, each with its own largest value: "plain" inputs, and inputs with a constant
# or a mean-1e4 column ("cols"): there the f32 difference x - mean of the first BN cancels (1/2 ulp(1e4) = 4.9e-4
# against a std of 1, and torch's one-thread f32 sum of a thousand values near 1e4 is further off; a constant column's
# f32 batch variance is 2e-13, not 0, under eps 1e-5) and that error, not rounding of the hidden layers, is what
# BN1 / BN2 see -- four orders of magnitude more.  One floor over both groups
# would leave the plain cases unchecked.  BN0 is derived instead: one rounding of the f64 stat to f32 and three f32
# operations.
BN0_K = 3.0
BN_F32_FLOOR = {"plain": {1: 4.4, 2: 10.9}, "cols": {1: 111600.0, 2: 32600.0}}
BN_MARGIN = 4.0


def _terms(a, b, kind, mag):
    """term[..., z] of a against b (longdouble), or the magnitude form when mag."""
    if kind == "tvd":
        return (np.abs(a) + np.abs(b)).sum(-1) if mag else np.abs(a - b).sum(-1)
    if kind == "l2":
        return np.sqrt(((b - a) ** 2).sum(-1))
    k = a.shape[-1] // 2
    dm = a[..., :k] - b[..., :k]
    s1, s2 = a[..., k:], b[..., k:]
    cross = 2 * np.sqrt(s1 * s2)
    return (dm * dm + (s1 + s2 + cross if mag else s1 + s2 - cross)).sum(-1)


def dist_ref(a, B, kind):
    """-> (d [H], scale [H]) in np.longdouble from the exact f32 entries."""
    a = np.asarray(a, np.float32).astype(LD)
    B = np.asarray(B, np.float32).astype(LD)
    if kind == "w2" and a.shape[-1] % 2:
        raise ValueError("w2 needs D = 2k")
    with np.errstate(invalid="ignore"):
        d = _terms(a[None], B, kind, False).mean(-1)
        scale = d if kind == "l2" else _terms(a[None], B, kind, True).mean(-1)
    return d, scale


def novelty_ref(d):
    """(min, argmin) of one row of distances by numpy's rules: first minimum; NaN wins, the first NaN is the argmin."""
    d = np.asarray(d)
    return d.min(), int(np.argmin(d))


def dist_f64(a, B, kind):
    """The kernel's own order in numpy float64: thread `lane` of the wave sums the terms of z = lane, lane + 64, ...
    (each term a left-to-right sum over d), the 64 partial sums meet in the xor butterfly 32, 16, .. 1, then / Z."""
    a = np.asarray(a, np.float32).astype(np.float64)
    B = np.asarray(B, np.float32).astype(np.float64)
    H, Z, D = B.shape
    term = np.zeros((H, Z))
    with np.errstate(invalid="ignore"):
        if kind == "tvd":
            for d in range(D):
                term = term + np.abs(a[None, :, d] - B[:, :, d])
        elif kind == "l2":
            for d in range(D):
                df = B[:, :, d] - a[None, :, d]
                term = term + df * df
            term = np.sqrt(term)
        else:
            k = D // 2
            for d in range(k):
                dm = a[None, :, d] - B[:, :, d]
                s1, s2 = a[None, :, k + d], B[:, :, k + d]
                term = term + (dm * dm + (s1 + s2 - 2.0 * np.sqrt(s1 * s2)))
        pad = (-Z) % 64
        term = np.concatenate([term, np.zeros((H, pad))], axis=1).reshape(H, -1, 64)
        acc = np.zeros((H, 64))
        for c in range(term.shape[1]):      # x + 0.0 == x: the padding adds nothing
            acc = acc + term[:, c]
        lane = np.arange(64)
        for m in (32, 16, 8, 4, 2, 1):
            acc = acc + acc[:, lane ^ m]
    return acc[:, 0] / float(Z)


def k_of(got, d, scale):
    """max |got - d| / (2^-53 scale) over the finite entries; where scale == 0 the value must be exact."""
    got, d, scale = np.asarray(got, LD), np.asarray(d, LD), np.asarray(scale, LD)
    zero = scale == 0
    assert np.all(got[zero] == d[zero]), "inexact where the magnitude is 0"
    ok = ~zero & np.isfinite(d)
    if not ok.any():
        return 0.0
    return float((np.abs(got[ok] - d[ok]) / (LD(U53) * scale[ok])).max())


def welford_ref(dim, start, partials):
    """oracle.obs_stats.Welford started at (mean, m2, count) and merged with the partials [(mean, m2, count)] in order."""
    w = oo.Welford(dim)
    w.mean_, w.m2, w.count = np.array(start[0], np.float32), np.array(start[1], np.float32), int(start[2])
    for m, v, c in partials:
        w.merge(m, v, c)
    return w


def welford_lane(states, coins):
    """One lane's Welford over its visited raw states [steps, n_in] where coins [steps] fall (worker/agent.py:37-39)."""
    w = oo.Welford(states.shape[1])
    for s, c in zip(states, coins):
        if c:
            w.update(s)
    return w


def vbn_n_act(P, n_in):
    n_act, r = divmod(P - opol.num_params("discrete", n_in, 0), opol.HIDDEN + 1)
    assert r == 0 and n_act > 0
    return n_act


def vbn_ref(theta, x, rm, rv, momentum):
    """-> [(new_mean, new_var, scale_mean, scale_var)] of BN0, BN1, BN2 (float64); rm / rv: [n_in | 64 | 64]."""
    theta, x = np.asarray(theta, np.float32), np.asarray(x, np.float32)
    n, n_in = x.shape
    assert n >= 2
    w = {k: v.astype(np.float64) for k, v in opol.unflatten("discrete", n_in, vbn_n_act(theta.size, n_in), theta).items()}
    rm, rv, m = np.asarray(rm, np.float32).astype(np.float64), np.asarray(rv, np.float32).astype(np.float64), float(momentum)
    h, off, out = x.astype(np.float64), 0, []
    for i in range(3):
        C = h.shape[1]
        mu = h.mean(0)
        var = ((h - mu) ** 2).mean(0)               # biased: what the batch is normalised with
        unb = var * n / (n - 1)
        om, ov = rm[off:off + C], rv[off:off + C]
        out.append((m * mu + (1 - m) * om, m * unb + (1 - m) * ov,
                    np.abs(m * mu) + np.abs((1 - m) * om), np.abs(m * unb) + np.abs((1 - m) * ov)))
        off += C
        if i < 2:
            y = (h - mu) / np.sqrt(var + BN_EPS) * w["bn%d.w" % i] + w["bn%d.b" % i]
            h = np.maximum(y @ w["l%d.w" % (i + 1)].T + w["l%d.b" % (i + 1)], 0.0)
    return out


def vbn_k(got_m, got_v, ref_layer):
    """A layer's worst distance from vbn_ref in units of 2^-24 scale (mean, var); where the scale is 0: 0 if exact,
    else inf."""
    nm, nv, sm, sv = ref_layer
    ks = []
    for got, new, s in ((got_m, nm, sm), (got_v, nv, sv)):
        got = np.asarray(got, np.float64)
        zero = s == 0
        k = float((np.abs(got - new)[~zero] / (U24 * s[~zero])).max()) if (~zero).any() else 0.0
        ks.append(k if np.all(got[zero] == new[zero]) else float("inf"))
    return tuple(ks)
