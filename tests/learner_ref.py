"""numpy restatement of the learner step in extended precision: the yardstick of the learner kernels' f64 arithmetic.

TEST INFRASTRUCTURE ONLY.  The formulas are the learner's (oracle/learner.py lists where each comes from); nothing
else is shared with it.  The oracle forms f32 rows v_i = lambda_i / ||lambda_i||^2 as the reference program does, so
it resolves 1e-5; here the rows stay what the kernels read -- f32 table entries, exact in any wider format -- and
every sum runs in np.longdouble (64-bit significand on x86: 2^-11 of an f64 ulp per operation), row after row in a
fixed order.  An f64 kernel is then judged at the project's rel-L2 1e-12, and what this file alone cannot resolve is
measured by tests/test_learner_ref.py (the reordering floor).

    norms               n2_i = sum_p fl32(sigma eps_i[p])^2
    weights             z-score (two-pass, population std, input unchanged when std == 0) | centred rank | raw
    coef_d              sum_k w_k sign_k sigma / n2_k over the direction's lanes with sign != 0
    coef_condition      how much of coef_d is cancellation between a direction's lanes (a condition on test inputs)
    grad                g[p] = sum_d coef_d table[idx_d + p]
    moments             [A | B | n | slots], grad_from_moments: g = (A - m B) / sd
    lambda_rows         fl32(+-fl32(sigma eps) + D)
    dsgd_mirror         the DSGD kernels' stated arithmetic, operation for operation
"""
import math

import numpy as np

LD = np.longdouble
F32 = np.float32


def _s64(sigma):
    """sigma as the kernels hold it: a float argument, widened."""
    return float(F32(sigma))


def norms(table, P, idx, sigma):
    """n2_i = sum_p fl32(sigma eps_i[p])^2 for rows eps_i = table[idx_i : idx_i + P], by one prefix sum over the
    table (longdouble), rounded to f64.  These are the kernels' INPUTS (the rollout kernel produces them), so both
    sides of every comparison use the same f64 values."""
    step = (F32(sigma) * np.asarray(table, F32)).astype(F32).astype(LD)
    S = np.concatenate([[LD(0)], np.cumsum(step * step)])
    idx = np.asarray(idx, np.int64)
    return (S[idx + P] - S[idx]).astype(np.float64)


def centred_ranks(x):
    """rank_i / (n - 1) - 0.5 with rank_i the position of x_i in a stable sort (ties by index); n == 1: 0.  f64, the
    kernel's own two operations: exact comparison."""
    x = np.asarray(x, np.float64)
    n = x.size
    if n == 1:
        return np.zeros(1)
    rank = np.empty(n, np.float64)
    rank[np.argsort(x, kind="stable")] = np.arange(n, dtype=np.float64)
    return rank / float(n - 1) - 0.5


def weights(rewards_all, policy_reward, mode):
    """Per-lane weights over ALL lanes (longdouble).  r' = r - policy_reward is formed in f64 as the learner and the
    kernels form it; the statistics over r' are longdouble.  mode: "zscore" | "centred_rank" | "raw"."""
    x = np.asarray(rewards_all, np.float64) - float(policy_reward)
    if mode == "centred_rank":
        return centred_ranks(np.asarray(rewards_all, np.float64)).astype(LD)
    x = x.astype(LD)
    if mode == "raw":
        return x
    assert mode == "zscore", mode
    mean = x.sum() / LD(x.size)
    sd = np.sqrt(((x - mean) ** 2).sum() / LD(x.size))
    return x if sd == 0 else (x - mean) / sd


def coef_d(w_local, sign, n2, lanes_per_dir, sigma):
    """coef_d = sum_k w_k sign_k sigma / n2_k over direction d's lanes with sign != 0 (longdouble [n_dirs])."""
    w = np.asarray(w_local, LD).reshape(-1, lanes_per_dir)
    sg = np.asarray(sign, np.int64).reshape(-1, lanes_per_dir)
    n2 = np.asarray(n2, np.float64).reshape(-1, lanes_per_dir)
    out = np.zeros(w.shape[0], LD)
    s = LD(_s64(sigma))
    for k in range(lanes_per_dir):
        use = sg[:, k] != 0
        out[use] += w[use, k] * sg[use, k].astype(LD) * s / n2[use, k].astype(LD)
    return out


def coef_condition(rewards_all, policy_reward, mode, lane_lo, sign, n2, lanes_per_dir, sigma):
    """kappa = ||m|| / ||coef|| over the directions, m_d the sum of the MAGNITUDES an f64 evaluation of coef_d
    handles: per lane (|r'| + |mean|) / sd (z-score), rank / (n - 1) + 0.5 (centred rank), |r'| + 2 max_k |r'_k|
    (the moments form's A, which the fused kernel shifts by the direction's first lane), times sigma / n2.  An f64
    kernel's coef_d carries an error of a few 2^-53 m_d, so a gradient's rel-L2 error from its coefficients alone is
    about (lanes_per_dir + 3) 2^-53 kappa: a direction whose lanes cancel (kappa large) has no 1e-12 to be held to."""
    n_local = len(sign)
    x = np.abs(weights(rewards_all, policy_reward, "raw"))
    if mode == "zscore":
        w = weights(rewards_all, policy_reward, "zscore")
        xs = weights(rewards_all, policy_reward, "raw")
        mean = xs.sum() / LD(xs.size)
        sd = np.sqrt(((xs - mean) ** 2).sum() / LD(xs.size))
        mag = x if sd == 0 else (x + abs(mean)) / sd
    elif mode == "centred_rank":
        w = weights(rewards_all, policy_reward, "centred_rank")
        mag = np.abs(w + LD(0.5)) + LD(0.5)
    else:
        assert mode == "raw", mode
        w = weights(rewards_all, policy_reward, "raw")
        xl = x[lane_lo:lane_lo + n_local].reshape(-1, lanes_per_dir)
        mag = np.zeros(x.size, LD)
        mag[lane_lo:lane_lo + n_local] = (xl + 2 * xl.max(1, keepdims=True)).reshape(-1)
    sl = slice(lane_lo, lane_lo + n_local)
    if not np.any(w[sl] != 0):
        return 1.0   # weights that are zero by definition (one lane's centred rank): nothing cancels
    c = coef_d(w[sl], sign, n2, lanes_per_dir, sigma)
    m = coef_d(mag[sl], np.abs(np.asarray(sign, np.int64)), n2, lanes_per_dir, sigma)
    nc = np.sqrt((c * c).sum())
    return float("inf") if nc == 0 else float(np.sqrt((m * m).sum()) / nc)


def grad(table, P, idx_dirs, coef, cols=None, dtype=LD, reverse=False):
    """g[p] = sum_d coef_d table[idx_d + p] for p in cols (default: all P columns), rows added one after another in
    direction order (reverse: last direction first), every operation in `dtype`."""
    cols = np.arange(P, dtype=np.int64) if cols is None else np.asarray(cols, np.int64)
    coef = np.asarray(coef).astype(dtype)
    acc = np.zeros(cols.size, dtype)
    order = range(len(idx_dirs) - 1, -1, -1) if reverse else range(len(idx_dirs))
    for d in order:
        acc += coef[d] * table[int(idx_dirs[d]) + cols].astype(dtype)
    return acc


def rel_l2(a, b):
    """||a - b|| / ||b|| in longdouble; b == 0: 0 if a == 0 everywhere, else inf.  NaN in a gives NaN (no <= holds)."""
    a, b = np.asarray(a).astype(LD), np.asarray(b).astype(LD)
    nb = np.sqrt((b * b).sum())
    if nb == 0:
        return 0.0 if np.all(a == 0) else float("inf")
    d = a - b
    return float(np.sqrt((d * d).sum()) / nb)


def moment_coefs(rewards_local, policy_reward, sign, n2, lanes_per_dir, sigma):
    """The two per-direction coefficient vectors of the moments form: A's (raw r' weights) and B's (all ones)."""
    x = weights(rewards_local, policy_reward, "raw")
    return (coef_d(x, sign, n2, lanes_per_dir, sigma),
            coef_d(np.ones(x.size, LD), sign, n2, lanes_per_dir, sigma))


def moments(table, P, idx_dirs, rewards_local, policy_reward, sign, n2, lanes_per_dir, sigma, lane_lo, n_all,
            cols=None):
    """One rank's [A | B | n_local | r' slots [n_all]] (longdouble; A and B on `cols` when given): A = sum r'_i v_i,
    B = sum v_i with v_i = sign_i sigma eps_i / n2_i; this rank's r' at its global lanes, 0 elsewhere."""
    cA, cB = moment_coefs(rewards_local, policy_reward, sign, n2, lanes_per_dir, sigma)
    x = weights(rewards_local, policy_reward, "raw")
    slots = np.zeros(n_all, LD)
    slots[lane_lo:lane_lo + x.size] = x
    return np.concatenate([grad(table, P, idx_dirs, cA, cols), grad(table, P, idx_dirs, cB, cols), [LD(x.size)],
                           slots])


def grad_from_moments(mom, P):
    """g = (A - m B) / sd from summed moments; m, sd the two-pass population statistics of the first n slots;
    sd == 0: A unchanged."""
    mom = np.asarray(mom).astype(LD)
    A, B = mom[:P], mom[P:2 * P]
    n = int(mom[2 * P])
    r = mom[2 * P + 1:2 * P + 1 + n]
    m = r.sum() / LD(n)
    sd = np.sqrt(((r - m) ** 2).sum() / LD(n))
    return A if sd == 0 else (A - m * B) / sd


def lambda_rows(table, P, idx, sign, slot, sigma, drift):
    """lambda_i = fl32(+-fl32(sigma eps_i) + D[slot_i]) as f32 [n, P]: sign < 0 negates, a slot outside
    [0, n_slots) adds nothing."""
    out = np.empty((len(idx), P), F32)
    n_slots = 0 if drift is None else len(drift)
    for i, (ix, sg, sl) in enumerate(zip(idx, sign, slot)):
        v = (F32(sigma) * table[int(ix):int(ix) + P]).astype(F32)
        v = -v if sg < 0 else v
        out[i] = (v + drift[sl]).astype(F32) if 0 <= sl < n_slots else v
    return out


def dsgd_mirror(theta, g, lr, lr_scale):
    """The DSGD kernels' arithmetic (fdr_dsgd.hip, dsgd_apply_cb_kernel), each operation in the format they use:

        gr    = fl32(-g)
        norm  = fl32(sqrt(sum gr^2))              the squares are exact in f64; the sum here is math.fsum (exact)
        c32   = fl32(lr * sqrt(P) * lr_scale / norm)        (f64, left to right)
        theta'= fl32(theta - fl32(c32 * gr))      two roundings: the kernels compile this with contraction off
        upd   = sqrt(sum fl32(theta - theta')^2)

    norm == 0 or NaN leaves theta untouched (upd 0).  Returns (theta', upd, norm, ambiguous).  The kernels sum gr^2
    in f64 in an order of their own; any order of P positive terms lands within ss (1 +- P 2^-52), and `ambiguous`
    says whether fl32(sqrt(.)) differs between the two ends of that interval.  When it does not, every correct
    summation order gives this norm, hence these theta bits."""
    theta = np.asarray(theta, F32)
    P = theta.size
    gr = (-np.asarray(g, np.float64)).astype(F32)
    sq = gr.astype(np.float64) ** 2
    if np.isnan(sq).any():
        return theta.copy(), 0.0, float("nan"), False
    ss = math.fsum(sq)
    norm = F32(math.sqrt(ss))
    eps = P * 2.0 ** -52
    ambiguous = bool(F32(math.sqrt(ss * (1.0 - eps))) != F32(math.sqrt(ss * (1.0 + eps))))
    if not norm > 0:
        return theta.copy(), 0.0, float(norm), ambiguous
    c32 = F32(lr * math.sqrt(float(P)) * lr_scale / float(norm))
    new = (theta - (c32 * gr).astype(F32)).astype(F32)
    dd = (theta - new).astype(F32).astype(np.float64)
    return new, math.sqrt(math.fsum(dd * dd)), float(norm), ambiguous
