"""np.longdouble restatement of the top-b direction weighting (include/fdr.h, FDR_WEIGHT_TOP_DIRS): scores, stable
selection, statistics over the kept lanes, weights.  TEST INFRASTRUCTURE ONLY: nothing is shared with the product; the
rest of the step (coefficients, gradient, DSGD) is learner_ref's.

    scores(r_all, lpd)            s_d = max of direction d's lpd returns, -inf when one of them is NaN
    selected(r_all, lpd, b)       rank_d = #{e : s_e > s_d, or s_e == s_d and e < d};  kept when rank_d < b
    weights(r_all, pr, lpd, b)    (x - m) / sd over the kept lanes (x when sd == 0), 0.0 elsewhere; x = r - pr in f64,
                                  m / sd the two-pass population statistics of the kept x in longdouble
    coef_condition(...)           learner_ref.coef_condition's argument with the kept set's m and sd
"""
import numpy as np

import learner_ref as ref

LD = np.longdouble


def scores(r_all, lpd):
    r = np.asarray(r_all, np.float64).reshape(-1, lpd)
    out = np.full(r.shape[0], -np.inf)
    for d in range(r.shape[0]):
        if not np.isnan(r[d]).any():
            out[d] = r[d].max()
    return out


def selected(r_all, lpd, b):
    """bool [D]: the b directions first in the stable descending order of the scores (ties to the lower index)."""
    s = scores(r_all, lpd)
    order = np.argsort(-s, kind="stable")      # -s ascending = s descending; equal scores (-0.0 == 0.0) keep index order
    keep = np.zeros(s.size, bool)
    keep[order[:b]] = True
    return keep


def _stats(x, lane_keep):
    xs = x[lane_keep]
    n = LD(xs.size)
    mean = xs.sum() / n
    sd = np.sqrt(((xs - mean) ** 2).sum() / n)
    return mean, sd


def weights(r_all, policy_reward, lpd, b):
    """-> (w longdouble [n_all], keep bool [D]).  A kept NaN makes every weight NaN."""
    keep = selected(r_all, lpd, b)
    lane_keep = np.repeat(keep, lpd)
    x = (np.asarray(r_all, np.float64) - float(policy_reward)).astype(LD)
    mean, sd = _stats(x, lane_keep)
    if np.isnan(sd):
        return np.full(x.size, LD("nan")), keep
    w = np.zeros(x.size, LD)
    w[lane_keep] = x[lane_keep] if sd == 0 else (x[lane_keep] - mean) / sd
    return w, keep


def coef_condition(r_all, policy_reward, lpd, b, lane_lo, sign, n2, sigma):
    """kappa = ||m|| / ||coef|| over the local directions (learner_ref.coef_condition): per kept lane an f64 evaluation
    handles the magnitudes (|x| + |mean|) / sd, mean and sd the kept set's; a lane that is not kept handles nothing."""
    n_local = len(sign)
    w, keep = weights(r_all, policy_reward, lpd, b)
    lane_keep = np.repeat(keep, lpd)
    x = (np.asarray(r_all, np.float64) - float(policy_reward)).astype(LD)
    mean, sd = _stats(x, lane_keep)
    mag = np.where(lane_keep, np.abs(x) if sd == 0 else (np.abs(x) + abs(mean)) / sd, LD(0))
    sl = slice(lane_lo, lane_lo + n_local)
    if not np.any(w[sl] != 0):
        return 1.0
    c = ref.coef_d(w[sl], sign, n2, lpd, sigma)
    m = ref.coef_d(mag[sl], np.abs(np.asarray(sign, np.int64)), n2, lpd, sigma)
    nc = np.sqrt((c * c).sum())
    return float("inf") if nc == 0 else float(np.sqrt((m * m).sum()) / nc)
