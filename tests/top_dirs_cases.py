"""The inputs of the top-b direction tests, shared by tests/test_gpu_top_dirs.py (which runs them on the kernels) and
tests/test_top_dirs_ref.py (which pins, on the CPU, that every one of them can be built and meets the project's
conditioning cap learner_cases.KAPPA_MAX).  TEST INFRASTRUCTURE ONLY.
"""
import functools

import numpy as np

import learner_cases as lc
import learner_ref as ref
import top_dirs_ref as tref
from learner_cases import PR, SIGMA

# ---- selection (fdr_top_dir_weights) -----------------------------------------------------------------------------
SEL_D = (1, 2, 3, 255, 256, 257, 2047, 2048, 2049, 4097)    # the 256-thread and 2048-score tile edges
SEL_LPD = (1, 2, 3)
SEL_RETURNS = ("normal", "five_values", "equal", "max_last", "nan", "signed_zero")


def sel_bs(D):
    """b in {1, 2, ceil(D / 2), D - 1, D} inside 1..D.  With the "nan" returns every b < D leaves the one NaN
    direction out (it ranks last) and b = D takes it in."""
    return sorted({b for b in (1, 2, (D + 1) // 2, D - 1, D) if 1 <= b <= D})


def sel_shards(D, lpd):
    """(lane_lo, n_local): the whole range; a middle slice whose lane_lo is no multiple of 256; the last slice."""
    out = [(0, D * lpd)]
    if D >= 3:
        d0 = D // 3
        if (d0 * lpd) % 256 == 0:
            d0 += 1
        assert (d0 * lpd) % 256 != 0
        out.append((d0 * lpd, max(1, D // 3) * lpd))
        dl = D - max(1, D // 4)
        out.append((dl * lpd, (D - dl) * lpd))
    return out


@functools.lru_cache(maxsize=None)
def sel_returns(D, lpd, kind):
    rs = np.random.RandomState(7 * D + 1000 * lpd + len(kind))
    n = D * lpd
    if kind == "normal":
        return rs.randn(n) * 3 + 1
    if kind == "five_values":       # ties everywhere, across the 2048-score tile boundaries too
        return np.clip(np.round(rs.randn(n) * 1.2), -2, 2)
    if kind == "equal":
        return np.full(n, 2.5)
    if kind == "max_last":          # every direction's maximum sits in its last lane
        r = (rs.randn(n) * 3 + 1).reshape(D, lpd)
        r[:, -1] = r.max(1) + np.abs(rs.randn(D))
        return r.reshape(-1)
    if kind == "nan":               # one NaN lane, not the first of its direction where there is a choice
        r = rs.randn(n) * 3 + 1
        r[(D // 2) * lpd + (lpd - 1)] = np.nan
        return r
    assert kind == "signed_zero", kind
    return rs.choice(np.array([-0.0, 0.0]), n)      # -0.0 == 0.0: one tie over all directions


# ---- gradient (fdr_fd_grad_fused_top) ----------------------------------------------------------------------------
GRAD_DIRS = (1, 3, 65, 130)
GRAD_P = (1, 255, 257, 1000)
GRAD_BIG = (2304, 1500, 2)      # multi-chunk, n_all = 4608: the statistics loops go round more than once
BIT_CASES = ((130, 1000, 2), (2304, 1500, 2))
STEP_CASE = (3, 257, 2)         # fdr_fd_step_top (test_gpu_learner_edges' fd_step case, one P)
STEP_OPT_CASE = (65, 1000, 2)   # fdr_fd_step_top_opt (test_gpu_optim's fused case, one shape)


def grad_b(n_all, lpd):
    return (n_all // lpd + 1) // 2


@functools.lru_cache(maxsize=None)
def grad_case(n_dirs, P, lpd=2, shard=False):
    """A learner_cases draw (sign-0 lanes with n2 = 0, offsets 0 and max_idx) whose top-b coefficients meet the
    conditioning cap: -> (case, b), b = ceil(D / 2) of the D directions of all ranks.  shard: two directions of
    another rank in front of the window and one behind it."""
    lo = 2 * lpd if shard else 0
    n_all = n_dirs * lpd + lo + (lpd if shard else 0)
    b = grad_b(n_all, lpd)
    for salt in range(64):
        c = lc._draw_case(n_dirs, P, lpd, lo, n_all, "normal", lc.ROOM, "mixed", salt)
        if kappa(c, b) <= lc.KAPPA_MAX:
            return c, b
    raise AssertionError("no well-conditioned draw for %r" % ((n_dirs, P, lpd, shard),))


def kappa(c, b):
    return tref.coef_condition(c.r_all, PR, c.lpd, b, c.lane_lo, c.sign, c.n2, SIGMA)


def coefs(c, b):
    """Reference per-direction coefficients of the local window (longdouble)."""
    w, _ = tref.weights(c.r_all, PR, c.lpd, b)
    return ref.coef_d(w[c.lane_lo:c.lane_lo + c.n_local], c.sign, c.n2, c.lpd, SIGMA)


def all_grad_cases():
    out = [grad_case(n, P, 2, shard=(n % 2 == 1)) for n in GRAD_DIRS for P in GRAD_P]
    out.append(grad_case(*GRAD_BIG))
    out.append(grad_case(*STEP_CASE))
    out.append(grad_case(*STEP_OPT_CASE))
    return out
