"""The inputs of the learner edge-shape tests, shared by tests/test_gpu_learner_edges.py (which runs them on the
kernels) and tests/test_learner_ref.py (which pins the conditions they must meet on the CPU: reordering floor,
unambiguous DSGD norm).  TEST INFRASTRUCTURE ONLY.

The tiling formulas of the two gradient kernels are restated here (grad_plan / fused_plan) so that every case can
assert the path it is meant to reach; a retune of either plan then fails those assertions instead of moving a case
off its edge unnoticed.
"""
import functools

import numpy as np

import learner_ref as ref

SIGMA = 0.02
PR = 0.75          # policy reward: near the returns' mean, so the moments form's A - m B stays well-conditioned
GUARD = 64         # NaN elements on either side of the device table
ROOM = 4096        # default max_idx: table_size = P + ROOM


# ---- the kernels' tilings --------------------------------------------------------------------------------------
def _cdiv(a, b):
    return (a + b - 1) // b


def grad_plan(n_dirs, P):
    """fdr_learner.hip grad_plan -> (col_blocks, rows_per_chunk, n_chunks)."""
    cb = _cdiv(P, 256)
    target = max(1, 1024 // max(1, cb))
    rpc = max(64, _cdiv(n_dirs, target))
    return cb, rpc, _cdiv(n_dirs, rpc)


def fused_plan(n_dirs, P):
    """fdr_learner_fused.hip fused_plan -> (col_blocks, rows_per_chunk, n_chunks)."""
    cb = _cdiv(P, 256)
    target = max(1, 1024 // max(1, cb))
    rows = max(64, _cdiv(n_dirs, target))
    rpc = min(1024, _cdiv(rows, 64) * 64)
    return cb, rpc, max(1, _cdiv(n_dirs, rpc))


#   (n_dirs, P)     -> fused (col_blocks, rows_per_chunk, n_chunks)      what the case is for
PLAN_TABLE = {
    (63, 1000): (4, 64, 1),        # one chunk, one row short of full
    (64, 1000): (4, 64, 1),        # one full chunk
    (65, 1000): (4, 64, 2),        # chunk seam: 64 + 1
    (67, 1000): (4, 64, 2),        # 64 + 3: the 4-row unroll tail of the staged kernel
    (130, 1000): (4, 64, 3),       # 64 + 64 + 2
    (130, 257): (2, 64, 3),        # one live column in the last block
    (4097, 300): (2, 64, 65),      # n_all 4097 (lpd 1): the statistics tail
    (2304, 1500): (6, 64, 36),     # n_all 4608 (lpd 2): the statistics tail
    (1600, 40000): (157, 320, 5),  # rows_per_chunk > 256: further directions per thread
    (1100, 131100): (513, 1024, 2),  # rows_per_chunk = kFusedMaxRows, chunks of 1024 + 76, 28 live columns at the end
}

GRID_DIRS = (1, 2, 3, 5, 63, 64, 65, 67, 130)
GRID_P = (1, 2, 255, 256, 257, 1000)
STAGED_LPD = (1, 2, 3, 5)
FUSED_LPD = (1, 3, 4, 5, 7)
# (n_dirs, lanes_per_dir, lane_lo, n_all): n_all in {1, 2, 1025, 4097}, the local window anywhere inside
N_ALL_CASES = ((1, 1, 0, 1), (1, 1, 1, 2), (3, 2, 1000, 1025), (5, 3, 4000, 4097))
BIG = ((4097, 300, 1), (2304, 1500, 2), (1600, 40000, 2), (1100, 131100, 1))   # (n_dirs, P, lanes_per_dir)
MODES = ("zscore", "centred_rank", "moments")

# Coefficient conditioning admitted (learner_ref.coef_condition): at (lanes_per_dir + 3) 2^-53 kappa <= 10 * 1.1e-16
# * 64 = 7e-14 the coefficients' own rounding stays inside the 2.5e-13 that test_learner_ref.py allows the inputs.
KAPPA_MAX = 64.0

DSGD_P = (1, 2, 255, 256, 257, 1023, 1024, 1025, 65535, 65536, 65537, 70001, 131100)
DSGD_LR, DSGD_SCALE = 0.01, 0.23


class Case(object):
    """One learner batch: table (f32 [size]), idx_dirs, per-lane idx / sign / n2, rewards over all lanes."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def n_local(self):
        return self.n_dirs * self.lpd

    @property
    def r_local(self):
        return self.r_all[self.lane_lo:self.lane_lo + self.n_local]

    def kappa(self):
        """The worst coefficient conditioning over the three weightings."""
        return max(ref.coef_condition(self.r_all, PR, m, self.lane_lo, self.sign, self.n2, self.lpd, SIGMA)
                   for m in ("zscore", "centred_rank", "raw"))

    def coefs(self, mode):
        """Reference per-direction coefficients (longdouble): one vector, or (A's, B's) for "moments"."""
        if mode == "moments":
            return ref.moment_coefs(self.r_local, PR, self.sign, self.n2, self.lpd, SIGMA)
        w = ref.weights(self.r_all, PR, mode)[self.lane_lo:self.lane_lo + self.n_local]
        return ref.coef_d(w, self.sign, self.n2, self.lpd, SIGMA)


@functools.lru_cache(maxsize=None)
def make_case(n_dirs, P, lpd, lane_lo=0, n_all=None, returns="normal", room=ROOM, signs="mixed"):
    """Offsets always include max_idx and (n_dirs > 1) 0; room = 0 makes the table exactly P long.  signs "mixed":
    drawn from {-1, 0, +1}, with n2 = 0 on the sign-0 lanes, a sign-0 lane in position 0 of direction 0 (lpd > 1) and
    at least one used lane; "zero": all 0 (g == 0).  returns: "normal" N(1, 3) | "equal" (all 2.5: r' = 1.75 and
    every partial sum of it is exact, so std == 0 exactly in any summation order).

    A draw whose coefficients are mostly cancellation between a direction's lanes (learner_ref.coef_condition above
    KAPPA_MAX in any weighting: with one direction and five lanes, centred ranks -6 + 5 + 1 do sum to zero) is
    replaced by the next draw: such a gradient is rounding residue in any arithmetic, the reference's included."""
    for salt in range(64):
        c = _draw_case(n_dirs, P, lpd, lane_lo, n_all, returns, room, signs, salt)
        if signs == "zero" or c.kappa() <= KAPPA_MAX:
            return c
    raise AssertionError("no well-conditioned draw for %r" % ((n_dirs, P, lpd, lane_lo, n_all, returns, room),))


def _draw_case(n_dirs, P, lpd, lane_lo, n_all, returns, room, signs, salt):
    rs = np.random.RandomState((1000003 * n_dirs + 101 * lpd + P + 7919 * salt) % (1 << 32))
    size = P + room
    table = rs.randn(size).astype(np.float32)
    idx_dirs = rs.randint(0, room + 1, size=n_dirs).astype(np.int64)
    idx_dirs[-1] = room
    if n_dirs > 1:
        idx_dirs[0] = 0
    n_local = n_dirs * lpd
    if signs == "zero":
        sign = np.zeros(n_local, np.int8)
    else:
        sign = rs.choice(np.array([-1, 0, 1], np.int8), n_local)
        if lpd > 1:
            sign[0] = 0
        if sign[lpd - 1] == 0:
            sign[lpd - 1] = 1
    n_all = n_local + lane_lo if n_all is None else n_all
    if returns == "normal":
        r_all = rs.randn(n_all) * 3 + 1
    else:
        assert returns == "equal", returns
        r_all = np.full(n_all, 2.5)
    n2 = np.where(sign != 0, np.repeat(ref.norms(table, P, idx_dirs, SIGMA), lpd), 0.0)
    return Case(n_dirs=n_dirs, P=P, lpd=lpd, lane_lo=lane_lo, n_all=n_all, table=table, idx_dirs=idx_dirs,
                idx=np.repeat(idx_dirs, lpd), sign=sign, n2=n2, r_all=r_all, max_idx=room)


def grid_cases(lpds):
    """The small grid: every (n_dirs, P, lanes_per_dir), lane_lo = 5 on the odd direction counts (3 lanes of other
    ranks behind the window), plus the n_all cases, all-equal returns, and a table exactly P long."""
    out = []
    for lpd in lpds:
        for n_dirs in GRID_DIRS:
            for P in GRID_P:
                lo = 5 if n_dirs % 2 else 0
                out.append(make_case(n_dirs, P, lpd, lane_lo=lo, n_all=n_dirs * lpd + lo + (3 if lo else 0)))
    for n_dirs, lpd, lo, n_all in N_ALL_CASES:
        out.append(make_case(n_dirs, 257, lpd, lane_lo=lo, n_all=n_all))
    for lpd in lpds:
        out.append(make_case(67, 257, lpd, returns="equal"))
        # table_size == P: 0 is the only legal offset.  One direction: several would all be the same row, and
        # their weights can sum to zero, which no summation order resolves
        out.append(make_case(1, 257, lpd, lane_lo=2, n_all=lpd + 5, room=0))
    out.append(make_case(1, 1, 1, returns="equal"))
    return out


def big_cols(P):
    """The columns on which a large-P case meets the reference: the first 512, the last 512 and 1024 random ones."""
    rs = np.random.RandomState(P)
    return np.unique(np.concatenate([np.arange(512), np.arange(P - 512, P), rs.randint(0, P, 1024)]))


@functools.lru_cache(maxsize=None)
def dsgd_inputs(P):
    rs = np.random.RandomState(P)
    theta = rs.randn(P).astype(np.float32) * np.float32(0.1)
    return theta, rs.randn(P)


@functools.lru_cache(maxsize=None)
def dsgd_moments_inputs(P):
    """Summed moments [A | B | n | slots] with a gradient of the same scale as dsgd_inputs'."""
    rs = np.random.RandomState(P + 7)
    theta = rs.randn(P).astype(np.float32) * np.float32(0.1)
    n = 37
    mom = np.concatenate([rs.randn(P), rs.randn(P) * 0.1, [float(n)], rs.randn(n) * 3 + 1])
    return theta, mom


def rank_returns(n_all, kind):
    rs = np.random.RandomState(n_all)
    if kind == "equal":
        return np.full(n_all, 1.25)
    return np.clip(np.round(rs.randn(n_all) * 1.2), -2, 2)      # five distinct values: ties everywhere


def lambda_case(n, P, n_slots=3):
    rs = np.random.RandomState(7919 * n + P)
    table = rs.randn(P + ROOM).astype(np.float32)
    idx = rs.randint(0, ROOM + 1, size=n).astype(np.int64)
    idx[-1] = ROOM
    if n > 1:
        idx[0] = 0
    sign = np.where(np.arange(n) % 3 == 1, -1, 1).astype(np.int8)
    slot = (np.arange(n) % (n_slots + 1) - 1).astype(np.int32)   # -1, 0, .., n_slots - 1 in turn
    drift = (rs.randn(n_slots, P) * 0.01).astype(np.float32)
    return table, idx, sign, slot, drift, rs.randn(n)
