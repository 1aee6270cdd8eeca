"""Cases and references of the run-batch tests (fdr_rollout_runs, fdr_obs_stats_merge_runs, fdr_fd_step_runs).
TEST INFRASTRUCTURE ONLY: pure numpy, and nothing here restates a formula -- a run's reference is learner_ref /
top_dirs_ref (the learner) or linear_ref (the rollout) applied to that run's slices.

Learner cases.  A batch is R runs of one shape (D directions, lpd lanes each, P parameters) over ONE shared table;
run i is of kind KINDS[(first + i) % len(KINDS)]:
    zscore   top_dirs NULL form: b = D in the reference
    top1     b = 1
    half     b = max(1, D // 2)
    all      b = D
    ties     returns from five values, b = max(1, D // 2): tied scores across the cut
    equal    all returns 2.5: sd == 0 exactly, the weights are x = r - pr unchanged
    nan      one NaN return, every direction kept (b = D): g NaN, theta untouched, out = [0, NaN]
    b0       b = 0: the run is poisoned the same way
    zero     every sign 0: g exactly 0, theta untouched, out = [0, 0]
Each run has its own sigma, learning rate, policy reward and theta.  A draw whose coefficients are mostly cancellation
(top_dirs_ref.coef_condition above learner_cases.KAPPA_MAX) is replaced by the next one, as learner_cases does;
tests/test_runs_host.py holds every case to that bound on the CPU.
"""
import functools

import numpy as np

import learner_cases as lc
import learner_ref as ref
import top_dirs_ref as tref

KINDS = ("zscore", "top1", "half", "all", "ties", "equal", "nan", "b0", "zero")
POISONED = ("nan", "b0")
ROOM = 4096
LR_SCALE = 0.23
EXTRA = 3      # lanes behind a run's training lanes (its eval lanes): never read

# (D, lpd, P, R, first kind): lpd = 1 at the small D only; 130 runs go through every kind 14 times
LEARNER_SHAPES = ((1, 1, 2, 1, 2), (1, 2, 3, 3, 0), (2, 1, 3, 3, 3), (2, 2, 8, 3, 6), (3, 1, 18, 3, 0), (3, 2, 8, 130, 0),
                  (255, 2, 18, 3, 2), (256, 2, 2, 3, 4), (257, 2, 18, 130, 0), (2048, 2, 18, 3, 1), (2048, 2, 8, 1, 4))


class Run(object):
    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def b_ref(self):
        """b of the reference: the NULL form keeps every direction."""
        return self.D if self.b is None else self.b

    def kappa(self):
        return tref.coef_condition(self.r, self.pr, self.lpd, self.b_ref, 0, self.sign, self.n2, self.sigma)

    def grad(self, table):
        """g in longdouble: learner_ref.grad over top_dirs_ref.weights."""
        w, _ = tref.weights(self.r, self.pr, self.lpd, self.b_ref)
        return ref.grad(table, self.P, self.idx_dirs, ref.coef_d(w, self.sign, self.n2, self.lpd, self.sigma))


def _b_of(kind, D):
    return {"zscore": None, "top1": 1, "half": max(1, D // 2), "all": D, "ties": max(1, D // 2),
            "equal": max(1, D // 2), "nan": D, "b0": 0, "zero": max(1, D // 2)}[kind]


def _draw(table, D, lpd, P, kind, i, salt):
    rs = np.random.RandomState((1000003 * D + 101 * lpd + P + 7919 * salt + 31 * i) % (1 << 32))
    idx_dirs = rs.randint(0, ROOM + 1, size=D).astype(np.int64)
    idx_dirs[-1] = ROOM if i % 2 else 0                         # both table edges over the runs
    n = D * lpd
    if kind == "zero":
        sign = np.zeros(n, np.int8)
    else:
        sign = rs.choice(np.array([-1, 0, 1], np.int8), n)
        if lpd > 1:
            sign[0] = 0
        if sign[lpd - 1] == 0:
            sign[lpd - 1] = 1
    if kind in ("ties",):
        r = np.clip(np.round(rs.randn(n) * 1.2), -2, 2)
    elif kind == "equal":
        r = np.full(n, 2.5)
    else:
        r = rs.randn(n) * 3 + 1
    sigma = float(np.float32(0.02 * (1 + (i % 5))))
    n2 = np.where(sign != 0, np.repeat(ref.norms(table, P, idx_dirs, sigma), lpd), 0.0)
    run = Run(D=D, lpd=lpd, P=P, kind=kind, b=_b_of(kind, D), idx_dirs=idx_dirs, idx=np.repeat(idx_dirs, lpd), sign=sign,
              n2=n2, r=r, pr=0.75 + 0.01 * (i % 7), sigma=sigma, lr=0.01 * (1 + (i % 3)),
              theta=(rs.randn(P) * 0.1).astype(np.float32))
    return run


def _run(table, D, lpd, P, kind, i):
    for salt in range(64):
        run = _draw(table, D, lpd, P, kind, i, salt)
        if kind in POISONED + ("zero",):
            if kind == "nan":      # a kept lane (every direction is kept): not the first lane of its direction
                run.r = run.r.copy()
                run.r[(D // 2) * lpd + (lpd - 1)] = np.nan
            return run
        if run.kappa() <= lc.KAPPA_MAX:
            return run
    raise AssertionError("no well-conditioned draw for %r" % ((D, lpd, P, kind, i),))


@functools.lru_cache(maxsize=None)
def learner_batch(D, lpd, P, R, first):
    """-> (table f32 [P + ROOM], [Run] * R)."""
    table = np.random.RandomState(17 * D + P).randn(P + ROOM).astype(np.float32)
    return table, [_run(table, D, lpd, P, KINDS[(first + i) % len(KINDS)], i) for i in range(R)]


def pack(runs, order=None):
    """The per-lane arrays of a launch, run_stride = n_train + EXTRA entries per run; the EXTRA lanes hold what must
    never be read (an out-of-range offset, NaN).  -> dict of numpy arrays."""
    order = range(len(runs)) if order is None else order
    n = runs[0].D * runs[0].lpd
    stride = n + EXTRA
    R = len(runs)
    idx = np.full((R, stride), -1, np.int64)
    sign = np.full((R, stride), 1, np.int8)
    n2 = np.full((R, stride), np.nan)
    r = np.full((R, stride), np.nan)
    for k, i in enumerate(order):
        u = runs[i]
        idx[k, :n], sign[k, :n], n2[k, :n], r[k, :n] = u.idx, u.sign, u.n2, u.r
    sel = [runs[i] for i in order]
    return dict(idx=idx.reshape(-1), sign=sign.reshape(-1), n2=n2.reshape(-1), r=r.reshape(-1), stride=stride, n_train=n,
                pr=np.array([u.pr for u in sel]), sigma=np.array([u.sigma for u in sel], np.float32),
                lr=np.array([u.lr for u in sel]), theta=np.stack([u.theta for u in sel]),
                top=np.array([u.b_ref if u.b is None else u.b for u in sel], np.int32),
                null_ok=all(u.b is None or u.b == u.D for u in sel))


def pair_stream_ids(offset, L, K):
    """Explicit stream ids of one run, int64 [L, K]: lanes 2p, 2p + 1 share the streams of lane 2p (an odd last lane
    keeps its own) -- worker.episode_stream_ids' "pair" rule at lanes_per_dir 2, for any L."""
    g = int(offset) + np.arange(L, dtype=np.int64)
    first = np.where(np.arange(L) < 2 * (L // 2), g - (np.arange(L) % 2), g)
    return first[:, None] * K + np.arange(K, dtype=np.int64)[None, :]
