"""The mixed objective (reward / novelty / entropy weights, FDR_WEIGHT_ZSCORE_MIX) restated in extended precision on
top of tests/learner_ref.py, and the novelty / entropy channels that go with the cases of tests/learner_cases.py.
TEST INFRASTRUCTURE ONLY: shared by tests/test_learner_mix_ref.py (CPU: the conditions the inputs meet) and
tests/test_gpu_learner_mix.py (the kernels).

    mix_weights     w_i = sum over the channels with a_c != 0, in the order reward, novelty, entropy, of a_c z_c[i];
                    z_c = learner_ref.weights(v_c, p_c, "zscore"): x_c = v_c - p_c in f64, two-pass mean / population
                    std in longdouble, x_c unchanged when the std is 0
    mix_kappa       learner_ref.coef_condition's ratio ||m|| / ||coef|| with the per-lane magnitude
                    sum_c |a_c| (|x_c| + |m_c|) / sd_c (|x_c| where sd_c == 0)
    channels        nov = 0.3 |randn|, ent = 1.4 + 0.05 randn over all lanes of a case, from a seed of the case's shape;
                    a draw whose mix_kappa exceeds learner_cases.KAPPA_MAX is replaced by the next salt
"""
import functools

import numpy as np

import learner_cases as lc
import learner_ref as ref
from learner_cases import PR, SIGMA

LD = np.longdouble
POLICY_NOVELTY, POLICY_ENTROPY = 0.2, 1.3
COEF_SETS = ((0.6, 0.4, 0.05), (0.0, 1.0, 0.0), (1.0, 0.0, 0.01), (0.25, 0.75, 0.0))
MAX_SALTS = 64


def policy_values(pr=PR):
    return (pr, POLICY_NOVELTY, POLICY_ENTROPY)


def _stats(x):
    """(x as longdouble, mean, population std) of an f64 array."""
    x = np.asarray(x, np.float64).astype(LD)
    mean = x.sum() / LD(x.size)
    return x, mean, np.sqrt(((x - mean) ** 2).sum() / LD(x.size))


def mix_weights_arrays(values, policy, coefs):
    """Per-lane mixed weights over ALL lanes (longdouble).  values / policy / coefs: (reward, novelty, entropy); the
    array of a channel whose coefficient is 0 is not looked at (it may be None)."""
    w = None
    for v, p, a in zip(values, policy, coefs):
        if a == 0:
            continue
        t = LD(a) * ref.weights(v, p, "zscore")
        w = t if w is None else w + t
    assert w is not None, "all three coefficients are 0"
    return w


def mix_weights(case, coefs, nov, ent, pr=PR):
    return mix_weights_arrays((case.r_all, nov, ent), policy_values(pr), coefs)


def mix_coefs(case, coefs, nov, ent, pr=PR):
    """Reference per-direction coefficients of the case's local lanes (longdouble [n_dirs])."""
    w = mix_weights(case, coefs, nov, ent, pr)[case.lane_lo:case.lane_lo + case.n_local]
    return ref.coef_d(w, case.sign, case.n2, case.lpd, SIGMA)


def mix_kappa(case, coefs, nov, ent, pr=PR):
    mag = np.zeros(case.n_all, LD)
    for v, p, a in zip((case.r_all, nov, ent), policy_values(pr), coefs):
        if a == 0:
            continue
        x, mean, sd = _stats(np.asarray(v, np.float64) - float(p))
        mag += LD(abs(a)) * (np.abs(x) if sd == 0 else (np.abs(x) + abs(mean)) / sd)
    sl = slice(case.lane_lo, case.lane_lo + case.n_local)
    w = mix_weights(case, coefs, nov, ent, pr)
    if not np.any(w[sl] != 0):
        return 1.0
    c = ref.coef_d(w[sl], case.sign, case.n2, case.lpd, SIGMA)
    m = ref.coef_d(mag[sl], np.abs(np.asarray(case.sign, np.int64)), case.n2, case.lpd, SIGMA)
    nc = np.sqrt((c * c).sum())
    return float("inf") if nc == 0 else float(np.sqrt((m * m).sum()) / nc)


def draw_channels(case, salt):
    rs = np.random.RandomState((7919 * case.n_dirs + 31 * case.P + case.lpd + 104729 * salt) % (1 << 32))
    nov = 0.3 * np.abs(rs.randn(case.n_all))
    ent = 1.4 + 0.05 * rs.randn(case.n_all)
    return nov, ent


@functools.lru_cache(maxsize=None)
def channels(case, coefs):
    """(nov, ent, salt, kappa) for a learner_cases case (cached objects: make_case is) and a coefficient set."""
    for salt in range(MAX_SALTS):
        nov, ent = draw_channels(case, salt)
        k = mix_kappa(case, coefs, nov, ent)
        if k <= lc.KAPPA_MAX:
            return nov, ent, salt, k
    raise AssertionError("no well-conditioned channels for %r, coefficients %r" % (
        (case.n_dirs, case.P, case.lpd, case.lane_lo, case.n_all), coefs))
