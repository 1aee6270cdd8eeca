"""GPU: fdr_strategy_distances (csrc/fdr_novelty.hip) at the edges of its domain, against the extended-precision
restatement tests/aux_ref.py.  Cases and why these shapes: tests/aux_cases.py; the yardsticks are pinned on the CPU by
tests/test_aux_ref.py.

  * every dists[i][h] within K 2^-53 scale of dist_ref, K = aux_ref.K_DEV = 8 k_cpu (k_cpu: the kernel's summation
    order in numpy float64 against the same reference, measured on the CPU, never on the kernel);
  * min_dist[i] bit-equal to min(dists[i]), argmin[i] = np.argmin of the device's own row, and dist_ref's argmin
    wherever the reference separates its two smallest entries (every non-tie case does: test_aux_ref.py);
  * exact ties (duplicated archive rows in one wave, in two waves, first / last row): the lower index;
  * routes: dists = NULL, min_dist = NULL, argmin = NULL leave the other outputs bit-equal;
  * W2 with stds equal to 1e-6 and exactly, a std of 0 (aux_cases "w2-near");
  * NaN: numpy's rule -- min is NaN, argmin the first NaN distance; a clean neighbour in the same launch untouched;
  * refusals leave sentinel-filled outputs untouched.

Measured on an MI355X (each test prints its own): device k per kind tvd 0.26, l2 2.99, w2 1.29 -- to the digits
shown the values of the CPU restatement of the kernel's order (k_cpu) -- against the bound 24.
"""
import numpy as np
import pytest
import torch

import aux_cases as ac
import aux_ref as ar

pytestmark = pytest.mark.gpu
SENT = -777.0


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from fdr import engine
    return engine


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def run(eng, c, full=True):
    out = eng.strategy_distances(dev(c["S"]), dev(c["B"]), c["kind"], full=full)
    return [t.cpu().numpy() for t in out]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def check_min_argmin(mn, am, d):
    """min bit-equal to the minimum of the device's own row, argmin numpy's of that row (NaN rule included)."""
    for i in range(len(d)):
        want, arg = ar.novelty_ref(d[i])
        assert bits(mn[i:i + 1])[0] == bits(np.array([want]))[0] or (np.isnan(want) and np.isnan(mn[i])), (i, mn[i], want)
        assert am[i] == arg, (i, am[i], arg)


_K = dict.fromkeys(ac.KINDS, 0.0)


@pytest.mark.parametrize("name", ac.DIST_CASES)
def test_distances_min_argmin(eng, name):
    c = ac.dist_case(name)
    mn, am, d = run(eng, c)
    assert d.shape == (len(c["S"]), len(c["B"]))
    worst = 0.0
    for i, a in enumerate(c["S"]):
        ref, scale = ar.dist_ref(a, c["B"], c["kind"])
        worst = max(worst, ar.k_of(d[i], ref, scale))
        if c["tie"] is None:
            assert am[i] == ar.novelty_ref(ref)[1], (name, i)
        else:
            assert am[i] == c["tie"], (name, i, am[i])
    _K[c["kind"]] = max(_K[c["kind"]], worst)
    print("%s: device k %.2f (bound %.0f); worst so far per kind %r" % (name, worst, ar.K_DEV, _K))
    assert worst <= ar.K_DEV, (name, worst)
    check_min_argmin(mn, am, d)
    if c["tie"] is not None:
        assert mn[0] == 0.0 and mn[1] > 0.0


@pytest.mark.parametrize("name", ["tvd-3x20x2", "l2-9x65x4", "w2-37x129x2", "w2-near", "l2-many", "tvd-tie6_9", "w2-tie2_6"])
def test_routes_are_bit_equal(eng, name):
    """full=False (dists = NULL: compute_novelty's and lane_novelty's route), then min_dist = NULL and argmin = NULL,
    each alone, through ctypes."""
    c = ac.dist_case(name)
    mn, am, d = run(eng, c)
    mn2, am2 = run(eng, c, full=False)
    np.testing.assert_array_equal(bits(mn2), bits(mn))
    np.testing.assert_array_equal(am2, am)
    S, B = dev(c["S"]), dev(c["B"])
    n, Z, D = S.shape
    H = B.shape[0]
    for drop in ("min", "arg"):
        o_mn = torch.full((n,), SENT, dtype=torch.float64, device="cuda")
        o_am = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        o_d = torch.full((n, H), SENT, dtype=torch.float64, device="cuda")
        rc = eng.lib.fdr_strategy_distances(None, eng._p(S), n, eng._p(B), H, Z, D, eng.DIST_KINDS[c["kind"]], eng._p(o_d),
                                            None if drop == "min" else eng._p(o_mn),
                                            None if drop == "arg" else eng._p(o_am), eng._stream(S.device))
        eng.check(rc, "fdr_strategy_distances")
        torch.cuda.synchronize()
        np.testing.assert_array_equal(bits(o_d.cpu().numpy()), bits(d))
        if drop == "min":
            np.testing.assert_array_equal(o_am.cpu().numpy(), am)
            assert np.all(o_mn.cpu().numpy() == SENT)
        else:
            np.testing.assert_array_equal(bits(o_mn.cpu().numpy()), bits(mn))
            assert np.all(o_am.cpu().numpy() == -7)


def test_no_strategies_is_a_no_op(eng):
    c = ac.dist_case("l2-5x64x6")
    mn, am, d = eng.strategy_distances(dev(c["S"][:0]), dev(c["B"]), "l2", full=True)
    assert mn.shape == (0,) and am.shape == (0,) and d.shape == (0, 5)


@pytest.mark.parametrize("kind", ac.KINDS)
def test_nan_strategy_scores_nan(eng, kind):
    """np.min over the archive (compute_strategy_novelty): a strategy with one NaN element has NaN distances to every
    entry, so min = NaN, argmin = 0; its clean neighbours in the same launch are what they are without it."""
    c = ac.nan_case(kind, "strategy")
    mn, am, d = run(eng, c)
    assert np.isnan(d[1]).all()
    assert np.isnan(mn[1]), "min_dist of a NaN strategy is %r, numpy's min is NaN" % mn[1]
    assert am[1] == 0, "argmin of a NaN strategy is %d, numpy's argmin is the first NaN (0)" % am[1]
    check_min_argmin(mn, am, d)
    clean = dict(c, S=c["S"][[0, 2]])
    mn0, am0, d0 = run(eng, clean)
    np.testing.assert_array_equal(bits(d[[0, 2]]), bits(d0))
    np.testing.assert_array_equal(bits(mn[[0, 2]]), bits(mn0))
    np.testing.assert_array_equal(am[[0, 2]], am0)
    for i in (0, 2):
        ref, scale = ar.dist_ref(c["S"][i], c["B"], kind)
        assert ar.k_of(d[i], ref, scale) <= ar.K_DEV and am[i] == ar.novelty_ref(ref)[1]
    mn2, am2 = run(eng, c, full=False)
    assert np.isnan(mn2[1]) and am2[1] == 0


@pytest.mark.parametrize("kind", ac.KINDS)
def test_nan_archive_entry_scores_nan(eng, kind):
    """Archive rows 7, 5 and 9 of 12 hold a NaN: every strategy's min is NaN and its argmin 5, the lowest NaN index
    (5 and 9 are walked by one wave, 7 by another); the other distances keep their bound."""
    c = ac.nan_case(kind, "archive")
    mn, am, d = run(eng, c)
    for i, a in enumerate(c["S"]):
        ref, scale = ar.dist_ref(a, c["B"], kind)
        np.testing.assert_array_equal(np.isnan(d[i]), np.isnan(ref))
        assert ar.k_of(d[i], ref, scale) <= ar.K_DEV
        assert np.isnan(mn[i]), "min_dist %r over a row with NaN distances, numpy's min is NaN" % mn[i]
        assert am[i] == min(ac.NAN_ARCHIVE_ROWS), "argmin %d, numpy's is the first NaN (%d)" % (am[i], min(ac.NAN_ARCHIVE_ROWS))
    check_min_argmin(mn, am, d)


def test_strategy_handler_passes_nan_through(eng):
    """lane_novelty of a lane whose theta' is NaN (NaN noise under its table offset) is NaN, not +inf -- +inf would rank
    the broken lane as the most novel one in the mixed objective.  A lane whose offset is out of range is never
    dereferenced: it runs theta itself (csrc/fdr_internal.h, LanesArgs::src), so it scores as the sign-0 lane."""
    from policies import DiscretePolicy
    from strategy import StrategyHandler
    from utils import math_helpers
    torch.manual_seed(124)
    pol = DiscretePolicy(4, 2, seed=124)
    P = pol.num_params
    table = np.random.RandomState(124).randn(1 << 16).astype(np.float32)
    table[50000:50000 + P] = np.nan
    tt = dev(table)
    h = StrategyHandler(pol, math_helpers.categorical_tvd, max_history_size=4)
    theta = pol.get_trainable_flat().copy()
    for i in (100, 20000, 40000):
        pol.set_trainable_flat((theta + np.float32(0.05) * table[i:i + P]).astype(np.float32))
        h.add_policy(pol)
    pol.set_trainable_flat(theta)
    h.set_zeta(np.random.RandomState(2).randn(20, 4).astype(np.float32))
    idx = np.array([5, 50000, 700, 0, table.size - P + 1], np.int64)
    sign = np.array([1, 1, -1, 0, 1], np.int8)
    nov = h.lane_novelty(tt, dev(idx), dev(sign), 0.02).cpu().numpy()
    assert np.isnan(nov[1]), "novelty of a NaN lane is %r" % nov[1]
    assert np.all(np.isfinite(nov[[0, 2, 3, 4]])) and np.all(nov[[0, 2, 3, 4]] > 0)
    assert nov[4] == nov[3]


def test_refusals_leave_outputs_untouched(eng):
    lib, _lib = eng.lib, eng._lib
    S = torch.zeros(2 * 8193, dtype=torch.float32, device="cuda")
    B = torch.zeros(3 * 8193, dtype=torch.float32, device="cuda")
    o_mn = torch.full((2,), SENT, dtype=torch.float64, device="cuda")
    o_am = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    o_d = torch.full((2, 3), SENT, dtype=torch.float64, device="cuda")

    def call(H, Z, D, kind):
        return lib.fdr_strategy_distances(None, eng._p(S), 2, eng._p(B), H, Z, D, kind, eng._p(o_d), eng._p(o_mn), eng._p(o_am),
                                          eng._stream(S.device))
    assert call(3, 8193, 1, _lib.FDR_DIST_L2) == _lib.FDR_ERR_UNSUPPORTED          # Z D = 8193
    assert call(3, 1, 8193, _lib.FDR_DIST_TVD) == _lib.FDR_ERR_UNSUPPORTED
    assert call(3, 20, 3, _lib.FDR_DIST_W2) == _lib.FDR_ERR_INVALID                # odd D with W2
    assert call(0, 20, 2, _lib.FDR_DIST_L2) == _lib.FDR_ERR_INVALID                # H = 0
    assert call(3, 0, 2, _lib.FDR_DIST_L2) == _lib.FDR_ERR_INVALID                 # Z = 0
    assert call(3, 20, 2, 3) == _lib.FDR_ERR_INVALID                               # unknown kind
    assert call(3, 20, 2, -1) == _lib.FDR_ERR_INVALID
    torch.cuda.synchronize()
    assert np.all(o_mn.cpu().numpy() == SENT) and np.all(o_am.cpu().numpy() == -7) and np.all(o_d.cpu().numpy() == SENT)
    assert call(3, 2048, 4, _lib.FDR_DIST_L2) == _lib.FDR_OK                       # Z D = 8192 is served
    torch.cuda.synchronize()
    assert np.all(o_mn.cpu().numpy() == 0.0) and np.all(o_am.cpu().numpy() == 0)
