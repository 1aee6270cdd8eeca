"""CPU: the extended-precision restatement of the learner step (tests/learner_ref.py) pinned against what the
reference program produced (tests/golden/g4_fd_step.npz) and against the oracle, and the conditions that the GPU
edge-shape tests (tests/test_gpu_learner_edges.py) put on their own inputs.

Measured here: g against the golden gradients rel-L2 1.0e-7, 9.1e-8 and 5.6e-8 (asserted at the project's 1e-5: the
reference forms f32 rows v_i, which is its own resolution); against oracle.learner.fd_gradient / fd_moments 1.0e-7
to 1.2e-7; centred ranks exact; dsgd_mirror against oracle.learner.dsgd_step at most 3.0e-8, two ulp (the torch
oracle takes its norm in f32, so the two are not bit-equal; asserted at the project's 1e-6).

Reordering floor: the same formula evaluated in f64 with its rows added in direction order and in reverse differs by
at most 1.4e-14 rel-L2 over every well-conditioned case the GPU tests use (asserted <= 2.5e-13: a quarter of
the 1e-12 at which the kernels are judged).  This is a property of the inputs, not of a kernel: a case above it
needs other inputs, never a wider tolerance.
"""
import numpy as np
import pytest

import learner_cases as lc
import learner_ref as ref
from oracle import learner as olearn
from oracle import noise as onoise

FLOOR = 2.5e-13


@pytest.mark.parametrize("case", ["cheetah_n16", "cheetah_n64", "trap_n16"])
def test_grad_matches_reference_program(golden, case):
    g = golden("g4_fd_step.npz")
    P = g[case + "_theta0"].size
    table = onoise.NoiseTable(2 ** 22, P, 124).table
    idx = g[case + "_idx"]
    sign = np.ones(idx.size, np.int8)
    n2 = ref.norms(table, P, idx, 0.02)
    direct = np.array([np.sum((np.float32(0.02) * table[i:i + P]).astype(np.float32).astype(np.longdouble) ** 2)
                       for i in idx]).astype(np.float64)
    np.testing.assert_allclose(n2, direct, rtol=1e-13)           # the prefix sum against the direct sum
    w = ref.weights(g[case + "_rewards"], 0.25, "zscore")
    mine = ref.grad(table, P, idx, ref.coef_d(w, sign, n2, 1, 0.02))
    rel = ref.rel_l2(mine, g[case + "_g"])
    print("%s: learner_ref g vs reference program rel-L2 %.2e" % (case, rel))
    assert rel <= 1e-5


def _oracle_case(lpd, seed):
    rs = np.random.RandomState(seed)
    n_dirs, P = 40, 777
    table = rs.randn(P + 5000).astype(np.float32)
    idx_dirs = rs.randint(0, 5001, n_dirs).astype(np.int64)
    sign = np.tile(np.array([1, -1, 1][:lpd], np.int8), n_dirs)
    rew = rs.randn(n_dirs * lpd) * 3 + 1
    n2 = np.repeat(ref.norms(table, P, idx_dirs, 0.02), lpd)
    return table, P, idx_dirs, np.repeat(idx_dirs, lpd), sign, rew, n2


@pytest.mark.parametrize("lpd", [1, 2, 3])
def test_grad_and_moments_match_oracle(lpd):
    table, P, idx_dirs, idx, sign, rew, n2 = _oracle_case(lpd, 5 + lpd)
    for mode in ("zscore", "centred_rank"):
        w = ref.weights(rew, 0.4, mode)
        mine = ref.grad(table, P, idx_dirs, ref.coef_d(w, sign, n2, lpd, 0.02))
        if mode == "zscore":
            theirs, z = olearn.fd_gradient(table, P, idx, sign, rew, 0.4, 0.02)
            np.testing.assert_allclose(w.astype(np.float64), z, rtol=1e-13, atol=1e-14)
        else:
            np.testing.assert_array_equal(w.astype(np.float64), olearn.centred_ranks(rew))
            theirs = olearn.fd_gradient_weights(table, P, idx, sign, olearn.centred_ranks(rew), 0.02)
        rel = ref.rel_l2(mine, theirs)
        print("lpd %d %s: learner_ref vs oracle rel-L2 %.2e" % (lpd, mode, rel))
        assert rel <= 1e-5
    # the moments form, one rank of two: lanes [lo, lo + n) of 2 n + 3
    n = rew.size
    lo, n_all = n, 2 * n + 3
    mom = ref.moments(table, P, idx_dirs, rew, 0.4, sign, n2, lpd, 0.02, lo, n_all)
    theirs = olearn.fd_moments(table, P, idx, sign, rew, 0.4, 0.02, lane_lo=lo, n_all=n_all, lanes_per_dir=lpd)
    assert mom.size == theirs.size == 2 * P + 1 + n_all
    assert ref.rel_l2(mom[:P], theirs[:P]) <= 1e-5
    if lpd == 2:   # antithetic pairs: B == 0 exactly on both sides
        assert np.all(mom[P:2 * P] == 0) and np.all(theirs[P:2 * P] == 0)
    else:
        assert ref.rel_l2(mom[P:2 * P], theirs[P:2 * P]) <= 1e-5
    np.testing.assert_array_equal(mom[2 * P:].astype(np.float64), theirs[2 * P:])
    # one rank holding every lane: its moments give the z-score gradient
    mom1 = ref.moments(table, P, idx_dirs, rew, 0.4, sign, n2, lpd, 0.02, 0, n)
    gz = ref.grad(table, P, idx_dirs, ref.coef_d(ref.weights(rew, 0.4, "zscore"), sign, n2, lpd, 0.02))
    assert ref.rel_l2(ref.grad_from_moments(mom1, P), gz) <= 1e-15
    th = olearn.grad_from_moments(olearn.fd_moments(table, P, idx, sign, rew, 0.4, 0.02, lanes_per_dir=lpd), P)
    assert ref.rel_l2(ref.grad_from_moments(mom1, P), th) <= 1e-5


def test_weights_edges():
    assert np.all(ref.weights(np.full(7, 2.5), 0.75, "zscore") == 1.75)      # std == 0: input unchanged
    assert ref.weights([3.0], 1.0, "zscore")[0] == 2.0                          # n == 1
    assert ref.centred_ranks([3.0])[0] == 0.0
    np.testing.assert_array_equal(ref.centred_ranks([1.0, 0.0, 1.0, 1.0]), np.array([1, 0, 2, 3]) / 3.0 - 0.5)
    # sign-0 lanes do not enter, whatever their n2
    c = ref.coef_d([1.0, 5.0, 2.0, 7.0], [1, 0, -1, 0], [4.0, 0.0, 8.0, 0.0], 2, 0.5)
    np.testing.assert_array_equal(c.astype(np.float64), [0.125, -0.125])


def test_lambda_rows_known_values():
    table = np.array([1.0, 2.0, 3.0, 4.0], np.float32)
    drift = np.array([[0.5, 0.25]], np.float32)
    lam = ref.lambda_rows(table, 2, [0, 2, 1], [1, -1, 1], [-1, 0, 1], 0.5, drift)
    np.testing.assert_array_equal(lam, np.array([[0.5, 1.0], [-1.0, -1.75], [1.0, 1.5]], np.float32))


def _floor(c, coef):
    fwd = ref.grad(c.table, c.P, c.idx_dirs, coef, dtype=np.float64)
    rev = ref.grad(c.table, c.P, c.idx_dirs, coef, dtype=np.float64, reverse=True)
    return ref.rel_l2(fwd, rev)


def test_reordering_floor_of_the_gpu_cases():
    """Every well-conditioned case of tests/test_gpu_learner_edges.py, in every weighting: what f64 summation order
    alone moves.  (The near-constant returns are judged at 1e-9 and are not among them.)"""
    worst, kappa = (-1.0, ()), 0.0
    for lpds in (lc.STAGED_LPD, lc.FUSED_LPD):
        for c in lc.grid_cases(lpds):
            assert c.kappa() <= lc.KAPPA_MAX, (c.n_dirs, c.P, c.lpd, c.kappa())
            kappa = max(kappa, c.kappa())
            for mode in lc.MODES:
                cs = c.coefs(mode)
                for coef in (cs if mode == "moments" else (cs,)):
                    f = _floor(c, coef)
                    assert f <= FLOOR, (c.n_dirs, c.P, c.lpd, mode, f)
                    worst = max(worst, (f, (c.n_dirs, c.P, c.lpd, mode)))
    print("reordering floor, small grid: worst %.2e at %s; coefficient conditioning at most %.1f" % (worst + (kappa,)))


@pytest.mark.parametrize("n_dirs,P,lpd", lc.BIG)
def test_reordering_floor_of_the_large_cases(n_dirs, P, lpd):
    c = lc.make_case(n_dirs, P, lpd)
    assert c.kappa() <= lc.KAPPA_MAX
    for mode in lc.MODES:
        cs = c.coefs(mode)
        for coef in (cs if mode == "moments" else (cs,)):
            f = _floor(c, coef)
            print("reordering floor (%d, %d) lpd %d %s: %.2e" % (n_dirs, P, lpd, mode, f))
            assert f <= FLOOR


def test_the_other_gpu_cases_are_well_conditioned():
    """The batches of the fd_step, three-rank moments and bad-offset tests."""
    cases = [lc.make_case(3, P, 2) for P in (1, 257, 65537, 70001)] + [lc.make_case(6, P, 2) for P in (65536, 65537)]
    cases += [lc.make_case(130, 1000, lpd) for lpd in (2, 5)]
    for c in cases:
        assert c.kappa() <= lc.KAPPA_MAX
        for mode in lc.MODES:
            cs = c.coefs(mode)
            for coef in (cs if mode == "moments" else (cs,)):
                assert _floor(c, coef) <= FLOOR, (c.n_dirs, c.P, c.lpd, mode)


def test_coef_condition_sees_cancelling_lanes():
    """One direction whose three used lanes' centred ranks cancel: the coefficient is zero in exact arithmetic and
    rounding residue in any other."""
    sign, n2 = np.array([0, 0, 1, 1, -1], np.int8), np.array([0.0, 0.0, 2.0, 2.0, 2.0])
    r = np.arange(13.0)            # rank == index: lanes 7, 8, 9 weigh (1 + 2 - 3) / 12
    assert ref.coef_condition(r, 0.0, "centred_rank", 5, sign, n2, 5, 0.02) > 1e12
    r[[0, 7, 11, 8, 5, 9]] = [7.0, 0.0, 8.0, 11.0, 9.0, 5.0]   # now ranks 0, 11, 5: (-6 + 5 + 1) / 12
    assert ref.coef_condition(r, 0.0, "centred_rank", 5, sign, n2, 5, 0.02) > 1e12
    r[[9, 10]] = [10.0, 5.0]       # ranks 0, 11, 10: (-6 + 5 - 4) / 12
    assert ref.coef_condition(r, 0.0, "centred_rank", 5, sign, n2, 5, 0.02) < 64


def test_plan_table():
    """The fused tiling of the cases that are chosen for it (tests/learner_cases.py PLAN_TABLE)."""
    for (n_dirs, P), plan in lc.PLAN_TABLE.items():
        assert lc.fused_plan(n_dirs, P) == plan, (n_dirs, P)
    assert lc.grad_plan(130, 1000) == (4, 64, 3) and lc.grad_plan(67, 1000) == (4, 64, 2)
    assert lc.grad_plan(1100, 131100) == (513, 1100, 1)


@pytest.mark.parametrize("P", lc.DSGD_P)
def test_dsgd_mirror_matches_oracle_and_is_unambiguous(P):
    theta, g = lc.dsgd_inputs(P)
    new, upd, norm, ambiguous = ref.dsgd_mirror(theta, g, lc.DSGD_LR, lc.DSGD_SCALE)
    assert not ambiguous
    o_new, o_upd = olearn.dsgd_step(theta, g, lc.DSGD_LR)     # min_scale 0.23 at omega 0
    err = float(np.abs(new.astype(np.float64) - o_new).max())
    print("P %d: dsgd_mirror vs oracle max |d theta| %.2e" % (P, err))
    assert err <= 1e-6
    assert abs(upd - o_upd) <= 1e-5 * max(o_upd, 1.0)
    # the moments-form inputs: unambiguous for the reference's own g (the GPU test repeats this for the device's)
    theta_m, mom = lc.dsgd_moments_inputs(P)
    gm = ref.grad_from_moments(mom, P).astype(np.float64)
    assert not ref.dsgd_mirror(theta_m, gm, lc.DSGD_LR, lc.DSGD_SCALE)[3]


def test_dsgd_mirror_zero_and_nan_gradient():
    theta, g = lc.dsgd_inputs(257)
    new, upd, norm, _ = ref.dsgd_mirror(theta, np.zeros(257), 0.01, 0.23)
    assert new.tobytes() == theta.tobytes() and upd == 0.0 and norm == 0.0
    gn = g.copy()
    gn[100] = np.nan
    new, upd, norm, _ = ref.dsgd_mirror(theta, gn, 0.01, 0.23)
    assert new.tobytes() == theta.tobytes() and upd == 0.0 and np.isnan(norm)


def test_dsgd_mirror_rounds_twice():
    """theta - fl32(c32 gr) with the product rounded first: the contracted form (one rounding) differs somewhere, so
    bit-equality with the mirror does tell the two apart."""
    theta, g = lc.dsgd_inputs(1025)
    new, _, norm, _ = ref.dsgd_mirror(theta, g, 0.01, 0.23)
    c32 = np.float32(0.01 * np.sqrt(1025.0) * 0.23 / norm)
    gr = (-g).astype(np.float32)
    fused = (theta.astype(np.float64) - c32.astype(np.float64) * gr.astype(np.float64)).astype(np.float32)
    assert np.count_nonzero(fused != new) > 0
