"""CPU checks of the top-b direction weighting: the extended-precision restatement tests/top_dirs_ref.py against a
brute-force statement of the definition, the conditions every GPU case of tests/test_gpu_top_dirs.py must meet, and the
new C entries' argument validation and workspace queries (reached without a device, as tests/test_abi.py does)."""
import ctypes

import numpy as np
import pytest

import learner_cases as lc
import learner_ref as ref
import top_dirs_cases as tc
import top_dirs_ref as tref
from learner_cases import PR, SIGMA

LD = np.longdouble


def brute_selected(r_all, lpd, b):
    """The definition, a double loop: rank_d = #{e : s_e > s_d, or s_e == s_d and e < d}."""
    r = np.asarray(r_all, np.float64).reshape(-1, lpd)
    D = r.shape[0]
    s = [(-np.inf if any(v != v for v in row) else max(row)) for row in r.tolist()]
    keep = np.zeros(D, bool)
    for d in range(D):
        rank = 0
        for e in range(D):
            if s[e] > s[d] or (s[e] == s[d] and e < d):
                rank += 1
        keep[d] = rank < b
    return keep


@pytest.mark.parametrize("kind", tc.SEL_RETURNS)
@pytest.mark.parametrize("lpd", tc.SEL_LPD)
def test_selection_equals_the_double_loop(lpd, kind):
    for D in (1, 2, 3, 17, 255, 257):
        r = tc.sel_returns(D, lpd, kind)
        for b in tc.sel_bs(D):
            keep = tref.selected(r, lpd, b)
            assert keep.sum() == b
            np.testing.assert_array_equal(keep, brute_selected(r, lpd, b), err_msg="D %d lpd %d b %d" % (D, lpd, b))


def test_selection_cases_are_what_they_claim():
    for lpd in tc.SEL_LPD:
        for D in tc.SEL_D:
            assert len(tc.sel_bs(D)) >= 1 and tc.sel_bs(D)[-1] == D
            shards = tc.sel_shards(D, lpd)
            assert shards[0] == (0, D * lpd)
            for lo, n in shards:
                assert lo % lpd == 0 and n % lpd == 0 and n >= lpd and lo + n <= D * lpd
            if D >= 3:
                assert shards[1][0] % 256 != 0 and shards[2][0] + shards[2][1] == D * lpd
            r = tc.sel_returns(D, lpd, "max_last").reshape(D, lpd)
            assert np.all(r.argmax(1) == lpd - 1)
            r = tc.sel_returns(D, lpd, "nan")
            assert np.isnan(r).sum() == 1
            nan_dir = int(np.flatnonzero(np.isnan(r))[0]) // lpd
            for b in tc.sel_bs(D):      # left out by every b < D, taken in by b = D
                assert tref.selected(r, lpd, b)[nan_dir] == (b == D)
            z = tc.sel_returns(D, lpd, "signed_zero")
            assert np.all(z == 0) and (D * lpd < 8 or (np.signbit(z).any() and not np.signbit(z).all()))
            np.testing.assert_array_equal(np.flatnonzero(tref.selected(z, lpd, tc.sel_bs(D)[0])),
                                          np.arange(tc.sel_bs(D)[0]))     # one tie: the lowest indices
    five = tc.sel_returns(4097, 1, "five_values")
    assert len(set(five.tolist())) == 5     # 4097 scores from five values: every value on both sides of both seams
    for v in set(five.tolist()):
        assert v in five[:2048] and v in five[2048:4096]


def test_all_directions_kept_is_the_zscore():
    for n_all, lpd in ((6, 2), (257, 1), (4608, 2), (15, 3)):
        r = np.random.RandomState(n_all).randn(n_all) * 3 + 1
        w, keep = tref.weights(r, PR, lpd, n_all // lpd)
        assert keep.all()
        np.testing.assert_array_equal(w, ref.weights(r, PR, "zscore"))


def test_weights_definition():
    r = np.array([1.0, 5.0, 2.0, 2.0, 9.0, -1.0, 0.5, 0.25])
    w, keep = tref.weights(r, 0.5, 2, 2)
    np.testing.assert_array_equal(keep, [True, False, True, False])     # scores 5, 2, 9, 0.5
    x = (r - 0.5)[[0, 1, 4, 5]].astype(LD)
    m = x.sum() / 4
    sd = np.sqrt(((x - m) ** 2).sum() / 4)
    np.testing.assert_array_equal(w[[0, 1, 4, 5]], (x - m) / sd)
    assert np.all(w[[2, 3, 6, 7]] == 0)
    # sd == 0 over the kept lanes: the input passes unchanged (standardize_arr); the other lanes still weigh 0
    w, keep = tref.weights(np.array([2.5, 2.5, 1.0, 0.0]), 0.75, 1, 2)
    np.testing.assert_array_equal(w, np.array([1.75, 1.75, 0.0, 0.0], LD))
    # a NaN that is not kept changes nothing; a kept one makes every weight NaN
    rn = np.array([1.0, np.nan, 3.0, 2.0, 0.0, 0.5])
    w, keep = tref.weights(rn, 0.0, 2, 2)
    np.testing.assert_array_equal(keep, [False, True, True])
    assert np.all(w[:2] == 0) and np.all(np.isfinite(w.astype(np.float64)))
    w, keep = tref.weights(rn, 0.0, 2, 3)
    assert keep.all() and np.isnan(w.astype(np.float64)).all()


def test_gpu_gradient_cases_meet_the_conditioning_cap():
    """Every case of tests/test_gpu_top_dirs.py that is held to rel-L2 1e-12 is built here; top_dirs_ref's
    coef_condition is learner_ref's argument with the kept set's mean and sd."""
    worst = 0.0
    for c, b in tc.all_grad_cases():
        assert 1 <= b <= c.n_all // c.lpd and c.lane_lo % c.lpd == 0 and c.n_all % c.lpd == 0
        k = tc.kappa(c, b)
        assert k <= lc.KAPPA_MAX, (c.n_dirs, c.P, k)
        worst = max(worst, k)
    for n_dirs, P, lpd in tc.BIT_CASES:     # b == D: the z-score's own condition
        c = lc.make_case(n_dirs, P, lpd)
        k = tc.kappa(c, c.n_all // lpd)
        assert k <= lc.KAPPA_MAX
        assert abs(k - ref.coef_condition(c.r_all, PR, "zscore", 0, c.sign, c.n2, lpd, SIGMA)) <= 1e-9 * k
        worst = max(worst, k)
    assert lc.fused_plan(*tc.GRAD_BIG[:2]) == lc.PLAN_TABLE[tc.GRAD_BIG[:2]] and lc.fused_plan(2304, 1500)[2] > 1
    print("top-b gradient cases: worst kappa %.1f (cap %.0f)" % (worst, lc.KAPPA_MAX))


# ---- the C entries without a device --------------------------------------------------------------------------------
FAKE = ctypes.c_void_p(4096)        # a non-NULL pointer no refused call may look behind


def test_workspace_queries_and_out_len():
    from fdr import _lib
    lib = _lib.lib
    assert _lib.FDR_WEIGHT_TOP_DIRS == 4
    assert lib.fdr_fd_grad_fused_out_len(_lib.FDR_WEIGHT_TOP_DIRS, 6092, 4096) == 6092
    assert lib.fdr_top_dir_weights_workspace_bytes(0) == -1
    assert lib.fdr_top_dir_weights_workspace_bytes(1) == 256
    assert lib.fdr_top_dir_weights_workspace_bytes(4096) == 4096
    base = lib.fdr_fd_grad_fused_workspace_bytes(2048, 2, 6092, _lib.FDR_WEIGHT_CENTERED_RANK)
    # the mask covers the lanes of ALL ranks: the query takes n_all
    assert lib.fdr_fd_grad_fused_top_workspace_bytes(2048, 2, 6092, 4096) == base + 4096
    assert lib.fdr_fd_grad_fused_top_workspace_bytes(2048, 2, 6092, 32768) == base + 32768
    assert lib.fdr_fd_grad_fused_top_workspace_bytes(2048, 0, 6092, 4096) == -1
    assert lib.fdr_fd_grad_fused_top_workspace_bytes(2048, 2, 6092, 0) == -1
    assert lib.fdr_fd_grad_fused_counter_bytes(2048, 6092) == 256      # the counter-bytes rule is unchanged


def _weights_call(lib, n_all, lpd, top, lo, n_local):
    return lib.fdr_top_dir_weights(None, FAKE, n_all, 0.0, lpd, top, lo, n_local, FAKE, None, FAKE, 1 << 20, None)


def _grad_call(lib, n_dirs, n_all, lpd, top, lo):
    return lib.fdr_fd_grad_fused_top(None, FAKE, 1 << 20, FAKE, n_dirs, 100, FAKE, n_all, 0.0, lo, FAKE, FAKE, lpd, 0.02,
                                     top, FAKE, 100, FAKE, 1 << 30, None)


@pytest.mark.parametrize("call", ["weights", "grad"])
def test_argument_validation_without_gpu(call):
    from fdr import _lib
    lib = _lib.lib

    def run(n_all, lpd, top, lo, n_local):
        if call == "weights":
            return _weights_call(lib, n_all, lpd, top, lo, n_local)
        return _grad_call(lib, n_local // lpd, n_all, lpd, top, lo)

    for args, text in (((12, 2, 0, 0, 4), b"top_dirs < 1"),
                       ((12, 2, -3, 0, 4), b"top_dirs < 1"),
                       ((12, 2, 7, 0, 4), b"top_dirs above"),
                       ((13, 2, 1, 0, 4), b"n_all is not a multiple"),
                       ((12, 2, 1, 1, 4), b"not a multiple of lanes_per_dir")):
        assert run(*args) == _lib.FDR_ERR_INVALID, args
        assert text in lib.fdr_last_error(), (args, lib.fdr_last_error())
    if call == "weights":
        assert _weights_call(lib, 12, 2, 1, 0, 3) == _lib.FDR_ERR_INVALID      # n_local no multiple of lpd
        assert b"not a multiple of lanes_per_dir" in lib.fdr_last_error()
        assert _weights_call(lib, 12, 2, 6, 4, 0) == _lib.FDR_OK               # n_local == 0: nothing launched
        assert _weights_call(lib, 12, 2, 1, 8, 6) == _lib.FDR_ERR_INVALID      # the window leaves rewards_all


def test_plain_entries_refuse_the_mode():
    """fdr_fd_grad_fused, fdr_fd_step and fdr_fd_step_opt refuse FDR_WEIGHT_TOP_DIRS as they refuse ZSCORE_MIX: b does
    not fit their arguments."""
    from fdr import _lib
    lib = _lib.lib
    m = _lib.FDR_WEIGHT_TOP_DIRS
    rc = lib.fdr_fd_grad_fused(None, FAKE, 1 << 20, FAKE, 2, 100, FAKE, 4, 0.0, 0, FAKE, FAKE, 2, 0.02, m, FAKE, 100,
                               FAKE, 1 << 30, None)
    assert rc == _lib.FDR_ERR_INVALID and b"fdr_fd_grad_fused_top" in lib.fdr_last_error()
    rc = lib.fdr_fd_step(None, FAKE, 1 << 20, FAKE, 2, 100, FAKE, 4, 0.0, FAKE, FAKE, 2, 0.02, m, FAKE, 0.01, 1.0, FAKE,
                         None, FAKE, FAKE, 1 << 30, None)
    assert rc == _lib.FDR_ERR_INVALID and b"fdr_fd_step_top" in lib.fdr_last_error()
    rc = lib.fdr_fd_step_opt(None, FAKE, 1 << 20, FAKE, 2, 100, FAKE, 4, 0.0, FAKE, FAKE, 2, 0.02, m, FAKE,
                             _lib.FDR_OPT_ADAM, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0.0, 0.0, 0, 1, FAKE, FAKE, FAKE, None, FAKE,
                             FAKE, 1 << 30, None)
    assert rc == _lib.FDR_ERR_INVALID and b"fdr_fd_step_top_opt" in lib.fdr_last_error()
    # the single-process entries hold n_all = n_local
    rc = lib.fdr_fd_step_top(None, FAKE, 1 << 20, FAKE, 2, 100, FAKE, 6, 0.0, FAKE, FAKE, 2, 0.02, 1, FAKE, 0.01, 1.0,
                             FAKE, None, FAKE, FAKE, 1 << 30, None)
    assert rc == _lib.FDR_ERR_INVALID and b"single-process" in lib.fdr_last_error()


def test_learner_and_runner_arguments():
    """Argument rules of FiniteDifferences(weighting="top_directions") that need no device."""
    from learner.finite_differences import _check_top_directions, resolve_top_directions
    for bad in (None, 0, -2, 0.0, 1.5, -0.25, True, "3"):
        with pytest.raises(ValueError):
            _check_top_directions(bad)
    assert resolve_top_directions(24, 96) == 24
    assert resolve_top_directions(200, 96) == 96        # clipped: the list route can deliver fewer returns
    assert resolve_top_directions(np.int64(5), 96) == 5
    assert resolve_top_directions(0.25, 96) == 24
    assert resolve_top_directions(0.25, 97) == 25       # ceil
    assert resolve_top_directions(1.0, 7) == 7
    assert resolve_top_directions(0.001, 7) == 1
    assert resolve_top_directions(1, 96) == 1           # the int 1 is one direction, the float 1.0 all of them
    assert resolve_top_directions(0.07, 100) == 8       # literally ceil(f D) in f64: 0.07 * 100 = 7.000000000000001


def test_command_line_weightings():
    """tools/physics_learning.py and tools/dist_check.py share one parser: an int where the text reads as one."""
    from learner.finite_differences import parse_weighting
    assert parse_weighting("zscore") == ("zscore", None)
    assert parse_weighting("centred_rank") == ("centred_rank", None)
    for text, top in (("512", 512), ("1", 1), ("0.25", 0.25), ("1e-1", 0.1), ("1.", 1.0)):
        got = parse_weighting("top_directions:" + text)
        assert got == ("top_directions", top) and type(got[1]) is type(top)
    for bad in ("top_directions:", "top_directions:many", "top_directions:0", "top_directions:1.5", "zscore:3"):
        with pytest.raises(ValueError):
            parse_weighting(bad)
