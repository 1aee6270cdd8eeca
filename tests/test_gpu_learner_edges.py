"""The learner kernels (fdr_learner.hip, fdr_learner_fused.hip, fdr_dsgd.hip) at the edges of their domain, against
the extended-precision restatement tests/learner_ref.py.  Cases and the kernels' tilings: tests/learner_cases.py.

Fused tiling of the cases chosen for a path, (n_dirs, P) -> (col_blocks, rows_per_chunk, n_chunks); each test
asserts the path it needs from the same formulas, so a retune of the plan fails here instead of moving a case:

    (63, 1000)   -> (4, 64, 1)       (64, 1000)    -> (4, 64, 1)        (65, 1000)     -> (4, 64, 2)
    (67, 1000)   -> (4, 64, 2)       (130, 1000)   -> (4, 64, 3)        (130, 257)     -> (2, 64, 3)
    (4097, 300)  -> (2, 64, 65)      (2304, 1500)  -> (6, 64, 36)       n_all 4097 / 4608: the statistics tail
    (1600, 40000)  -> (157, 320, 5)      rows_per_chunk > 256: further directions per thread
    (1100, 131100) -> (513, 1024, 2)     rows_per_chunk = kFusedMaxRows, chunks 1024 + 76, 28 live columns at the end

The device table is a slice of a NaN-filled buffer, buf[64 : 64 + size]: a read one element outside the table turns
the result NaN, and a broken bounds guard yields a wrong number inside the allocation, never a fault.  Offsets
include 0 and max_idx; one case has table_size == P.

Tolerances (the project's): f64 kernels against the reference rel-L2 1e-12; ranks exact; theta after DSGD bit-equal
to learner_ref.dsgd_mirror; out[0] = ||d theta|| relative P 2^-52 (the bound of any f64 summation order of P
positive terms); out[1] exactly the mirror's norm.

Worst measured on an MI355X (each test prints its own), next to the tolerance:
    staged fd_weights + fd_grad, small grid          6.8e-15   1e-12
    fused small grid: zscore / centred_rank / moments   1.3e-14 / 2.6e-15 / 5.7e-15   1e-12
    fused large cases, vs reference and vs staged    6.1e-16   1e-12
    moments of three ranks -> g                      2.3e-16   1e-12
    lambda norms / gradient                          4.0e-16   1e-12
    fd_step g                                        1.4e-16   1e-12
    g from moments in the DSGD launch                1.3e-16   1e-12
    DSGD ||d theta|| relative                        3.8e-16   P 2^-52 (2.2e-16 at P = 1 .. 2.9e-11)
    theta, theta_hist, ranks, out[1]                 bit-equal / exact
A library copy with five in-bounds arithmetic changes (the statistics tail dropped, the three DSGD updates contracted
to one rounding, the rank tie-break by tile-local lane) passed every earlier learner test and failed 43 of these.
"""
import numpy as np
import pytest
import torch

import learner_cases as lc
import learner_ref as ref
from learner_cases import PR, SIGMA
from oracle import noise as onoise

pytestmark = pytest.mark.gpu

TOL = 1e-12
NAN = float("nan")


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from fdr import engine
    return engine


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def dev_table(table):
    """The table as buf[GUARD : GUARD + size] of a NaN-filled device buffer (a contiguous view, not a copy)."""
    buf = torch.full((table.size + 2 * lc.GUARD,), NAN, dtype=torch.float32, device="cuda")
    view = buf[lc.GUARD:lc.GUARD + table.size]
    view.copy_(torch.from_numpy(table))
    assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + 4 * lc.GUARD
    return view


class Dev(object):
    """A Case's arrays on the device."""

    def __init__(self, c, idx_dirs=None):
        idx_dirs = c.idx_dirs if idx_dirs is None else idx_dirs
        self.table = dev_table(c.table)
        self.idx_dirs = dev(idx_dirs)
        self.idx = dev(np.repeat(idx_dirs, c.lpd))
        self.sign, self.n2, self.r_all = dev(c.sign), dev(c.n2), dev(c.r_all)
        self.r_local = self.r_all[c.lane_lo:c.lane_lo + c.n_local]


def what(c):
    return "n_dirs %d P %d lpd %d lo %d n_all %d max_idx %d" % (c.n_dirs, c.P, c.lpd, c.lane_lo, c.n_all, c.max_idx)


def run_fused(eng, c, d, mode):
    if mode == "moments":
        return eng.fd_grad_fused(d.table, d.idx, d.r_local, PR, c.lane_lo, d.sign, d.n2, c.lpd, SIGMA, c.P,
                                 mode=mode, n_all=c.n_all).cpu().numpy()
    return eng.fd_grad_fused(d.table, d.idx, d.r_all, PR, c.lane_lo, d.sign, d.n2, c.lpd, SIGMA, c.P,
                             mode=mode).cpu().numpy()


def expected_slots(c):
    slots = np.zeros(c.n_all)
    slots[c.lane_lo:c.lane_lo + c.n_local] = c.r_local - PR
    return slots


def fused_error(c, out, mode, cols=None):
    """Worst rel-L2 of a fused result against the reference (on `cols` when given); the moments form's count and
    slots are checked exactly."""
    P = c.P
    sel = slice(None) if cols is None else cols
    cs = c.coefs(mode)
    if mode != "moments":
        assert out.size == P
        return ref.rel_l2(out[sel], ref.grad(c.table, P, c.idx_dirs, cs, cols))
    assert out.size == 2 * P + 1 + c.n_all
    assert out[2 * P] == c.n_local, what(c)
    np.testing.assert_array_equal(out[2 * P + 1:], expected_slots(c), err_msg=what(c))
    return max(ref.rel_l2(out[:P][sel], ref.grad(c.table, P, c.idx_dirs, cs[0], cols)),
               ref.rel_l2(out[P:2 * P][sel], ref.grad(c.table, P, c.idx_dirs, cs[1], cols)))


# ---- staged fd_weights + fd_grad ---------------------------------------------------------------------------------
@pytest.mark.parametrize("lpd", lc.STAGED_LPD)
def test_staged_weights_and_grad_small_grid(eng, lpd):
    """n_dirs over the 4-row unroll tails and the 64-row chunk seam, P around one column block, sign-0 lanes with
    n2 = 0, lane_lo > 0, n_all in {1, 2, 1025, 4097}, std == 0, table_size == P."""
    assert lc.grad_plan(65, 1000)[2] == 2 and lc.grad_plan(130, 1000) == (4, 64, 3)
    worst = 0.0
    for c in lc.grid_cases((lpd,)):
        d = Dev(c)
        coef = eng.fd_weights(d.r_all, PR, c.lane_lo, d.sign, d.n2, c.lpd, SIGMA)
        g = eng.fd_grad(d.table, d.idx_dirs, coef, c.P).cpu().numpy()
        cref = c.coefs("zscore")
        e = max(ref.rel_l2(coef.cpu().numpy(), cref), ref.rel_l2(g, ref.grad(c.table, c.P, c.idx_dirs, cref)))
        assert e <= TOL, (what(c), e)
        worst = max(worst, e)
    print("staged fd_weights + fd_grad, lpd %d: worst rel-L2 %.2e (tolerance %.0e)" % (lpd, worst, TOL))


# ---- fused, every mode -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", lc.MODES)
@pytest.mark.parametrize("lpd", lc.FUSED_LPD)
def test_fused_small_grid(eng, lpd, mode):
    """The same grid through fdr_fd_grad_fused: lanes_per_dir 1, 3, 4 (the register path), 5, 7 (the path above
    kMaxLpd), a sign-0 lane in position 0 of a direction."""
    assert lc.fused_plan(65, 1000) == lc.PLAN_TABLE[(65, 1000)] and lc.fused_plan(130, 257) == lc.PLAN_TABLE[(130, 257)]
    worst = 0.0
    for c in lc.grid_cases((lpd,)):
        assert c.lpd == 1 or (c.sign[0] == 0 and c.n2[0] == 0)
        d = Dev(c)
        out = run_fused(eng, c, d, mode)
        e = fused_error(c, out, mode)
        assert e <= TOL, (what(c), mode, e)
        worst = max(worst, e)
    print("fused %s, lpd %d: worst rel-L2 %.2e (tolerance %.0e)" % (mode, lpd, worst, TOL))


@pytest.mark.parametrize("mode", lc.MODES)
@pytest.mark.parametrize("n_dirs,P,lpd", lc.BIG)
def test_fused_large_cases(eng, n_dirs, P, lpd, mode):
    """The statistics tail (n_all > 4096), rows_per_chunk > 256 and = 1024 with a ragged last chunk, in every mode:
    against the reference (all columns, or the first 512, last 512 and 1024 random ones) and, full vector, against
    the staged fd_grad with the same coefficients."""
    cb, rpc, n_chunks = plan = lc.fused_plan(n_dirs, P)
    assert plan == lc.PLAN_TABLE[(n_dirs, P)]
    c = lc.make_case(n_dirs, P, lpd)
    if P <= 1500:
        assert c.n_all > 4096 and n_chunks > 1                    # the tail of the statistics loops
    else:
        assert rpc > 256 and n_chunks > 1                         # further directions per thread
    if P == 131100:   # the LDS arrays full, a ragged last chunk, a mostly idle last column block
        assert rpc == 1024 and n_dirs - rpc == 76 and P - (cb - 1) * 256 == 28
    d = Dev(c)
    out = run_fused(eng, c, d, mode)
    np.testing.assert_array_equal(run_fused(eng, c, d, mode), out)   # the tickets were left at zero
    cols = None if n_dirs * P <= (1 << 22) else lc.big_cols(P)
    e = fused_error(c, out, mode, cols)
    cs = c.coefs(mode)
    for k, coef in enumerate(cs if mode == "moments" else (cs,)):
        staged = eng.fd_grad(d.table, d.idx_dirs, dev(coef.astype(np.float64)), P).cpu().numpy()
        e = max(e, ref.rel_l2(out[k * P:(k + 1) * P], staged))
    if mode == "zscore":
        coef = eng.fd_weights(d.r_all, PR, 0, d.sign, d.n2, lpd, SIGMA)
        e = max(e, ref.rel_l2(out, eng.fd_grad(d.table, d.idx_dirs, coef, P).cpu().numpy()))
    print("fused %s (%d, %d) lpd %d: worst rel-L2 %.2e (tolerance %.0e)" % (mode, n_dirs, P, lpd, e, TOL))
    assert e <= TOL


@pytest.mark.parametrize("P", [65536, 65537])
def test_moments_of_three_ranks_then_dsgd(eng, P):
    """Three rank slices' moments summed (the all-reduce), DSGD from the sum: g_out against grad_from_moments, theta
    bit-equal to the mirror of that g, on both sides of the one-workgroup DSGD's limit."""
    c = lc.make_case(6, P, 2)
    d = Dev(c)
    mom = torch.zeros(2 * P + 1 + c.n_all, dtype=torch.float64, device="cuda")
    for r in range(3):
        lo, hi = 4 * r, 4 * r + 4
        mom += eng.fd_grad_fused(d.table, d.idx[lo:hi], d.r_all[lo:hi], PR, lo, d.sign[lo:hi], d.n2[lo:hi], 2, SIGMA, P,
                                 mode="moments", n_all=c.n_all)
    m = mom.cpu().numpy()
    assert m[2 * P] == c.n_all
    np.testing.assert_array_equal(m[2 * P + 1:], c.r_all - PR)
    g_ref = ref.grad_from_moments(ref.moments(c.table, P, c.idx_dirs, c.r_all, PR, c.sign, c.n2, 2, SIGMA, 0, c.n_all), P)
    theta = lc.dsgd_inputs(P)[0]
    t, g_out = dev(theta), torch.full((P,), NAN, dtype=torch.float64, device="cuda")
    out = eng.dsgd_step_ex(t, mom, True, lc.DSGD_LR, lc.DSGD_SCALE, g_out=g_out).cpu().numpy()
    e = ref.rel_l2(g_out.cpu().numpy(), g_ref)
    print("moments of 3 ranks, P %d: g rel-L2 %.2e (tolerance %.0e)" % (P, e, TOL))
    assert e <= TOL
    check_dsgd(theta, g_out.cpu().numpy(), t, out)


# ---- centred ranks -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["five_values", "equal"])
@pytest.mark.parametrize("n_all", [1, 2, 2047, 2048, 2049, 4100])
def test_rank_weights_across_the_tile_seam(eng, n_all, kind):
    """rank_weights_kernel tiles n_all by 2048: ties (broken by global lane) on both sides of the seam, windows
    that straddle it."""
    r = lc.rank_returns(n_all, kind)
    want = ref.centred_ranks(r)
    windows = [(0, n_all), (n_all - 1, 1)]
    if n_all > 2048:
        windows += [(2040, min(20, n_all - 2040)), (2047, 2)]
    rd = dev(r)
    for lo, n in windows:
        np.testing.assert_array_equal(eng.rank_weights(rd, lo, n).cpu().numpy(), want[lo:lo + n])


# ---- delayed returns ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 255, 257, 6092])
def test_lambda_norms_and_grad(eng, P):
    worst = 0.0
    for n in (1, 2, 3, 64, 65, 129):
        table, idx, sign, slot, drift, coef = lc.lambda_case(n, P)
        assert set(slot) == set(range(-1, 3)[:min(n, 4)])
        lam = ref.lambda_rows(table, P, idx, sign, slot, SIGMA, drift).astype(np.longdouble)
        tab, di, ds, dl, dd = dev_table(table), dev(idx), dev(sign), dev(slot), dev(drift)
        n2 = eng.fd_lambda_norms(tab, di, ds, dl, SIGMA, dd, P).cpu().numpy()
        n2_ref = (lam * lam).sum(1)
        e = float(np.max(np.abs(n2 - n2_ref) / n2_ref))
        g = eng.fd_grad_lambda(tab, di, ds, dl, dev(coef), SIGMA, dd, P).cpu().numpy()
        g_ref = np.zeros(P, np.longdouble)
        for i in range(n):
            g_ref += np.longdouble(coef[i]) * lam[i]
        e = max(e, ref.rel_l2(g, g_ref))
        assert e <= TOL, (n, P, e)
        worst = max(worst, e)
    assert lc.grad_plan(129, 6092)[2] == 3
    print("lambda norms and gradient, P %d: worst relative error %.2e (tolerance %.0e)" % (P, worst, TOL))


# ---- perturbation rows -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("room", [0, 4096])
@pytest.mark.parametrize("P", [1, 257, 1000])
def test_perturb_at_table_edges(eng, P, room):
    rs = np.random.RandomState(P + room)
    table = rs.randn(P + room).astype(np.float32)
    theta = rs.randn(P).astype(np.float32)
    idx = np.array([0, room, room // 2, room, 0, room], np.int64)
    sign = np.array([1, -1, 0, 1, -1, 0], np.int8)
    out = eng.perturb(dev(theta), dev_table(table), dev(idx), dev(sign), SIGMA).cpu().numpy()
    assert out.tobytes() == onoise.perturb(theta, table, idx, sign, SIGMA).tobytes()


# ---- DSGD --------------------------------------------------------------------------------------------------------
def check_dsgd(theta0, g_used, theta_dev, out, hist=None):
    """theta bit-equal to the mirror fed the gradient the kernel used; out = (||d theta||, norm)."""
    P = theta0.size
    new, upd, norm, ambiguous = ref.dsgd_mirror(theta0, g_used, lc.DSGD_LR, lc.DSGD_SCALE)
    assert not ambiguous, "the inputs leave fl32(norm) to the summation order: choose others"
    got = theta_dev.cpu().numpy()
    assert got.tobytes() == new.tobytes(), "theta differs from the mirror in %d of %d" % ((got != new).sum(), P)
    if hist is not None:
        assert hist.cpu().numpy().tobytes() == got.tobytes()
    assert out[1] == norm or (np.isnan(out[1]) and np.isnan(norm))
    rel = abs(out[0] - upd) / upd if upd > 0 else abs(out[0])
    assert rel <= P * 2.0 ** -52, (out[0], upd)
    return rel


@pytest.mark.parametrize("P", lc.DSGD_P)
def test_dsgd_from_gradient_and_from_moments(eng, P):
    """fdr_dsgd_step_ex on both sides of the one-workgroup limit (65536) and with most of the workgroup idle."""
    theta, g = lc.dsgd_inputs(P)
    t = dev(theta)
    out = eng.dsgd_step_ex(t, dev(g), False, lc.DSGD_LR, lc.DSGD_SCALE).cpu().numpy()
    rel = check_dsgd(theta, g, t, out)
    theta, mom = lc.dsgd_moments_inputs(P)
    t, g_out = dev(theta), torch.full((P,), NAN, dtype=torch.float64, device="cuda")
    out = eng.dsgd_step_ex(t, dev(mom), True, lc.DSGD_LR, lc.DSGD_SCALE, g_out=g_out).cpu().numpy()
    gd = g_out.cpu().numpy()
    e = ref.rel_l2(gd, ref.grad_from_moments(mom, P))
    assert e <= TOL, e
    rel = max(rel, check_dsgd(theta, gd, t, out))
    print("DSGD P %d: theta bit-equal; ||d theta|| relative %.2e (bound %.2e); g from moments rel-L2 %.2e"
          % (P, rel, P * 2.0 ** -52, e))


@pytest.mark.parametrize("mode", ["zscore", "centred_rank"])
@pytest.mark.parametrize("P", [1, 257, 65537, 70001])
def test_fd_step_small_batches(eng, P, mode):
    """fdr_fd_step with few directions: g against the reference, theta bit-equal to the mirror of the device's own
    g, theta_hist bit-equal to theta; above 65536 columns dsgd_apply_cb_kernel's staging loop goes round twice.
    Two steps on the same workspace."""
    c = lc.make_case(3, P, 2)
    assert c.lane_lo == 0 and c.n_all == c.n_local
    if P > 65536:
        assert lc.fused_plan(3, P)[0] > 256
    d = Dev(c)
    g_ref = ref.grad(c.table, P, c.idx_dirs, c.coefs(mode))
    theta = lc.dsgd_inputs(P)[0]
    t = dev(theta)
    for _ in range(2):
        g = torch.full((P,), NAN, dtype=torch.float64, device="cuda")
        hist = torch.full((P,), NAN, dtype=torch.float32, device="cuda")
        out = eng.fd_step(d.table, d.idx, d.r_all, PR, d.sign, d.n2, 2, SIGMA, t, lc.DSGD_LR, lc.DSGD_SCALE,
                          mode=mode, g=g, theta_hist=hist).cpu().numpy()
        gd = g.cpu().numpy()
        e = ref.rel_l2(gd, g_ref)
        assert e <= TOL, e
        rel = check_dsgd(theta, gd, t, out, hist)
        theta = t.cpu().numpy()
    print("fd_step %s P %d: g rel-L2 %.2e, ||d theta|| relative %.2e" % (mode, P, e, rel))


def _bad_dirs(c, where, bad):
    idx_dirs = c.idx_dirs.copy()
    idx_dirs[where] = c.max_idx + 1 if bad == "past" else -1
    return idx_dirs


@pytest.mark.parametrize("kind", ["zero", "nan"])
@pytest.mark.parametrize("path,P", [("g", 257), ("g", 65537), ("moments", 257), ("moments", 65537),
                                    ("fd_step", 257), ("fd_step", 70001)])
def test_dsgd_leaves_theta_alone_without_a_norm(eng, path, P, kind):
    """A zero gradient and a NaN gradient: theta bit-unchanged, out[0] == 0, out[1] == 0 / NaN, on all three DSGD
    implementations; the step after it is a normal one."""
    theta = lc.dsgd_inputs(P)[0]
    t = dev(theta)
    hist = None
    if path == "fd_step":
        c = lc.make_case(3, P, 2, signs="zero") if kind == "zero" else lc.make_case(3, P, 2)
        d = Dev(c, None if kind == "zero" else _bad_dirs(c, 1, "past"))
        g = torch.full((P,), 1.0, dtype=torch.float64, device="cuda")
        hist = torch.full((P,), NAN, dtype=torch.float32, device="cuda")
        out = eng.fd_step(d.table, d.idx, d.r_all, PR, d.sign, d.n2, 2, SIGMA, t, lc.DSGD_LR, lc.DSGD_SCALE, g=g,
                          theta_hist=hist).cpu().numpy()
        gd = g.cpu().numpy()
        assert np.all(gd == 0) if kind == "zero" else np.all(np.isnan(gd))
    elif path == "g":
        g = np.zeros(P) if kind == "zero" else lc.dsgd_inputs(P)[1].copy()
        if kind == "nan":
            g[P // 2] = NAN
        out = eng.dsgd_step_ex(t, dev(g), False, lc.DSGD_LR, lc.DSGD_SCALE).cpu().numpy()
    else:
        mom = lc.dsgd_moments_inputs(P)[1].copy()
        if kind == "zero":
            mom[:2 * P] = 0.0
        else:
            mom[P // 2] = NAN
        g_out = torch.empty(P, dtype=torch.float64, device="cuda")
        out = eng.dsgd_step_ex(t, dev(mom), True, lc.DSGD_LR, lc.DSGD_SCALE, g_out=g_out).cpu().numpy()
    assert t.cpu().numpy().tobytes() == theta.tobytes()
    if hist is not None:
        assert hist.cpu().numpy().tobytes() == theta.tobytes()
    assert out[0] == 0.0
    assert out[1] == 0.0 if kind == "zero" else np.isnan(out[1])
    if path == "fd_step":   # the tickets of both launches were left at zero: a clean step on the same workspace
        c = lc.make_case(3, P, 2)
        d = Dev(c)
        g = torch.empty(P, dtype=torch.float64, device="cuda")
        out = eng.fd_step(d.table, d.idx, d.r_all, PR, d.sign, d.n2, 2, SIGMA, t, lc.DSGD_LR, lc.DSGD_SCALE,
                          g=g).cpu().numpy()
        assert ref.rel_l2(g.cpu().numpy(), ref.grad(c.table, P, c.idx_dirs, c.coefs("zscore"))) <= TOL
        check_dsgd(theta, g.cpu().numpy(), t, out)


# ---- out-of-range offsets ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", ["past", "negative"])
def test_bad_offset_perturb(eng, bad):
    """max_idx + 1 / -1 in one row: NaN in that row only, the others bit-equal to a run without it."""
    P, room = 300, 1000
    rs = np.random.RandomState(3)
    table, theta = rs.randn(P + room).astype(np.float32), rs.randn(P).astype(np.float32)
    idx = np.array([0, room, 17, room, 0, 500], np.int64)
    sign = np.array([1, -1, 1, 0, -1, 1], np.int8)
    tab, th = dev_table(table), dev(theta)
    clean = eng.perturb(th, tab, dev(idx), dev(sign), SIGMA).cpu().numpy()
    for row in (2, 3):   # a perturbed lane and a sign-0 lane
        bidx = idx.copy()
        bidx[row] = room + 1 if bad == "past" else -1
        out = eng.perturb(th, tab, dev(bidx), dev(sign), SIGMA).cpu().numpy()
        assert np.all(np.isnan(out[row]))
        keep = np.arange(6) != row
        assert out[keep].tobytes() == clean[keep].tobytes()


@pytest.mark.parametrize("bad", ["past", "negative"])
@pytest.mark.parametrize("lpd", [2, 5])
def test_bad_offset_poisons_the_gradient_only(eng, lpd, bad):
    """One bad row among 130 (3 chunks; the bad one in the second): every element of g (A and B) is NaN, the moments
    form's count and slots are untouched, and the next clean call on the same workspace equals the reference."""
    c = lc.make_case(130, 1000, lpd)
    assert lc.fused_plan(130, 1000)[2] == 3 and lc.grad_plan(130, 1000)[2] == 3
    good, poisoned = Dev(c), Dev(c, _bad_dirs(c, 70, bad))
    P = c.P
    coef = eng.fd_weights(good.r_all, PR, 0, good.sign, good.n2, lpd, SIGMA)
    assert np.all(np.isnan(eng.fd_grad(poisoned.table, poisoned.idx_dirs, coef, P).cpu().numpy()))
    g = eng.fd_grad(good.table, good.idx_dirs, coef, P).cpu().numpy()
    assert ref.rel_l2(g, ref.grad(c.table, P, c.idx_dirs, c.coefs("zscore"))) <= TOL
    for mode in lc.MODES:
        out = run_fused(eng, c, poisoned, mode)
        assert np.all(np.isnan(out[:P])), mode
        if mode == "moments":
            assert np.all(np.isnan(out[P:2 * P]))
            assert out[2 * P] == c.n_local
            np.testing.assert_array_equal(out[2 * P + 1:], expected_slots(c))
        assert fused_error(c, run_fused(eng, c, good, mode), mode) <= TOL, mode


@pytest.mark.parametrize("bad", ["past", "negative"])
def test_bad_offset_lambda(eng, bad):
    n, P, row = 65, 257, 40
    table, idx, sign, slot, drift, coef = lc.lambda_case(n, P)
    bidx = idx.copy()
    bidx[row] = lc.ROOM + 1 if bad == "past" else -1
    tab, ds, dl, dd, dc = dev_table(table), dev(sign), dev(slot), dev(drift), dev(coef)
    clean = eng.fd_lambda_norms(tab, dev(idx), ds, dl, SIGMA, dd, P).cpu().numpy()
    n2 = eng.fd_lambda_norms(tab, dev(bidx), ds, dl, SIGMA, dd, P).cpu().numpy()
    assert np.isnan(n2[row])
    keep = np.arange(n) != row
    assert n2[keep].tobytes() == clean[keep].tobytes()
    assert np.all(np.isnan(eng.fd_grad_lambda(tab, dev(bidx), ds, dl, dc, SIGMA, dd, P).cpu().numpy()))
    lam = ref.lambda_rows(table, P, idx, sign, slot, SIGMA, drift).astype(np.longdouble)
    g_ref = (coef.astype(np.longdouble)[:, None] * lam).sum(0)
    assert ref.rel_l2(eng.fd_grad_lambda(tab, dev(idx), ds, dl, dc, SIGMA, dd, P).cpu().numpy(), g_ref) <= TOL
