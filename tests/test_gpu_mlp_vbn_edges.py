"""GPU: DiscretePolicy.compute_vbn on the device (fdr_bn_refresh, csrc/fdr_mlp_vbn.hip) at its edges, against the
float64 restatement aux_ref.vbn_ref.  Cases: aux_cases.VBN_CASES -- n = 2 (the smallest legal batch), 3, 255 / 256 / 257
(col_stats_kernel's 256-thread stride), 1000; n_in 1, 4, 63, 64; a constant input column (batch variance 0), a column
of mean 1e4 and std 1, a hidden unit dead over the whole batch; momentum 0.1, 0 and 1.  The running stats start from
non-trivial values and every case runs twice, the second pass from the stats the first left.

Bounds, in units of 2^-24 scale (scale = |momentum stat| + |(1 - momentum) old|, from vbn_ref):
  BN0 (statistics of x itself, accumulated in f64): 3, derived -- one rounding of the f64 stat to f32 and three f32
      operations (two products, one sum);
  BN1 / BN2 (they see f32 hidden activations): 4 x the floor the installed torch's CPU f32 train-mode pass shows
      against vbn_ref over the same cases (aux_ref.BN_F32_FLOOR, per group of cases; test_aux_ref.py measures it).
The workspace passed is exactly fdr_bn_refresh_workspace_bytes(n) bytes of a NaN-filled buffer; what follows stays NaN.

Measured on an MI355X (each case prints its own): BN0 <= 1.82; BN1 / BN2 plain cases 2.18 / 10.97 (allowed 17.6 / 43.6),
cases with a constant or mean-1e4 column 4553 / 851 (allowed 446400 / 130400: there the floor is torch's f32 batch
statistics of those columns, which the kernel's f64 statistics beat by far, so for these cases the hidden-layer bound
says little; BN0, the exact-zero assertions of test_degenerate_columns and the plain cases carry the check).
"""
import ctypes

import numpy as np
import pytest
import torch

import aux_cases as ac
import aux_ref as ar

pytestmark = pytest.mark.gpu
GUARD = 1024        # floats after the workspace
NAN = float("nan")


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from fdr import engine
    return engine


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def refresh(eng, n_in, theta, x, rm, rv, momentum, n=None, ws_short=0):
    """fdr_bn_refresh through ctypes with a workspace of exactly the queried size inside a NaN-filled buffer.
    -> (rc, rm, rv) with the stats read back."""
    n = x.shape[0] if n is None else n
    nb = eng.lib.fdr_bn_refresh_workspace_bytes(max(n, 2))
    assert nb % 4 == 0
    buf = torch.full((nb // 4 + GUARD,), NAN, dtype=torch.float32, device="cuda")
    th, xd, rmd, rvd = dev(theta), dev(x), dev(rm), dev(rv)
    pd = eng.PolicySpec("discrete", n_in, ac.VBN_N_ACT, theta.size).desc(None, None)
    rc = eng.lib.fdr_bn_refresh(None, ctypes.byref(pd), eng._p(th), eng._p(xd), n, float(momentum), eng._p(rmd), eng._p(rvd),
                                eng._p(buf), nb - ws_short, eng._stream(xd.device))
    torch.cuda.synchronize()
    assert torch.isnan(buf[nb // 4:]).all(), "write past the workspace"
    return rc, rmd.cpu().numpy(), rvd.cpu().numpy()


def layer_slices(n_in):
    return [slice(0, n_in), slice(n_in, n_in + 64), slice(n_in + 64, n_in + 128)]


@pytest.mark.parametrize("name", sorted(ac.VBN_CASES))
def test_bn_refresh_against_vbn_ref(eng, name):
    theta, x, rm, rv, momentum = ac.vbn_case(name)
    n, n_in = x.shape
    floor = ar.BN_F32_FLOOR[ac.vbn_group(name)]
    allowed = [ar.BN0_K, ar.BN_MARGIN * floor[1], ar.BN_MARGIN * floor[2]]
    for p in range(2):
        rc, gm, gv = refresh(eng, n_in, theta, x, rm, rv, momentum)
        eng.check(rc, "fdr_bn_refresh")
        want = ar.vbn_ref(theta, x, rm, rv, momentum)
        ks = [ar.vbn_k(gm[s], gv[s], want[i]) for i, s in enumerate(layer_slices(n_in))]
        print("%s pass %d: k (mean, var) BN0 %.2f %.2f  BN1 %.2f %.2f  BN2 %.2f %.2f; allowed %.0f / %.1f / %.1f"
              % ((name, p) + ks[0] + ks[1] + ks[2] + tuple(allowed)))
        for i in range(3):
            assert max(ks[i]) <= allowed[i], (name, p, i, ks[i], allowed[i])
        if momentum == 0.0:         # the running stats are bit-unchanged
            np.testing.assert_array_equal(bits(gm), bits(rm))
            np.testing.assert_array_equal(bits(gv), bits(rv))
        if momentum == 1.0:         # the old stats are discarded
            rc, gm2, gv2 = refresh(eng, n_in, theta, x, (rm * 3 + 1).astype(np.float32), (rv * 5).astype(np.float32), momentum)
            eng.check(rc, "fdr_bn_refresh")
            np.testing.assert_array_equal(bits(gm2), bits(gm))
            np.testing.assert_array_equal(bits(gv2), bits(gv))
        rm, rv = gm, gv


def test_degenerate_columns(eng):
    """A constant input column has batch variance exactly 0 (the f64 sum of n equal f32 values is exact), and a hidden
    unit dead over the whole batch has mean = var = 0: their running stats are fl32(fl32(1 - momentum) * old)."""
    keep = np.float32(1.0) - np.float32(0.1)
    theta, x, rm, rv, momentum = ac.vbn_case("n255_const")
    rc, gm, gv = refresh(eng, 4, theta, x, rm, rv, momentum)
    eng.check(rc, "fdr_bn_refresh")
    assert gv[1] == np.float32(keep * rv[1])
    theta, x, rm, rv, momentum = ac.vbn_case("n257_dead")
    rc, gm, gv = refresh(eng, 4, theta, x, rm, rv, momentum)
    eng.check(rc, "fdr_bn_refresh")
    assert gm[4 + 5] == np.float32(keep * rm[4 + 5]) and gv[4 + 5] == np.float32(keep * rv[4 + 5])


def test_refusals_leave_the_stats_untouched(eng):
    _lib = eng._lib
    theta, x, rm, rv, momentum = ac.vbn_case("n256_big")

    def refused(rc, code, text, gm, gv, rm=rm, rv=rv):
        assert rc == code, (rc, code)
        assert text in eng.lib.fdr_last_error().decode(), eng.lib.fdr_last_error()
        np.testing.assert_array_equal(bits(gm), bits(rm))
        np.testing.assert_array_equal(bits(gv), bits(rv))
    rc, gm, gv = refresh(eng, 4, theta, x, rm, rv, momentum, n=1)
    refused(rc, _lib.FDR_ERR_INVALID, "train-mode BatchNorm needs n >= 2 samples", gm, gv)
    rc, gm, gv = refresh(eng, 4, theta, x, rm, rv, momentum, ws_short=1)
    refused(rc, _lib.FDR_ERR_WORKSPACE, "bn refresh workspace too small", gm, gv)
    rs = np.random.RandomState(65)
    P65 = ar.opol.num_params("discrete", 65, ac.VBN_N_ACT)
    th65, x65 = rs.randn(P65).astype(np.float32), rs.randn(8, 65).astype(np.float32)
    rm65, rv65 = rs.randn(65 + 128).astype(np.float32), (1 + rs.rand(65 + 128)).astype(np.float32)
    rc, gm, gv = refresh(eng, 65, th65, x65, rm65, rv65, momentum)
    refused(rc, _lib.FDR_ERR_UNSUPPORTED, "n_in must be in 1..64", gm, gv, rm65, rv65)
    rc, gm, gv = refresh(eng, 4, theta, x, rm, rv, momentum)       # and the same call, unrefused, is served
    eng.check(rc, "fdr_bn_refresh")
    assert np.any(bits(gm) != bits(rm))
