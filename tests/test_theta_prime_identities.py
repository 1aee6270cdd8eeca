"""The IEEE identities ParamSrc (csrc/fdr_common.h) rests on, checked in numpy f32 / f64.  No GPU.

The rollouts form theta' = fl32(t +/- fl32(sigma eps)) with the sign carried on sigma, a -0.0f step on an unperturbed
lane and the norm term as one f64 FMA.  That gives the two-sided form's bits if

  1  fl32((-sigma) eps) = -fl32(sigma eps)  and  t - x = t + (-x), bit for bit, signed zeros included;
  2  t + (-0.0f) = t bit for bit for every t (t + (+0.0f) is not: it turns -0.0f into +0.0f);
  3  the f64 product of two f32-valued doubles is exact, so fma(d, d, n2) -- one rounding of the exact n2 + d d --
     is the two-step n2 + fl64(d d); and (-0.0)^2 = +0.0, the unperturbed lane's "n2 += 0.0".

Over 10^6 seeded (t, sigma, eps) triples plus the specials the GPU test plants (zeros of both signs, denormals, steps
that round to a denormal or to zero); the exactness claims against fractions.Fraction on a few thousand of them.
"""
from fractions import Fraction

import numpy as np
import pytest

N = 1_000_000


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def triples():
    rs = np.random.RandomState(20240)
    # magnitudes from denormal to large: a normal draw times 2^k, k in [-140, 40] for a tenth of them
    def draw(n):
        v = rs.randn(n).astype(np.float32)
        k = np.where(rs.rand(n) < 0.1, rs.randint(-140, 41, size=n), 0)
        return np.ldexp(v, k).astype(np.float32)
    t, eps = draw(N), draw(N)
    sigma = np.where(rs.rand(N) < 0.5, np.float32(0.02), np.abs(draw(N))).astype(np.float32)
    sp = np.array([0.0, -0.0, 1e-40, -1e-40, 1.4e-45, -1.4e-45, 1e-37, -1e-37, 1.17549435e-38, 1.0, -1.0, 3.4e38,
                   0.02, 5e-37, 7e-44], np.float32)
    g = np.array(np.meshgrid(sp, np.abs(sp), sp, indexing="ij")).reshape(3, -1)
    t = np.concatenate([t, g[0]])
    sigma = np.concatenate([sigma, g[1]])
    eps = np.concatenate([eps, g[2]])
    with np.errstate(over="ignore", invalid="ignore"):
        keep = np.isfinite(sigma * eps) & np.isfinite(t + sigma * eps) & np.isfinite(t - sigma * eps)
    return t[keep], sigma[keep], eps[keep]


def test_signed_sigma_gives_the_two_sided_bits(triples):
    t, sigma, eps = triples
    assert t.size >= N and t.dtype == sigma.dtype == eps.dtype == np.float32
    st = (sigma * eps).astype(np.float32)
    stn = ((-sigma) * eps).astype(np.float32)
    assert np.array_equal(bits32(stn), bits32(-st))                       # the product's rounding is symmetric
    assert np.array_equal(bits32(t - st), bits32(t + stn))                # lane sign -1
    den = (st != 0) & (np.abs(st) < np.float32(1.17549435e-38))
    assert den.sum() > 100 and (bits32(st) << 1 == 0).sum() > 100         # denormal and zero steps are in the set


def test_minus_zero_step_returns_t_itself(triples):
    t = triples[0]
    mz = np.float32(-0.0)
    assert np.array_equal(bits32(t + mz), bits32(t))
    nz = np.array([-0.0], np.float32)
    assert bits32(nz + mz)[0] == 0x80000000 and bits32(nz + np.float32(0.0))[0] == 0   # what +0.0f would break
    assert (bits32(t) == 0x80000000).sum() > 0


def test_f64_square_of_an_f32_is_exact_and_fma_is_the_two_step_sum(triples):
    t, sigma, eps = triples
    st = (sigma * eps).astype(np.float32)
    rs = np.random.RandomState(3)
    pick = np.concatenate([rs.randint(0, N, size=3000), np.arange(N, st.size)[::7]])
    d = st[pick].astype(np.float64)
    sq = d * d
    n2 = np.abs(rs.randn(pick.size)) * np.ldexp(1.0, rs.randint(-80, 10, size=pick.size))
    two_step = n2 + sq
    for di, si, ni, ti in zip(d.tolist(), sq.tolist(), n2.tolist(), two_step.tolist()):
        exact = Fraction(di) * Fraction(di)
        assert Fraction(si) == exact                                       # no rounding in d * d
        assert float(Fraction(ni) + exact) == ti                           # fma(d, d, n2): one correct rounding
    # all of them, without Fraction: a 24-bit significand squared fits 48 bits (and the exponent range of f64)
    dd = st.astype(np.float64)
    m, _ = np.frexp(dd)
    assert np.all(np.ldexp(m, 24) == np.rint(np.ldexp(m, 24)))
    assert np.all((dd * dd != 0) | (dd == 0))                              # no underflow: |d| >= 2^-149
    mz = np.array([-0.0], np.float64)
    assert bits64(mz * mz)[0] == 0                                         # unperturbed lane: n2 += +0.0
    assert np.array_equal(bits64(n2 + (mz * mz)[0]), bits64(n2))
    assert np.isnan(np.float64("nan") + sq[:4]).all()                      # an out-of-range lane's NaN norm stays
