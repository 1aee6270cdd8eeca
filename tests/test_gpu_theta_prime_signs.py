"""theta' with the lane's sign carried on sigma (ParamSrc, csrc/fdr_common.h): the same bits as numpy's two-sided form
on the smallest lane sets at which that form can go wrong, with the values planted where the identities it rests on
(tests/test_theta_prime_identities.py) have their edges.

Lane sets: 2 to 5 lanes, so one to three pair waves -- waves of perturbed lanes only, of unperturbed lanes only and
mixed ones (both sides of any per-wave "no unperturbed lane" shortcut a loader may take), an idle half that shadows
its partner, and an out-of-range lane beside a perturbed one.
Planted: -0.0, +0.0 and a denormal in theta (in the first layer, the second and the head); +0.0, -0.0 and an eps whose
sigma * eps is denormal in every table row the lanes use, the zeros under theta's own zeros.

Driven as tests/test_gpu_theta_prime.py drives fdr_diag_theta_prime and the real kernels, at that file's tolerances.
"""
import numpy as np
import pytest
import torch

from test_gpu_theta_prime import DEV, IMPLS, SIGMA, TABLE_SIZE, Case, _roll, bits, dev

pytestmark = pytest.mark.gpu

DENORMAL = np.float32(1e-40)
EPS_DENORMAL_STEP = np.float32(1e-37)     # fl32(0.02 * 1e-37) = 2e-39 < 2^-126
_CASES = {}


class SignCase(Case):
    """test_gpu_theta_prime.Case with planted values; `offsets`: the table offsets the lane sets use."""

    def __init__(self, name):
        super().__init__(name)
        P = self.P
        self.theta = self.theta.copy()
        self.table = self.table.copy()
        self.offsets = [self.mid, 0, self.max_idx, self.mid + 17, 64]
        self.zeros_at = []
        for p0 in (1, P // 2, P - 4):          # first layer, second layer, head
            self.theta[p0:p0 + 3] = [-0.0, 0.0, DENORMAL]
            self.zeros_at.append(p0)
        for off in self.offsets:
            for p0 in (1, P // 2, P - 4):
                self.table[off + p0:off + p0 + 3] = [0.0, -0.0, EPS_DENORMAL_STEP]
            self.table[off + 8:off + 11] = [-0.0, 0.0, -EPS_DENORMAL_STEP]
        self.buf[P:P + TABLE_SIZE] = dev(self.table)
        self.theta_d = dev(self.theta)
        step = np.float32(SIGMA) * EPS_DENORMAL_STEP
        assert step != 0 and abs(step) < np.float32(1.17549435e-38)

    def sets(self):
        """name -> (sign, idx)"""
        o = self.offsets
        s = {"plus_zero": ([1, 0], o[:2]), "zero_minus": ([0, -1], o[:2]), "zero_zero": ([0, 0], o[:2]),
             "plus_minus": ([1, -1], [o[0], o[0]]), "three": ([1, -1, 1], o[:3]),
             "five": ([1, -1, 0, 1, -1], o), "out_of_range": ([1, -1], [self.max_idx + 1, o[0]]),
             "out_of_range_neg": ([-1, 1], [-1, o[2]])}
        return {k: (np.array(sg, np.int8), np.array(ix, np.int64)) for k, (sg, ix) in s.items()}


def case(name):
    if name not in _CASES:
        _CASES[name] = SignCase(name)
    return _CASES[name]


_ORACLE = {}


def oracle(c, name, key, idx, sign):
    if (name, key) not in _ORACLE:
        _ORACLE[(name, key)] = c.oracle(idx, sign)
    return _ORACLE[(name, key)]


@pytest.fixture(scope="module")
def eng():
    from fdr import engine
    return engine


def test_planted_values_reach_the_oracle_rows():
    c = case("cartpole")
    sign, idx = c.sets()["plus_minus"]
    ref = c.thetas(idx, sign)
    p0 = c.zeros_at[0]
    # theta = -0.0 over eps = +0.0: the + lane rounds to +0.0, the - lane keeps -0.0
    assert bits(ref[0, p0:p0 + 1])[0] == 0 and bits(ref[1, p0:p0 + 1])[0] == 0x80000000
    assert ref[0, p0 + 2] != c.theta[p0 + 2] and abs(ref[0, p0 + 2]) < 1.17549435e-38      # denormal + denormal


@pytest.mark.parametrize("loader", ["lane", "pair"])
@pytest.mark.parametrize("name", ["cheetah", "cartpole"])
def test_loader_theta_prime_bitwise_on_small_sign_sets(eng, name, loader):
    c = case(name)
    reads_ref = None
    for key, (sign, idx) in c.sets().items():
        L = len(idx)
        ok = c.in_range(idx)
        ref = c.thetas(idx, sign)
        out, reads, counted, n2 = [t.cpu().numpy() for t in eng.theta_prime(c.spec(eng), c.lanes(eng, idx, sign), L,
                                                                              loader)]
        diff = np.argwhere(out.view(np.int32) != ref.view(np.int32))
        print("%s/%s/%s: %d of %d theta' elements differ" % (name, loader, key, len(diff), out.size))
        assert len(diff) == 0, (key, diff[:8])
        for i in np.nonzero((sign == 0) | ~ok)[0]:          # unperturbed (or out of range): theta itself, -0.0 kept
            assert np.array_equal(out[i].view(np.int32), c.theta.view(np.int32)), key
            assert all(bits(out[i, p:p + 1])[0] == 0x80000000 for p in c.zeros_at), key
        # read and counted as the two-sided form did: every element loaded, and in norm2 exactly once; the loads do
        # not depend on the signs
        assert reads.min() >= 1 and np.all(counted == 1), key
        if reads_ref is None:
            reads_ref = reads[0]
        assert np.all(reads == reads_ref[None, :]), key
        ref_n2 = c.norm2(idx, sign)
        assert np.all(np.isnan(n2[~ok])), key
        np.testing.assert_allclose(n2[ok], ref_n2[ok], rtol=1e-9, atol=0, err_msg=key)
        assert np.all(n2[ok & (sign == 0)] == 0.0), key
        if not ok.all():                                    # the out-of-range lane's neighbour is untouched
            j = int(np.nonzero(ok)[0][0])
            alone = eng.theta_prime(c.spec(eng), c.lanes(eng, idx[j:j + 1], sign[j:j + 1]), 1, loader)
            assert np.array_equal(alone[0].cpu().numpy()[0].view(np.int32), out[j].view(np.int32)), key
            assert alone[3].cpu().numpy()[0] == n2[j], key
    assert c.guards_intact()


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("name", ["cheetah", "cartpole"])
def test_rollout_kernels_on_small_sign_sets(eng, name, impl):
    c = case(name)
    for key, (sign, idx) in c.sets().items():
        L = len(idx)
        ok = c.in_range(idx)
        idx2, sign2 = c.legal(idx, sign)        # the out-of-range lanes as plain unperturbed lanes
        idx2[~ok] = c.mid
        try:
            eng.context().set_rollout_impl(impl)
            a = _roll(eng, c, c.lanes(eng, idx, sign), L)
            b = _roll(eng, c, c.lanes(eng, idx2, sign2), L) if not ok.all() else a
        finally:
            eng.context().set_rollout_impl("auto")
        r_ret, r_ent, r_steps, _ = oracle(c, name, key, idx, sign)
        r_n2 = c.norm2(idx, sign)
        ret, ent, steps, n2 = (a.reward.cpu().numpy(), a.entropy.cpu().numpy(), a.timesteps.cpu().numpy(),
                               a.norm2.cpu().numpy())
        print("%s/%s/%s: max |ret - ref| %.3g, max |ent - ref| %.3g" % (
            name, impl, key, np.abs(ret[ok] - r_ret[ok]).max(), np.abs(ent[ok] - r_ent[ok]).max()))
        np.testing.assert_allclose(ret[ok], r_ret[ok], rtol=1e-4, atol=1e-4, err_msg=key)
        np.testing.assert_allclose(ent[ok], r_ent[ok], rtol=1e-5, atol=1e-5, err_msg=key)
        assert np.array_equal(steps, r_steps), key
        np.testing.assert_allclose(n2[ok], r_n2[ok], rtol=1e-9, atol=0, err_msg=key)
        assert np.all(np.isnan(n2[~ok])) and np.all(n2[ok & (sign == 0)] == 0.0), key
        if not ok.all():                        # every lane bit-equal to the run without an out-of-range offset
            for f in ("reward", "entropy", "timesteps"):
                assert torch.equal(getattr(a, f), getattr(b, f)), (key, f)
            okt = torch.as_tensor(ok, device=DEV)
            assert torch.equal(a.norm2[okt], b.norm2[okt]) and torch.all(b.norm2[~okt] == 0.0), key
    assert c.guards_intact()
