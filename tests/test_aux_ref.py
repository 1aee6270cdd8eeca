"""CPU: pins tests/aux_ref.py and tests/aux_cases.py, the yardsticks of the auxiliary-kernel edge tests.

  * dist_ref against G9 (the reference's own math_helpers) and oracle.novelty at their f32 tolerance 1e-5;
  * the f64 floor: the kernel's summation order restated in numpy float64 (aux_ref.dist_f64) against dist_ref at every
    distance case, k_cpu = max |d64 - d_ref| / (2^-53 scale); it must stay <= aux_ref.K_CPU <= 4;
  * every non-tie case separates its two smallest reference distances by more than twice the device bound, so the
    device argmin is determined; every tie case has bit-equal duplicates below every other distance;
  * vbn_ref against torch CPU float64 train mode, and against the torch f32 case of test_gpu_api.py at 1e-5;
  * the torch f32 floor of BN1 / BN2 over the BN cases (aux_ref.BN_F32_FLOOR);
  * the merge order case differs between lane order and reversed order in at least one bit.
"""
import numpy as np
import pytest
import torch
import torch.nn as nn

import aux_cases as ac
import aux_ref as ar
from oracle import novelty as on
from oracle import policies as opol


# ---- distances ----------------------------------------------------------------------------------------------------
def test_dist_ref_matches_reference_golden(golden):
    g = golden("g9_novelty.npz")
    for kind, a, b in (("tvd", "cat_a", "cat_b"), ("l2", "cat_a", "cat_b"), ("w2", "gau_a", "gau_b")):
        d, scale = ar.dist_ref(g[a], g[b], kind)
        np.testing.assert_allclose(d.astype(np.float64), g[kind], rtol=1e-5)
        assert np.all(scale >= d)
        mn, am = ar.novelty_ref(d)
        assert abs(float(mn) - float(g["nov_" + kind])) <= 1e-5 * abs(float(g["nov_" + kind]))
        assert am == int(np.argmin(g[kind]))
    for i, row in enumerate(g["pair_tvd"]):
        d, _ = ar.dist_ref(g["cat_b"][i], g["cat_b"], "tvd")
        np.testing.assert_allclose(d.astype(np.float64), row, rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("name", [n for n in ac.DIST_CASES if "near" not in n and "tie" not in n])
def test_dist_ref_matches_oracle(name):
    c = ac.dist_case(name)
    for a in c["S"][:3]:
        d, _ = ar.dist_ref(a, c["B"], c["kind"])
        np.testing.assert_allclose(d.astype(np.float64), on.DISTANCES[c["kind"]](a, c["B"]), rtol=1e-5)


def test_novelty_ref_follows_numpy():
    nan = float("nan")
    assert ar.novelty_ref([3.0, 1.0, 1.0, 2.0]) == (1.0, 1)
    mn, am = ar.novelty_ref([3.0, nan, 0.5, nan])
    assert np.isnan(mn) and am == 1
    for kind in ac.KINDS:
        c = ac.nan_case(kind, "strategy")
        rows = [ar.dist_ref(a, c["B"], kind)[0] for a in c["S"]]
        assert np.isnan(rows[1]).all() and np.isfinite(rows[0]).all() and np.isfinite(rows[2]).all()
        c = ac.nan_case(kind, "archive")
        for a in c["S"]:
            d = ar.dist_ref(a, c["B"], kind)[0]
            assert sorted(np.nonzero(np.isnan(d))[0]) == sorted(ac.NAN_ARCHIVE_ROWS)
            assert ar.novelty_ref(d)[1] == min(ac.NAN_ARCHIVE_ROWS)


def test_f64_floor_of_the_kernels_order():
    worst = dict.fromkeys(ac.KINDS, 0.0)
    for name in ac.DIST_CASES:
        c = ac.dist_case(name)
        for a in c["S"][:8]:
            d, scale = ar.dist_ref(a, c["B"], c["kind"])
            worst[c["kind"]] = max(worst[c["kind"]], ar.k_of(ar.dist_f64(a, c["B"], c["kind"]), d, scale))
    print("k_cpu per kind: " + ", ".join("%s %.2f" % kv for kv in sorted(worst.items())))
    assert max(worst.values()) <= ar.K_CPU <= 4.0, worst
    assert ar.K_DEV == 8 * ar.K_CPU


@pytest.mark.parametrize("name", ac.DIST_CASES)
def test_argmin_is_determined(name):
    c = ac.dist_case(name)
    for i, a in enumerate(c["S"]):
        d, scale = ar.dist_ref(a, c["B"], c["kind"])
        bound = ar.K_DEV * ar.U53 * scale
        if c["tie"] is None:
            if len(d) > 1:
                o = np.argsort(d)
                assert d[o[1]] - d[o[0]] > 2 * (bound[o[0]] + bound[o[1]]), (name, i)
        else:
            lo = c["tie"]
            hi = [h for h in range(len(d)) if h != lo and np.array_equal(c["B"][h], c["B"][lo])]
            assert len(hi) == 1 and d[hi[0]] == d[lo]
            rest = np.delete(d, [lo, hi[0]])
            assert np.all(rest - d[lo] > 2 * bound.max()), (name, i)
            assert (d[lo] == 0) == (i == 0)


# ---- Welford ------------------------------------------------------------------------------------------------------
def test_merge_order_case_is_order_sensitive():
    o = ac.ORDER_CASE
    acc, mean, m2, count = ac.merge_case(o["dim"], o["n"], o["start"], o["zeros"])
    fwd = ar.welford_ref(o["dim"], acc, zip(mean, m2, count))
    rev = ar.welford_ref(o["dim"], acc, zip(mean[::-1], m2[::-1], count[::-1]))
    assert fwd.count == rev.count == o["start"] + int(count.sum())
    assert np.any(fwd.mean_.view(np.uint32) != rev.mean_.view(np.uint32)) or \
        np.any(fwd.m2.view(np.uint32) != rev.m2.view(np.uint32))


def test_merge_cases_cover_the_rounded_counts():
    for start in (2 ** 24 + 1, 2 ** 31 + 5):
        assert int(np.float32(start)) != start                  # (float)c rounds
    acc, mean, m2, count = ac.merge_case(65, 300, 2 ** 31 + 5, "ends")
    assert count[0] == 0 and count[150] == 0 and count[-1] == 0 and (count > 0).sum() == 297
    assert acc[2] + int(count.sum()) > 2 ** 31
    assert np.abs(mean).min() < 2e-3 and np.abs(mean).max() > 5e3


# ---- BN refresh ---------------------------------------------------------------------------------------------------
def _torch_pass(theta, x, rm, rv, momentum, dtype, passes=1):
    """The reference model in train mode (oracle.policies.build_model) -> per pass [(rm, rv)] of the three BNs."""
    n_in = x.shape[1]
    model = opol.build_model("discrete", n_in, ar.vbn_n_act(theta.size, n_in)).to(dtype)
    nn.utils.vector_to_parameters(torch.as_tensor(theta).to(dtype), model.parameters())
    bns = [m for m in model if isinstance(m, nn.BatchNorm1d)]
    off = 0
    for m in bns:
        C = m.num_features
        m.momentum = momentum
        m.running_mean.copy_(torch.as_tensor(rm[off:off + C]).to(dtype))
        m.running_var.copy_(torch.as_tensor(rv[off:off + C]).to(dtype))
        off += C
    model.train()
    out = []
    threads = torch.get_num_threads()
    torch.set_num_threads(1)        # f32 sums depend on how they are split over threads: one thread, one answer
    try:
        with torch.no_grad():
            for _ in range(passes):
                model(torch.as_tensor(x).to(dtype))
                out.append([(m.running_mean.numpy().copy(), m.running_var.numpy().copy()) for m in bns])
    finally:
        torch.set_num_threads(threads)
    return out


def _flat(stats):
    return np.concatenate([s[0] for s in stats]).astype(np.float32), np.concatenate([s[1] for s in stats]).astype(np.float32)


@pytest.mark.parametrize("name", sorted(ac.VBN_CASES))
def test_vbn_ref_matches_torch_f64(name):
    theta, x, rm, rv, momentum = ac.vbn_case(name)
    want = _torch_pass(theta, x, rm, rv, momentum, torch.float64)[0]
    for (nm, nv, sm, sv), (tm, tv) in zip(ar.vbn_ref(theta, x, rm, rv, momentum), want):
        assert np.all(np.abs(nm - tm) <= 1e-10 * sm + 1e-300) and np.all(np.abs(nv - tv) <= 1e-10 * sv + 1e-300)


def test_vbn_ref_matches_the_torch_f32_case():
    """The inputs of test_gpu_api.py::test_compute_vbn_on_device_vs_torch_train_mode, at its tolerance."""
    torch.manual_seed(124)
    ref = opol.TorchPolicy("discrete", 4, 2, seed=124)
    theta = ref.get_flat()
    buf = (np.random.RandomState(3).randn(500, 4) * 2 + 0.5).astype(np.float32)
    rm, rv = np.zeros(132, np.float32), np.ones(132, np.float32)
    ref.model.train()
    for _ in range(2):
        with torch.no_grad():
            ref.model(torch.as_tensor(buf))
        got = ar.vbn_ref(theta, buf, rm, rv, 0.1)
        rm, rv = _flat(got)
        for (nm, nv, _, _), m in zip(got, [m for m in ref.model if isinstance(m, nn.BatchNorm1d)]):
            np.testing.assert_allclose(m.running_mean.numpy(), nm, rtol=1e-5, atol=1e-6)
            np.testing.assert_allclose(m.running_var.numpy(), nv, rtol=1e-5, atol=1e-6)


def test_torch_f32_floor_of_the_hidden_bns():
    """torch's CPU f32 train-mode pass against vbn_ref, two passes per case (the second from the f32 stats the first
    left), in units of 2^-24 scale, per group of cases (aux_cases.vbn_group) and hidden BN.  Single-threaded: with
    more threads torch splits its f32 sums and the floor of the "cols" group moves by a factor of 8."""
    worst = {g: {1: 0.0, 2: 0.0} for g in ar.BN_F32_FLOOR}
    for name in sorted(ac.VBN_CASES):
        theta, x, rm, rv, momentum = ac.vbn_case(name)
        w = worst[ac.vbn_group(name)]
        for stats in _torch_pass(theta, x, rm, rv, momentum, torch.float32, passes=2):
            want = ar.vbn_ref(theta, x, rm, rv, momentum)
            for i in (1, 2):
                w[i] = max((w[i],) + ar.vbn_k(stats[i][0], stats[i][1], want[i]))
            rm, rv = _flat(stats)
    print("torch f32 floor, units of 2^-24 scale: %r" % worst)
    for g in worst:
        for i in (1, 2):
            assert worst[g][i] <= ar.BN_F32_FLOOR[g][i], worst
