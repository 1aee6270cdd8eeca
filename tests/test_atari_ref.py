"""CPU: the float64 AtariPolicy reference (tests/atari_ref.py) and the edge-parity cases (tests/atari_cases.py) are
trustworthy before any device runs them.

  * the reference reproduces the goldens G11 (forward) and G16 (compute_vbn) to f32 rounding and agrees with the f32
    oracle on the inputs of the earlier GPU tests;
  * every case is conditioned: each visited state's entropy lies in [0.2, 0.98] ln(n_act) (a saturated softmax hides a
    wrong weight: (1, 0, 0, ...) either way);
  * the comparison can see an indexing error: rolling ANY parameter section, or any running-stat block, by one element
    moves the features or the probabilities by at least 100 x the tolerance the device is held to;
  * no decision of any case is closer to its boundary than 100 x the probability tolerance, so actions, integer
    rewards and steps of the device must be exact (zero decisions excluded; the cap would be 1 %).

Bounds "to f32 rounding": an f32 dot product of K terms in any order is within about sqrt(K) 2^-24 of the exact one
relative to the size of its terms; K = 256, 256, 2592 -> 1e-6, 1e-6, 3e-6 relative to the largest feature / logit.
The goldens are f32 torch-CPU outputs, so the reference may differ from them by that: features 4e-6 relative to the
largest feature (two stacked convs, factor 2), probabilities 2e-6 absolute.
"""
import numpy as np
import pytest

import atari_cases as ac
import atari_ref as ar
from oracle import atari as oa

FEAT_F32 = 4e-6
PROB_F32 = 2e-6
NAMES = [c["name"] for c in ac.CASES]


# ---- the reference against the goldens and the oracle ---------------------------------------------------------------
def test_reference_reproduces_forward_golden(golden):
    g = golden("g11_atari.npz")
    A = int(g["A"])
    theta = oa.init_theta(A, 124)
    probs, feat = ar.forward(ar.unflatten(theta, A), ar.split_bn(g["rm"], g["rv"]), g["frames"])
    d_feat = ac.feat_distance(g["feat"], feat.numpy())
    d_prob = float(np.abs(g["probs"] - probs.numpy()).max())
    print("G11: feat %.2e  probs %.2e" % (d_feat, d_prob))
    assert d_feat <= FEAT_F32
    assert d_prob <= PROB_F32
    np.testing.assert_allclose(ar.features(ar.unflatten(theta, A), ar.split_bn(g["rm"], g["rv"]), g["frames"]).numpy(),
                               feat.numpy(), rtol=0, atol=0)


def test_reference_reproduces_vbn_golden(golden):
    g = golden("g16_atari_vbn.npz")
    A, P = int(g["A"]), int(g["P"])
    flat = (np.random.RandomState(int(g["param_seed"])).randn(P) * float(g["param_scale"])).astype(np.float32)
    p = ar.unflatten(flat, A)
    rm, rv = g["rm"], g["rv"]
    for tag in ("a", "a2"):
        # chained as the golden was: the f32 stats of the first call feed the second
        rm, rv = ar.compute_vbn(p, rm, rv, g["frames"], float(g["momentum"]))
        np.testing.assert_allclose(rm, g[tag + "_rm"], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(rv, g[tag + "_rv"], rtol=1e-5, atol=1e-6)
        rm, rv = g[tag + "_rm"], g[tag + "_rv"]


@pytest.mark.parametrize("E,det", [(2, 0), (1, 1)])
def test_reference_agrees_with_oracle_on_earlier_rollout_inputs(E, det):
    """tests/test_gpu_atari.py::test_rollout_vs_oracle's inputs."""
    A, T = 6, 3
    theta = oa.init_theta(A, 124)
    table = np.random.RandomState(124).randn(1 << 21).astype(np.float32)
    idx = np.array([11, 400000, 1000000], np.int64)
    sign = np.array([1, -1, 1], np.int8)
    dets = np.full(3, det, bool)
    rm, rv = np.zeros(304, np.float32), np.ones(304, np.float32)
    args = (theta, table, idx, sign, 0.02, A, E, T, 21, 9, rm, rv)
    ref = ar.evaluate_lanes(*args, deterministic=dets, lane_offset=3)
    orc = oa.evaluate_lanes(*args, deterministic=dets, lane_offset=3, record=True)
    assert np.abs(orc["probs"] - ref["probs"]).max() <= PROB_F32
    assert np.abs(orc["ent"] - ref["ent"]).max() <= PROB_F32 * np.log(A)
    np.testing.assert_array_equal(orc["actions"], ref["actions"])
    np.testing.assert_array_equal(orc["ret"], ref["ret"])
    np.testing.assert_array_equal(orc["norm2"], ref["norm2"])


def test_reference_agrees_with_oracle_on_earlier_vbn_inputs():
    """tests/test_gpu_atari_vbn.py::test_compute_vbn_matches_oracle_larger_buffer's inputs, under its _check rule."""
    A, n = 4, 37
    rs = np.random.RandomState(3)
    flat = (0.03 * rs.randn(oa.num_params(A))).astype(np.float32)
    rm = (rs.randn(304) * 5).astype(np.float32)
    rv = (1.0 + rs.rand(304) * 20).astype(np.float32)
    frames = rs.randint(0, 256, size=(n, 4, 84, 84)).astype(np.float32)
    o_rm, o_rv = oa.compute_vbn(oa.unflatten(flat, A), rm, rv, frames, 0.1)
    r_rm, r_rv = ar.compute_vbn(ar.unflatten(flat, A), rm, rv, frames, 0.1)
    for got, want in ((o_rm, r_rm), (o_rv, r_rv)):
        for _, lo, hi in ar.STAT_BLOCKS:
            floor = 1e-6 * max(1.0, float(np.abs(want[lo:hi]).max()))
            np.testing.assert_allclose(got[lo:hi], want[lo:hi], rtol=1e-5, atol=floor)


def test_reference_entropy_and_decisions_by_hand():
    p = np.array([[0.5, 0.25, 0.25], [1.0, 0.0, 0.0]])
    np.testing.assert_allclose(ar.entropy(p).numpy(), [1.5 * np.log(2), 0.0], rtol=1e-15, atol=0)
    a, m = ar.decide(p, np.array([0.6, 0.999], np.float32))
    assert a.tolist() == [1, 0]
    np.testing.assert_allclose(m, [0.1, 1.0 - float(np.float32(0.999))], rtol=1e-6)
    a, m = ar.decide(p, None)
    assert a.tolist() == [0, 0] and m.tolist() == [0.25, 1.0]
    a, m = ar.decide(np.ones((2, 1)), np.array([0.3, 0.9], np.float32))
    assert a.tolist() == [0, 0] and np.isinf(m).all()


def test_frame_counter_word_field_overlaps_the_step_field():
    """Known property of the build-defined env, pinned so that neither side changes alone: the counter is
    (gid << 32) | (t << 11) | w and an Atari frame has 3528 words, so words 2048.. carry the step field's lowest bit:
    at an even step they are the first 1480 words of the next step, at an odd step of the frame itself."""
    assert oa.FRAME_WORDS == 3528
    f = [oa.frames(9, [5], t)[0].reshape(-1) for t in range(4)]
    for t in (0, 2):
        np.testing.assert_array_equal(f[t][2048 * 8:], f[t + 1][:1480 * 8])
        assert not np.array_equal(f[t][2048 * 8:], f[t][:1480 * 8])
    for t in (1, 3):
        np.testing.assert_array_equal(f[t][2048 * 8:], f[t][:1480 * 8])


# ---- every GPU parity case: conditioned, decided, covering the shape space ------------------------------------------
def test_case_table_covers_the_issue_shapes():
    shapes = {(c["n_act"], c["E"]) for c in ac.CASES if c["n_lanes"] == 9}
    assert {a for a, _ in shapes} == {1, 2, 7, 31, 32} and {e for _, e in shapes} == {1, 2, 4}
    assert {(1, 4), (32, 4), (32, 1)} <= shapes
    assert {c["n_lanes"] for c in ac.CASES if c["E"] == 2} >= {1, 7, 8, 9, 17}
    assert {c["T"] for c in ac.CASES} >= {1, 3}
    for c in ac.CASES:
        assert c["T"] <= 3
        ids = (c["lane_offset"] + np.arange(c["n_lanes"] + 1)) * c["E"]
        if c["name"] == "T3_2p31":
            assert ids[0] < 2 ** 31 < ids[-1]
        if c["name"] == "T3_2p32":
            assert ids[0] < 2 ** 32 < ids[-1]
        x = ac.inputs(c)
        P = x["theta"].size
        edge = x["idx"] == ac.TABLE_SIZE - P     # exactly one lane at the table's end, and it is perturbed
        assert edge.sum() == 1 and x["sign"][edge][0] != 0
        assert (x["idx"] >= 0).all() and (x["idx"] <= ac.TABLE_SIZE - P).all() and len(set(x["idx"].tolist())) == len(edge)
        if c["n_lanes"] >= 3:
            assert set(x["sign"].tolist()) == {1, -1, 0} and set(x["det"].tolist()) == {0, 1}


def test_theta_and_stats_have_no_trivial_section():
    x = ac.inputs(ac.BY_NAME["A7_E2"])
    p = oa.unflatten(x["theta"], 7)
    for name, v in p.items():
        v = v.numpy().ravel()
        assert v.size == 1 or (v[1:] != v[:-1]).all(), name       # a shift by one moves every element
        if v.size <= 512:                                           # (660k f32 draws do collide somewhere)
            assert len(np.unique(v)) == v.size, name
        if name in ("bn1.w", "bn2.w", "bn3.w"):
            assert (v == 0).sum() == 1 and (v > 0).any() and (v < 0).any(), name
            assert np.abs(v[v != 0]).min() >= 0.5
    for s in (x["rm"], x["rv"]):
        assert len(np.unique(s)) == 304
    assert np.abs(x["rm"]).min() > 1e-4 and np.abs(x["rv"] - 1).min() > 1e-4 and x["rv"].min() > 1e-3


@pytest.mark.parametrize("name", NAMES)
def test_case_is_conditioned(name):
    c = ac.BY_NAME[name]
    ref, orc, d = ac.reference(c)
    A = c["n_act"]
    h = ref["step_ent"]
    print("%s: entropy / ln A in [%.3f, %.3f]  d_oracle probs %.2e ent %.2e"
          % (name, h.min() / max(np.log(A), 1e-300), h.max() / max(np.log(A), 1e-300), d["probs"], d["ent"]))
    assert np.isfinite(ref["probs"]).all()
    if A == 1:
        assert (ref["probs"] == 1.0).all() and (h == 0.0).all()
        return
    assert h.min() >= 0.2 * np.log(A), h.min() / np.log(A)
    assert h.max() <= 0.98 * np.log(A), h.max() / np.log(A)


@pytest.mark.parametrize("name", NAMES)
def test_case_decisions_are_far_from_their_boundaries(name):
    """Zero excluded decisions: every margin >= 100 x the probability tolerance; and the f32 oracle, which is within
    that tolerance by construction, takes the same actions."""
    c = ac.BY_NAME[name]
    ref, orc, d = ac.reference(c)
    need = 100.0 * ac.tol(d["probs"])
    m = ref["margin"]
    print("%s: smallest margin %.3e, needed %.3e" % (name, m.min(), need))
    assert int((m < need).sum()) == 0, (float(m.min()), need)
    np.testing.assert_array_equal(orc["actions"], ref["actions"])
    np.testing.assert_array_equal(orc["ret"], ref["ret"])


# ---- section sensitivity -------------------------------------------------------------------------------------------
SENS_CASES = ["A2_E1", "A7_E2", "A31_E2", "A32_E4", "A32_E1"]
FEATURE_SECTIONS = ("c1.w", "c1.b", "bn1.w", "bn1.b", "c2.w", "c2.b", "bn2.w", "bn2.b")


@pytest.mark.parametrize("name", SENS_CASES)
def test_rolling_any_section_by_one_element_is_visible(name):
    """An indexing error in any of the parameter sections (the 14 tensors of parameters() order; the pack holds them as
    13 runs plus the head pair) or in any running-stat block shows at >= 100 x the device tolerance: in the features
    for what feeds them, in the probabilities for all."""
    c = ac.BY_NAME[name]
    x = ac.inputs(c)
    A = c["n_act"]
    frames = ac.env_frames(4)
    theta, rm, rv = x["theta"], x["rm"], x["rv"]

    def run(th, m, v):
        pr, ft = ar.forward(ar.unflatten(th, A), ar.split_bn(m, v), frames)
        return pr.numpy(), ft.numpy()

    p0, f0 = run(theta, rm, rv)
    po, fo = oa.forward(oa.unflatten(theta, A), oa.split_bn(rm, rv), frames)
    need_p = 100.0 * ac.tol(np.abs(po.numpy() - p0).max())
    need_f = 100.0 * ac.tol(ac.feat_distance(fo.numpy(), f0))
    seen = {}
    off = 0
    for sec, shape in oa.layout(A):
        n = int(np.prod(shape))
        th = theta.copy()
        th[off:off + n] = np.roll(theta[off:off + n], 1)
        off += n
        p1, f1 = run(th, rm, rv)
        seen[sec] = (ac.feat_distance(f1, f0), float(np.abs(p1 - p0).max()))
        if sec not in FEATURE_SECTIONS:
            assert seen[sec][0] == 0.0
    for blk, lo, hi in ar.STAT_BLOCKS:
        for which in ("rm", "rv"):
            m, v = rm.copy(), rv.copy()
            s = m if which == "rm" else v
            s[lo:hi] = np.roll(s[lo:hi], 1)
            p1, f1 = run(theta, m, v)
            seen["%s.%s" % (blk, which)] = (ac.feat_distance(f1, f0), float(np.abs(p1 - p0).max()))
    for sec, (df, dp) in seen.items():
        print("%s %-8s feat %.2e (need %.2e)  probs %.2e (need %.2e)" % (name, sec, df, need_f, dp, need_p))
    assert len(seen) == 14 + 6
    for sec, (df, dp) in seen.items():
        assert df >= need_f or dp >= need_p, (sec, df, need_f, dp, need_p)
        if sec in FEATURE_SECTIONS or sec.startswith(("bn1.r", "bn2.r")):
            assert df >= need_f, (sec, df, need_f)
