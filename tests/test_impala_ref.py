"""CPU: the float64 ImpalaPolicy reference (tests/impala_ref.py) and the edge-parity cases (tests/impala_cases.py) are
trustworthy before any device runs them.

  * the reference reproduces the goldens G8 (features, h, c, probs) and G14 (compute_vbn) to f32 rounding and agrees
    with the f32 oracle on the inputs of the earlier GPU tests (distances printed);
  * every case is conditioned: each visited state's entropy (rollout and replay) lies in [0.2, 0.98] ln(n_act), and at
    most GATE_SHARE of a step's 1024 LSTM gate pre-activations lie beyond +-6 (sigmoid / tanh within 2.5e-3 of their
    limits): a saturated unit hides a wrong weight;
  * the comparison can see an indexing error: rolling ANY of the 72 parameter tensors (oracle.layout: 12 + 48 + 12; the
    figure 84 sometimes quoted for this net counts no further tensor), or the rm or rv of any of the 17
    BNs, by one element moves a compared output (features, h, probabilities) by >= 100 x the f32 device tolerance and
    by >= 10 x the fp16 tolerance of that output;
  * no decision of any case is closer to its boundary than 100 x the f32 probability tolerance, so f32 actions, integer
    rewards and steps must be exact (zero decisions excluded); for the fp16 forms the cases whose smallest margin lies
    within the fp16 probability tolerance are listed (there the GPU test follows the kernel's actions).

Bounds "to f32 rounding": G8 / G14 are f32 torch-CPU outputs after 15 convs (K <= 288), the fc (K = 2048) and the LSTM
(K = 513): an f32 dot product of K terms is within ~sqrt(K) 2^-24 of the exact one relative to its terms, and the
stages stack, so features within 1e-5 of the largest feature, state and probabilities within 1e-5 absolute -- the
existing tests' own 1e-5.
"""
import numpy as np
import pytest
import torch

import impala_cases as ic
import impala_ref as ir
from oracle import impala as oi

F32_BOUND = 1e-5
GATE_SHARE = 0.10
NAMES = [c["name"] for c in ic.CASES]


def _g_theta(g):
    A, P = int(g["A"]), int(g["P"])
    tab = np.random.RandomState(int(g["table_seed"])).randn(2 ** 22).astype(np.float32)
    off = int(g["param_offset"])
    return A, (tab[off:off + P] * np.float32(0.1)).astype(np.float32)


# ---- the reference against the goldens and the oracle ---------------------------------------------------------------
def test_reference_reproduces_forward_golden(golden):
    g = golden("g8_impala.npz")
    A, theta = _g_theta(g)
    p, bn = ir.unflatten(theta, A), ir.split_bn(g["rm"], g["rv"])
    nq, T = g["frames"].shape[:2]
    h = torch.zeros(nq, 256, dtype=torch.float64)
    c = torch.zeros(nq, 256, dtype=torch.float64)
    worst = dict(feat=0.0, h=0.0, c=0.0, probs=0.0)
    for t in range(T):
        pr, h, c, ft, _, _ = ir.forward(p, bn, g["frames"][:, t], g["rewards"][:, t], h, c,
                                        1.0 - g["dones"][:, t].astype(np.float64))
        worst["feat"] = max(worst["feat"], ic.feat_distance(g["feat"][:, t], ft.numpy()))
        for k, v in (("h", h), ("c", c), ("probs", pr)):
            worst[k] = max(worst[k], float(np.abs(g[k][:, t] - v.numpy()).max()))
    print("G8: " + "  ".join("%s %.2e" % kv for kv in worst.items()))
    assert max(worst.values()) <= F32_BOUND, worst


def test_reference_reproduces_vbn_golden(golden):
    g = golden("g14_impala_vbn.npz")
    A, theta = _g_theta(g)
    p = ir.unflatten(theta, A)
    mom = float(g["momentum"])
    runs = {tag: ir.compute_vbn(p, g["rm"], g["rv"], g["frames"], g["rewards"], bool(g[tag + "_dones"][0]), g["h0"],
                                g["c0"], mom) for tag in ("a", "b")}
    # chained as the golden was: the f32 results of the first call feed the second
    runs["a2"] = ir.compute_vbn(p, g["a_rm"], g["a_rv"], g["frames"], g["rewards"], False, g["a_h"], g["a_c"], mom)
    for tag, res in runs.items():
        for name, got in zip(("rm", "rv", "h", "c"), res):
            want = g[tag + "_" + name]
            print("G14 %s %s: %.2e" % (tag, name, float(np.abs(got - want).max())))
            np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-6 if name[0] == "r" else 2e-5)


def test_reference_agrees_with_oracle_on_earlier_rollout_inputs():
    """tests/test_gpu_impala.py::test_rollout_deterministic_with_bn_stats_and_lane_offset's inputs (its _theta)."""
    A, E, T = 4, 1, 3
    torch.manual_seed(124)
    parts = []
    for name, shape in oi.layout(A):
        if ".bn" in name:
            parts.append((torch.ones(shape) if name.endswith(".w") else torch.zeros(shape)).reshape(-1))
        else:
            bound = 1.0 / np.sqrt(int(np.prod(shape[1:])) if len(shape) > 1 else shape[0])
            parts.append(torch.empty(shape).uniform_(-bound, bound).reshape(-1))
    theta = torch.cat(parts).numpy().astype(np.float32)
    table = np.random.RandomState(124).randn(2 ** 22).astype(np.float32)
    rs = np.random.RandomState(3)
    rm = (0.1 * rs.randn(ic.NBN)).astype(np.float32)
    rv = (1.0 + 0.5 * np.abs(rs.randn(ic.NBN))).astype(np.float32)
    args = (theta, table, np.array([77, 2_000_000, 3_000_000]), np.array([1, 0, -1]), 0.02, A, E, T, 11, 5, rm, rv)
    kw = dict(deterministic=np.array([1, 1, 0], bool), lane_offset=5)
    ref = ir.evaluate_lanes(*args, **kw)
    orc = oi.evaluate_lanes(*args, record=True, **kw)
    d = ic.distances(orc, ref)
    print("earlier rollout inputs: probs %.2e ent %.2e" % (d["probs"], d["ent"]))
    assert d["probs"] <= F32_BOUND and d["ent"] <= F32_BOUND
    np.testing.assert_array_equal(orc["actions"], ref["actions"])
    np.testing.assert_array_equal(orc["ret"], ref["ret"])
    np.testing.assert_array_equal(orc["norm2"], ref["norm2"])


def test_reference_entropy_and_decisions_by_hand():
    p = np.array([[0.5, 0.25, 0.25], [1.0, 0.0, 0.0]])
    np.testing.assert_allclose(ir.entropy(p).numpy(), [1.5 * np.log(2), 0.0], rtol=1e-15, atol=0)
    a, m = ir.decide(p, np.array([0.6, 0.999], np.float32))
    assert a.tolist() == [1, 0]
    np.testing.assert_allclose(m, [0.1, 1.0 - float(np.float32(0.999))], rtol=1e-6)
    a, m = ir.decide(p, None)
    assert a.tolist() == [0, 0] and m.tolist() == [0.25, 1.0]
    a, m = ir.decide(np.ones((2, 1)), np.array([0.3, 0.9], np.float32))
    assert a.tolist() == [0, 0] and np.isinf(m).all()


def test_staged_weights_are_the_documented_roundings():
    c = ic.BY_NAME["A7_E2_P8"]
    x = ic.inputs(c)
    A = c["n_act"]
    sel = np.nonzero(x["sign"])[0][:2]      # two perturbed lanes
    assert set(x["sign"][sel].tolist()) == {1, -1}
    lane = ir.lane_params(x["theta"], x["table"], x["idx"][sel], x["sign"][sel], ic.SIGMA, A, "lane")
    pair = ir.lane_params(x["theta"], x["table"], x["idx"][sel], x["sign"][sel], ic.SIGMA, A, "pair")
    plain = ir.lane_params(x["theta"], x["table"], x["idx"][sel], x["sign"][sel], ic.SIGMA, A)
    assert len(ir.F16_WEIGHTS) == 15 + 3
    for name, _ in oi.layout(A):
        for l in range(2):
            if name in ir.F16_WEIGHTS:
                assert torch.equal(lane[l][name], plain[l][name].half().double()) and not torch.equal(lane[l][name], plain[l][name])
                same = torch.equal(pair[l][name], lane[l][name])
                assert same != (name in ir.CORE_WEIGHTS), name
                assert (pair[l][name] - plain[l][name]).abs().max() <= 2.0 ** -10 * plain[l][name].abs().max()
            else:
                assert torch.equal(lane[l][name], plain[l][name]) and torch.equal(pair[l][name], plain[l][name]), name


# ---- every GPU parity case: conditioned, decided, covering the shape space ------------------------------------------
def test_case_table_covers_the_issue_shapes():
    nine = {(c["n_act"], c["E"]) for c in ic.CASES if c["n_lanes"] == 9}
    assert nine >= {(1, 4), (2, 1), (7, 2), (31, 2), (32, 1), (32, 4), (7, 8), (32, 8)}
    hp = {(c["n_act"], c["E"], c["n_lanes"]) for c in ic.CASES if ic.staged_form(c, "hp") == "pair" and "hp" in c["forms"]}
    assert hp >= {(a, 4, 4) for a in (4, 5, 8, 9, 16, 17, 32)} | {(a, 2, 4) for a in (8, 9, 32)} | {(32, 1, 8)}
    assert hp >= {(7, 2, 8), (32, 4, 8)}
    # both sides of each head_split threshold A * 4E <= 64 / <= 128 / <= 256
    prod = sorted({a * 4 * e for a, e, n in hp})
    for thr in (64, 128, 256):
        assert any(p <= thr for p in prod) and any(thr < p <= 2 * thr + 32 for p in prod), (thr, prod)
    assert {c["n_lanes"] for c in ic.CASES if (c["n_act"], c["E"]) == (7, 2) and "h" in c["forms"]} >= {1, 7, 8, 9, 17}
    assert {c["n_lanes"] for c in ic.CASES if (c["n_act"], c["E"]) == (7, 2) and "hp" in c["forms"]} >= {2, 6, 8}
    assert ic.staged_form(ic.BY_NAME["L6_P"], "hp") == "lane"      # n_lanes % 4 == 2: the fp16 call runs per lane
    assert {c["T"] for c in ic.CASES} >= {1, 2, 3, 65}
    combos = set()
    for c in ic.CASES:
        assert c["T"] <= 3 or (c["T"] == 65 and c["n_lanes"] == 2 and c["E"] == 1)
        assert c["n_lanes"] <= 9 or c["name"] == "L17"
        ids = (c["lane_offset"] + np.arange(c["n_lanes"] + 1)) * c["E"]
        if c["name"] == "T3_2p31":
            assert ids[0] < 2 ** 31 < ids[-1]
        if c["name"] == "T3_2p32":
            assert ids[0] < 2 ** 32 < ids[-1]
        x = ic.inputs(c)
        P = x["theta"].size
        assert P == oi.num_params(c["n_act"])
        edge = x["idx"] == ic.TABLE_SIZE - P
        assert (x["idx"] >= 0).all() and (x["idx"] <= ic.TABLE_SIZE - P).all()
        if c["pair_lanes"]:
            assert (x["idx"][0::2] == x["idx"][1::2]).all() and len(set(x["idx"][0::2].tolist())) == c["n_lanes"] // 2
            combos |= set(zip(x["sign"][0::2].tolist(), x["sign"][1::2].tolist()))
            assert edge.sum() == 2 and x["sign"][edge].any()
        else:
            assert len(set(x["idx"].tolist())) == c["n_lanes"]
            assert edge.sum() == 1 and x["sign"][edge][0] != 0
            if c["n_lanes"] >= 3:
                assert set(x["sign"].tolist()) == {1, -1, 0}
        if c["n_lanes"] >= 3:
            assert set(x["det"].tolist()) == {0, 1}
    assert combos == {(a, b) for a in (1, -1, 0) for b in (1, -1, 0)}


def test_theta_and_stats_have_no_trivial_section():
    x = ic.inputs(ic.BY_NAME["A7_E2"])
    p = oi.unflatten(x["theta"], 7)
    assert len(p) == 72
    for name, v in p.items():
        v = v.numpy().ravel()
        assert v.size == 1 or (v[1:] != v[:-1]).all(), name       # a shift by one moves every element
        if v.size <= 512:
            assert len(np.unique(v)) == v.size, name
        if ".bn" in name and name.endswith(".w"):
            assert (v == 0).sum() == 1 and ((v > 0).any() and (v < 0).any() or v.size == 3), name   # (3 channels: one is 0)
            assert np.abs(v[v != 0]).min() >= 0.5 and np.abs(v).max() <= 1.5
        elif name.endswith(".b") or ".b_" in name:
            assert 0.1 <= np.abs(v).mean() <= 1.0, (name, np.abs(v).mean())
    assert len(oi.bn_layout()) == 17
    for s in (x["rm"], x["rv"]):
        assert (s[1:] != s[:-1]).all()
    assert np.abs(x["rv"] - 1).min() > 1e-6 and x["rv"].min() > 1e-6


@pytest.mark.parametrize("name", NAMES)
def test_case_is_conditioned(name):
    c = ic.BY_NAME[name]
    ref, orc, d = ic.reference(c)
    A = c["n_act"]
    h = np.concatenate([ref["step_ent"], ref["replay_ent"]], -1) / max(np.log(A), 1e-300)
    print("%s: entropy / ln A in [%.3f, %.3f]  gates beyond +-%g: <= %.3f of a step (largest |gate| %.1f)  d_oracle probs "
          "%.2e ent %.2e" % (name, h.min(), h.max(), ir.GATE_SAT, ref["gate_sat"].max(), ref["gate_max"].max(), d["probs"],
                             d["ent"]))
    assert np.isfinite(ref["probs"]).all()
    assert ref["gate_sat"].max() <= GATE_SHARE
    if A == 1:
        assert (ref["probs"] == 1.0).all() and (h == 0.0).all()
        return
    assert h.min() >= 0.2, h.min()
    assert h.max() <= 0.98, h.max()


@pytest.mark.parametrize("name", NAMES)
def test_case_decisions_are_far_from_their_boundaries(name):
    """f32: zero excluded decisions -- every margin >= 100 x the probability tolerance, and the f32 oracle, which is
    within that tolerance by construction, takes the same actions.  fp16: report whether every margin also exceeds the
    form's probability limit (the GPU test demands equal actions exactly then)."""
    c = ic.BY_NAME[name]
    ref, orc, d = ic.reference(c)
    need = 100.0 * ic.tol(d["probs"])
    m = ref["margin"]
    print("%s: smallest margin %.3e, needed %.3e" % (name, m.min(), need))
    assert int((m < need).sum()) == 0, (float(m.min()), need)
    np.testing.assert_array_equal(orc["actions"], ref["actions"])
    np.testing.assert_array_equal(orc["ret"], ref["ret"])
    for mode in sorted({ic.staged_form(c, f) for f in c["forms"]} - {None}):
        st, ds = ic.staged(c, mode)
        lim = ic.tol16(ds["probs"])
        exact = m.min() >= lim
        print("%s fp16 %s: d_staged probs %.2e ent %.2e, limit %.2e -> %s" % (
            name, mode, ds["probs"], ds["ent"], lim, "actions exact" if exact else "FOLLOWS the kernel's actions"))
        if exact:   # then the staged model itself, which lies within the limit, decides as the reference does
            np.testing.assert_array_equal(st["own_actions"], ref["actions"])


# ---- section sensitivity -------------------------------------------------------------------------------------------
SENS_CASES = ["A7_E2", "A32_E4"]


@pytest.mark.parametrize("name", SENS_CASES)
def test_rolling_any_tensor_by_one_element_is_visible(name):
    """An indexing error in any of the 72 parameter tensors or in any BN's running-stat block shows in a compared
    output (features relative, h, probabilities; one step from a carried state over 4 env frames) at >= 100 x the f32
    device tolerance and >= 10 x the fp16 tolerance of that output."""
    c = ic.BY_NAME[name]
    x = ic.inputs(c)
    A = c["n_act"]
    frames, rewards, notdone, h0, c0 = ic.forward_inputs("env", 4)
    theta, rm, rv = x["theta"], x["rm"], x["rv"]

    def run(th, m, v, staged=None, feat=None):
        p, bn = ir.staged_params(th, A, staged), ir.split_bn(m, v)
        ft = ir.features(p, bn, frames[0], staged) if feat is None else feat
        pr, h, _, _ = ir.lstm_head(p, bn, ir.core_input(p, bn, ft, rewards[0], staged), h0, c0, notdone[0], staged)
        return dict(feat=ft.numpy(), h=h.numpy(), probs=pr.numpy()), ft

    def dist(a, b):
        return dict(feat=ic.feat_distance(a["feat"], b["feat"]), h=float(np.abs(a["h"] - b["h"]).max()),
                    probs=float(np.abs(a["probs"] - b["probs"]).max()))

    base, ft0 = run(theta, rm, rv)
    po, bo = oi.unflatten(theta, A), oi.split_bn(rm, rv)
    pr32, h32, _, f32, _ = oi.forward(po, bo, frames[0], rewards[0], h0, c0, notdone[0])
    d32 = dist(dict(feat=f32.numpy(), h=h32.numpy(), probs=pr32.numpy()), base)
    d16 = dist(run(theta, rm, rv, "lane")[0], base)
    need32 = {k: 100.0 * ic.tol(v) for k, v in d32.items()}
    need16 = {k: 10.0 * ic.tol16(v) for k, v in d16.items()}
    print("%s: d_oracle %s  d_staged %s" % (name, d32, d16))
    conv_names = {n for n, _ in oi.layout(A) if n.startswith(("feat", "res"))}
    seen = {}
    off = 0
    for sec, shape in oi.layout(A):
        n = int(np.prod(shape))
        th = theta.copy()
        th[off:off + n] = np.roll(theta[off:off + n], 1)
        off += n
        seen[sec] = dist(run(th, rm, rv, feat=None if sec in conv_names else ft0)[0], base)
        if sec not in conv_names:
            assert seen[sec]["feat"] == 0.0
    o = 0
    for blk, nf in oi.bn_layout():
        for which in ("rm", "rv"):
            m, v = rm.copy(), rv.copy()
            s = m if which == "rm" else v
            s[o:o + nf] = np.roll(s[o:o + nf], 1)
            seen["%s.%s" % (blk, which)] = dist(run(theta, m, v, feat=None if blk.startswith(("feat", "res")) else ft0)[0], base)
        o += nf
    assert len(seen) == 72 + 34
    r32 = {sec: max(dd[k] / need32[k] for k in dd) for sec, dd in seen.items()}
    r16 = {sec: max(dd[k] / need16[k] for k in dd) for sec, dd in seen.items()}
    for sec in seen:
        print("%s %-18s feat %.2e h %.2e probs %.2e   f32 ratio %.1f  fp16 ratio %.2f"
              % (name, sec, seen[sec]["feat"], seen[sec]["h"], seen[sec]["probs"], 100 * r32[sec], 10 * r16[sec]))
    # the rollout tests compare probabilities (and entropy) only: the same ratios on the probabilities alone
    p32 = {sec: dd["probs"] / need32["probs"] for sec, dd in seen.items()}
    p16 = {sec: dd["probs"] / need16["probs"] for sec, dd in seen.items()}
    q32, q16 = min(p32, key=p32.get), min(p16, key=p16.get)
    print("%s least visible in the probabilities alone: f32 %s at %.0f x the tolerance, fp16 %s at %.1f x the tolerance"
          % (name, q32, 100 * p32[q32], q16, 10 * p16[q16]))
    assert p32[q32] >= 1.0, (q32, 100 * p32[q32])
    lo32, lo16 = min(r32, key=r32.get), min(r16, key=r16.get)
    print("%s least visible: f32 %s at %.0f x the tolerance, fp16 %s at %.1f x the tolerance"
          % (name, lo32, 100 * r32[lo32], lo16, 10 * r16[lo16]))
    assert r32[lo32] >= 1.0, (lo32, 100 * r32[lo32])
    assert r16[lo16] >= 1.0, (lo16, 10 * r16[lo16])
