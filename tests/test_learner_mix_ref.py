"""CPU side of the mixed objective: the conditions tests/learner_mix.py's inputs meet, the restatement's own
identities, and the C boundary's three prototypes and size queries (no GPU)."""
import numpy as np

import learner_cases as lc
import learner_mix as lm
import learner_ref as ref
import test_abi_layout as abi
from learner_cases import PR

LD = np.longdouble
GRID = (1, 3, 4, 5, 7)


def test_generator_keeps_the_conditioning_cap():
    """Every case of the small grid finds channels with mix_kappa <= KAPPA_MAX within its salts; the generator alone
    nearly always does (at most 3 of the 285 cases per coefficient set need another draw)."""
    cases = lc.grid_cases(GRID)
    assert len(cases) == 285
    for coefs in lm.COEF_SETS:
        redrawn, worst, worst_salt = 0, 0.0, 0
        for c in cases:
            nov, ent, salt, k = lm.channels(c, coefs)      # raises when the salts run out
            assert k <= lc.KAPPA_MAX and nov.shape == ent.shape == (c.n_all,)
            redrawn += salt > 0
            worst, worst_salt = max(worst, k), max(worst_salt, salt)
        print("coefficients %r: %d of %d redrawn (last salt %d), worst admitted kappa %.1f" % (
            coefs, redrawn, len(cases), worst_salt, worst))
        assert redrawn <= 3, (coefs, redrawn)


def test_reward_only_is_the_zscore():
    for c in (lc.make_case(67, 257, 3), lc.make_case(5, 2, 5, lane_lo=5, n_all=33), lc.make_case(67, 257, 4,
                                                                                                  returns="equal")):
        nan = np.full(c.n_all, np.nan)
        w = lm.mix_weights(c, (1.0, 0.0, 0.0), nan, None)
        z = ref.weights(c.r_all, PR, "zscore")
        assert w.dtype == LD and np.array_equal(w, z)
        np.testing.assert_array_equal(lm.mix_coefs(c, (1.0, 0.0, 0.0), nan, nan), c.coefs("zscore"))


def test_a_constant_channel_contributes_its_raw_difference():
    """sd_c == 0: z_c = x_c (standardize_arr's rule, per channel), so the channel adds a_c (v_c - p_c) to every lane."""
    c = lc.make_case(65, 257, 3)
    nov, ent, _, _ = lm.channels(c, lm.COEF_SETS[0])
    flat = np.full(c.n_all, 0.45)
    a = (0.6, 0.4, 0.05)
    with_flat = lm.mix_weights(c, a, flat, ent)
    without = lm.mix_weights(c, (a[0], 0.0, a[2]), None, ent)
    want = without + LD(a[1]) * LD(0.45 - lm.POLICY_NOVELTY)
    assert ref.rel_l2(with_flat, want) <= 2.0 ** -60
    # all three constant: the weight is the same number on every lane
    eq = lc.make_case(67, 257, 3, returns="equal")
    w = lm.mix_weights(eq, a, np.full(eq.n_all, 0.45), np.full(eq.n_all, 1.5))
    x = [LD(2.5 - PR), LD(0.45 - lm.POLICY_NOVELTY), LD(1.5 - lm.POLICY_ENTROPY)]
    assert np.all(w == w[0]) and abs(w[0] - sum(LD(k) * v for k, v in zip(a, x))) <= 2.0 ** -60


def test_kappa_is_coef_condition_on_the_reward_channel():
    c = lc.make_case(5, 257, 3)
    k = lm.mix_kappa(c, (1.0, 0.0, 0.0), None, None)
    assert k == ref.coef_condition(c.r_all, PR, "zscore", c.lane_lo, c.sign, c.n2, c.lpd, lc.SIGMA)


def test_header_and_exports():
    from fdr import _lib, engine
    protos = abi.header_prototypes()
    ch = ["P", "P", "P", "i32"] + ["f64"] * 6
    assert protos["fdr_fd_grad_fused_mix"] == ("i32", ["P", "P", "i64", "P", "i32", "i64"] + ch + [
        "i32", "P", "P", "i32", "f32", "P", "i64", "P", "i64", "P"])
    assert protos["fdr_fd_step_mix"] == ("i32", ["P", "P", "i64", "P", "i32", "i64"] + ch + [
        "P", "P", "i32", "f32", "P", "f64", "f64", "P", "P", "P", "P", "i64", "P"])
    assert protos["fdr_fd_weights_mix"] == ("i32", ["P"] + ch + ["i32", "i32", "P", "P", "i32", "f32", "P", "P"])
    for name in ("fdr_fd_grad_fused_mix", "fdr_fd_step_mix", "fdr_fd_weights_mix"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib, name)
    header = open(abi.HEADER).read()
    assert "#define FDR_WEIGHT_ZSCORE_MIX 3" in header
    assert _lib.FDR_WEIGHT_ZSCORE_MIX == 3 and 3 in engine.WEIGHT_MODES.values()
    assert _lib.version().startswith("fdr 0.5")
    lib = _lib.lib
    assert lib.fdr_fd_grad_fused_out_len(3, 6092, 4096) == 6092
    assert lib.fdr_fd_grad_fused_out_len(7, 6092, 4096) == -1
    assert lib.fdr_fd_grad_fused_workspace_bytes(2048, 2, 6092, 3) == 1593088
    assert lib.fdr_fd_grad_fused_workspace_bytes(2048, 2, 6092, 0) == 1593088
