"""GPU: edge-shape parity of the ImpalaPolicy kernels (fdr_impala.hip, fdr_impala_f32.hip, fdr_impala_h.hip, their share
of fdr_pack.hip) against the float64 reference of tests/impala_ref.py, on the cases of tests/impala_cases.py (shown
conditioned, decided and sensitive to an indexing error of any section by tests/test_impala_ref.py).

Tolerances are measured, not fixed (impala_cases.tol / tol16).  f32 forms: per case and quantity d_oracle is the
distance of the f32 torch-CPU oracle from the float64 reference on the case's own inputs; the device must be within
4 x d_oracle, floor 2^-23 x scale.  fp16 forms: d_staged is the distance of the staged float64 restatement (the fp16
mode's rounding points in float64, "pair" where the call runs the MFMA pair core) from the float64 reference; the
device must be within 4 x d_staged and never beyond the product bound 2e-2.  Features are relative to the frame's
largest |feature|; h, c, probabilities and entropy absolute (entropy's scale ln n_act).  norm2 rel 1e-9 and equal
within a pair, ret bit-equal including the jiggle, steps exact; f32 actions exact; fp16 actions exact where every
decision margin of the case exceeds the fp16 probability limit, elsewhere the reference follows the kernel's actions
and each differing decision must be explained by its margin (at most 1 % of the decisions).  Every launch runs twice
and must equal itself bit for bit.  Each test prints d_oracle / d_staged and the device's distance.
"""
import ctypes

import numpy as np
import pytest
import torch

import impala_cases as ic
import impala_ref as ir
from impala_cases import SIGMA
from oracle import impala as oi
from oracle import rng as crng
from oracle.noise import perturb

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROLLOUTS = [(c["name"], f) for c in ic.CASES for f in c["forms"]]


@pytest.fixture(scope="module")
def engine():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from fdr import engine
    return engine


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def _lanes(engine, x, sigma=SIGMA, lane_offset=0, idx=None, sign=None, det=None, base=None, base_stride=0,
           no_table=False):
    base = _t(x["theta"] if base is None else base)
    if no_table:
        return engine.lanes_desc(base, base_stride, None, None, None, 0.0, _t(x["det"] if det is None else det),
                                 lane_offset=lane_offset)
    return engine.lanes_desc(base, base_stride, _t(x["table"]), _t(x["idx"] if idx is None else idx),
                             _t(x["sign"] if sign is None else sign), sigma, _t(x["det"] if det is None else det),
                             lane_offset=lane_offset)


def _spec(engine, c, form, entropy=True):
    return engine.ImpalaSpec(c["n_act"], c["E"], c["T"], entropy=entropy, env_seed=c["env_seed"],
                             fp16=form in ("h", "hp"), pairs=form in ("f32p", "hp"))


def _rollout(engine, c, x, form="f32", jiggle=None, entropy=True, n_lanes=None, **lane_kw):
    """One fdr_impala_rollout of the case (record = True) -> numpy arrays shaped [L, E, ...]."""
    E, T, A = c["E"], c["T"], c["n_act"]
    L = n_lanes or (len(lane_kw["idx"]) if lane_kw.get("idx") is not None else len(x["idx"]))
    lanes = _lanes(engine, x, lane_offset=c["lane_offset"], **lane_kw)
    out = engine.impala_rollout(_spec(engine, c, form, entropy), lanes, L, c["seed"],
                                jiggle=c["jiggle"] if jiggle is None else jiggle, bn_mean=_t(x["rm"]), bn_var=_t(x["rv"]),
                                record=True)
    torch.cuda.synchronize()
    return dict(ret=out.reward.cpu().numpy().reshape(L, E), ent=out.entropy.cpu().numpy().reshape(L, E),
                steps=out.timesteps.cpu().numpy().reshape(L, E), norm2=out.norm2.cpu().numpy(),
                actions=out.actions.cpu().numpy().reshape(L, E, T), probs=out.probs.cpu().numpy().reshape(L, E, T, A))


def _same_bits(a, b, what="", keys=None):
    for k in keys or a:
        assert a[k].tobytes() == b[k].tobytes(), "%s: %s differs" % (what, k)


def _report(tag, quantity, d_ref, d_dev, limit):
    print("IMPALA-EDGE %-22s %-6s d_ref %.3e  device %.3e  limit %.3e  share %.2f"
          % (tag, quantity, d_ref, d_dev, limit, d_dev / limit if limit > 0 else 0.0))


def _product_bound(tag, probs, ref_probs, ent=None, ref_ent=None):
    """the fp16 product bound as the earlier tests state it (tests/test_gpu_impala.py F16_RTOL): every probability, and
    every entropy, within 2e-2 RELATIVE of the reference's; the measured limits above are never looser than this"""
    rel = float((np.abs(np.asarray(probs, np.float64) - ref_probs) / ref_probs).max())
    print("IMPALA-EDGE %-22s probs  largest relative distance %.3e (product bound %.0e)" % (tag, rel, ic.F16_PRODUCT_BOUND))
    assert rel <= ic.F16_PRODUCT_BOUND, rel
    if ent is not None and (ref_ent > 0).all():
        rel = float((np.abs(ent - ref_ent) / ref_ent).max())
        assert rel <= ic.F16_PRODUCT_BOUND, rel


def _check_exact_parts(c, x, got, ref):
    T = c["T"]
    np.testing.assert_array_equal(got["ret"], ref["ret"])      # integer sum (+ the oracle's +-1e-12), the same f64 ops
    np.testing.assert_array_equal(got["steps"], T)
    np.testing.assert_allclose(got["norm2"], ref["norm2"], rtol=1e-9)
    assert (got["norm2"][x["sign"] == 0] == 0.0).all()
    if c["pair_lanes"]:
        both = (x["sign"][0::2] != 0) & (x["sign"][1::2] != 0)
        assert (got["norm2"][0::2][both] == got["norm2"][1::2][both]).all()


def _check_rollout(c, x, form, got, tag):
    """the comparison of one rollout result with the case's references, by the module docstring's rules"""
    ref, _, d = ic.reference(c)
    A = c["n_act"]
    scale_e = max(np.log(A), 1.0)
    assert all(np.isfinite(got[k]).all() for k in ("probs", "ent", "ret", "norm2"))
    mode = ic.staged_form(c, form)
    if mode is None:
        lim_p, lim_e, d_ref = ic.tol(d["probs"]), ic.tol(d["ent"], scale_e), d
    else:
        _, d_ref = ic.staged(c, mode)
        lim_p, lim_e = ic.tol16(d_ref["probs"]), ic.tol16(d_ref["ent"], scale_e)
        if not (got["actions"] == ref["actions"]).all():
            assert ref["margin"].min() < lim_p, "%s: actions differ though every margin exceeds the limit" % tag
            ref = ic.follow(c, got["actions"])
            stg = ic.staged(c, mode, actions=got["actions"])
            d_ref = ic.distances(stg, ref)
            lim_p, lim_e = ic.tol16(d_ref["probs"]), ic.tol16(d_ref["ent"], scale_e)
            diff = ref["own_actions"] != got["actions"]
            print("IMPALA-EDGE %-22s %d of %d decisions differ from the reference's own" % (tag, diff.sum(), diff.size))
            # explained by its margin: the device's own probabilities put the decision on the other side, i.e. the
            # margin is within the measured distance of the two cumulative sums (argmax: of the two top probabilities)
            dev, rp = got["probs"].astype(np.float64), ref["probs"]
            cs = np.abs(np.cumsum(dev, -1) - np.cumsum(rp, -1))
            reach = np.where(np.asarray(x["det"], bool)[:, None, None], 2.0 * np.abs(dev - rp).max(-1),
                             cs.max(-1) + cs[..., -1]) + 2.0 ** -22
            assert (ref["margin"][diff] <= reach[diff]).all(), "a differing action is not explained by its margin"
            assert (reach[diff] <= 2.0 * A * lim_p).all()
            assert 100 * int(diff.sum()) <= diff.size, (int(diff.sum()), diff.size)   # at most 1 % of the decisions
    d_p = float(np.abs(got["probs"].astype(np.float64) - ref["probs"]).max())
    d_e = float(np.abs(got["ent"] - ref["ent"]).max())
    _report(tag, "probs", d_ref["probs"], d_p, lim_p)
    _report(tag, "ent", d_ref["ent"], d_e, lim_e)
    if A == 1:  # one action: p = 1, H = 0, the target and target + 1 coincide -> +1 every step
        assert (got["probs"] == 1.0).all() and (got["ent"] == 0.0).all()
        np.testing.assert_array_equal(np.round(got["ret"]), float(c["T"]))
    assert d_p <= lim_p, (d_p, lim_p)
    assert d_e <= lim_e, (d_e, lim_e)
    if mode is not None:
        _product_bound(tag, got["probs"], ref["probs"], got["ent"], ref["ent"])
    np.testing.assert_array_equal(got["actions"], ref["actions"])
    _check_exact_parts(c, x, got, ref)


# ---- rollout --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,form", ROLLOUTS)
def test_rollout_matches_float64_reference(engine, name, form):
    c = ic.BY_NAME[name]
    x = ic.inputs(c)
    got = _rollout(engine, c, x, form)
    _same_bits(got, _rollout(engine, c, x, form), "%s/%s twice" % (name, form))
    _check_rollout(c, x, form, got, "%s/%s" % (name, form))


@pytest.mark.parametrize("form", ic.BY_NAME["T65"]["forms"])
def test_replay_without_the_projection_gemm(engine, form):
    """T = 65 = one 64-step replay chunk and a one-step tail, with the per-step streaming replay (set_replay_gemm(0)):
    the same reference, the same limits; f32: bit-equal to the GEMM form (identical fma chains)."""
    c = ic.BY_NAME["T65"]
    x = ic.inputs(c)
    with_gemm = _rollout(engine, c, x, form)
    try:
        engine.context().set_replay_gemm(0)
        got = _rollout(engine, c, x, form)
    finally:
        engine.context().set_replay_gemm(True)
    _check_rollout(c, x, form, got, "T65/%s/nogemm" % form)
    if form == "f32":
        _same_bits(got, with_gemm, "replay gemm on / off")


def test_f32_pair_form_is_the_lane_form_bitwise(engine):
    for name in ("A7_E2_P8", "A32_E4_P8", "L2_P", "T3_2p32"):
        c = ic.BY_NAME[name]
        x = ic.inputs(c)
        _same_bits(_rollout(engine, c, x, "f32"), _rollout(engine, c, x, "f32p"), name)


# ---- lanes descriptor -----------------------------------------------------------------------------------------------
def test_per_lane_base_rows_under_pairs(engine):
    """base_stride = P silently leaves the pair form.  Rows = theta'_l (formed on the host exactly as the device forms
    them) with sign 0: every lane bit-equal to the shared-base launch; rows = theta with the case's signs: the same."""
    c = ic.BY_NAME["A7_E2_P8"]
    x = ic.inputs(c)
    P, L = x["theta"].size, c["n_lanes"]
    want = _rollout(engine, c, x, "f32")
    rows = perturb(x["theta"], x["table"], x["idx"], x["sign"], SIGMA)
    keys = ("probs", "ent", "actions", "ret", "steps")
    for form in ("f32p", "f32"):
        got = _rollout(engine, c, x, form, base=rows, base_stride=P, sign=np.zeros(L, np.int8))
        _same_bits(got, want, "theta' rows / %s" % form, keys)
        assert (got["norm2"] == 0.0).all()
        got = _rollout(engine, c, x, form, base=np.tile(x["theta"], (L, 1)), base_stride=P)
        _same_bits(got, want, "theta rows / %s" % form, keys + ("norm2",))
    # fp16: rows run per lane with or without `pairs` -- the same launch, and it meets the reference
    a = _rollout(engine, c, x, "h", base=np.tile(x["theta"], (L, 1)), base_stride=P)
    _same_bits(a, _rollout(engine, c, x, "hp", base=np.tile(x["theta"], (L, 1)), base_stride=P), "fp16 rows")
    _check_rollout(dict(c, forms=("f32", "h")), x, "h", a, "A7_E2_P8/h/rows")


@pytest.mark.parametrize("form", ["f32", "f32p", "h", "hp"])
def test_null_table_runs_theta_on_every_lane(engine, form):
    c = ic.BY_NAME["A7_E2_P8"]
    x = ic.inputs(c)
    L = c["n_lanes"]
    got = _rollout(engine, c, x, form, n_lanes=L, no_table=True)
    zero = _rollout(engine, c, x, "h" if form in ("h", "hp") else "f32", sign=np.zeros(L, np.int8))
    _same_bits(got, zero, "NULL table vs sign 0 / %s" % form)
    assert (got["norm2"] == 0.0).all()
    if form == "f32":   # and that is the reference's sign-0 lane of the same envs
        ref, _, d = ic.reference(c)
        s0 = x["sign"] == 0
        assert s0.any()
        assert np.abs(got["probs"][s0] - ref["probs"][s0]).max() <= ic.tol(d["probs"])


@pytest.mark.parametrize("form", ["f32", "f32p", "h", "hp"])
def test_sigma_zero_equals_the_unperturbed_lane_bitwise(engine, form):
    """sigma = 0: EVERY lane, whatever its sign, is bit-equal to the same launch with every sign 0; and the sign-0 lanes
    of the sigma = 0.02 launch are those lanes too"""
    c = ic.BY_NAME["A7_E2_P8"]
    x = ic.inputs(c)
    L = c["n_lanes"]
    a = _rollout(engine, c, x, form)
    b = _rollout(engine, c, x, form, sigma=0.0)
    z = _rollout(engine, c, x, form, sign=np.zeros(L, np.int8))
    s0 = x["sign"] == 0
    assert s0.any() and (x["sign"] == 1).any() and (x["sign"] == -1).any()
    _same_bits(b, z, "sigma 0 vs sign 0 / %s" % form, ("probs", "ent", "actions", "ret", "steps"))
    assert (b["norm2"] == 0.0).all() and (z["norm2"] == 0.0).all()
    for k in ("probs", "ent", "actions", "ret"):
        assert a[k][s0].tobytes() == b[k][s0].tobytes(), k
    assert (a["probs"][~s0] != b["probs"][~s0]).any()


@pytest.mark.parametrize("form", ["f32", "h"])
def test_bad_table_offset_poisons_norm_without_fault(engine, form):
    """idx = table_size - P + 1 and idx = -1 are never dereferenced: the lane runs unperturbed (bitwise the sign-0
    lane), reports norm2 = NaN, and its neighbours are what they are without it (the existing contract)."""
    c = dict(ic.BY_NAME["A7_E2"], n_lanes=5)
    x = ic.inputs(ic.BY_NAME["A7_E2"])
    P = x["theta"].size
    idx = x["idx"][:5].copy()
    sign = np.array([1, 1, -1, -1, 1], np.int8)
    det = x["det"][:5]
    bad_idx, clean_sign = idx.copy(), sign.copy()
    bad_idx[1], bad_idx[3] = ic.TABLE_SIZE - P + 1, -1
    clean_sign[1] = clean_sign[3] = 0
    bad = _rollout(engine, c, x, form, idx=bad_idx, sign=sign, det=det)
    clean = _rollout(engine, c, x, form, idx=idx, sign=clean_sign, det=det)
    assert np.isnan(bad["norm2"][[1, 3]]).all()
    ok = [0, 2, 4]
    assert bad["norm2"][ok].tobytes() == clean["norm2"][ok].tobytes() and (clean["norm2"][[1, 3]] == 0).all()
    _same_bits(bad, clean, "bad offsets", ("probs", "ent", "actions", "ret", "steps"))


# ---- options --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["f32", "f32p", "h", "hp"])
def test_entropy_off_changes_nothing_else(engine, form):
    c = ic.BY_NAME["A7_E2_P8"]
    x = ic.inputs(c)
    on = _rollout(engine, c, x, form)
    off = _rollout(engine, c, x, form, entropy=False)
    assert (off["ent"] == 0.0).all() and (on["ent"] != 0.0).all()
    _same_bits(on, off, "entropy on / off", ("probs", "actions", "ret", "steps", "norm2"))


def test_jiggle_is_the_oracles_and_absent_when_off(engine):
    c = ic.BY_NAME["T3_2p32"]       # global env ids across 2^32: the jiggle's counter takes them whole
    x = ic.inputs(c)
    on = _rollout(engine, c, x, jiggle=True)["ret"]
    off = _rollout(engine, c, x, jiggle=False)["ret"]
    L, E = c["n_lanes"], c["E"]
    np.testing.assert_array_equal(off, np.round(off))
    envs = np.arange(L * E, dtype=np.uint64) + np.uint64(c["lane_offset"] * E)
    jig = crng.jiggle(c["seed"], envs).reshape(L, E)
    assert set(np.unique(jig).tolist()) == {-1e-12, 1e-12}
    np.testing.assert_array_equal(on, off + jig)


# ---- raw C entry points: memory discipline, optional outputs and refusals ------------------------------------------
SENT_F64, SENT_I32, SENT_F32, TAIL = -777.25, -77, -55.5, 0xA5


class _Raw(object):
    """fdr_impala_rollout through ctypes with sentinel-filled outputs one lane longer than needed and a workspace of
    exactly `ws_bytes` bytes at the head of a buffer whose tail holds a byte pattern."""

    def __init__(self, engine, n_lanes, E, T, A, ws_bytes):
        ne = (n_lanes + 1) * E
        self.out = dict(ret=torch.full((ne,), SENT_F64, dtype=torch.float64, device=DEV),
                        ent=torch.full((ne,), SENT_F64, dtype=torch.float64, device=DEV),
                        steps=torch.full((ne,), SENT_I32, dtype=torch.int32, device=DEV),
                        norm2=torch.full((n_lanes + 1,), SENT_F64, dtype=torch.float64, device=DEV),
                        actions=torch.full((ne * T,), SENT_I32, dtype=torch.int32, device=DEV),
                        probs=torch.full((ne * T * max(A, 1),), SENT_F32, dtype=torch.float32, device=DEV))
        self.used = dict(ret=n_lanes * E, ent=n_lanes * E, steps=n_lanes * E, norm2=n_lanes,
                         actions=n_lanes * E * T, probs=n_lanes * E * T * max(A, 1))
        self.ws_bytes = int(ws_bytes)
        self.buf = torch.full((self.ws_bytes + 4096,), TAIL, dtype=torch.uint8, device=DEV)
        self.engine = engine

    def call(self, desc, lanes, n_lanes, seed=5, jiggle=1, ws_bytes=None, null=()):
        e, o = self.engine, self.out
        p = {k: (None if k in null else e._p(v)) for k, v in o.items()}
        rc = e.lib.fdr_impala_rollout(e._c(torch.device(DEV, 0)), ctypes.byref(desc), ctypes.byref(lanes), n_lanes,
                                      ctypes.c_uint64(seed), jiggle, p["ret"], p["ent"], p["steps"], p["norm2"],
                                      p["actions"], p["probs"], e._p(self.buf),
                                      self.ws_bytes if ws_bytes is None else ws_bytes, e._stream(torch.device(DEV, 0)))
        torch.cuda.synchronize()
        return rc, e.lib.fdr_last_error().decode(errors="replace")

    def get(self, k, shape):
        return self.out[k][:self.used[k]].cpu().numpy().reshape(shape)

    def assert_tail_intact(self):
        assert (self.buf[self.ws_bytes:] == TAIL).all(), "the workspace tail was written"

    def assert_untouched(self, beyond_only=False, only=None):
        for k, t in self.out.items():
            if only is not None and k not in only:
                continue
            part = t[self.used[k]:] if beyond_only else t
            sent = SENT_I32 if t.dtype == torch.int32 else (SENT_F32 if t.dtype == torch.float32 else SENT_F64)
            assert (part == sent).all(), "%s was written%s" % (k, " beyond its lanes" if beyond_only else "")


def _desc(engine, A, E, T, rm=None, rv=None, n_params=None, env_seed=9, fp16=0, pairs=0, entropy=1):
    from fdr import _lib
    P = engine.impala_num_params(A) if n_params is None else n_params
    return _lib.ImpalaDesc(A, E, T, entropy, env_seed, P, None if rm is None else rm.data_ptr(),
                           None if rv is None else rv.data_ptr(), fp16, pairs)


@pytest.mark.parametrize("form", ["f32", "f32p", "h", "hp"])
def test_rollout_memory_discipline(engine, form):
    """each of the four core forms in a workspace of exactly the queried size"""
    from fdr import _lib
    c = ic.BY_NAME["A7_E2_P8"]
    x = ic.inputs(c)
    rm, rv = _t(x["rm"]), _t(x["rv"])
    L, E, T, A = c["n_lanes"], c["E"], c["T"], c["n_act"]
    d = _desc(engine, A, E, T, rm, rv, fp16=int(form in ("h", "hp")), pairs=int(form in ("f32p", "hp")))
    nb = engine.lib.fdr_impala_workspace_bytes(ctypes.byref(d), L)
    assert nb > 0
    lanes = _lanes(engine, x)
    raw = _Raw(engine, L, E, T, A, nb)
    rc, msg = raw.call(d, lanes, L, ws_bytes=nb - 1)
    assert rc == _lib.FDR_ERR_WORKSPACE, (rc, msg)
    raw.assert_untouched()
    raw.assert_tail_intact()
    rc, msg = raw.call(d, lanes, L, seed=c["seed"], jiggle=int(c["jiggle"]))
    assert rc == _lib.FDR_OK, msg
    raw.assert_tail_intact()
    raw.assert_untouched(beyond_only=True)
    got = dict(ret=raw.get("ret", (L, E)), ent=raw.get("ent", (L, E)), steps=raw.get("steps", (L, E)),
               norm2=raw.get("norm2", (L,)), actions=raw.get("actions", (L, E, T)), probs=raw.get("probs", (L, E, T, A)))
    _same_bits(got, _rollout(engine, c, x, form), "raw call vs engine call / %s" % form)
    # NULL norm2 / actions / probs: the other outputs bit-equal, the omitted buffers untouched
    raw2 = _Raw(engine, L, E, T, A, nb)
    rc, msg = raw2.call(d, lanes, L, seed=c["seed"], jiggle=int(c["jiggle"]), null=("norm2", "actions", "probs"))
    assert rc == _lib.FDR_OK, msg
    raw2.assert_untouched(only=("norm2", "actions", "probs"))
    raw2.assert_tail_intact()
    for k in ("ret", "ent", "steps"):
        assert raw2.get(k, (L, E)).tobytes() == got[k].tobytes(), k
    # n_lanes = 0: FDR_OK, nothing written
    raw0 = _Raw(engine, 0, E, T, A, engine.lib.fdr_impala_workspace_bytes(ctypes.byref(d), 0))
    rc, msg = raw0.call(d, lanes, 0)
    assert rc == _lib.FDR_OK, msg
    raw0.assert_untouched()
    raw0.assert_tail_intact()


@pytest.mark.parametrize("what,code,text", [
    ("E3", "UNSUPPORTED", "envs_per_lane must be 1, 2, 4 or 8"), ("E16", "UNSUPPORTED", "envs_per_lane must be 1, 2, 4 or 8"),
    ("A0", "UNSUPPORTED", "n_act must be in 1..32"), ("A33", "UNSUPPORTED", "n_act must be in 1..32"),
    ("T0", "INVALID", "episode_len out of range"), ("T2p20", "INVALID", "episode_len out of range"),
    ("P+1", "INVALID", "n_params does not match"), ("P-1", "INVALID", "n_params does not match"),
    ("null_ret", "INVALID", "NULL output"), ("odd_pairs", "INVALID", "n_lanes must be even")])
def test_rollout_refusals_leave_the_outputs_untouched(engine, what, code, text):
    from fdr import _lib
    c = ic.BY_NAME["A7_E2"]
    x = ic.inputs(c)
    A, E, T, L, pairs = 7, 2, 2, 2, 0
    P = engine.impala_num_params(A)
    if what[0] == "E":
        E = int(what[1:])
    elif what[0] == "A":
        A = int(what[1:])
    elif what == "T0":
        T = 0
    elif what == "T2p20":
        T = 1 << 20
    elif what[0] == "P":
        P += int(what[1:])
    elif what == "odd_pairs":
        L, pairs = 3, 1
    d = _desc(engine, A, E, T, n_params=P, pairs=pairs)
    lanes = _lanes(engine, x, idx=x["idx"][:3], sign=x["sign"][:3], det=x["det"][:3])
    # outputs and workspace sized for the largest legal neighbour of the refused shape; nothing may be launched
    raw = _Raw(engine, 3, 16, 2, 33, 64 << 20)
    rc, msg = raw.call(d, lanes, L, null=("ret",) if what == "null_ret" else ())
    assert rc == getattr(_lib, "FDR_ERR_" + code), (rc, msg)
    assert text in msg, msg
    raw.assert_untouched()
    raw.assert_tail_intact()


# ---- forward --------------------------------------------------------------------------------------------------------
def _device_forward(engine, fp16, kind, n):
    c = ic.BY_NAME[ic.FORWARD_CASE]
    x = ic.inputs(c)
    spec = engine.ImpalaSpec(c["n_act"], fp16=fp16)
    th, rm, rv = _t(x["theta"]), _t(x["rm"]), _t(x["rv"])

    def step(fr, rw, h, cc, nd):
        h, cc = _t(np.array(h, np.float32)), _t(np.array(cc, np.float32))
        pr, ft = engine.impala_forward(spec, th, _t(fr), h, cc, reward=_t(rw), notdone=_t(nd), bn_mean=rm, bn_var=rv,
                                       feat=True)
        torch.cuda.synchronize()
        return pr.cpu().numpy(), h.cpu().numpy(), cc.cpu().numpy(), ft.cpu().numpy()
    return ic.forward_run(step, kind, n)


def _check_forward(engine, fp16, kind, n):
    ref, d_oracle, d_staged = ic.forward_reference(kind, n)
    got = _device_forward(engine, fp16, kind, n)
    again = _device_forward(engine, fp16, kind, n)
    for a, b in zip(got, again):
        _same_bits(a, b, "forward twice")
    dd = ic.forward_distance(got, ref)
    d_ref = d_staged if fp16 else d_oracle
    tag = "fwd_%s_n%d/%s" % (kind, n, "h" if fp16 else "f32")
    scale = {k: 1.0 if k in ("feat", "probs") else max(float(np.abs(r[k]).max()) for r in ref) for k in dd}
    for k in ("feat", "h", "c", "probs"):
        _report(tag, k, d_ref[k], dd[k], (ic.tol16 if fp16 else ic.tol)(d_ref[k], scale[k]))
    for k in ("feat", "h", "c", "probs"):
        assert all(np.isfinite(g[k]).all() for g in got)
        assert dd[k] <= (ic.tol16 if fp16 else ic.tol)(d_ref[k], scale[k]), (k, dd[k], d_ref[k])
    if fp16:
        _product_bound(tag, np.stack([g["probs"] for g in got]), np.stack([r["probs"] for r in ref]))


@pytest.mark.parametrize("fp16", [False, True])
@pytest.mark.parametrize("n", ic.FORWARD_N)
def test_forward_matches_float64_reference(engine, n, fp16):
    """3 steps from a carried non-zero state, rewards outside [-1, 1], a 0 / 1 notdone mix: feat, h, c, probs per step"""
    _check_forward(engine, fp16, "env", n)


@pytest.mark.parametrize("fp16", [False, True])
@pytest.mark.parametrize("kind", ["zeros", "full", "mixed"])
def test_forward_on_extreme_frames(engine, kind, fp16):
    """all 0, all 255, and both beside env frames in one call; 9 rows, each from its own carried state and reward (the
    conv features of the constant frames coincide, so fewer rows would leave d_oracle a maximum over very few sums)"""
    _check_forward(engine, fp16, kind, 9)


# ---- strategies -----------------------------------------------------------------------------------------------------
_STRAT = {}


def _strategy_reference(n_lanes, Z, carried, mode):
    """float64 (or staged) lane strategies, cached; the modes share their conv features per precision"""
    key = (n_lanes, Z, carried, mode)
    if key not in _STRAT:
        c, x = ic.strategy_inputs(n_lanes, Z, pair=n_lanes % 2 == 0)
        fkey = (n_lanes, Z, "feats", mode is not None)
        res = ir.lane_strategies(x["theta"], x["table"], x["idx"], x["sign"], SIGMA, c["n_act"], x["frames"],
                                 x["rewards"], x["rm"], x["rv"], x["h0"] if carried else None,
                                 x["c0"] if carried else None, staged=mode, feats=_STRAT.get(fkey))
        _STRAT[fkey] = res[3]
        _STRAT[key] = res[:3]
    return _STRAT[key]


def _strategy_oracle(n_lanes, Z, carried):
    c, x = ic.strategy_inputs(n_lanes, Z, pair=n_lanes % 2 == 0)
    bn = oi.split_bn(x["rm"], x["rv"])
    out = [oi.strategy(oi.unflatten(th, c["n_act"]), bn, x["frames"], x["rewards"],
                       x["h0"][l] if carried else None, x["c0"][l] if carried else None)
           for l, th in enumerate(perturb(x["theta"], x["table"], x["idx"], x["sign"], SIGMA))]
    return (np.stack([o[0] for o in out]), np.stack([o[1].view(-1).numpy() for o in out]),
            np.stack([o[2].view(-1).numpy() for o in out]))


@pytest.mark.parametrize("carried", [False, True])
@pytest.mark.parametrize("form", ["f32", "h", "hp"])
@pytest.mark.parametrize("n_lanes,Z", ic.STRATEGY_SHAPES)
def test_strategies_match_float64_reference(engine, n_lanes, Z, form, carried):
    """Probabilities per step and the end state, from the reset state (NULL h / c) and from a given one.  Under pairs
    an odd lane count is refused; 8 and 4 lanes run the fp16 pair recurrence; Z = 65 crosses the 64-step chunk."""
    from fdr._lib import FDRError
    c, x = ic.strategy_inputs(n_lanes, Z, pair=n_lanes % 2 == 0)
    A = c["n_act"]
    spec = engine.ImpalaSpec(A, fp16=form in ("h", "hp"), pairs=form == "hp")
    rm, rv = _t(x["rm"]), _t(x["rv"])

    def run():
        h = _t(x["h0"].copy()) if carried else None
        cc = _t(x["c0"].copy()) if carried else None
        out = engine.impala_strategies(spec, _lanes(engine, x), n_lanes, _t(x["frames"]), reward=_t(x["rewards"]), h=h,
                                       c=cc, bn_mean=rm, bn_var=rv)
        torch.cuda.synchronize()
        return dict(probs=out.cpu().numpy(), **({"h": h.cpu().numpy(), "c": cc.cpu().numpy()} if carried else {}))
    if form == "hp" and n_lanes % 2:
        with pytest.raises(FDRError, match="n_lanes must be even"):
            run()
        return
    got = run()
    _same_bits(got, run(), "strategies twice")
    assert got["probs"].shape == (n_lanes, Z, A) and np.isfinite(got["probs"]).all()
    ref = _strategy_reference(n_lanes, Z, carried, None)
    if form == "f32":
        other = _strategy_oracle(n_lanes, Z, carried)
        limit = ic.tol
    else:
        other = _strategy_reference(n_lanes, Z, carried, "pair" if form == "hp" and n_lanes % 4 == 0 else "lane")
        limit = ic.tol16
    tag = "strat_%dx%d/%s/%s" % (n_lanes, Z, form, "carried" if carried else "reset")
    for i, k in enumerate(("probs", "h", "c")):
        if k not in got:
            continue
        d_ref = float(np.abs(np.asarray(other[i], np.float64) - ref[i]).max())
        d_dev = float(np.abs(got[k].astype(np.float64) - ref[i]).max())
        lim = limit(d_ref, 1.0 if k == "probs" else float(np.abs(ref[i]).max()))
        _report(tag, k, d_ref, d_dev, lim)
        assert d_dev <= lim, (k, d_dev, d_ref)
    if form != "f32":
        _product_bound(tag, got["probs"], ref[0])
    if n_lanes > 1 and form == "f32":  # the lanes differ: one lane's pack served to another would show
        j = next(l for l in range(1, n_lanes) if (x["idx"][l], x["sign"][l]) != (x["idx"][0], x["sign"][0]))
        assert np.abs(ref[0][0] - ref[0][j]).max() > 100 * ic.tol(float(np.abs(other[0] - ref[0]).max()))


def test_strategies_memory_discipline(engine):
    from fdr import _lib
    n_lanes, Z = 8, 9
    c, x = ic.strategy_inputs(n_lanes, Z, pair=True)
    A = c["n_act"]
    rm, rv = _t(x["rm"]), _t(x["rv"])
    fr, rw = _t(x["frames"].reshape(Z, -1)), _t(x["rewards"])
    lanes = _lanes(engine, x)
    dev = torch.device(DEV, 0)
    for fp16, pairs in ((0, 0), (1, 0), (1, 1)):
        d = _desc(engine, A, 1, 1, rm, rv, fp16=fp16, pairs=pairs)
        nb = engine.lib.fdr_impala_strategies_workspace_bytes(ctypes.byref(d), n_lanes, Z)
        assert nb > 0
        buf = torch.full((nb + 4096,), TAIL, dtype=torch.uint8, device=DEV)
        probs = torch.full(((n_lanes + 1) * Z * A,), SENT_F32, dtype=torch.float32, device=DEV)
        h = torch.full(((n_lanes + 1) * 256,), SENT_F32, dtype=torch.float32, device=DEV)
        cc = h.clone()
        h[:n_lanes * 256] = _t(x["h0"]).reshape(-1)
        cc[:n_lanes * 256] = _t(x["c0"]).reshape(-1)

        def call(ws_bytes):
            rc = engine.lib.fdr_impala_strategies(engine._c(dev), ctypes.byref(d), ctypes.byref(lanes), n_lanes, Z,
                                                  engine._p(fr), engine._p(rw), engine._p(h), engine._p(cc),
                                                  engine._p(probs), engine._p(buf), ws_bytes, engine._stream(dev))
            torch.cuda.synchronize()
            return rc, engine.lib.fdr_last_error().decode(errors="replace")
        rc, msg = call(nb - 1)
        assert rc == _lib.FDR_ERR_WORKSPACE, (rc, msg)
        assert (probs == SENT_F32).all() and (buf[nb:] == TAIL).all()
        assert (h[:n_lanes * 256] == _t(x["h0"]).reshape(-1)).all()
        rc, msg = call(nb)
        assert rc == _lib.FDR_OK, msg
        assert (probs[n_lanes * Z * A:] == SENT_F32).all() and (buf[nb:] == TAIL).all()
        assert (h[n_lanes * 256:] == SENT_F32).all() and (cc[n_lanes * 256:] == SENT_F32).all()
        assert (probs[:n_lanes * Z * A] != SENT_F32).all()


def test_forward_memory_discipline(engine):
    from fdr import _lib
    c = ic.BY_NAME[ic.FORWARD_CASE]
    x = ic.inputs(c)
    A, n = c["n_act"], 9
    rm, rv = _t(x["rm"]), _t(x["rv"])
    th, fr = _t(x["theta"]), _t(ic.env_frames(n).reshape(n, -1))
    dev = torch.device(DEV, 0)
    for fp16 in (0, 1):
        d = _desc(engine, A, 1, 1, rm, rv, fp16=fp16)
        nb = engine.lib.fdr_impala_forward_workspace_bytes(A, n, fp16)
        assert nb > 0
        buf = torch.full((nb + 4096,), TAIL, dtype=torch.uint8, device=DEV)
        probs = torch.full(((n + 1) * A,), SENT_F32, dtype=torch.float32, device=DEV)
        feat = torch.full(((n + 1) * 2048,), SENT_F32, dtype=torch.float32, device=DEV)
        h = torch.full(((n + 1) * 256,), SENT_F32, dtype=torch.float32, device=DEV)
        cc = h.clone()
        h[:n * 256] = 0.25
        cc[:n * 256] = -0.5

        def call(ws_bytes):
            rc = engine.lib.fdr_impala_forward(engine._c(dev), ctypes.byref(d), engine._p(th), n, engine._p(fr), None,
                                               None, engine._p(h), engine._p(cc), engine._p(probs), engine._p(feat),
                                               engine._p(buf), ws_bytes, engine._stream(dev))
            torch.cuda.synchronize()
            return rc, engine.lib.fdr_last_error().decode(errors="replace")
        rc, msg = call(nb - 1)
        assert rc == _lib.FDR_ERR_WORKSPACE, (rc, msg)
        assert (probs == SENT_F32).all() and (feat == SENT_F32).all() and (buf[nb:] == TAIL).all()
        assert (h[:n * 256] == 0.25).all() and (cc[:n * 256] == -0.5).all()
        rc, msg = call(nb)
        assert rc == _lib.FDR_OK, msg
        assert (probs[n * A:] == SENT_F32).all() and (feat[n * 2048:] == SENT_F32).all() and (buf[nb:] == TAIL).all()
        assert (h[n * 256:] == SENT_F32).all() and (cc[n * 256:] == SENT_F32).all()
        assert (probs[:n * A] != SENT_F32).all() and (h[:n * 256] != 0.25).all()


# ---- env frames ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_act", [1, 32])
@pytest.mark.parametrize("env_id", [0, 1 << 31, (1 << 32) - 1])
def test_env_frames_bit_exact(engine, env_id, n_act):
    from fdr._lib import FDRError
    env_seed = 9
    for t0 in (0, 1, (1 << 20) - 2):
        for n in (0, 1, 3):
            if t0 + n >= (1 << 20):     # steps beyond the counter's 20 bits of t are refused, nothing written
                with pytest.raises(FDRError, match="bad range"):
                    engine.impala_env_frames(env_seed, n_act, env_id, t0, n)
                continue
            for given in (False, True):
                # the actions: the step's target, target + 1 and another one, so that +1, -1 and 0 all occur
                tg = np.array([oi.targets(env_seed, [env_id], t0 + i, n_act)[0] for i in range(n)], np.int64)
                acts = ((tg + np.arange(n)) % n_act).astype(np.int32) if given else None
                fr, rw = engine.impala_env_frames(env_seed, n_act, env_id, t0, n,
                                                  actions=None if acts is None else _t(acts))
                torch.cuda.synchronize()
                assert tuple(fr.shape) == (n, 3, 64, 64)
                for i in range(n):
                    want = oi.frames(env_seed, [env_id], t0 + i)[0].astype(np.float32)
                    np.testing.assert_array_equal(fr[i].cpu().numpy(), want)
                    r = oi.rewards(env_seed, [env_id], t0 + i, [acts[i] if given else 0], n_act)[0] if given else 0.0
                    assert rw[i].item() == r


def test_env_frames_refuses_ids_beyond_the_counter(engine):
    """env_id >= 2^32 would alias env_id mod 2^32 (the counter is env_id << 32): refused, nothing written"""
    from fdr import _lib
    fr = torch.full((3 * 64 * 64,), SENT_F32, dtype=torch.float32, device=DEV)
    rw = torch.full((1,), SENT_F32, dtype=torch.float32, device=DEV)
    for env_id, ok in (((1 << 32) - 1, True), (1 << 32, False), ((1 << 32) + 5, False), (-1, False)):
        fr.fill_(SENT_F32)
        rw.fill_(SENT_F32)
        rc = engine.lib.fdr_impala_env_frames(ctypes.c_uint64(9), 7, ctypes.c_int64(env_id), 0, 1, None, engine._p(fr),
                                              engine._p(rw), engine._stream(torch.device(DEV, 0)))
        torch.cuda.synchronize()
        if ok:
            assert rc == _lib.FDR_OK and (fr != SENT_F32).all()
        else:
            assert rc == _lib.FDR_ERR_INVALID and "bad range" in engine.lib.fdr_last_error().decode()
            assert (fr == SENT_F32).all() and (rw == SENT_F32).all()
