"""GPU: edge-shape parity of the AtariPolicy kernels (fdr_atari.hip, its share of fdr_pack.hip) against the float64
reference of tests/atari_ref.py, on the cases of tests/atari_cases.py (shown conditioned, decided and sensitive to an
indexing error of any section by tests/test_atari_ref.py).

Tolerances are measured, not fixed (atari_cases.tol): per case and quantity d_oracle is the distance of the f32
torch-CPU oracle from the float64 reference on the case's own inputs; the device must be within 4 x d_oracle, floor
2^-23 x scale (features: relative to the frame's largest |feature|; probabilities and entropy: absolute, entropy's
scale ln n_act).  Actions, integer rewards and steps are exact (every decision margin is >= 100 x the probability
tolerance), norm2 rel 1e-9.  Every launch runs twice and must equal itself bit for bit (no atomics in these kernels).
Each test prints d_oracle and the device's distance ("AtariPolicy edge parity", holds the table).
"""
import ctypes

import numpy as np
import pytest
import torch

import atari_cases as ac
import atari_ref as ar
from atari_cases import SIGMA
from oracle import atari as oa
from oracle import rng as crng

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = [c["name"] for c in ac.CASES]


@pytest.fixture(scope="module")
def engine():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from fdr import engine
    return engine


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def _lanes(engine, x, sigma=SIGMA, lane_offset=0, idx=None, sign=None, det=None):
    return engine.lanes_desc(_t(x["theta"]), 0, _t(x["table"]), _t(x["idx"] if idx is None else idx),
                             _t(x["sign"] if sign is None else sign), sigma, _t(x["det"] if det is None else det),
                             lane_offset=lane_offset)


def _rollout(engine, c, x, jiggle=None, **lane_kw):
    """One fdr_atari_rollout of the case (record = True) -> numpy arrays shaped [L, E, ...]."""
    E, T, A = c["E"], c["T"], c["n_act"]
    L = len(lane_kw["idx"]) if lane_kw.get("idx") is not None else len(x["idx"])
    lanes = _lanes(engine, x, lane_offset=c["lane_offset"], **lane_kw)
    spec = engine.AtariSpec(A, E, T, env_seed=c["env_seed"])
    out = engine.atari_rollout(spec, lanes, L, c["seed"], jiggle=c["jiggle"] if jiggle is None else jiggle,
                               bn_mean=_t(x["rm"]), bn_var=_t(x["rv"]), record=True)
    torch.cuda.synchronize()
    return dict(ret=out.reward.cpu().numpy().reshape(L, E), ent=out.entropy.cpu().numpy().reshape(L, E),
                steps=out.timesteps.cpu().numpy().reshape(L, E), norm2=out.norm2.cpu().numpy(),
                actions=out.actions.cpu().numpy().reshape(L, E, T), probs=out.probs.cpu().numpy().reshape(L, E, T, A))


def _same_bits(a, b, what=""):
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), "%s: %s differs between two identical launches" % (what, k)


def _report(tag, quantity, d_oracle, d_dev, limit):
    print("ATARI-EDGE %-14s %-6s d_oracle %.3e  device %.3e  limit %.3e" % (tag, quantity, d_oracle, d_dev, limit))


# ---- rollout --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_rollout_matches_float64_reference(engine, name):
    c = ac.BY_NAME[name]
    x = ac.inputs(c)
    ref, _, d = ac.reference(c)
    A, T = c["n_act"], c["T"]
    got = _rollout(engine, c, x)
    _same_bits(got, _rollout(engine, c, x), name)
    assert np.isfinite(got["probs"]).all() and np.isfinite(got["ent"]).all() and np.isfinite(got["ret"]).all()
    d_p = float(np.abs(got["probs"].astype(np.float64) - ref["probs"]).max())
    d_e = float(np.abs(got["ent"] - ref["ent"]).max())
    lim_p, lim_e = ac.tol(d["probs"]), ac.tol(d["ent"], max(np.log(A), 1.0))
    _report(name, "probs", d["probs"], d_p, lim_p)
    _report(name, "ent", d["ent"], d_e, lim_e)
    if A == 1:  # one action: p = 1, H = 0, the target and target + 1 coincide -> +1 every step
        assert (got["probs"] == 1.0).all() and (got["ent"] == 0.0).all()
        np.testing.assert_array_equal(np.round(got["ret"]), float(T))
    assert d_p <= lim_p
    assert d_e <= lim_e
    np.testing.assert_array_equal(got["actions"], ref["actions"])
    np.testing.assert_array_equal(got["ret"], ref["ret"])          # integer sum (+ the oracle's +-1e-12), same f64 ops
    np.testing.assert_array_equal(got["steps"], T)
    np.testing.assert_allclose(got["norm2"], ref["norm2"], rtol=1e-9)
    assert (got["norm2"][x["sign"] == 0] == 0.0).all()


def test_sigma_zero_equals_the_unperturbed_lane_bitwise(engine):
    c = ac.BY_NAME["A7_E2"]
    x = ac.inputs(c)
    a = _rollout(engine, c, x)
    b = _rollout(engine, c, x, sigma=0.0)
    s0 = x["sign"] == 0
    assert s0.any() and (~s0).any()
    for k in ("probs", "ent", "actions", "ret"):
        assert a[k][s0].tobytes() == b[k][s0].tobytes(), k
    assert (a["probs"][~s0] != b["probs"][~s0]).any()
    assert (b["norm2"] == 0.0).all()


def test_jiggle_is_the_oracles_and_absent_when_off(engine):
    c = ac.BY_NAME["A7_E2"]
    x = ac.inputs(c)
    on = _rollout(engine, c, x, jiggle=True)["ret"]
    off = _rollout(engine, c, x, jiggle=False)["ret"]
    L, E = c["n_lanes"], c["E"]
    np.testing.assert_array_equal(off, np.round(off))
    envs = (np.arange(L * E, dtype=np.uint64) + np.uint64(c["lane_offset"] * E))
    jig = crng.jiggle(c["seed"], envs).reshape(L, E)
    assert set(np.unique(jig).tolist()) == {-1e-12, 1e-12}
    np.testing.assert_array_equal(on, off + jig)


def test_saturated_head_gives_exact_one_hot(engine):
    """A head bias of +200 on one action: exp(l - max) underflows to 0 for every other action -> p exactly (0, .., 1,
    .., 0), entropy exactly 0 (0 * log clamp, never NaN); a deterministic lane picks that action."""
    c = ac.BY_NAME["A7_E2"]
    x = dict(ac.inputs(c))
    A, k = c["n_act"], 3
    th = x["theta"].copy()
    th[th.size - A + k] += 200.0
    x["theta"] = th
    got = _rollout(engine, c, x)
    want = np.zeros(A, np.float32)
    want[k] = 1.0
    assert (got["probs"] == want).all()
    assert (got["ent"] == 0.0).all() and np.isfinite(got["ent"]).all()
    assert (got["actions"] == k).all()      # argmax on deterministic lanes; the inverse CDF of a one-hot on the others
    assert x["det"].any() and not x["det"].all()


def test_bad_table_offset_poisons_norm_without_fault(engine):
    """idx = table_size - P + 1 and idx = -1 are never dereferenced: the lane runs unperturbed (bitwise the sign-0
    lane), reports norm2 = NaN, and its neighbours are what they are without it."""
    c = dict(ac.BY_NAME["A7_E2"], n_lanes=5)
    x = ac.inputs(ac.BY_NAME["A7_E2"])
    P = x["theta"].size
    idx = x["idx"][:5].copy()
    sign = np.array([1, 1, -1, -1, 1], np.int8)
    det = x["det"][:5]
    bad_idx, clean_sign = idx.copy(), sign.copy()
    bad_idx[1], bad_idx[3] = ac.TABLE_SIZE - P + 1, -1
    clean_sign[1] = clean_sign[3] = 0
    bad = _rollout(engine, c, x, idx=bad_idx, sign=sign, det=det)
    clean = _rollout(engine, c, x, idx=idx, sign=clean_sign, det=det)
    assert np.isnan(bad["norm2"][[1, 3]]).all()
    ok = [0, 2, 4]
    assert bad["norm2"][ok].tobytes() == clean["norm2"][ok].tobytes() and (clean["norm2"][[1, 3]] == 0).all()
    for k in ("probs", "ent", "actions", "ret", "steps"):
        assert bad[k].tobytes() == clean[k].tobytes(), k


# ---- raw C entry points: memory discipline and refusals -----------------------------------------------------------
SENT_F64, SENT_I32, SENT_F32, TAIL = -777.25, -77, -55.5, 0xA5


class _Raw(object):
    """fdr_atari_rollout through ctypes with sentinel-filled outputs one lane longer than needed and a workspace of
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

    def call(self, desc, lanes, n_lanes, seed=5, jiggle=1, ws_bytes=None, null_ret=False):
        e, o = self.engine, self.out
        rc = e.lib.fdr_atari_rollout(e._c(torch.device(DEV, 0)), ctypes.byref(desc), ctypes.byref(lanes), n_lanes,
                                     ctypes.c_uint64(seed), jiggle, None if null_ret else e._p(o["ret"]), e._p(o["ent"]),
                                     e._p(o["steps"]), e._p(o["norm2"]), e._p(o["actions"]), e._p(o["probs"]),
                                     e._p(self.buf), self.ws_bytes if ws_bytes is None else ws_bytes,
                                     e._stream(torch.device(DEV, 0)))
        torch.cuda.synchronize()
        return rc, e.lib.fdr_last_error().decode(errors="replace")

    def assert_tail_intact(self):
        assert (self.buf[self.ws_bytes:] == TAIL).all(), "the workspace tail was written"

    def assert_untouched(self, beyond_only=False):
        for k, t in self.out.items():
            part = t[self.used[k]:] if beyond_only else t
            sent = SENT_I32 if t.dtype == torch.int32 else (SENT_F32 if t.dtype == torch.float32 else SENT_F64)
            assert (part == sent).all(), "%s was written%s" % (k, " beyond its lanes" if beyond_only else "")


def _desc(engine, A, E, T, x=None, n_params=None, env_seed=9):
    from fdr import _lib
    P = engine.atari_num_params(A) if n_params is None else n_params
    d = _lib.AtariDesc(A, E, T, 0, env_seed, P, None if x is None else x["_rm"].data_ptr(),
                       None if x is None else x["_rv"].data_ptr())
    return d


def test_rollout_memory_discipline(engine):
    from fdr import _lib
    c = ac.BY_NAME["A7_E2"]
    x = dict(ac.inputs(c))
    x["_rm"], x["_rv"] = _t(x["rm"]), _t(x["rv"])
    L, E, T, A = c["n_lanes"], c["E"], c["T"], c["n_act"]
    d = _desc(engine, A, E, T, x)
    nb = engine.lib.fdr_atari_workspace_bytes(ctypes.byref(d), L)
    assert nb > 0
    lanes = _lanes(engine, x)
    raw = _Raw(engine, L, E, T, A, nb)
    rc, msg = raw.call(d, lanes, L, ws_bytes=nb - 1)
    assert rc == _lib.FDR_ERR_WORKSPACE and "workspace too small" in msg
    raw.assert_untouched()
    raw.assert_tail_intact()
    rc, msg = raw.call(d, lanes, L, seed=c["seed"])
    assert rc == _lib.FDR_OK, msg
    raw.assert_tail_intact()
    raw.assert_untouched(beyond_only=True)
    ref, _, dd = ac.reference(c)
    got = raw.out["probs"][:raw.used["probs"]].cpu().numpy().reshape(L, E, T, A)
    assert np.abs(got - ref["probs"]).max() <= ac.tol(dd["probs"])
    np.testing.assert_array_equal(raw.out["actions"][:raw.used["actions"]].cpu().numpy().reshape(L, E, T),
                                  ref["actions"])
    # n_lanes = 0: FDR_OK, nothing written
    raw0 = _Raw(engine, 0, E, T, A, 256)
    rc, msg = raw0.call(d, lanes, 0)
    assert rc == _lib.FDR_OK, msg
    raw0.assert_untouched()
    raw0.assert_tail_intact()


@pytest.mark.parametrize("what,code,text", [
    ("E3", "UNSUPPORTED", "envs_per_lane must be 1, 2 or 4"), ("E8", "UNSUPPORTED", "envs_per_lane must be 1, 2 or 4"),
    ("A0", "UNSUPPORTED", "n_act must be in 1..32"), ("A33", "UNSUPPORTED", "n_act must be in 1..32"),
    ("T0", "INVALID", "episode_len out of range"), ("T2p20", "INVALID", "episode_len out of range"),
    ("null_ret", "INVALID", "NULL output")])
def test_rollout_refusals_leave_the_outputs_untouched(engine, what, code, text):
    from fdr import _lib
    c = ac.BY_NAME["A7_E2"]
    x = ac.inputs(c)
    A, E, T = 7, 2, 2
    P = engine.atari_num_params(A)
    if what[0] == "E":
        E = int(what[1:])
    elif what[0] == "A":
        A = int(what[1:])
    elif what == "T0":
        T = 0
    elif what == "T2p20":
        T = 1 << 20
    d = _desc(engine, A, E, T, n_params=P)
    lanes = _lanes(engine, x, idx=x["idx"][:2], sign=x["sign"][:2], det=x["det"][:2])
    # outputs and workspace sized for the largest legal neighbour of the refused shape; nothing may be launched
    raw = _Raw(engine, 2, 8, 2, 33, 16 << 20)
    rc, msg = raw.call(d, lanes, 2, null_ret=(what == "null_ret"))
    assert rc == getattr(_lib, "FDR_ERR_" + code), (rc, msg)
    assert text in msg, msg
    raw.assert_untouched()
    raw.assert_tail_intact()


# ---- forward --------------------------------------------------------------------------------------------------------
def _forward(engine, frames, feat):
    c = ac.BY_NAME[ac.FORWARD_CASE]
    x = ac.inputs(c)
    spec = engine.AtariSpec(c["n_act"])
    out = engine.atari_forward(spec, _t(x["theta"]), _t(frames), bn_mean=_t(x["rm"]), bn_var=_t(x["rv"]), feat=feat)
    torch.cuda.synchronize()
    return (out[0].cpu().numpy(), out[1].cpu().numpy()) if feat else (out.cpu().numpy(), None)


def _check_forward(engine, tag, frames):
    pr, ft, d = ac.forward_reference(frames)
    p1, f1 = _forward(engine, frames, True)
    p2, f2 = _forward(engine, frames, True)
    p3, _ = _forward(engine, frames, False)
    assert p1.tobytes() == p2.tobytes() and f1.tobytes() == f2.tobytes(), "two identical launches differ"
    assert p1.tobytes() == p3.tobytes(), "probabilities depend on whether the features are requested"
    d_f, d_p = ac.feat_distance(f1, ft), float(np.abs(p1 - pr).max())
    lim_f, lim_p = ac.tol(d["feat"]), ac.tol(d["probs"])
    _report(tag, "feat", d["feat"], d_f, lim_f)
    _report(tag, "probs", d["probs"], d_p, lim_p)
    assert np.isfinite(p1).all() and np.isfinite(f1).all()
    assert d_f <= lim_f
    assert d_p <= lim_p


@pytest.mark.parametrize("n", ac.FORWARD_N)
def test_forward_matches_float64_reference(engine, n):
    _check_forward(engine, "fwd_n%d" % n, ac.env_frames(n))


@pytest.mark.parametrize("kind", ["zeros", "full", "mixed"])
def test_forward_on_extreme_frames(engine, kind):
    _check_forward(engine, "fwd_" + kind, ac.extreme_frames()[kind])


def test_forward_memory_discipline(engine):
    from fdr import _lib
    c = ac.BY_NAME[ac.FORWARD_CASE]
    x = ac.inputs(c)
    A, n = c["n_act"], 9
    frames = ac.env_frames(n)
    rm, rv = _t(x["rm"]), _t(x["rv"])
    d = _lib.AtariDesc(A, 1, 1, 0, 0, engine.atari_num_params(A), rm.data_ptr(), rv.data_ptr())
    nb = engine.lib.fdr_atari_forward_workspace_bytes(A, n)
    assert nb > 0
    buf = torch.full((nb + 4096,), TAIL, dtype=torch.uint8, device=DEV)
    probs = torch.full(((n + 1) * A,), SENT_F32, dtype=torch.float32, device=DEV)
    feat = torch.full(((n + 1) * 2592,), SENT_F32, dtype=torch.float32, device=DEV)
    th, fr = _t(x["theta"]), _t(frames.reshape(n, -1))
    dev = torch.device(DEV, 0)

    def call(ws_bytes):
        rc = engine.lib.fdr_atari_forward(engine._c(dev), ctypes.byref(d), engine._p(th), n, engine._p(fr),
                                          engine._p(probs), engine._p(feat), engine._p(buf), ws_bytes,
                                          engine._stream(dev))
        torch.cuda.synchronize()
        return rc, engine.lib.fdr_last_error().decode(errors="replace")
    rc, msg = call(nb - 1)
    assert rc == _lib.FDR_ERR_WORKSPACE and "workspace too small" in msg
    assert (probs == SENT_F32).all() and (feat == SENT_F32).all() and (buf[nb:] == TAIL).all()
    rc, msg = call(nb)
    assert rc == _lib.FDR_OK, msg
    assert (probs[n * A:] == SENT_F32).all() and (feat[n * 2592:] == SENT_F32).all() and (buf[nb:] == TAIL).all()
    pr, ft, dd = ac.forward_reference(frames)
    assert np.abs(probs[:n * A].cpu().numpy().reshape(n, A) - pr).max() <= ac.tol(dd["probs"])
    assert ac.feat_distance(feat[:n * 2592].cpu().numpy().reshape(n, 2592), ft) <= ac.tol(dd["feat"])


# ---- strategies -----------------------------------------------------------------------------------------------------
def _strategy_inputs(n_lanes):
    c = ac.BY_NAME[ac.FORWARD_CASE]
    x = dict(ac.inputs(c))
    x["idx"], x["sign"], x["det"] = ac.lanes(n_lanes, x["theta"].size)
    return c, x


@pytest.mark.parametrize("n_lanes,Z", ac.STRATEGY_SHAPES)
def test_strategies_match_float64_reference(engine, n_lanes, Z):
    """Against an independent reference (theta' per lane, the float64 forward), not the per-lane device path.  257
    lanes: two chunks (256 + 1); lanes 0..8, 254, 255 and the second chunk's lone lane 256 are compared."""
    c, x = _strategy_inputs(n_lanes)
    A = c["n_act"]
    frames = ac.env_frames(Z)
    spec = engine.AtariSpec(A)
    rm, rv = _t(x["rm"]), _t(x["rv"])

    def run():
        out = engine.atari_strategies(spec, _lanes(engine, x), n_lanes, _t(frames), bn_mean=rm, bn_var=rv)
        torch.cuda.synchronize()
        return out.cpu().numpy()
    got = run()
    assert got.tobytes() == run().tobytes(), "two identical launches differ"
    assert got.shape == (n_lanes, Z, A) and np.isfinite(got).all()
    sel = ac.strategy_lanes(n_lanes)
    if n_lanes >= 3:
        assert {int(s) for s in x["sign"][sel]} == {1, -1, 0}
    ref = ar.strategies(x["theta"], x["table"], x["idx"][sel], x["sign"][sel], SIGMA, A, frames, x["rm"], x["rv"])
    from oracle.noise import perturb
    bn = oa.split_bn(x["rm"], x["rv"])
    orc = np.stack([oa.forward(oa.unflatten(th, A), bn, frames)[0].numpy()
                    for th in perturb(x["theta"], x["table"], x["idx"][sel], x["sign"][sel], SIGMA)])
    d = float(np.abs(orc - ref).max())
    d_dev = float(np.abs(got[sel] - ref).max())
    _report("strat_%dx%d" % (n_lanes, Z), "probs", d, d_dev, ac.tol(d))
    assert d_dev <= ac.tol(d)
    if n_lanes > 1:  # the lanes differ: one lane's pack served to another would show
        assert np.abs(ref[0] - ref[1]).max() > 100 * ac.tol(d)


def test_strategies_memory_discipline(engine):
    from fdr import _lib
    n_lanes, Z = 9, 2
    c, x = _strategy_inputs(n_lanes)
    A = c["n_act"]
    rm, rv = _t(x["rm"]), _t(x["rv"])
    d = _lib.AtariDesc(A, 1, 1, 0, 0, engine.atari_num_params(A), rm.data_ptr(), rv.data_ptr())
    nb = engine.lib.fdr_atari_strategies_workspace_bytes(ctypes.byref(d), n_lanes, Z)
    assert nb > 0
    buf = torch.full((nb + 4096,), TAIL, dtype=torch.uint8, device=DEV)
    probs = torch.full(((n_lanes + 1) * Z * A,), SENT_F32, dtype=torch.float32, device=DEV)
    fr = _t(ac.env_frames(Z).reshape(Z, -1))
    lanes = _lanes(engine, x)
    dev = torch.device(DEV, 0)

    def call(ws_bytes):
        rc = engine.lib.fdr_atari_strategies(engine._c(dev), ctypes.byref(d), ctypes.byref(lanes), n_lanes, Z,
                                             engine._p(fr), engine._p(probs), engine._p(buf), ws_bytes,
                                             engine._stream(dev))
        torch.cuda.synchronize()
        return rc, engine.lib.fdr_last_error().decode(errors="replace")
    rc, msg = call(nb - 1)
    assert rc == _lib.FDR_ERR_WORKSPACE and "workspace too small" in msg
    assert (probs == SENT_F32).all() and (buf[nb:] == TAIL).all()
    rc, msg = call(nb)
    assert rc == _lib.FDR_OK, msg
    assert (probs[n_lanes * Z * A:] == SENT_F32).all() and (buf[nb:] == TAIL).all()
    assert (probs[:n_lanes * Z * A] != SENT_F32).all()


# ---- env frames ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env_id", [0, 1 << 31, (1 << 32) - 1])
def test_env_frames_bit_exact(engine, env_id):
    from fdr._lib import FDRError
    env_seed = 9
    for t0 in (0, 1, (1 << 20) - 2):
        for n in (0, 1, 3):
            if t0 + n >= (1 << 20):     # steps beyond the counter's 20 bits of t are refused, nothing written
                with pytest.raises(FDRError, match="bad range"):
                    engine.atari_env_frames(env_seed, env_id, t0, n)
                continue
            got = engine.atari_env_frames(env_seed, env_id, t0, n)
            torch.cuda.synchronize()
            assert tuple(got.shape) == (n, 4, 84, 84)
            for i in range(n):
                want = oa.frames(env_seed, [env_id], t0 + i)[0].astype(np.float32)
                np.testing.assert_array_equal(got[i].cpu().numpy(), want)
    with pytest.raises(FDRError, match="bad range"):
        engine.atari_env_frames(env_seed, 1 << 32, 0, 1)
