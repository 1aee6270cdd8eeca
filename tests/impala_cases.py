"""The ImpalaPolicy edge-parity cases: one table, read by tests/test_impala_ref.py (CPU: is every case conditioned, can
the comparison see an indexing error, is every decision far from its boundary) and tests/test_gpu_impala_edges.py (the
device against the float64 reference of tests/impala_ref.py).

TEST INFRASTRUCTURE ONLY.

theta     make_theta: every one of the 72 tensors holds distinct entries of a size its consumer can see -- weights at
          fan-in scale (the net neither dead nor saturated), conv / fc / LSTM / head biases and BN biases O(0.1 - 1),
          BN weights of mixed sign in +-[0.5, 1.5] with ONE exact 0 per BN.  (The earlier tests' theta has every BN
          weight 1 and bias 0: a wrong pack offset of any of those 34 sections moves nothing.)
stats     make_stats: the batch statistics of 16 env frames under theta (impala_ref.compute_vbn, momentum 1), then per
          channel the variance times a factor in [0.5, 2] and the mean shifted by up to half a standard deviation.  Two
          floors keep the net conditioned under the sigma = 0.02 perturbation (VAR_FLOOR, HEAD_VAR_FLOOR below).
seeds     theta_seed and the action seed of each case were searched (on the reference alone) so that the entropy band,
          the gate measure and the decision margins of tests/test_impala_ref.py hold.
lanes     per-lane cases: sign cycles +1, -1, 0; deterministic cycles 0, 1, 1, 0; offsets distinct.  Pair cases (forms
          with a "p"): idx[2p] == idx[2p+1], the pairs' sign combinations walk through all nine of {+1, -1, 0}^2
          starting at (+1, -1), the start moving with the case so that the table as a whole runs every combination.
          The last perturbed lane / pair sits at exactly table_size - P.  sigma = 0.02, the table has 2^21 entries.
forms     "f32" per lane, "f32p" pairs = 1, "h" fp16 per lane, "hp" fp16 with pairs = 1 (the MFMA pair core where
          n_lanes % 4 == 0 and E <= 4, else per lane -- staged_form() says which staging models the call).

Tolerance rule (tol): f32 -- a device quantity may be 4 x as far from the float64 reference as the f32 torch-CPU oracle
is on the same inputs (d_oracle, measured at run time), floor 2^-23 x scale: two f32 evaluations of the same sums in
another order differ by up to the sum of their errors (2 x), and d_oracle is a maximum over a small sample (2 x).
fp16 -- 4 x d_staged, the distance of the staged float64 restatement (impala_ref, staged = "lane" / "pair") from the
float64 reference: f32 accumulation in another order flips individual f16 roundings, each an error of the size the
model already carries (2 x), small sample (2 x); never looser than the product bound 2e-2.
"""
import numpy as np

from oracle import impala as oi

import impala_ref as ir

TABLE_SIZE = 1 << 21
TABLE_SEED = 124
SIGMA = 0.02
STAT_FRAMES = 16
F16_PRODUCT_BOUND = 2e-2     # SURVEY 8c, tests/test_gpu_impala.py F16_RTOL
NBN = oi.num_bn()
# make_stats floors every batch variance at this share of its BN's mean variance: of the 2048 ReLU'd features some are 0
# in all 16 frames (variance 0), and 1 / sqrt(eps) = 316 x such a feature in a 17th frame saturates the LSTM gates
VAR_FLOOR = 0.3
# ... and the head BN's variances at this absolute value: h lies in (-1, 1) and, one or two steps from the reset state over
# i.i.d.-noise frames, spreads by only ~0.07 per unit; normalised by that, the shift of h under the sigma = 0.02
# perturbation is 2 - 3 standard deviations on all 256 units (|z| ~ 40), and the head weights' own perturbation alone
# then moves a logit by ~1: the perturbed lanes' policies saturate at random
HEAD_VAR_FLOOR = 0.04

# gains of make_theta on top of the fan-in scale 1 / sqrt(fan_in) (weights) / absolute sizes (biases)
GAIN = {"conv.w": 1.0, "conv.b": 0.3, "bn.b": 0.3, "fc.w": 0.6, "fc.b": 0.3, "lstm.w": 0.7, "lstm.b": 0.2,
        "head.w": 0.6, "head.b": 1.0}

PAIR_SIGNS = [(1, -1), (-1, 1), (1, 1), (0, 1), (-1, -1), (1, 0), (0, -1), (-1, 0), (0, 0)]


def _case(name, n_act, E, n_lanes, T, forms, theta_seed=1, seed=1, lane_offset=0, jiggle=True, env_seed=9):
    return dict(name=name, n_act=n_act, E=E, n_lanes=n_lanes, T=T, forms=tuple(forms), theta_seed=theta_seed, seed=seed,
                lane_offset=lane_offset, jiggle=jiggle, env_seed=env_seed, pair_lanes=any("p" in f for f in forms))


LANE, LANE_H = ("f32",), ("f32", "h")
PAIR = ("f32", "f32p", "hp")
PAIR_H = ("f32", "f32p", "h", "hp")

CASES = [
    # n_act x E corners at 9 lanes (per lane: 9 is odd); the 8-lane twins run the pair forms
    _case("A1_E4", 1, 4, 9, 2, LANE_H),
    _case("A2_E1", 2, 1, 9, 2, LANE_H, jiggle=False, theta_seed=18),
    _case("A7_E2", 7, 2, 9, 2, LANE_H, seed=28),
    _case("A31_E2", 31, 2, 9, 2, LANE_H, seed=59),
    _case("A32_E1", 32, 1, 9, 2, LANE_H, jiggle=False, seed=45),
    _case("A32_E4", 32, 4, 9, 2, LANE_H, theta_seed=2, seed=46),
    _case("A7_E8", 7, 8, 9, 2, LANE_H, seed=112),
    _case("A32_E8", 32, 8, 9, 2, LANE_H, theta_seed=2, seed=18),
    _case("A7_E2_P8", 7, 2, 8, 2, PAIR, seed=38),
    _case("A32_E4_P8", 32, 4, 8, 2, PAIR, theta_seed=3, seed=354),
    # fp16 pair head split: 8 / 4 / 2 / 1 partial sums at A * 4E <= 64 / <= 128 / <= 256 / above
    _case("HS_E4_A4", 4, 4, 4, 2, PAIR), _case("HS_E4_A5", 5, 4, 4, 2, PAIR), _case("HS_E4_A8", 8, 4, 4, 2, PAIR, seed=7),
    _case("HS_E4_A9", 9, 4, 4, 2, PAIR, theta_seed=2), _case("HS_E4_A16", 16, 4, 4, 2, PAIR, seed=15), _case("HS_E4_A17", 17, 4, 4, 2, PAIR, seed=48),
    _case("HS_E4_A32", 32, 4, 4, 2, PAIR, theta_seed=2, seed=213),
    _case("HS_E2_A8", 8, 2, 4, 2, PAIR, seed=5), _case("HS_E2_A9", 9, 2, 4, 2, PAIR, theta_seed=2, seed=80), _case("HS_E2_A32", 32, 2, 4, 2, PAIR, theta_seed=2, seed=258),
    _case("HS_E1_A32", 32, 1, 8, 2, PAIR, seed=24),
    # lane counts at A = 7, E = 2 (9 lanes: A7_E2; 8 lanes in pairs: A7_E2_P8)
    _case("L1", 7, 2, 1, 2, LANE_H), _case("L7", 7, 2, 7, 2, LANE_H, jiggle=False), _case("L8", 7, 2, 8, 2, LANE_H, seed=7),
    _case("L17", 7, 2, 17, 2, LANE_H, seed=228),
    _case("L2_P", 7, 2, 2, 2, PAIR, seed=2), _case("L6_P", 7, 2, 6, 2, PAIR),
    # steps; global env ids (lane_offset + l) * E + e crossing 2^31 and 2^32 inside the launch; the 64-step replay chunk
    # (ids beyond 2^32 are outside fdr_impala_rollout's precondition: device and oracle both wrap them mod 2^32, and
    # T3_2p32 pins that the two wrap alike -- include/fdr.h)
    _case("T1", 7, 2, 4, 1, PAIR_H),
    _case("T3_2p31", 7, 2, 4, 3, PAIR_H, lane_offset=(1 << 30) - 2, seed=4),
    _case("T3_2p32", 7, 2, 4, 3, PAIR_H, lane_offset=(1 << 31) - 2, jiggle=False, seed=17),
    _case("T65", 7, 1, 2, 65, PAIR_H, theta_seed=3, seed=30),
]
BY_NAME = {c["name"]: c for c in CASES}
for _i, _c in enumerate(CASES):
    _c["start"] = _i        # where the case's pairs start in PAIR_SIGNS


def staged_form(case, form):
    """which staging of impala_ref models the call (None: f32): the fp16 pair core runs where the header says it does"""
    if form in ("f32", "f32p"):
        return None
    if form == "hp" and case["n_lanes"] % 4 == 0 and case["E"] <= 4:
        return "pair"
    return "lane"


def tol(d, scale=1.0):
    return max(4.0 * float(d), 2.0 ** -23 * float(scale))


def tol16(d_staged, scale=1.0):
    return min(tol(d_staged, scale), F16_PRODUCT_BOUND * float(scale))


_TABLE = []


def table():
    if not _TABLE:
        _TABLE.append(np.random.RandomState(TABLE_SEED).randn(TABLE_SIZE).astype(np.float32))
    return _TABLE[0]


def _kind(name):
    if ".bn" in name:
        return "bn.w" if name.endswith(".w") else "bn.b"
    for k in ("conv", "fc", "head"):
        if name.split(".")[-2].startswith(k) or name.startswith(k + "."):
            return k + "." + name[-1]
    return "lstm.w" if name.startswith("lstm.w") else "lstm.b"


def make_theta(n_act, seed):
    rs = np.random.RandomState(1000 + seed)
    parts = []
    for name, shape in oi.layout(n_act):
        n = int(np.prod(shape))
        kind = _kind(name)
        if kind == "bn.w":
            v = rs.uniform(0.5, 1.5, n) * rs.choice([-1.0, 1.0], n)
            v[rs.randint(n)] = 0.0
        elif kind.endswith(".w"):
            v = GAIN[kind] / np.sqrt(np.prod(shape[1:])) * rs.randn(n)
        else:
            v = GAIN[kind] * rs.randn(n)
        parts.append(v)
    return np.concatenate(parts).astype(np.float32)


_STATS = {}


def make_stats(theta, n_act, env_seed, first_env, seed):
    key = (n_act, env_seed, int(first_env), seed)
    if key not in _STATS:
        rs = np.random.RandomState(2000 + seed)
        envs = np.uint64(first_env) + np.arange(STAT_FRAMES // 2, dtype=np.uint64)
        fr = np.concatenate([oi.frames(env_seed, envs, 0), oi.frames(env_seed, envs, 1)])
        rm, rv, _, _ = ir.compute_vbn(ir.unflatten(theta, n_act), np.zeros(NBN), np.ones(NBN), fr, momentum=1.0)
        o = 0
        for _, nf in oi.bn_layout():      # a feature that is 0 in all 16 frames: see VAR_FLOOR
            rv[o:o + nf] = np.maximum(rv[o:o + nf], VAR_FLOOR * rv[o:o + nf].mean())
            if _ == "head.bn":
                rv[o:o + nf] = np.maximum(rv[o:o + nf], HEAD_VAR_FLOOR)
            o += nf
        rv = rv * rs.uniform(0.5, 2.0, NBN)
        rm = rm + rs.uniform(-0.5, 0.5, NBN) * np.sqrt(rv)
        _STATS[key] = (rm.astype(np.float32), rv.astype(np.float32))
    return _STATS[key]


def lanes(n_lanes, P, pair=False, start=0):
    """sign, deterministic and table offset of each lane (see the module docstring)."""
    span = TABLE_SIZE - P
    det = np.array([(0, 1, 1, 0)[l % 4] for l in range(n_lanes)], np.int8)
    if pair:
        assert n_lanes % 2 == 0
        sign = np.array([PAIR_SIGNS[(start + l // 2) % 9][l % 2] for l in range(n_lanes)], np.int8)
        idx = np.array([(7919 * (l // 2 + 1) * 131) % span for l in range(n_lanes)], np.int64)
        last = np.nonzero(sign)[0][-1] // 2
        idx[2 * last:2 * last + 2] = span
    else:
        sign = np.array([(1, -1, 0)[l % 3] for l in range(n_lanes)], np.int8)
        idx = np.array([(7919 * (l + 1) * 131) % span for l in range(n_lanes)], np.int64)
        idx[np.nonzero(sign)[0][-1]] = span     # the last PERTURBED lane reads the table's last P entries
    return idx, sign, det


_INPUTS = {}


def inputs(case):
    """The case's arrays (cached): theta, table, idx, sign, det, rm, rv."""
    key = case["name"]
    if key not in _INPUTS:
        A, E = case["n_act"], case["E"]
        theta = make_theta(A, case["theta_seed"])
        idx, sign, det = lanes(case["n_lanes"], theta.size, case["pair_lanes"], start=case["start"])
        rm, rv = make_stats(theta, A, case["env_seed"], case["lane_offset"] * E, case["theta_seed"])
        _INPUTS[key] = dict(theta=theta, table=table(), idx=idx, sign=sign, det=det, rm=rm, rv=rv)
    return _INPUTS[key]


def _args(case, x):
    return (x["theta"], x["table"], x["idx"], x["sign"], SIGMA, case["n_act"], case["E"], case["T"], case["seed"],
            case["env_seed"], x["rm"], x["rv"])


def _kw(case, x):
    return dict(deterministic=x["det"].astype(bool), jiggle=case["jiggle"], lane_offset=case["lane_offset"])


def distances(got, ref):
    """{"probs", "ent"}: largest absolute distance of a rollout result (dict of [L, E, ...] arrays) from the reference"""
    return dict(probs=float(np.abs(np.asarray(got["probs"], np.float64) - ref["probs"]).max()),
                ent=float(np.abs(np.asarray(got["ent"], np.float64) - ref["ent"]).max()))


_REFS = {}


def reference(case):
    """(float64 reference, f32 oracle, d_oracle {"probs", "ent"}) of the case's rollout, computed once."""
    key = case["name"]
    if key not in _REFS:
        x = inputs(case)
        ref = ir.evaluate_lanes(*_args(case, x), **_kw(case, x))
        orc = oi.evaluate_lanes(*_args(case, x), record=True, **_kw(case, x))
        _REFS[key] = (ref, orc, distances(orc, ref))
    return _REFS[key]


_STAGED = {}


def staged(case, mode, actions=None):
    """(staged restatement ALONG THE REFERENCE'S ACTIONS (or `actions`), d_staged {"probs", "ent"}), cached per mode;
    the two modes share their conv features (same conv weights), which do not depend on the actions."""
    key = (case["name"], mode)
    x = inputs(case)
    ref = reference(case)[0]
    feats = next((v[0]["feat"] for k, v in _STAGED.items() if k[0] == case["name"]), None)
    if actions is not None:
        return ir.follow_lanes(*_args(case, x), actions=actions, staged=mode, feats=feats, **_kw(case, x))
    if key not in _STAGED:
        st = ir.follow_lanes(*_args(case, x), actions=ref["actions"], staged=mode, feats=feats, **_kw(case, x))
        _STAGED[key] = (st, distances(st, ref))
    return _STAGED[key]


def follow(case, actions):
    """the float64 reference along a kernel's own actions (the conv features are the reference's: same frames)"""
    x = inputs(case)
    return ir.follow_lanes(*_args(case, x), actions=actions, feats=reference(case)[0]["feat"], **_kw(case, x))


# ---- forward / strategies: the A7_E2 theta and stats ---------------------------------------------------------------
FORWARD_CASE = "A7_E2"
FORWARD_N = (1, 7, 8, 9)
FORWARD_STEPS = 3
STRATEGY_SHAPES = ((1, 1), (9, 1), (8, 9), (4, 65), (17, 2))   # (lanes, Z)


def env_frames(n, t=0):
    return oi.frames(BY_NAME[FORWARD_CASE]["env_seed"], np.arange(n, dtype=np.uint64), t).astype(np.float32)


def forward_inputs(kind, n):
    """frames [steps][n, 3, 64, 64], rewards [steps][n] (some outside [-1, 1]), notdone [steps][n] (a 0 / 1 mix), and a
    non-zero carried state h0, c0 [n, 256].  kind: "env" | "zeros" | "full" | "mixed"."""
    rs = np.random.RandomState(77 + n)
    frames = []
    for t in range(FORWARD_STEPS):
        f = env_frames(n, t)
        if kind == "zeros":
            f = np.zeros_like(f)
        elif kind == "full":
            f = np.full_like(f, 255.0)
        elif kind == "mixed":
            f[0::3] = 0.0
            f[2::3] = 255.0
        frames.append(f)
    rewards = [rs.choice([-3.0, -1.0, -0.25, 0.0, 0.5, 1.0, 2.5], n).astype(np.float32) for _ in range(FORWARD_STEPS)]
    notdone = [((np.arange(n) + t) % 3 != 1).astype(np.float32) for t in range(FORWARD_STEPS)]
    h0 = (0.4 * rs.randn(n, 256)).astype(np.float32)
    c0 = (0.6 * rs.randn(n, 256)).astype(np.float32)
    return frames, rewards, notdone, h0, c0


def feat_distance(got, ref):
    """largest |got - ref| of a frame relative to the frame's largest |ref| (a frame whose features are all 0: absolute)"""
    ref = np.asarray(ref, np.float64)
    scale = np.abs(ref).max(-1)
    scale = np.where(scale > 0, scale, 1.0)
    return float((np.abs(np.asarray(got, np.float64) - ref).max(-1) / scale).max())


def forward_run(step_fn, kind, n):
    """run FORWARD_STEPS steps of `step_fn(frames, reward, h, c, notdone) -> probs, h, c, feat` from the carried state
    -> [dict(probs, h, c, feat)] per step (numpy)"""
    frames, rewards, notdone, h, c = forward_inputs(kind, n)
    out = []
    for t in range(FORWARD_STEPS):
        pr, h, c, ft = step_fn(frames[t], rewards[t], h, c, notdone[t])
        out.append(dict(probs=np.asarray(pr), h=np.asarray(h), c=np.asarray(c), feat=np.asarray(ft)))
    return out


def forward_distance(got, ref):
    """{"feat" (relative), "h", "c", "probs" (absolute)}: the largest over the steps"""
    d = dict(feat=0.0, h=0.0, c=0.0, probs=0.0)
    for g, r in zip(got, ref):
        d["feat"] = max(d["feat"], feat_distance(g["feat"], r["feat"]))
        for k in ("h", "c", "probs"):
            d[k] = max(d[k], float(np.abs(np.asarray(g[k], np.float64) - r[k]).max()))
    return d


_FWD = {}


def forward_reference(kind, n):
    """(float64 per-step results, d_oracle, d_staged) for FORWARD_CASE's theta (unperturbed) and stats"""
    if (kind, n) not in _FWD:
        c = BY_NAME[FORWARD_CASE]
        x = inputs(c)
        A = c["n_act"]
        bn = ir.split_bn(x["rm"], x["rv"])

        def f64(staged):
            p = ir.staged_params(x["theta"], A, staged)

            def step(fr, rw, h, cc, nd):
                pr, h2, c2, ft, _, _ = ir.forward(p, bn, fr, rw, h, cc, nd, staged)
                return pr.numpy(), h2.numpy(), c2.numpy(), ft.numpy()
            return forward_run(step, kind, n)

        po, bo = oi.unflatten(x["theta"], A), oi.split_bn(x["rm"], x["rv"])

        def step32(fr, rw, h, cc, nd):
            pr, h2, c2, ft, _ = oi.forward(po, bo, fr, rw, h, cc, nd)
            return pr.numpy(), h2.numpy(), c2.numpy(), ft.numpy()
        ref = f64(None)
        _FWD[(kind, n)] = (ref, forward_distance(forward_run(step32, kind, n), ref), forward_distance(f64("lane"), ref))
    return _FWD[(kind, n)]


def strategy_inputs(n_lanes, Z, pair=False):
    """FORWARD_CASE's theta and stats under `n_lanes` lanes; Z probe frames with rewards; a carried state [n_lanes, 256]"""
    c = BY_NAME[FORWARD_CASE]
    x = dict(inputs(c))
    x["idx"], x["sign"], x["det"] = lanes(n_lanes, x["theta"].size, pair, start=Z)
    rs = np.random.RandomState(500 + 31 * n_lanes + Z)
    x["frames"] = env_frames(Z, 1)
    x["rewards"] = rs.choice([-2.0, -1.0, 0.0, 0.5, 1.0], Z).astype(np.float32)
    x["h0"] = (0.4 * rs.randn(n_lanes, 256)).astype(np.float32)
    x["c0"] = (0.6 * rs.randn(n_lanes, 256)).astype(np.float32)
    return c, x
