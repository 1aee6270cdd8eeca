"""The AtariPolicy edge-parity cases: one table, read by tests/test_atari_ref.py (CPU: is every case conditioned, can
the comparison see an indexing error, is every decision far from its boundary) and tests/test_gpu_atari_edges.py (the
device against the float64 reference of tests/atari_ref.py).

TEST INFRASTRUCTURE ONLY.

theta     make_theta: every section of the parameter vector holds distinct entries of a size that its consumer can
          see -- conv / fc biases comparable to the pre-activations they shift, BN weights of mixed sign in
          +-[0.5, 1.5] with ONE exact 0 per BN, BN biases and the head bias O(1).  (init_theta has every bias 0 and
          every BN weight / bias 1 / 0: a wrong pack offset of such a section moves nothing.)
stats     make_stats: the batch statistics of 16 env frames under theta (atari_ref.compute_vbn, momentum 1), then per
          channel the variance times a factor in [0.5, 2] and the mean shifted by up to half a standard deviation:
          every rm / rv entry distinct and far from 0 / 1, and the net still unsaturated (carelessly drawn stats make
          the softmax one-hot, where a probability comparison shows nothing).
lanes     lane l: sign cycles +1, -1, 0; deterministic cycles 0, 1 with another period; table offsets distinct, the
          last perturbed lane's exactly table_size - P.
seeds     theta_seed and the action seed of each case were searched (on the reference alone) so that the entropy band
          and the decision margins of tests/test_atari_ref.py hold.

Tolerance rule (tol): a device quantity may be 4 x as far from the float64 reference as the f32 torch-CPU oracle is on
the same inputs (d_oracle, measured at run time), with a floor of 2^-23 x scale.  Both are f32 evaluations with the
same K (256, 256, 2592, 256) in another summation order (MFMA k-steps of 4, four wave partials for the fc, FMA
contraction): two independent roundings of that size differ by up to their sum (2 x), and the other 2 x allows for
d_oracle being a maximum over a small sample.
"""
import numpy as np

from oracle import atari as oa

import atari_ref as ar

TABLE_SIZE = 1 << 21
TABLE_SEED = 124
SIGMA = 0.02
STAT_FRAMES = 16

# per-section scale of make_theta (see the module docstring); BN weights are drawn apart
SCALES = {"c1.w": 0.05, "c1.b": 5.0, "bn1.b": 0.5, "c2.w": 0.1, "c2.b": 0.5, "bn2.b": 0.5, "fc.w": 0.03, "fc.b": 0.5,
          "bn3.b": 0.5, "head.w": 0.04, "head.b": 0.8}


def _case(name, n_act, E, n_lanes, T, theta_seed, seed, lane_offset=0, jiggle=True, env_seed=9):
    return dict(name=name, n_act=n_act, E=E, n_lanes=n_lanes, T=T, theta_seed=theta_seed, seed=seed,
                lane_offset=lane_offset, jiggle=jiggle, env_seed=env_seed)


# name, n_act, envs_per_lane, n_lanes, T, theta_seed, action seed
CASES = [
    # shapes at 9 lanes: every n_act of {1, 2, 7, 31, 32} and every E of {1, 2, 4}, the corners (1,4), (32,4), (32,1)
    _case("A1_E4", 1, 4, 9, 2, 1, 1),
    _case("A2_E1", 2, 1, 9, 2, 8, 41, jiggle=False),
    _case("A7_E2", 7, 2, 9, 2, 1, 1),
    _case("A31_E2", 31, 2, 9, 2, 1, 3, jiggle=False),
    _case("A32_E4", 32, 4, 9, 2, 2, 278),
    _case("A32_E1", 32, 1, 9, 2, 1, 265),
    # lane counts at E = 2: the conv kernel's lane = (slot / E) * 8 + xcd and its early return (9 lanes: A7_E2)
    _case("L1", 7, 2, 1, 2, 1, 91),
    _case("L7", 7, 2, 7, 2, 1, 1, jiggle=False),
    _case("L8", 7, 2, 8, 2, 1, 3),
    _case("L17", 7, 2, 17, 2, 1, 1),
    # step counts; global env ids (lane_offset + l) * E + e that cross 2^31 and 2^32 inside the launch
    _case("T1", 7, 2, 4, 1, 1, 3),
    _case("T3_2p31", 7, 2, 4, 3, 1, 1, lane_offset=(1 << 30) - 2),
    _case("T3_2p32", 7, 2, 4, 3, 1, 1, lane_offset=(1 << 31) - 2, jiggle=False),
]
BY_NAME = {c["name"]: c for c in CASES}


def tol(d_oracle, scale=1.0):
    return max(4.0 * float(d_oracle), 2.0 ** -23 * float(scale))


_TABLE = []


def table():
    if not _TABLE:
        _TABLE.append(np.random.RandomState(TABLE_SEED).randn(TABLE_SIZE).astype(np.float32))
    return _TABLE[0]


def make_theta(n_act, seed):
    rs = np.random.RandomState(1000 + seed)
    parts = []
    for name, shape in oa.layout(n_act):
        n = int(np.prod(shape))
        if name in ("bn1.w", "bn2.w", "bn3.w"):
            v = rs.uniform(0.5, 1.5, n) * rs.choice([-1.0, 1.0], n)
            v[rs.randint(n)] = 0.0
        else:
            v = SCALES[name] * rs.randn(n)
        parts.append(v)
    return np.concatenate(parts).astype(np.float32)


def make_stats(theta, n_act, env_seed, first_env, seed):
    rs = np.random.RandomState(2000 + seed)
    envs = np.uint64(first_env) + np.arange(STAT_FRAMES // 2, dtype=np.uint64)
    fr = np.concatenate([oa.frames(env_seed, envs, 0), oa.frames(env_seed, envs, 1)])
    rm, rv = ar.compute_vbn(ar.unflatten(theta, n_act), np.zeros(304), np.ones(304), fr, 1.0)
    rv = rv * rs.uniform(0.5, 2.0, 304)
    rm = rm + rs.uniform(-0.5, 0.5, 304) * np.sqrt(rv)
    return rm.astype(np.float32), rv.astype(np.float32)


def lanes(n_lanes, P):
    """sign, deterministic and table offset of each lane: every lane differs from its neighbours."""
    sign = np.array([(1, -1, 0)[l % 3] for l in range(n_lanes)], np.int8)
    det = np.array([(0, 1, 1, 0)[l % 4] for l in range(n_lanes)], np.int8)
    span = TABLE_SIZE - P
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
        idx, sign, det = lanes(case["n_lanes"], theta.size)
        rm, rv = make_stats(theta, A, case["env_seed"], case["lane_offset"] * E, case["theta_seed"])
        _INPUTS[key] = dict(theta=theta, table=table(), idx=idx, sign=sign, det=det, rm=rm, rv=rv)
    return _INPUTS[key]


_REFS = {}


def reference(case):
    """(float64 reference, f32 oracle, d_oracle) of the case's rollout, computed once.
    d_oracle: {"probs": max |oracle - ref|, "ent": max |oracle - ref|}."""
    key = case["name"]
    if key not in _REFS:
        x = inputs(case)
        args = (x["theta"], x["table"], x["idx"], x["sign"], SIGMA, case["n_act"], case["E"], case["T"], case["seed"],
                case["env_seed"], x["rm"], x["rv"])
        kw = dict(deterministic=x["det"].astype(bool), jiggle=case["jiggle"], lane_offset=case["lane_offset"])
        ref = ar.evaluate_lanes(*args, **kw)
        orc = oa.evaluate_lanes(*args, record=True, **kw)
        d = dict(probs=float(np.abs(orc["probs"].astype(np.float64) - ref["probs"]).max()),
                 ent=float(np.abs(orc["ent"] - ref["ent"]).max()))
        _REFS[key] = (ref, orc, d)
    return _REFS[key]


# ---- forward / strategies: the A7_E2 theta and stats (7 actions, sensitive sections), frames of envs 0.. at step 0 ----
FORWARD_CASE = "A7_E2"
FORWARD_N = (1, 7, 8, 9)
STRATEGY_SHAPES = ((1, 1), (9, 1), (9, 9), (257, 2))   # (lanes, Z)


def env_frames(n, t=0):
    return oa.frames(BY_NAME[FORWARD_CASE]["env_seed"], np.arange(n, dtype=np.uint64), t).astype(np.float32)


def extreme_frames():
    """all 0, all 255, and one frame of each beside an env frame in the same call"""
    z = np.zeros((1, 4, 84, 84), np.float32)
    return {"zeros": np.repeat(z, 2, 0), "full": np.repeat(z + 255, 2, 0),
            "mixed": np.concatenate([z, env_frames(1), z + 255])}


def forward_reference(frames):
    """-> (probs f64 [n, A], feat f64 [n, 2592], d_oracle {"probs": abs, "feat": relative to each frame's largest
    |feature|}) for FORWARD_CASE's theta (unperturbed) and stats."""
    c = BY_NAME[FORWARD_CASE]
    x = inputs(c)
    A = c["n_act"]
    pr, ft = ar.forward(ar.unflatten(x["theta"], A), ar.split_bn(x["rm"], x["rv"]), frames)
    po, fo = oa.forward(oa.unflatten(x["theta"], A), oa.split_bn(x["rm"], x["rv"]), frames)
    pr, ft = pr.numpy(), ft.numpy()
    d = dict(probs=float(np.abs(po.numpy() - pr).max()), feat=feat_distance(fo.numpy(), ft))
    return pr, ft, d


def feat_distance(got, ref):
    """largest |got - ref| of a frame relative to the frame's largest |ref| (a frame whose features are all 0: absolute)"""
    ref = np.asarray(ref, np.float64)
    scale = np.maximum(np.abs(ref).max(-1), 1e-300)
    return float((np.abs(np.asarray(got, np.float64) - ref).max(-1) / scale).max())


def strategy_lanes(n_lanes):
    """The lanes whose strategies are compared: all of a small launch; of 257 the first chunk's first 9, its last two
    (255 is the chunk's last, 256 the lone lane of the second chunk) -- and lane 254 beside them."""
    return list(range(n_lanes)) if n_lanes <= 9 else list(range(9)) + [254, 255, 256]
