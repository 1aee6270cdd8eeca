"""Inputs of the auxiliary-kernel edge tests (tests/test_aux_ref.py on the CPU, test_gpu_novelty_edges.py,
test_gpu_obs_stats_edges.py, test_gpu_mlp_vbn_edges.py on the device).  Everything is built deterministically from
RandomState seeds (a case's seed is the CRC32 of its name); pure numpy.

Distances.  strategy_dist_kernel: one 256-thread block per strategy, wave w walks the archive entries h = w, w + 4, ..,
its 64 threads the probe states z = lane, lane + 64, ..; one strategy (Z D <= 8192 floats) sits in LDS.  The shapes
(H, Z, D) therefore cross: H < 4 (waves without an entry), H = 1, H = 4 / 5 / 9 / 37 (one entry per wave, a second
round, a ragged last round), Z < 64, Z = 63 / 64 / 65 / 129 (a wave's threads partly idle, exactly full, one state
in the second round), Z D = 8192 both ways, D = 1.
"""
import zlib

import numpy as np

from oracle import policies as opol

F32 = np.float32
KINDS = ("tvd", "l2", "w2")
SHAPES = ((1, 1, 2), (3, 20, 2), (4, 63, 4), (5, 64, 6), (9, 65, 4), (37, 129, 2), (6, 2048, 4), (6, 128, 64),
          (5, 7, 1))
# (lo, hi, H): archive rows lo and hi are bit-equal.  2 / 6 and 0 / 8 sit in one wave; 1 / 6 in waves 1 and 2; 6 / 9
# in waves 2 and 1, the lower index in the wave the cross-wave scan meets second.
TIES = ((2, 6, 9), (1, 6, 9), (0, 8, 9), (6, 9, 10))
NAN_ARCHIVE_ROWS = (7, 5, 9)        # of H = 12: 5 and 9 in wave 1, 7 in wave 3; the first NaN distance is h = 5


def _rs(name):
    return np.random.RandomState(zlib.crc32(name.encode()))


def _strategies(rs, kind, n, Z, D):
    """[n, Z, D] f32.  tvd / l2: entries in [0, 1); w2: [mean | std] with std = 0.55 + 0.45 tanh, as MujocoPolicy."""
    if kind != "w2":
        return rs.rand(n, Z, D).astype(F32)
    k = D // 2
    mean = rs.randn(n, Z, k).astype(F32)
    std = (F32(0.55) + F32(0.45) * np.tanh(rs.randn(n, Z, k).astype(F32))).astype(F32)
    return np.concatenate([mean, std], -1)


def _names():
    out = []
    for H, Z, D in SHAPES:
        out += ["%s-%dx%dx%d" % (k, H, Z, D) for k in KINDS if k != "w2" or D % 2 == 0]
    out += ["w2-near"]
    out += ["%s-many" % k for k in KINDS]
    out += ["%s-tie%d_%d" % (k, lo, hi) for k in KINDS for lo, hi, _ in TIES]
    return out


def dist_case(name):
    """-> dict(name, kind, S [n, Z, D], B [H, Z, D], tie): tie = the lower index of a duplicated archive row, or None."""
    rs = _rs(name)
    kind, what = name.split("-")
    tie = None
    if what == "near":
        # W2 cancellation: B[0] = S[0] with stds * (1 + 1e-6) (s1 + s2 - 2 sqrt(s1 s2) ~ 1e-13 s), B[1] = other means,
        # exactly S[0]'s stds (the std terms cancel to 0), one std of exactly 0 on either side.
        H, Z, D, n = 5, 64, 6, 2
        S, B = _strategies(rs, kind, n, Z, D), _strategies(rs, kind, H, Z, D)
        B[0] = S[0]
        B[0, :, 3:] = (S[0, :, 3:] * F32(1 + 1e-6)).astype(F32)
        B[1, :, 3:] = S[0, :, 3:]
        B[2, 3, 3] = 0.0
        S[1, 5, 4] = 0.0
    elif what == "many":
        H, Z, D, n = 5, 20, 2, 70
        S, B = _strategies(rs, kind, n, Z, D), _strategies(rs, kind, H, Z, D)
    elif what.startswith("tie"):
        lo, hi = (int(v) for v in what[3:].split("_"))
        H = dict(((a, b), h) for a, b, h in TIES)[(lo, hi)]
        Z, D, n = 65, 4, 2
        B = _strategies(rs, kind, H, Z, D)
        B[hi] = B[lo]
        # S[0] is the duplicated row itself (distance 0 to both); S[1] sits next to it (equal non-zero distances)
        S = np.stack([B[lo], (B[lo] + F32(0.01) * rs.rand(Z, D).astype(F32)).astype(F32)])
        tie = lo
    else:
        H, Z, D = (int(v) for v in what.split("x"))
        n = 3 if Z * D < 8192 else 2
        S, B = _strategies(rs, kind, n, Z, D), _strategies(rs, kind, H, Z, D)
    return dict(name=name, kind=kind, S=S, B=B, tie=tie)


DIST_CASES = _names()


def nan_case(kind, where):
    """H = 12, Z = 65, D = 4, three strategies.  where = "strategy": S[1] has one NaN element, S[0] and S[2] are clean;
    "archive": rows NAN_ARCHIVE_ROWS of B have one each."""
    rs = _rs("%s-nan-%s" % (kind, where))
    S, B = _strategies(rs, kind, 3, 65, 4), _strategies(rs, kind, 12, 65, 4)
    if where == "strategy":
        S[1, 7, 2] = np.nan
    else:
        for r, h in enumerate(NAN_ARCHIVE_ROWS):
            B[h, 3 + 20 * r, r] = np.nan
    return dict(name="%s-nan-%s" % (kind, where), kind=kind, S=S, B=B, tie=None)


# ---- Welford merge ------------------------------------------------------------------------------------------------
MERGE_DIMS = (1, 63, 64, 65, 1024)
MERGE_NS = (0, 1, 5, 300)
MERGE_STARTS = (0, 7, 2 ** 24 + 1, 2 ** 31 + 5)
ORDER_CASE = dict(dim=17, n=5, start=7, zeros="none")


def _spread(rs, shape):
    """Signed values whose magnitudes span 1e-3 .. 1e4."""
    return (np.where(rs.rand(*shape) < 0.5, -1.0, 1.0) * 10.0 ** rs.uniform(-3, 4, size=shape)).astype(F32)


def merge_case(dim, n, start, zeros="none"):
    """-> ((mean0, m2_0, count0), mean [n, dim], m2 [n, dim], count [n] int32).  zeros: "none" | "all" |
    "ends" (counts zero at the first, a middle and the last lane)."""
    rs = _rs("merge-%d-%d-%d-%s" % (dim, n, start, zeros))
    mean, count = _spread(rs, (n, dim)), rs.randint(1, 2000, size=n).astype(np.int32)
    m2 = (rs.rand(n, dim) * count[:, None] * np.abs(mean)).astype(F32)
    if zeros == "all":
        count[:] = 0
    elif zeros == "ends":
        count[[0, n // 2, n - 1]] = 0
    if start == 0:
        acc = (np.zeros(dim, F32), np.zeros(dim, F32), 0)
    else:
        acc = (_spread(rs, (dim,)), (rs.rand(dim) * min(start, 1e6)).astype(F32), start)
    return acc, mean, m2, count


# ---- BN refresh ---------------------------------------------------------------------------------------------------
# name -> (n, n_in, momentum, columns, dead): columns = {index: "const" | "big"} (a constant column; mean 1e4, std 1),
# dead: hidden unit 5 of the first layer gets bias -1e3, so it is 0 over the whole batch.
VBN_CASES = {
    "n2": (2, 4, 0.1, {}, False),
    "n3_in1": (3, 1, 0.1, {}, False),
    "n255_const": (255, 4, 0.1, {1: "const"}, False),
    "n256_big": (256, 4, 0.1, {2: "big"}, False),
    "n257_dead": (257, 4, 0.1, {}, True),
    "n1000_in64": (1000, 64, 0.1, {0: "const", 63: "big"}, False),
    "n64_in63": (64, 63, 0.1, {62: "big"}, True),
    "n256_mom0": (256, 4, 0.0, {}, False),
    "n257_mom1": (257, 4, 1.0, {3: "const"}, False),
}
VBN_N_ACT = 2


def vbn_group(name):
    """"cols" where the input has a constant or a mean-1e4 column, else "plain" (aux_ref.BN_F32_FLOOR)."""
    return "cols" if VBN_CASES[name][3] else "plain"


def vbn_case(name):
    """-> (theta [P], x [n, n_in], rm, rv [n_in + 128], momentum), all f32."""
    n, n_in, momentum, columns, dead = VBN_CASES[name]
    rs = _rs("vbn-" + name)
    P = opol.num_params("discrete", n_in, VBN_N_ACT)
    theta = (rs.randn(P) * 0.3).astype(F32)
    w = opol.unflatten("discrete", n_in, VBN_N_ACT, theta)      # views of theta
    for i in range(3):
        w["bn%d.w" % i][:] = (1.0 + 0.2 * rs.randn(w["bn%d.w" % i].size)).astype(F32)
    if dead:
        w["l1.b"][5] = -1e3
    x = (rs.randn(n, n_in) * 2 + 0.5).astype(F32)
    for c, what in columns.items():
        x[:, c] = F32(1.7) if what == "const" else (1e4 + rs.randn(n)).astype(F32)
    rm = (rs.randn(n_in + 128) * 0.5).astype(F32)
    rv = (0.5 + rs.rand(n_in + 128)).astype(F32)
    return theta, x, rm, rv, momentum
