"""numpy restatement of the counter-based noise generator (include/fdr.h fdr_noise_fill).

TEST INFRASTRUCTURE ONLY: written from the definition, nothing shared with csrc/fdr_noise_fill.hip.

    philox4x32_10   the integer block function, uint64 arithmetic and masks; arrays of counters at once
    rows            [n_rows, row_stride] f64 normals + each element's Box-Muller radius r

Row id d under seed s, element quad j (elements 4j .. 4j+3):
    counter = (j, d & 0xffffffff, d >> 32, 0)      key = (s & 0xffffffff, s >> 32)
    round:  c <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)),  k <- k + (W0, W1);  10 rounds
    pairs (x0, x1), (x2, x3):  u1 = ((a >> 8) + 1) 2^-24,  u2 = (b >> 8) 2^-24,  r = sqrt(-2 log u1),
                               (z0, z1) = (r cos(2 pi u2), r sin(2 pi u2))
The normals are computed in f64 (u1, u2 are exact there too), so this is the generator's real-arithmetic value to
~1e-16: the yardstick the f32 kernel is held to.
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)
# the moments case the CPU and the GPU test share: 172 x 6092 = 1,047,824 normals, ids across the 32-bit carry
MOMENT_SEED, MOMENT_ROWS, MOMENT_FIRST, MOMENT_P = 123, 172, 2 ** 32 - 3, 6092


def philox4x32_10(ctr, key):
    """ctr: four uint32-valued arrays (or ints) of one shape, key: two -> the four output words as uint64 arrays
    holding 32-bit values."""
    c = [np.asarray(v, dtype=np.uint64) & MASK for v in np.broadcast_arrays(*ctr)]
    k0, k1 = (int(v) & 0xFFFFFFFF for v in key)
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]      # < 2^64: both factors are below 2^32
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> S32) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> S32) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0 = (k0 + W0) & 0xFFFFFFFF
        k1 = (k1 + W1) & 0xFFFFFFFF
    return c


def _pair(a, b):
    u1 = ((a >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24
    u2 = (b >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    r = np.sqrt(-2.0 * np.log(u1))
    ang = 2.0 * np.pi * u2
    return r * np.cos(ang), r * np.sin(ang), r


def rows(seed, ids, row_stride):
    """(eps, r) f64 [len(ids), row_stride]: the normals of each row id and the radius each element was scaled by."""
    assert row_stride % 4 == 0
    ids = [int(d) & 0xFFFFFFFFFFFFFFFF for d in ids]
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    q = row_stride // 4
    j = np.tile(np.arange(q, dtype=np.uint64), len(ids))
    d_lo = np.repeat(np.array([d & 0xFFFFFFFF for d in ids], np.uint64), q)
    d_hi = np.repeat(np.array([d >> 32 for d in ids], np.uint64), q)
    x = philox4x32_10((j, d_lo, d_hi, np.zeros_like(j)), (seed & 0xFFFFFFFF, seed >> 32))
    z0, z1, ra = _pair(x[0], x[1])
    z2, z3, rb = _pair(x[2], x[3])
    eps = np.stack([z0, z1, z2, z3], axis=1).reshape(len(ids), row_stride)
    r = np.stack([ra, ra, rb, rb], axis=1).reshape(len(ids), row_stride)
    return eps, r


def moments_z(x):
    """(mean sqrt(N), (var - 1) / sqrt(2 / N), (m4 - 3) / sqrt(96 / N)) of a sample of standard normals: each is
    ~N(0, 1) when the sample is (Var of the sample variance 2 / N, of the fourth central moment 96 / N)."""
    x = np.asarray(x, np.float64).reshape(-1)
    n = x.size
    m = x.mean()
    c = x - m
    return m * np.sqrt(n), ((c ** 2).mean() - 1.0) / np.sqrt(2.0 / n), ((c ** 4).mean() - 3.0) / np.sqrt(96.0 / n)
