"""The pair rollout kernel's counter word by addition (fdr_rollout_pair.hip, FDR_PAIR_CTR_ADD) in numpy uint64.

hash_ctr_word(key, lane, t, k) = key + ((lane << 32) | (t << 4) | k) * G mod 2^64 (fdr_common.h, oracle/rng.py).  The
kernel's thread holding draw (step offset ds, dim dk) of a batch forms A = key + ((lane << 32) | (ds << 4) | dk) * G
once (hash_ctr_base) and adds kStepsPerBatch * 16 * G per batch; the word it reaches must be the word formed afresh,
bit for bit, for every key / lane / draw slot, from any batch start, after 1, 2 and 200 batches.  The jiggle bit's word
(t = kJiggleT, k = 15) is formed by hash_ctr_word as before and shares no state with the running word.
"""
import numpy as np
import pytest

from oracle import rng as orng

G = np.uint64(0x9E3779B97F4A7C15)
STEPS_PER_BATCH = 5  # 32 // 6 draws per step (NA = 6)
K_JIGGLE_T = (1 << 28) - 1

KEYS = [0, 2 ** 64 - 1, 0x243F6A8885A308D3]  # the last: an arbitrary ("random") key
LANES = [0, 1, 2 ** 31 - 1, 2 ** 32 - 1]
STARTS = [0, 5, 995, 2 ** 27]


def word(key, lane, t, k):
    """hash_ctr_word in Python integers (no numpy: the reference of this test)"""
    c = (lane << 32) | (t << 4) | k
    return (key + c * int(G)) % 2 ** 64


def base(key, lane, low):
    """hash_ctr_base: uint64 arithmetic as the device does it"""
    with np.errstate(over="ignore"):
        return np.uint64(key) + ((np.uint64(lane) << np.uint64(32)) | np.uint64(low)) * G


def oracle_word(key, lane, t, k):
    """the word oracle/rng.py's hash_bits feeds to mix64, for a given key"""
    with np.errstate(over="ignore"):
        return int(np.uint64(key) + orng.counter(lane, t, k) * np.uint64(orng.GOLDEN))


def test_oracle_rng_word_is_the_reference_word():
    """the formula this file restates is the one the oracle's stream uses"""
    assert int(G) == orng.GOLDEN and K_JIGGLE_T == orng.JIGGLE_T
    for key in KEYS:
        for lane in LANES:
            for t, k in ((0, 0), (777, 3), (2 ** 27 + 1004, 5), (K_JIGGLE_T, 15)):
                assert oracle_word(key, lane, t, k) == word(key, lane, t, k)


@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("lane", LANES)
def test_recurrence_equals_the_word_formed_afresh(key, lane):
    inc = np.uint64((STEPS_PER_BATCH * 16 * int(G)) % 2 ** 64)
    with np.errstate(over="ignore"):
        for st in STARTS:
            for ds in range(STEPS_PER_BATCH):
                for dk in range(6):
                    # the running word at batch start st: base word plus st steps
                    w = base(key, lane, (ds << 4) | dk) + np.uint64(st) * np.uint64(16) * G
                    assert int(w) == word(key, lane, st + ds, dk)
                    done = 0
                    for n in (1, 2, 200):
                        for _ in range(n - done):
                            w = w + inc
                        done = n
                        t = st + n * STEPS_PER_BATCH + ds
                        assert int(w) == word(key, lane, t, dk), (hex(key), lane, st, ds, dk, n)


def test_first_batch_drawn_ahead():
    """the kernel's first draw_part(0): base word + one increment = hash_ctr_word(key, lane, kStepsPerBatch + ds, dk)"""
    inc = np.uint64((STEPS_PER_BATCH * 16 * int(G)) % 2 ** 64)
    with np.errstate(over="ignore"):
        for key in KEYS:
            for lane in LANES:
                for t in range(32):  # thread of the half; threads 30, 31 hold draws of a sixth step nobody reads
                    ds, dk = t // 6, t % 6
                    w = base(key, lane, (ds << 4) | dk) + inc
                    assert int(w) == word(key, lane, STEPS_PER_BATCH + ds, dk)


def test_no_carry_into_the_lane_bits_up_to_the_jiggle_step():
    """(t << 4) | k stays below 2^32 for every t <= kJiggleT: the `|` with lane << 32 is an add, the word linear in t"""
    assert ((K_JIGGLE_T << 4) | 15) == 2 ** 32 - 1
    for lane in LANES:
        assert ((lane << 32) | (K_JIGGLE_T << 4) | 15) == (lane << 32) + (K_JIGGLE_T << 4) + 15


def test_jiggle_word_unaffected():
    """the jiggle bit reads hash_ctr(key, lane, kJiggleT, 15): no step of a rollout (t < 2^27 + 1005 here) reaches its
    word, whatever the running word went through"""
    for key in KEYS:
        for lane in LANES:
            jw = word(key, lane, K_JIGGLE_T, 15)
            assert jw == (key + ((lane << 32) | 0xFFFFFFFF) * int(G)) % 2 ** 64
            assert jw == oracle_word(key, lane, orng.JIGGLE_T, 15)
            # distinct counters give distinct words (G is odd: multiplication by it is a bijection mod 2^64)
            for st in STARTS:
                for n in (1, 2, 200):
                    t = st + n * STEPS_PER_BATCH + 4
                    assert t < K_JIGGLE_T and word(key, lane, t, 5) != jw
