"""CPU checks of the counter-based noise source: the numpy restatement (tests/philox_ref.py) against Random123's
published known answers and the normal moments, the fdr_noise_fill ABI's argument checks, and the source predicates.
No GPU: the kernel itself is held to the restatement in tests/test_gpu_counter_noise.py."""
import ctypes

import numpy as np

import philox_ref
from philox_ref import MOMENT_FIRST, MOMENT_P, MOMENT_ROWS, MOMENT_SEED


def _words(ctr, key):
    return [int(w) for w in philox_ref.philox4x32_10(ctr, key)]


def test_random123_known_answers():
    """philox4x32-10 of Random123's kat_vectors."""
    assert _words((0, 0, 0, 0), (0, 0)) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    ones = 0xffffffff
    assert _words((ones,) * 4, (ones, ones)) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    assert _words((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0)) == \
        [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


def test_restatement_rows_are_pure_and_laid_out_by_quads():
    eps, r = philox_ref.rows(123, [5, 2 ** 32, 5], 8)
    assert eps.shape == r.shape == (3, 8)
    np.testing.assert_array_equal(eps[0], eps[2])
    x = philox_ref.philox4x32_10((1, 0, 1, 0), (123, 0))   # row id 2^32, quad 1
    z0, z1, rr = philox_ref._pair(x[0], x[1])
    assert eps[1, 4] == z0 and eps[1, 5] == z1 and r[1, 4] == r[1, 5] == rr
    # a longer stride continues the row's stream: the first elements do not move
    np.testing.assert_array_equal(philox_ref.rows(123, [5], 16)[0][0, :8], eps[0])


def test_restatement_moments():
    ids = np.arange(MOMENT_ROWS, dtype=np.uint64) + np.uint64(MOMENT_FIRST)
    eps, _ = philox_ref.rows(MOMENT_SEED, ids, MOMENT_P)
    assert eps.size == 1047824
    zm, zv, z4 = philox_ref.moments_z(eps)
    print("restatement moments (sigma units): mean %.2f  var %.2f  m4 %.2f" % (zm, zv, z4))
    assert abs(zm) <= 5 and abs(zv) <= 5 and abs(z4) <= 5


def test_noise_fill_is_exported_and_validates_without_gpu():
    """Invalid calls are rejected, and an empty one accepted, before any device work."""
    from fdr import _lib
    assert "fdr_noise_fill" in _lib.EXPORTS
    fill = _lib.lib.fdr_noise_fill
    buf = (ctypes.c_float * 8)()                        # a non-NULL, 16-byte aligned address; never written
    out = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15) if ctypes.addressof(buf) % 16 else \
        ctypes.cast(buf, ctypes.c_void_p)
    assert fill(None, 123, None, 0, 1, 5, 8, None, None) == _lib.FDR_ERR_INVALID
    assert b"out" in _lib.lib.fdr_last_error()
    assert fill(None, 123, None, 0, 1, 5, 6, out, None) == _lib.FDR_ERR_INVALID
    assert b"row_stride" in _lib.lib.fdr_last_error()
    assert fill(None, 123, None, 0, 1, 5, 4, out, None) == _lib.FDR_ERR_INVALID      # below n_params rounded up
    assert fill(None, 123, None, 0, -1, 5, 8, out, None) == _lib.FDR_ERR_INVALID
    assert b"n_rows" in _lib.lib.fdr_last_error()
    assert fill(None, 123, None, 0, 1, 0, 8, out, None) == _lib.FDR_ERR_INVALID
    assert b"n_params" in _lib.lib.fdr_last_error()
    assert fill(None, 123, None, 0, 0, 5, 8, out, None) == _lib.FDR_OK


def test_counter_source_is_neither_table_nor_host():
    from utils.noise_sources import (CounterNoiseSource, is_counter_noise, is_device_table, is_host_noise,
                                     require_noise_source)
    src = CounterNoiseSource(6092, random_seed=123)
    assert is_counter_noise(src) and not is_host_noise(src) and not is_device_table(src)
    require_noise_source(src, "test")
    assert src.row_stride == 6092 and CounterNoiseSource(5).row_stride == 8 and CounterNoiseSource(1).row_stride == 4
    assert src.next_id == 0
    np.testing.assert_array_equal(src.peek_ids(3), np.array([0, 1, 2], np.uint64))
    assert src.next_id == 0
    ids = src.sample_ids(3)
    assert ids.dtype == np.uint64 and list(ids) == [0, 1, 2] and src.next_id == 3
    assert list(src.sample_ids(2)) == [3, 4]


def test_counter_source_refuses_a_buffer_above_max_bytes():
    import pytest
    from utils.noise_sources import CounterNoiseSource
    src = CounterNoiseSource(1000, max_bytes=1 << 20)
    with pytest.raises(ValueError, match=r"1052000.*1048576"):
        src.rows(0, 263)      # 263 rows x 1000 x 4 bytes: refused before any device work
