"""CPU: the host side of fdr_rollout_episodes -- the stream-id builder, the export, and the seeds of the GPU file's
oracle comparisons (tests/test_gpu_rollout_episodes.py), verified on the CPU restatement where they are used."""
import numpy as np
import pytest

import episodes_ref as eref
from worker.worker import crn_mode, episode_stream_ids


def test_ids_by_hand():
    sign = np.array([1, -1, 1, -1, 0, 0], np.int8)
    assert episode_stream_ids(False, sign, 0, 3, 2) is None
    np.testing.assert_array_equal(episode_stream_ids("pair", sign, 0, 3, 2),
                                  [[0, 1, 2], [0, 1, 2], [6, 7, 8], [6, 7, 8], [12, 13, 14], [15, 16, 17]])
    np.testing.assert_array_equal(episode_stream_ids(True, sign, 4, 2, 2),
                                  [[8, 9], [8, 9], [12, 13], [12, 13], [16, 17], [18, 19]])
    np.testing.assert_array_equal(episode_stream_ids("batch", sign, 4, 2, 2), [[0, 1]] * 6)
    # one lane per direction: a lane shares with nobody
    np.testing.assert_array_equal(episode_stream_ids("pair", sign[:3], 5, 1, 1), [[5], [6], [7]])
    ids = episode_stream_ids("pair", sign, 0, 3, 2)
    assert ids.dtype == np.int64 and ids.flags.c_contiguous
    assert episode_stream_ids("batch", sign, 0, 3, 2).flags.c_contiguous


@pytest.mark.parametrize("mode", ["pair", "batch"])
@pytest.mark.parametrize("lane_offset,K,lpd", [(0, 1, 2), (32, 3, 2), (12, 4, 4), (7, 2, 1)])
def test_ids_against_the_rule(mode, lane_offset, K, lpd):
    rs = np.random.RandomState(3)
    sign = rs.choice(np.array([1, -1, 0], np.int8), size=24)
    np.testing.assert_array_equal(episode_stream_ids(mode, sign, lane_offset, K, lpd),
                                  eref.expected_ids(mode, sign, lane_offset, K, lpd))


def test_ids_are_functions_of_the_global_lane():
    sign = np.tile(np.array([1, -1], np.int8), 16)
    whole = episode_stream_ids("pair", sign, 0, 3, 2)
    np.testing.assert_array_equal(episode_stream_ids("pair", sign[16:], 16, 3, 2), whole[16:])


def test_id_errors():
    sign = np.ones(4, np.int8)
    for mode in (False, "pair", "batch"):
        with pytest.raises(ValueError, match="multiple of lanes_per_dir"):
            episode_stream_ids(mode, sign, 3, 2, 2)
    with pytest.raises(ValueError, match="2\\^32"):
        episode_stream_ids("pair", sign, (1 << 32) // 4, 4, 2)
    with pytest.raises(ValueError):
        episode_stream_ids("rows", sign, 0, 1, 1)
    assert crn_mode(True) == "pair" and crn_mode(False) is False and crn_mode("batch") == "batch"


def test_export_is_declared():
    from fdr import _lib
    assert "fdr_rollout_episodes" in _lib.EXPORTS and hasattr(_lib.lib, "fdr_rollout_episodes")


@pytest.mark.parametrize("mode,seed,n_border", eref.ORACLE_CASES)
def test_oracle_case_seeds(mode, seed, n_border):
    (idx, sign, det), ids, o = eref.cartpole_case(mode, seed)
    assert len(idx) == eref.CASE_LANES and ids.shape == (eref.CASE_LANES, eref.CASE_K)
    print("mode %r seed %d: %d borderline lanes, steps %d .. %d" % (mode, seed, o["borderline"].sum(),
                                                                   o["steps"].min(), o["steps"].max()))
    assert int(o["borderline"].sum()) == n_border
    assert n_border <= 2
    assert o["steps"].max() < eref.CASE_K * 500     # no lane rides the time limit in all its episodes
    if mode == "pair":      # partners share the reset and the draws, yet their episodes are not all the same
        assert np.any(o["steps"][0::2] != o["steps"][1::2])
