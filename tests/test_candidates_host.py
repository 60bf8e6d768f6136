"""CPU: the candidate entry points' ABI surface and the NumPy restatement of the top-K peak rule
(tests/cand_ref.py) on hand-built maps with known answers."""
import os
import re

import numpy as np

from cand_ref import find_peaks, topk_peaks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mq_decode_udp_topk", "mq_viterbi_filter_multi", "mq_triangulate_possible")


def test_entry_points_declared_and_bound():
    from mqhip import _lib
    header = open(os.path.join(ROOT, "include", "mq_hip.h")).read()
    for name in NAMES:
        assert name in _lib.EXPORTED and name in _lib._SIGS, name
        m = re.search(r"int %s\(([^;]*)\);" % name, header)
        assert m, f"{name} is not declared in include/mq_hip.h"
        assert len(m.group(1).split(",")) == len(_lib._SIGS[name][1]), name
    assert _lib.ABI_VERSION == 8
    assert re.search(r"#define MQ_ABI_VERSION 8\b", header)


def _map():
    return np.zeros((8, 6), dtype=np.float32)   # 8 rows, 6 columns: flat index = 6 * y + x


def test_plateau_gives_one_peak_at_the_lower_index():
    H = _map()
    H[3, 2] = H[3, 3] = 0.5
    assert find_peaks(H) == [3 * 6 + 2]
    peak, score = topk_peaks(H, 3)
    np.testing.assert_array_equal(peak, [20, -1, -1])
    np.testing.assert_array_equal(score, np.array([0.5, 0, 0], dtype=np.float32))


def test_corner_peak():
    H = _map()
    H[7, 5] = 0.9
    H[0, 0] = 0.4
    assert find_peaks(H) == [0, 47]
    peak, score = topk_peaks(H, 2)
    np.testing.assert_array_equal(peak, [47, 0])
    np.testing.assert_array_equal(score, np.array([0.9, 0.4], dtype=np.float32))


def test_near_maximum_suppressed_far_lower_one_taken():
    H = _map()
    H[1, 1] = 1.0
    H[1, 3] = 0.8      # 2 px from the first: suppressed at min_sep = 3
    H[7, 1] = 0.3      # 6 px away: taken
    assert find_peaks(H) == [7, 9, 43]
    peak, score = topk_peaks(H, 3, min_sep=3)
    np.testing.assert_array_equal(peak, [7, 43, -1])
    np.testing.assert_array_equal(score, np.array([1.0, 0.3, 0], dtype=np.float32))
    peak, _ = topk_peaks(H, 3, min_sep=1)
    np.testing.assert_array_equal(peak, [7, 9, 43])


def test_fewer_peaks_than_slots():
    H = _map()
    H[2, 2] = 0.6
    H[6, 4] = 0.2
    peak, score = topk_peaks(H, 4)
    np.testing.assert_array_equal(peak, [14, 40, -1, -1])
    np.testing.assert_array_equal(score, np.array([0.6, 0.2, 0, 0], dtype=np.float32))
    peak, score = topk_peaks(H, 4, min_score=0.25)     # the lower one is not above min_score
    np.testing.assert_array_equal(peak, [14, -1, -1, -1])


def test_all_negative_map_has_no_peaks():
    H = -np.ones((8, 6), dtype=np.float32)
    H[4, 4] = -0.25
    assert find_peaks(H) == []
    assert find_peaks(H, min_score=-1.0) == []          # the maximum is <= max(0, min_score)
    peak, score = topk_peaks(H, 3)
    np.testing.assert_array_equal(peak, [28, -1, -1])   # slot 0 stays the first argmax (mq_decode_udp)
    np.testing.assert_array_equal(score, np.array([-0.25, 0, 0], dtype=np.float32))
