"""The greedy-NMS checker (tests/nms_checker.py) accepts the oracle's answer and rejects the two one-box perturbations of it, on
slide-like sets of ~32 k boxes: that is what lets tests/test_gpu_nms_grid.py verify results at sizes the O(M x kept) oracle cannot
serve.  CPU only."""
import numpy as np
import pytest

from hd_yolo_amd import synth
from nms_checker import assert_is_greedy_nms, is_greedy_nms
from oracle import nms_ref


@pytest.mark.parametrize('seed', [1, 2])
def test_checker_accepts_the_oracle_and_rejects_perturbations(seed):
    b, s = synth.synth_slide_boxes(16000, 4000, seed)
    assert 30000 < len(b) < 34000
    thr = 0.45
    k = nms_ref.nms_c(b, s, thr)
    assert_is_greedy_nms(b, s, thr, k)
    ok, why = is_greedy_nms(b, s, thr, np.delete(k, 100))                     # one kept row dropped
    assert not ok and 'violate' in why
    rank = np.argsort(np.argsort(-s, kind='stable'), kind='stable')
    sup = np.setdiff1d(np.arange(len(b)), k)[:1]                              # one suppressed row added, in its rank position
    k2 = np.concatenate([k, sup])
    k2 = k2[np.argsort(rank[k2])]
    ok, why = is_greedy_nms(b, s, thr, k2)
    assert not ok and 'violate' in why
    ok, why = is_greedy_nms(b, s, thr, k[::-1])                               # right set, wrong order
    assert not ok and 'order' in why


def test_checker_on_improper_boxes_and_small_sets():
    b = np.array([[0, 0, 10, 10], [1, 1, 11, 11], [5, 5, 5, 9], [9, 9, 3, 3], [100, 100, 110, 110]], np.float32)
    s = np.array([0.9, 0.8, 0.7, 0.6, 0.5], np.float32)
    k = nms_ref.nms_c(b, s, 0.5)
    assert list(k) == [0, 2, 3, 4]                                            # zero-area and inverted boxes never interact
    assert_is_greedy_nms(b, s, 0.5, k)
    assert not is_greedy_nms(b, s, 0.5, [0, 1, 2, 3, 4])[0]
    assert_is_greedy_nms(b[:1], s[:1], 0.5, [0])
    assert_is_greedy_nms(b[:0], s[:0], 0.5, [])
