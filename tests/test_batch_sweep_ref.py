"""tests/batch_sweep_ref.py on the CPU: the membership check of the pipelined test must reject what it is there to reject, and the launch-table
readers must read the names zly_op_kernel_name writes."""
import numpy as np
import pytest

import batch_sweep_ref as bs
from oracle_lib import DET_DTYPE


def _dets(rows, ts=0):
    d = np.zeros(len(rows), dtype=DET_DTYPE)
    for i, (x, conf, cls) in enumerate(rows):
        d[i]["x"], d[i]["y"], d[i]["w"], d[i]["h"], d[i]["confidence"], d[i]["class_id"], d[i]["timestamp"] = x, 0.5, 0.1, 0.2, conf, cls, ts
    return d, len(rows)


def _table():
    """two frames, three batch sizes; frame 0 gives the same result at n = 1 and n = 3, frame 1 differs from frame 0 everywhere"""
    return {0: {1: _dets([(0.25, 0.9, 3)]), 2: _dets([(0.25, 0.8984375, 3)]), 3: _dets([(0.25, 0.9, 3)])},
            1: {1: _dets([(0.75, 0.7, 5), (0.1, 0.6, 1)]), 2: _dets([(0.75, 0.7, 5)]), 3: _dets([])}}


def test_membership_accepts_any_batch_size_of_the_frame_and_ignores_the_timestamp():
    t = _table()
    assert bs.matching_batch_sizes(_dets([(0.25, 0.9, 3)], ts=1_700_000_000_000), t[0]) == [1, 3]
    assert bs.matching_batch_sizes(_dets([(0.25, 0.8984375, 3)]), t[0]) == [2]
    assert bs.matching_batch_sizes(_dets([]), t[1]) == [3]
    got = bs.check_membership([(0, _dets([(0.25, 0.9, 3)], ts=7)), (1, _dets([(0.75, 0.7, 5)])), (1, _dets([]))], t)
    assert got == [[1, 3], [2], [3]]


def test_membership_rejects_a_result_that_matches_no_batch_size():
    t = _table()
    one_ulp = np.nextafter(np.float32(0.9), np.float32(1.0))
    for wrong in (_dets([(0.25, one_ulp, 3)]),                  # one ulp in the confidence
                  _dets([(0.25, 0.9, 4)]),                      # another class
                  _dets([(0.25, 0.9, 3), (0.25, 0.9, 3)]),      # one detection too many
                  (_dets([(0.25, 0.9, 3)])[0], 2),              # the right detections under a wrong count
                  _dets([])):
        assert bs.matching_batch_sizes(wrong, t[0]) == []
        with pytest.raises(AssertionError, match="equals no batch size's entry"):
            bs.check_membership([(0, _dets([(0.25, 0.9, 3)])), (0, wrong)], t)


def test_membership_rejects_another_frames_entry():
    t = _table()
    swapped = _dets([(0.75, 0.7, 5)])                             # frame 1 at n = 2, returned for a ticket of frame 0
    assert bs.matching_batch_sizes(swapped, t[1]) == [2] and bs.matching_batch_sizes(swapped, t[0]) == []
    with pytest.raises(AssertionError, match=r"result 0 of frame 0 .* equals an entry of frame\(s\) \[1\]"):
        bs.check_membership([(0, swapped)], t)


def test_slab_records():
    hdr_t = np.dtype([("n_kept", "<i4"), ("n_candidates", "<i4"), ("flags", "<u4"), ("frame_tag", "<u4")])
    h = np.array([(1, 4, 0, 9)], dtype=hdr_t)[0]
    g = np.array([(1, 4, 0, 2)], dtype=hdr_t)[0]
    c = np.array([(1, 5, 0, 9)], dtype=hdr_t)[0]
    a, b = _dets([(0.25, 0.9, 3)], ts=1)[0], _dets([(0.25, 0.9, 3)], ts=2)[0]
    assert bs.slab_key(h, a) == bs.slab_key(h, b) and a["timestamp"][0] == 1          # the timestamp apart, the caller's array untouched
    assert bs.slab_key(h, a) != bs.slab_key(g, a) and bs.slab_key(h, a, with_tag=False) == bs.slab_key(g, a, with_tag=False)
    assert bs.slab_key(h, a) != bs.slab_key(c, a) and bs.slab_key(h, a) != bs.slab_key(h, _dets([(0.25, 0.9, 4)])[0])
    assert bs.same_slab((h, a), (h, b)) and not bs.same_slab((h, a), (g, a)) and not bs.same_slab((h, a), (c, a))


def test_launch_table_readers():
    back = "c2f_kernel<C=32,NW=16,bottleneck+cv2,13x26 tiles>"
    front = "c2f_kernel<C=32,NW=8,cv1+bottleneck,8x16 tiles>"
    whole = "c2f_kernel<C=32,NW=8,cv1+bottleneck+cv2,12x13 tiles>"
    c16 = "c2f_kernel<C=16,cv1+bottleneck+cv2,8x32 tiles>"
    assert bs.c2f_shape(back) == (32, 16, 13, 26) and bs.c2f_shape(c16) == (16, None, 8, 32) and bs.c2f_shape("conv3x3_ws_kernel<TPW=2,4 channel tiles>") is None
    assert bs.carries_to_cv2(back) and bs.carries_to_cv2(whole) and not bs.carries_to_cv2(front) and not bs.carries_to_cv2(c16)
    assert bs.pixel_tiles_per_wave(back) == (22, 16) and bs.pixel_tiles_per_wave(whole) == (10, 8)
    names = ["model.4.cv1", "model.4.m.0.cv1", "model.22.cv2.0.1+x", "detect.tail.P3"]
    tables = {1: [front, "(fused into the C2f kernel at model.4.cv1)", "conv_igemm_multi_kernel<CT=2> (the 6 Detect branch convs)", "head_fused_kernel"],
              2: [front, "(fused into the C2f kernel at model.4.cv1)", bs.TAIL_BOX_NOTE, "head_fused_kernel (+ box conv in k-step order P3:ws)"],
              3: ["conv1x1_ws_kernel<NK=2,4 channel tiles,64 px>", "bottleneck_pair_kernel<32>", bs.TAIL_BOX_NOTE, "head_fused_kernel"]}
    ids, count = bs.table_ids(tables)
    assert ids == {1: 0, 2: 1, 3: 2} and count == 3 and bs.table_ids({1: ["a"], 2: ["b"], 5: ["a"]}) == ({1: 0, 2: 1, 5: 0}, 2)
    assert bs.fused_block_names(names, tables) == {"model.4.cv1": {1: front, 2: front}}
    assert bs.count_launches(tables[1], "conv_igemm_multi_kernel") == 1 and bs.count_launches(tables[2], "head_fused_kernel") == 1
    assert bs.tail_box_levels(names, tables[1]) == [] and bs.tail_box_levels(names, tables[2]) == [0]
