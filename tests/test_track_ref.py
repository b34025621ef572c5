"""CPU tests of the tracking oracle (tests/track_ref.py) and of the crafted cases (tests/track_cases.py): the hand cases against their
hand-written ids, what the random scenes cover, and the harness's batch-composition invariance -- trivially true for the oracle, but it pins
the harness tests/test_gpu_track.py holds the GPU against."""
import numpy as np
import pytest

import track_cases as tc
import track_ref
import zly

HAND = tc.hand_cases()


@pytest.mark.parametrize("case", HAND, ids=[c.name for c in HAND])
def test_hand_case(case):
    t = track_ref.Tracker(case.T, case.cap, case.match_iou, case.max_lost)
    if case.first_id:
        t.reset(case.first_id)
    for k, f in enumerate(case.frames):
        got = t.step(f, None if case.n_kept is None else case.n_kept[k])
        assert got.tolist() == list(case.want[k]), f"{case.name}, frame {k}: {got.tolist()} != {case.want[k]}"
        assert all(i != 0 for i in got)


def test_tie_boxes_really_tie():
    a, b = track_ref.iou(tc.TIE_LEFT, tc.TIE_MID), track_ref.iou(tc.TIE_RIGHT, tc.TIE_MID)
    assert a.tobytes() == b.tobytes() and a == np.float32(0.6)
    assert track_ref.iou(tc.TIE_MID, tc.TIE_LEFT).tobytes() == a.tobytes()


def test_greedy_case_is_not_the_optimal_assignment():
    c = next(c for c in HAND if c.name == "greedy_not_optimal")
    t, d = c.frames[0], c.frames[1]
    box = lambda r: (r["x"], r["y"], r["w"], r["h"])
    v = [[float(track_ref.iou(box(d[i]), box(t[j]))) for j in range(2)] for i in range(2)]
    assert v[0][1] > v[0][0] > c.match_iou and v[1][1] > c.match_iou and v[1][0] == 0.0      # optimal: (d0, t0) + (d1, t1); greedy: (d0, t1) alone


def test_full_table_counts_evictions():
    c = next(c for c in HAND if c.name == "full_table_evicts_all")
    t = track_ref.Tracker(c.T, c.cap, c.match_iou, c.max_lost)
    for f in c.frames:
        t.step(f)
    assert t.state() == dict(frame_no=5, next_id=17, n_live=8, evictions=8)


def test_random_scenes_cover_the_tracker():
    cov = tc.coverage()
    for k, floor in tc.COVERAGE_FLOOR.items():
        assert cov[k] >= floor, (k, cov)
    for sc in tc.SCENES:
        frames, ids, _ = tc.scene(sc)
        assert len(frames) == sc.n_streams and all(len(f) == sc.n_frames for f in frames)
        assert all(len(f) <= sc.cap for fs in frames for f in fs)
        assert all((i != 0).all() for s in ids for i in s)
    # the scene on the 64-slot table uses the upper half of the wave: detections and slots beyond 32
    wide = next(sc for sc in tc.SCENES if sc.name == "wide_T64_cap64")
    assert max(len(f) for fs in tc.scene(wide)[0] for f in fs) > 32


def test_reset_keeps_or_sets_next_id():
    t = track_ref.Tracker(8, 8)
    t.step(tc.dets([tc.ROW8[0], tc.ROW8[1]]))
    t.reset(0)
    assert t.state() == dict(frame_no=0, next_id=3, n_live=0, evictions=0)
    assert t.step(tc.dets([tc.ROW8[0]])).tolist() == [3]
    t.reset(100)
    assert t.step(tc.dets([tc.ROW8[0]])).tolist() == [100]


@pytest.mark.parametrize("sc", tc.SCENES[:2], ids=[s.name for s in tc.SCENES[:2]])
def test_oracle_is_invariant_to_batch_composition(sc):
    frames, ids, _ = tc.scene(sc)
    rng = np.random.default_rng(5)
    # all streams interleaved in a shuffled order that keeps every stream's own order, with untracked frames in between
    seq = [s for s in range(sc.n_streams) for _ in range(sc.n_frames)]
    rng.shuffle(seq)
    nxt = [0] * sc.n_streams
    fl, sl, where = [], [], []
    for s in seq:
        if rng.random() < .2:
            fl.append(frames[s][0]); sl.append(-1); where.append(None)
        fl.append(frames[s][nxt[s]]); sl.append(s); where.append((s, nxt[s]))
        nxt[s] += 1
    trk = {s: track_ref.Tracker(sc.T, sc.cap, sc.match_iou, sc.max_lost) for s in range(sc.n_streams)}
    got = track_ref.run_streams(trk, fl, sl)
    for g, w in zip(got, where):
        if w is None:
            assert g is None
        else:
            assert g.tolist() == ids[w[0]][w[1]].tolist()


def test_slab_builders_round_trip():
    f = [tc.dets([tc.ROW8[0], tc.ROW8[1]]), tc.dets([])]
    raw = tc.build_slabs(f, 4)
    assert raw.shape == (2, 16 + 4 * 40) and (raw[0, 16 + 80:] == tc.FILL).all()
    out = tc.with_ids(raw, [np.array([7, 9], dtype=np.uint32), None], 4)
    assert tc.slab_ids(out[0], 4).tolist() == [7, 9] and tc.slab_ids(out[1], 4).tolist() == []
    diff = np.flatnonzero(out != raw)
    assert diff.tolist() == [16 + 24, 16 + 40 + 24]                                # only the ids' low bytes
    hdr, d = zly.parse_slabs(out.reshape(-1), 2, 4)[0]
    assert int(hdr["n_kept"]) == 2 and d["track_id"].tolist() == [7, 9]
