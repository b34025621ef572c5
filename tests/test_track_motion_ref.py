"""The motion oracle itself (tests/track_motion_ref.py) and the cases built on it (tests/track_motion_cases.py), without a GPU: the hand cases
against their hand-written ids -- and the plain oracle against its own where a case says what the plain tracker does instead --, v_max = 0 as
the bit-exact bridge to the plain oracle on every case and scene of tests/track_cases.py, THE RULE on interleaved streams, and fewer id
switches against ground truth than the plain tracker on the moving scenes."""
import numpy as np
import pytest

import track_cases as tc
import track_motion_cases as mc
import track_motion_ref as mr
import track_ref
from track_ref import F

HAND = mc.hand_cases()
by_name = {c.name: c for c in HAND}


def _bits(v):
    return np.asarray(v, dtype=np.float32).view(np.uint32).tolist()


@pytest.mark.parametrize("case", HAND, ids=[c.name for c in HAND])
def test_hand_case(case):
    motion, plain = mc.case_trackers(case)
    assert [g.tolist() for g in mc.run_case(case, motion)] == case.want
    if case.plain is not None:
        assert [g.tolist() for g in mc.run_case(case, plain)] == case.plain


def _final(name):
    t = mc.case_trackers(by_name[name])[0]
    mc.run_case(by_name[name], t)
    return t


def test_the_cases_do_what_their_names_say():
    t = _final("accelerating_box_keeps_id")
    assert t.counts["rescued"] >= 4 and t.read()["hits"].tolist() == [8]
    t = _final("gap_of_two_frames_reacquired")
    assert t.counts["coasted"] == 1 and t.counts["rescued"] == 1
    # hits == 1: the gain is 1 and the velocity is exactly fl(rx / 1)
    t = _final("first_match_takes_the_full_displacement")
    x0, x1 = (F(b[0]) for b in mc.STEP_03[:2])
    r = t.read()
    assert _bits(r["vx"]) == _bits([F(x1 - x0)]) and _bits(r["vy"]) == [0] and r["hits"].tolist() == [2] and _bits(r["x"]) == _bits([x1])
    t = _final("clamped_velocity_still_matches")
    assert t.counts["clamped"] == 6 and _bits(t.read()["vx"]) == _bits([F(0.03)])
    t = _final("clamped_velocity_loses_the_match")
    assert t.counts["clamped"] >= 1 and t.counts["births"] == 5
    t = _final("standing_box_keeps_zero_velocity")
    assert _bits(t.read()["vx"]) == [0] and _bits(t.read()["vy"]) == [0] and t.read()["hits"].tolist() == [4]
    t = _final("eviction_replaces_a_moving_track")
    r = t.read()
    assert t.evictions == 1 and len(r) == 8
    assert (int(r[0]["id"]), int(r[0]["class_id"]), int(r[0]["hits"]), _bits(r[0]["vx"]), _bits(r[0]["vy"])) == (9, 1, 1, 0, 0)
    assert r["hits"][1:].tolist() == [3] * 7
    t = _final("reset_mid_sequence")
    r = t.read()
    assert t.state() == dict(frame_no=3, next_id=3, n_live=1, evictions=0) and r["id"].tolist() == [2] and r["hits"].tolist() == [3]


def test_reset_clears_velocities_and_hits():
    t = mc.case_trackers(by_name["accelerating_box_keeps_id"])[0]
    mc.run_case(by_name["accelerating_box_keeps_id"], t)
    assert t.read()["vx"][0] > 0
    t.reset(0)
    assert len(t.read()) == 0 and not any(t.vx) and not any(t.vy) and not any(t.hits) and t.state() == dict(frame_no=0, next_id=2, n_live=0, evictions=0)


def _bridge(T, cap, match_iou, max_lost, first_id=0):
    m, p = mr.MotionTracker(T, cap, match_iou, max_lost, beta=0.5, v_max=0.0), track_ref.Tracker(T, cap, match_iou, max_lost)
    if first_id:
        m.reset(first_id)
        p.reset(first_id)
    return m, p


def _same_table(m, p):
    assert m.state() == p.state()
    live = [t for t in range(p.T) if p.live[t]]
    r = m.read()
    assert r["id"].tolist() == [p.id[t] for t in live] and r["last_seen"].tolist() == [p.last_seen[t] for t in live]
    assert r["class_id"].tolist() == [p.cls[t] for t in live]
    for k, name in enumerate("xywh"):
        assert _bits(r[name]) == _bits([p.box[t][k] for t in live])
    assert not np.abs(r["vx"]).any() and not np.abs(r["vy"]).any()                # +0 or -0: a velocity clamped to -v_max is -0.0


@pytest.mark.parametrize("case", tc.hand_cases(), ids=[c.name for c in tc.hand_cases()])
def test_v_max_0_is_the_plain_tracker_on_its_hand_cases(case):
    m, p = _bridge(case.T, case.cap, case.match_iou, case.max_lost, case.first_id)
    for k, f in enumerate(case.frames):
        nk = None if case.n_kept is None else case.n_kept[k]
        got = m.step(f, nk)
        assert got.tolist() == p.step(f, nk).tolist() == case.want[k], (case.name, k)
    _same_table(m, p)


@pytest.mark.parametrize("sc", tc.SCENES, ids=[s.name for s in tc.SCENES])
def test_v_max_0_is_the_plain_tracker_on_its_scenes(sc):
    frames, ids, trackers = tc.scene(sc)
    for s in range(sc.n_streams):
        m, _ = _bridge(sc.T, sc.cap, sc.match_iou, sc.max_lost)
        for k, f in enumerate(frames[s]):
            assert m.step(f).tolist() == ids[s][k].tolist(), (sc.name, s, k)
        _same_table(m, trackers[s])


@pytest.mark.parametrize("sc", mc.SCENES, ids=[s.name for s in mc.SCENES])
def test_a_streams_ids_do_not_depend_on_the_interleaving(sc):
    frames, _, ids, trackers, _ = mc.scene(sc)
    rng = np.random.default_rng(sc.seed)
    seq = [s for s in range(sc.n_streams) for _ in range(sc.n_frames)]
    rng.shuffle(seq)
    nxt, fl, streams, where = [0] * sc.n_streams, [], [], []
    for s in seq:
        if rng.random() < .2:
            fl.append(frames[0][0]); streams.append(-1); where.append(None)       # an untracked frame in between
        fl.append(frames[s][nxt[s]]); streams.append(s); where.append((s, nxt[s]))
        nxt[s] += 1
    trk = {s: mr.MotionTracker(sc.T, sc.cap, sc.match_iou, sc.max_lost, sc.beta, sc.v_max) for s in range(sc.n_streams)}
    got = mr.run_streams(trk, fl, streams)
    for g, w in zip(got, where):
        assert (g is None) == (w is None)
        if w is not None:
            assert g.tolist() == ids[w[0]][w[1]].tolist(), w
    for s in range(sc.n_streams):
        assert trk[s].state() == trackers[s].state() and np.array_equal(trk[s].read().view(np.uint8), trackers[s].read().view(np.uint8))


def test_fewer_id_switches_than_the_plain_tracker():
    motion = plain = 0
    for sc in mc.SCENES:
        _, gt, ids, _, plain_ids = mc.scene(sc)
        for s in range(sc.n_streams):
            motion += mc.switches(ids[s], gt[s])
            plain += mc.switches(plain_ids[s], gt[s])
    assert motion < plain, (motion, plain)


def test_the_scenes_cover_the_model():
    cov = mc.coverage()
    assert all(cov[k] >= v for k, v in mc.COVERAGE_FLOOR.items()), cov
