"""The numpy oracle of the zoom regions' plan (tests/zoom_ref.py) against regions written by hand (tests/zoom_cases.py): the cases cover every branch
of steps 1-6 of include/zly.h, "Zoom regions".  No GPU, no library."""
import numpy as np
import pytest

import zoom_ref
from track_ref import Tracker
from track_motion_ref import MotionTracker
from zly import DET_DTYPE
from zoom_cases import hand_cases, random_case

CASES = hand_cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_hand_case(case):
    _, t, cfg, W, H, expected = case
    rw, rh, _, _ = zoom_ref.size(cfg, W, H)
    got = zoom_ref.plan(t, cfg, W, H)
    want = [(x0, y0, rw, rh, slot, t.id[slot] if slot >= 0 else 0) for x0, y0, slot in expected]
    assert [tuple(int(v) for v in r) for r in got] == want


def test_covered_slots_are_reported():
    by_name = {c[0]: c for c in CASES}
    for name, covered in (("covered", [1]), ("covered-hi-at", [1]), ("covered-lo-at", [1]), ("covered-hi-miss", []), ("covered-lo-miss", []), ("full-table", [1, 2, 4]),
                          ("small-surface", [1])):
        _, t, cfg, W, H, _ = by_name[name]
        assert zoom_ref.plan(t, cfg, W, H, with_covered=True)[1] == covered, name


def test_invariants_on_random_tables():
    """even origins inside the surface, one region per slot at most, fallbacks last and centred"""
    rng = np.random.default_rng(11)
    for _ in range(300):
        t, cfg, W, H = random_case(rng)
        rw, rh, xmax, ymax = zoom_ref.size(cfg, W, H)
        out = zoom_ref.plan(t, cfg, W, H)
        slots = [int(r["slot"]) for r in out]
        live = [s for s in slots if s >= 0]
        assert len(set(live)) == len(live) and slots == live + [-1] * (len(slots) - len(live))
        for r in out:
            assert r["x0"] % 2 == 0 and r["y0"] % 2 == 0 and 0 <= r["x0"] <= xmax and 0 <= r["y0"] <= ymax and (r["w"], r["h"]) == (rw, rh)
            if r["slot"] < 0:
                assert (int(r["x0"]), int(r["y0"])) == zoom_ref.fallback(cfg, W, H) and r["track_id"] == 0
            else:
                assert t.live[r["slot"]] and r["track_id"] == t.id[r["slot"]]


def test_the_fused_case_can_tell_an_fma():
    """the hand case 'product-rounded-first' is worth its name: one rounding of x + vx * dtf (float64 holds it exactly) gives another float and another
    origin, and the motion tracker's oracle produces exactly that velocity from the two boxes the GPU test feeds"""
    import zoom_cases as zc
    x, vx = zc.FUSED_X2, zc.FUSED_VX
    unfused = zoom_ref.F(x + zoom_ref.F(vx * zoom_ref.F(3)))
    fused = zoom_ref.F(float(x) + float(vx) * 3.0)
    assert unfused != fused
    origin = lambda p: min(max(int(zoom_ref.F(p * zoom_ref.F(zc.FUSED_W))) - 104, 0), 994) & ~1
    assert (origin(unfused), origin(fused)) == (zc.FUSED_X0, zc.FUSED_X0_IF_FUSED)
    trk = MotionTracker(64, 64)
    for boxes in ([(zc.FUSED_X1, 0.5, zc.FUSED_SIZE, zc.FUSED_SIZE)], [], [], [(zc.FUSED_X2, 0.5, zc.FUSED_SIZE, zc.FUSED_SIZE)], [], []):
        trk.step(_dets(boxes))
    t = zoom_ref.table_of(trk)
    assert t.live[0] and t.vx[0] == vx and t.box[0][0] == x and (t.frame_no, t.last_seen[0]) == (6, 4)
    assert int(zoom_ref.plan(t, zoom_ref.Config(regions=3, region_w=208, region_h=208), zc.FUSED_W, 480)[0]["x0"]) == zc.FUSED_X0


def _dets(boxes, cls=0):
    d = np.zeros(len(boxes), dtype=DET_DTYPE)
    for i, (x, y, w, h) in enumerate(boxes):
        d[i]["x"], d[i]["y"], d[i]["w"], d[i]["h"], d[i]["class_id"], d[i]["confidence"] = x, y, w, h, cls, 0.9
    return d


def test_composes_with_the_tracking_oracles():
    """a target 1/16 wide that moves right by 1/32 per frame (IoU 1/3 with its last box: both trackers keep it): the motion tracker's table puts the
    region one step ahead of the plain tracker's"""
    cfg = zoom_ref.Config(regions=1, region_w=208, region_h=208)
    plain, motion = Tracker(64, 64), MotionTracker(64, 64, v_max=0.25)
    for k in range(3):
        d = _dets([(0.25 + k / 32, 0.5, 0.0625, 0.0625)])
        plain.step(d)
        motion.step(d)
    assert plain.state()["n_live"] == 1 and motion.state()["n_live"] == 1
    # the last box is at 0.3125: cx = 200 -> 96; with vx = 1/32 the prediction is 0.34375: cx = 220 -> 116
    assert tuple(zoom_ref.plan(zoom_ref.table_of(plain), cfg, 640, 480)[0])[:2] == (96, 136)
    assert tuple(zoom_ref.plan(zoom_ref.table_of(motion), cfg, 640, 480)[0])[:2] == (116, 136)
