"""Crafted sequences for the tracker's motion model (include/zly.h, "tracking": steps P, 2', 4'), in the manner of tests/track_cases.py: hand cases
with hand-written ids -- and, where the point of a case is what the plain tracker does instead, the plain tracker's ids too -- and seeded scenes of
MOVING objects with their ground-truth object indices, so that id switches can be counted.  Slabs are built by track_cases.build_slabs.

The module asserts ON THE ORACLE (tests/track_motion_ref.py), when it is imported and before anything runs on a GPU, that the scenes together
contain at least 50 rescued matches (accepted pairs the plain tracker could not have made), 20 matches with dt > 1, 20 births, 10 expiries and 5
updates where the clamp changed a velocity.
"""
from collections import namedtuple
from typing import Dict, List

import numpy as np

import track_motion_ref
import track_ref
from track_cases import ROW8, dets
from zly import DET_DTYPE

# One stream's sequence.  want: the motion tracker's ids per frame, written by hand; plain: the plain tracker's (None = not the point of the case);
# reset_before: zly_track_reset(stream, 0) is called before the frames with these indices
MCase = namedtuple("MCase", "name T cap match_iou max_lost beta v_max frames want plain reset_before")


def _walk(x0, steps, w=.1, h=.1, y=.5):
    """a box that starts at x0 and moves by steps[k] before frame k + 1"""
    xs = [x0]
    for s in steps:
        xs.append(xs[-1] + s)
    return [(x, y, w, h) for x in xs]


ACCEL = _walk(.2, [.02, .04, .06, .08, .08, .08, .08])                 # width 0.1: the plain tracker loses it from the step of .06 on
STEADY = _walk(.2, [.04] * 8)                                          # 0.04 per frame
FAST_WIDE = _walk(.2, [.05] * 6, w=.2, h=.2)                           # 0.05 per frame, width 0.2
STEP_03 = _walk(.25, [.03] * 5)


def hand_cases() -> List[MCase]:
    c: List[MCase] = []
    add = lambda name, frames, want, plain=None, T=8, cap=8, match_iou=0.3, max_lost=2, beta=0.5, v_max=0.25, reset_before=(): c.append(
        MCase(name, T, cap, match_iou, max_lost, beta, v_max, frames, want, plain, tuple(reset_before)))
    none = dets([])
    add("accelerating_box_keeps_id", [dets([b]) for b in ACCEL], [[1]] * 8, plain=[[1], [1], [1], [2], [3], [4], [5], [6]])
    gap = [dets([b]) for b in STEADY]
    gap[4] = gap[5] = none
    add("gap_of_two_frames_reacquired", gap, [[1]] * 4 + [[], []] + [[1]] * 3, plain=[[1]] * 4 + [[], []] + [[2]] * 3)
    add("first_match_takes_the_full_displacement", [dets([b]) for b in STEP_03[:2]], [[1], [1]])
    # the velocity saturates at 0.03 while the box does 0.05 per frame: the prediction lags by 0.02 of a width of 0.2 and still matches
    add("clamped_velocity_still_matches", [dets([b]) for b in FAST_WIDE], [[1]] * 7, plain=[[1]] * 7, v_max=0.03)
    # the accelerating box again: with v_max = 0.02 the prediction falls behind until the step of .08 leaves IoU 0.25; each later box is born at rest
    add("clamped_velocity_loses_the_match", [dets([b]) for b in ACCEL], [[1], [1], [1], [1], [2], [3], [4], [5]], v_max=0.02)
    add("standing_box_keeps_zero_velocity", [dets([(.5, .5, .2, .2)])] * 4, [[1]] * 4, plain=[[1]] * 4)
    # the class is part of the match as before; the class-0 track coasts over the frame of class 1 and is found at its predicted place
    add("class_change_new_id", [dets([STEP_03[0]], [0]), dets([STEP_03[1]], [0]), dets([STEP_03[2]], [1]), dets([STEP_03[3]], [0])], [[1], [1], [2], [1]])
    # a full table: slot 0 moves once (so it has a velocity and two hits), then misses a frame in which a box of another class finds no free slot
    # and evicts it -- the only slot not matched in that frame.  The newcomer starts at rest with one hit
    moved = [(ROW8[0][0] + .01,) + ROW8[0][1:]] + ROW8[1:]
    add("eviction_replaces_a_moving_track", [dets(ROW8), dets(moved), dets(ROW8[1:] + [(.5, .2, .1, .1)], [0] * 7 + [1])],
        [list(range(1, 9)), list(range(1, 9)), list(range(2, 10))], max_lost=6)
    add("reset_mid_sequence", [dets([b]) for b in STEP_03], [[1]] * 3 + [[2]] * 3, reset_before=[3])
    return c


def run_case(case: MCase, tracker) -> List[np.ndarray]:
    """the case's frames through a tracker of either oracle, with the case's resets"""
    out = []
    for k, f in enumerate(case.frames):
        if k in case.reset_before:
            tracker.reset(0)
        out.append(tracker.step(f))
    return out


def case_trackers(case: MCase):
    """(a fresh motion oracle, a fresh plain oracle) with the case's configuration"""
    return (track_motion_ref.MotionTracker(case.T, case.cap, case.match_iou, case.max_lost, case.beta, case.v_max),
            track_ref.Tracker(case.T, case.cap, case.match_iou, case.max_lost))


# ---- seeded moving scenes ------------------------------------------------------------------------------------------------------------
MScene = namedtuple("MScene", "name T cap objects max_lost match_iou beta v_max sigma n_frames n_streams seed classes")
SCENES = [
    MScene("moving_T8_5", 8, 8, 5, 3, 0.3, 0.5, 0.25, 0.015, 24, 4, 21, 2),
    MScene("moving_T64_40", 64, 64, 40, 3, 0.3, 0.5, 0.25, 0.012, 16, 2, 22, 4),
    MScene("moving_T64_60", 64, 64, 60, 3, 0.3, 0.5, 0.25, 0.012, 16, 2, 23, 4),
    MScene("moving_T8_5_vmax_small", 8, 8, 5, 3, 0.3, 0.5, 0.01, 0.015, 24, 4, 24, 2),          # velocities beyond v_max: the clamp works
]


def scene_frames(sc: MScene):
    """(frames[stream][k], gt[stream][k]): objects with a velocity each (sigma per frame, perturbed by a random walk of a quarter of that), reflected
    at the borders, with dropouts of 1..3 frames; at most cap detections in NMS's output order; gt = the object index of every stored detection"""
    frames_out, gt_out = [], []
    for s in range(sc.n_streams):
        rng = np.random.default_rng(sc.seed * 1000 + s)
        pos = rng.uniform(.1, .9, (sc.objects, 2))
        vel = rng.normal(0, sc.sigma, (sc.objects, 2))
        size = rng.uniform(.06, .12, (sc.objects, 2))
        cls = rng.integers(0, sc.classes, sc.objects)
        hidden = np.zeros(sc.objects, dtype=int)
        frames, gts = [], []
        for _ in range(sc.n_frames):
            vel = vel + rng.normal(0, sc.sigma / 4, vel.shape)
            pos = pos + vel
            for edge, beyond in ((.05, pos < .05), (.95, pos > .95)):
                pos = np.where(beyond, 2 * edge - pos, pos)
                vel = np.where(beyond, -vel, vel)
            for o in range(sc.objects):
                if hidden[o] > 0:
                    hidden[o] -= 1
                elif rng.random() < .1:
                    hidden[o] = int(rng.integers(1, 4))
            vis = [o for o in range(sc.objects) if hidden[o] == 0]
            conf = rng.uniform(.5, .99, len(vis))
            order = sorted(range(len(vis)), key=lambda i: (cls[vis[i]], -conf[i]))[:sc.cap]
            f = np.zeros(len(order), dtype=DET_DTYPE)
            for k, i in enumerate(order):
                o = vis[i]
                f[k]["x"], f[k]["y"], f[k]["w"], f[k]["h"] = pos[o][0], pos[o][1], size[o][0], size[o][1]
                f[k]["confidence"], f[k]["class_id"] = conf[i], cls[o]
            frames.append(f)
            gts.append(np.array([vis[i] for i in order], dtype=int))
        frames_out.append(frames)
        gt_out.append(gts)
    return frames_out, gt_out


def switches(ids: List[np.ndarray], gt: List[np.ndarray]) -> int:
    """id switches of one stream against ground truth: how often an object is given another id than at its previous appearance"""
    last: Dict[int, int] = {}
    n = 0
    for f_ids, f_gt in zip(ids, gt):
        for i, o in zip(f_ids.tolist(), f_gt.tolist()):
            if o in last and last[o] != i:
                n += 1
            last[o] = i
    return n


_SCENE_CACHE: Dict[str, tuple] = {}


def scene(sc: MScene):
    """(frames[stream][k], gt[stream][k], ids[stream][k] by the motion oracle, the streams' final motion oracles, ids[stream][k] by the plain oracle);
    computed once, never modified"""
    if sc.name not in _SCENE_CACHE:
        frames, gt = scene_frames(sc)
        trk = [track_motion_ref.MotionTracker(sc.T, sc.cap, sc.match_iou, sc.max_lost, sc.beta, sc.v_max) for _ in range(sc.n_streams)]
        ids = [[trk[s].step(f) for f in frames[s]] for s in range(sc.n_streams)]
        plain = [track_ref.Tracker(sc.T, sc.cap, sc.match_iou, sc.max_lost) for _ in range(sc.n_streams)]
        plain_ids = [[plain[s].step(f) for f in frames[s]] for s in range(sc.n_streams)]
        _SCENE_CACHE[sc.name] = (frames, gt, ids, trk, plain_ids)
    return _SCENE_CACHE[sc.name]


def coverage() -> Dict[str, int]:
    """what the moving scenes contain, summed over scenes and streams"""
    tot = dict(rescued=0, coasted=0, births=0, expiries=0, clamped=0)
    for sc in SCENES:
        for t in scene(sc)[3]:
            for k in tot:
                tot[k] += t.counts[k]
    return tot


COVERAGE_FLOOR = dict(rescued=50, coasted=20, births=20, expiries=10, clamped=5)
_cov = coverage()
assert all(_cov[k] >= v for k, v in COVERAGE_FLOOR.items()), f"the moving scenes no longer cover the motion model: {_cov} against {COVERAGE_FLOOR}"
