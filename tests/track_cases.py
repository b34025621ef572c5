"""Crafted slab sequences for the tracker (include/zly.h, "tracking"), in the manner of tests/nms_cases.py: hand cases with hand-written
expected ids, seeded random scenes, and the slab builders that tests/test_gpu_track.py feeds to zly_track_slabs.

The module asserts ON THE ORACLE (tests/track_ref.py), when it is imported and before anything runs on a GPU, that the random scenes as a whole
contain at least 100 matches, 20 births, 10 expiries, 10 evictions and 10 re-acquisitions: a generator that stopped producing one of them
would leave the GPU tests green and empty.
"""
from collections import namedtuple
from typing import Dict, List, Optional, Sequence

import numpy as np

import track_ref
from zly import DET_DTYPE, SLAB_HDR_DTYPE, SLAB_OVERFLOW

FILL = 0xA5                       # bytes of a slab behind its stored detections: the tracker must leave them alone
TAG0 = 0x51AB0000

# One stream's sequence.  frames: detection records per frame; n_kept: the headers' counts (None = len(frame)); want: the expected ids per frame,
# written by hand (None for the random scenes: the oracle says); first_id: zly_track_reset's argument before the first frame (0 = keep)
Case = namedtuple("Case", "name T cap match_iou max_lost first_id frames n_kept want")


def dets(boxes: Sequence[Sequence[float]], classes: Optional[Sequence[int]] = None, conf: float = 0.75) -> np.ndarray:
    """detection records as NMS leaves them: track_id 0, timestamp 0"""
    out = np.zeros(len(boxes), dtype=DET_DTYPE)
    for i, b in enumerate(boxes):
        out[i]["x"], out[i]["y"], out[i]["w"], out[i]["h"] = b
        out[i]["confidence"] = conf
        out[i]["class_id"] = 0 if classes is None else classes[i]
    return out


def slab_bytes(cap: int) -> int:
    return SLAB_HDR_DTYPE.itemsize + cap * DET_DTYPE.itemsize


def build_slabs(frames: Sequence[np.ndarray], cap: int, n_kept: Optional[Sequence[Optional[int]]] = None, tag0: int = TAG0) -> np.ndarray:
    """u8 [len(frames)][slab_bytes]: header + the first min(len, cap) records, FILL behind them"""
    raw = np.full((len(frames), slab_bytes(cap)), FILL, dtype=np.uint8)
    for i, f in enumerate(frames):
        nk = len(f) if n_kept is None or n_kept[i] is None else n_kept[i]
        hdr = raw[i, :16].view(SLAB_HDR_DTYPE)
        hdr["n_kept"], hdr["n_candidates"], hdr["flags"], hdr["frame_tag"] = nk, max(nk, 0) + 3, SLAB_OVERFLOW if nk > cap else 0, (tag0 + i) & 0xFFFFFFFF
        k = min(len(f), cap)
        raw[i, 16:16 + 40 * k] = np.ascontiguousarray(f[:k]).view(np.uint8)
    return raw


def with_ids(raw: np.ndarray, ids: Sequence[Optional[np.ndarray]], cap: int) -> np.ndarray:
    """the slabs the tracker must leave: `raw` with ids[i] in the track_id fields of slab i (None: untouched)"""
    out = raw.copy()
    for i, v in enumerate(ids):
        if v is None:
            continue
        d = out[i, 16:].view(DET_DTYPE)
        assert len(v) <= cap
        d["track_id"][:len(v)] = v
    return out


def slab_ids(raw_row: np.ndarray, cap: int) -> np.ndarray:
    """track ids of the stored detections of one slab"""
    k = max(0, min(int(raw_row[:16].view(SLAB_HDR_DTYPE)["n_kept"][0]), cap))
    return raw_row[16:].view(DET_DTYPE)["track_id"][:k].copy()


# ---- hand cases --------------------------------------------------------------------------------------------------------------------
TIE_MID, TIE_LEFT, TIE_RIGHT = (.5, .5, .25, .25), (.4375, .5, .25, .25), (.5625, .5, .25, .25)      # dyadic: both neighbours have IoU 0.6 with the middle, identical bits
IOU_TIE = track_ref.iou(TIE_LEFT, TIE_MID)
ROW8 = [(0.0625 + 0.125 * j, .5, .0625, .25) for j in range(8)]                                      # eight disjoint boxes


def hand_cases() -> List[Case]:
    c: List[Case] = []
    add = lambda name, frames, want, T=8, cap=8, match_iou=0.3, max_lost=2, first_id=0, n_kept=None: c.append(
        Case(name, T, cap, match_iou, max_lost, first_id, frames, n_kept, want))
    add("drift_keeps_id", [dets([(.5 + .01 * k, .5, .2, .2)]) for k in range(5)], [[1]] * 5)
    box = [(.5, .5, .2, .2)]
    add("class_change_new_id", [dets(box, [0]), dets(box, [1]), dets(box, [0])], [[1], [2], [1]])
    none = dets([])
    add("gap_max_lost_reacquires", [dets(box), none, none, dets(box)], [[1], [], [], [1]], max_lost=2)
    add("gap_max_lost_plus_1_expires", [dets(box), none, none, none, dets(box)], [[1], [], [], [], [2]], max_lost=2)
    add("max_lost_0_expires_at_once", [dets(box), none, dets(box)], [[1], [], [2]], max_lost=0)
    add("iou_equal_to_threshold_no_match", [dets([TIE_MID]), dets([TIE_RIGHT])], [[1], [2]], match_iou=float(IOU_TIE))
    add("iou_just_above_threshold_matches", [dets([TIE_MID]), dets([TIE_RIGHT])], [[1], [1]], match_iou=float(np.nextafter(IOU_TIE, np.float32(0))))
    add("tie_two_dets_one_track", [dets([TIE_MID]), dets([TIE_LEFT, TIE_RIGHT])], [[1], [1, 2]])
    add("tie_two_dets_one_track_swapped", [dets([TIE_MID]), dets([TIE_RIGHT, TIE_LEFT])], [[1], [1, 2]])
    add("tie_one_det_two_tracks", [dets([TIE_LEFT, TIE_RIGHT]), dets([TIE_MID])], [[1, 2], [1]])
    add("tie_one_det_two_tracks_swapped", [dets([TIE_RIGHT, TIE_LEFT]), dets([TIE_MID])], [[1, 2], [1]])
    # greedy is not the optimal assignment: detection 0 overlaps track 2 more than track 1 and takes it; detection 1 only overlaps track 2 and is born
    add("greedy_not_optimal", [dets([(.30, .5, .2, .2), (.42, .5, .2, .2)]), dets([(.37, .5, .2, .2), (.50, .5, .2, .2)])], [[1, 2], [2, 3]])
    # a full table, slot j holding box j: last_seen becomes 1 2 1 3 1 2 3 2, then boxes of another class evict by (last_seen, slot) = slots 0 2 4 1 5 7 3 6
    pick = lambda js, cls=0: dets([ROW8[j] for j in js], [cls] * len(js))
    warm = [pick(range(8)), pick([1, 3, 5, 7]), pick([3, 6])]
    add("full_table_evicts_all", warm + [pick(range(8), 1), pick(range(8), 1)],
        [list(range(1, 9)), [2, 4, 6, 8], [4, 7], list(range(9, 17)), list(range(9, 17))], max_lost=6)
    add("full_table_eviction_order_3", warm + [pick([0, 1, 2], 1), pick(range(8))],
        [list(range(1, 9)), [2, 4, 6, 8], [4, 7], [9, 10, 11], [12, 2, 13, 4, 14, 6, 7, 8]], max_lost=6)
    add("full_table_eviction_order_5", warm + [pick([0, 1, 2, 3, 4], 1), pick(range(8))],
        [list(range(1, 9)), [2, 4, 6, 8], [4, 7], [9, 10, 11, 12, 13], [14, 15, 16, 4, 17, 18, 7, 8]], max_lost=6)
    more = dets([(0.04 + 0.08 * j, .5, .04, .25) for j in range(11)])
    add("n_kept_above_cap", [more, more], [list(range(1, 9))] * 2, n_kept=[11, 11])
    add("n_kept_zero", [none, dets(box), none], [[], [1], []])
    add("n_kept_negative_is_zero", [dets(box), dets(box)], [[], [1]], n_kept=[-3, None])
    add("id_wrap", [dets([ROW8[0], ROW8[1], ROW8[2]])], [[0xFFFFFFFF, 1, 2]], first_id=0xFFFFFFFF)
    return c


# ---- seeded random scenes ----------------------------------------------------------------------------------------------------------
Scene = namedtuple("Scene", "name T cap objects max_lost match_iou n_frames n_streams seed classes")
SCENES = [
    Scene("walks_T8_lost2", 8, 8, 6, 2, 0.3, 24, 4, 11, 3),
    Scene("crowd_T8_lost6", 8, 8, 8, 6, 0.3, 24, 4, 12, 3),
    Scene("wide_T64_cap64", 64, 64, 40, 3, 0.3, 12, 2, 13, 6),
    Scene("wide_T64_cap8", 64, 8, 8, 6, 0.3, 24, 2, 14, 2),
    Scene("full_T64_cap64", 64, 64, 60, 12, 0.3, 14, 1, 15, 4),          # the 64-slot table fills up: evictions ranked over the whole wave
]


def scene_frames(sc: Scene) -> List[List[np.ndarray]]:
    """frames[stream][k]: objects on random walks, with dropouts (1..4 frames) and teleports; at most cap detections, in NMS's output order"""
    out = []
    for s in range(sc.n_streams):
        rng = np.random.default_rng(sc.seed * 1000 + s)
        pos = rng.uniform(.15, .85, (sc.objects, 2))
        size = rng.uniform(.08, .2, (sc.objects, 2))
        cls = rng.integers(0, sc.classes, sc.objects)
        hidden = np.zeros(sc.objects, dtype=int)
        frames = []
        for _ in range(sc.n_frames):
            pos = np.clip(pos + rng.normal(0, .012, pos.shape), .05, .95)
            for o in range(sc.objects):
                if hidden[o] > 0:
                    hidden[o] -= 1
                elif rng.random() < .12:
                    hidden[o] = int(rng.integers(1, 5))
                if rng.random() < .06:
                    pos[o] = rng.uniform(.15, .85, 2)
            vis = [o for o in range(sc.objects) if hidden[o] == 0]
            conf = rng.uniform(.5, .99, len(vis))
            order = sorted(range(len(vis)), key=lambda i: (cls[vis[i]], -conf[i]))[:sc.cap]
            f = np.zeros(len(order), dtype=DET_DTYPE)
            for k, i in enumerate(order):
                o = vis[i]
                f[k]["x"], f[k]["y"], f[k]["w"], f[k]["h"] = pos[o][0], pos[o][1], size[o][0], size[o][1]
                f[k]["confidence"], f[k]["class_id"] = conf[i], cls[o]
            frames.append(f)
        out.append(frames)
    return out


_SCENE_CACHE: Dict[str, tuple] = {}


def scene(sc: Scene):
    """(frames[stream][k], ids[stream][k] by the oracle, the streams' final oracle trackers); computed once, never modified"""
    if sc.name not in _SCENE_CACHE:
        frames = scene_frames(sc)
        trk = [track_ref.Tracker(sc.T, sc.cap, sc.match_iou, sc.max_lost) for _ in range(sc.n_streams)]
        ids = [[trk[s].step(f) for f in frames[s]] for s in range(sc.n_streams)]
        _SCENE_CACHE[sc.name] = (frames, ids, trk)
    return _SCENE_CACHE[sc.name]


def coverage() -> Dict[str, int]:
    """what the random scenes contain, summed over scenes and streams"""
    tot = dict(matches=0, births=0, expiries=0, evictions=0, reacquisitions=0)
    for sc in SCENES:
        for t in scene(sc)[2]:
            for k in tot:
                tot[k] += t.counts[k]
    return tot


COVERAGE_FLOOR = dict(matches=100, births=20, expiries=10, evictions=10, reacquisitions=10)
_cov = coverage()
assert all(_cov[k] >= v for k, v in COVERAGE_FLOOR.items()), f"the random scenes no longer cover the tracker: {_cov} against {COVERAGE_FLOOR}"
