"""Crafted slabs for the tile merge (include/zly.h, "Tiles"), in the manner of tests/track_cases.py: hand cases whose expected survivors are
written out by hand as (slab, position) lists, seeded random scenes cut into zly_tile_grid tiles, and the builders that
tests/test_gpu_merge.py feeds to zly_merge_slabs.  Tiles are plain tuples (group, x0, y0, w, h, W, H) here.

The hand cases' numbers are dyadic, so that every mapped box and every measure is exact and the expectations can be checked on paper:
surface 256 x 256; tile A = columns 0..128, tile B = columns 64..192 (they overlap in 64..128), both full height.  A box of the surface at
centre X px, width BW px, lies in a tile at x = (X - x0) / 128, bw = BW / 128.

tests/test_merge_ref.py asserts ON THE ORACLE that the scenes hold the candidate counts they are meant to and that candidates are suppressed
and survive in them: a generator that stopped producing either would leave the GPU tests green and empty.
"""
from collections import namedtuple
from typing import Dict, List, Optional, Sequence

import numpy as np

import merge_ref
from merge_ref import IOS, IOU
from track_cases import FILL, build_slabs, dets, slab_bytes      # the slab layout and builders are the tracker cases'
from zly import DET_DTYPE, SLAB_HDR_DTYPE, SLAB_OVERFLOW

POISON = 0xC3                     # what the output buffer holds before a merge: records at or beyond the stored count must keep it
TAG0 = 0x7111E000

# frames: detection records per slab; n_kept: the headers' counts (None = len); want[g]: the survivors of group g in output order, as (slab, position)
Case = namedtuple("Case", "name cap metric thr tiles frames n_kept n_groups want")

A = (0, 0, 0, 128, 256, 256, 256)
B = (0, 64, 0, 128, 256, 256, 256)
QUARTERS = [(0, 0, 0, 128, 128, 256, 256), (0, 128, 0, 128, 128, 256, 256), (0, 0, 128, 128, 128, 256, 256), (0, 128, 128, 128, 128, 256, 256)]
WHOLE = (0, 0, 0, 256, 256, 256, 256)


def in_tile(t, X, Y, BW, BH):
    """the box (centre X, Y, size BW, BH, surface pixels) as fractions of tile t; exact for the dyadic numbers of the hand cases"""
    _, x0, y0, w, h, _, _ = t
    return ((X - x0) / w, (Y - y0) / h, BW / w, BH / h)


def grp(t, g):
    return (g,) + tuple(t[1:])


def one(box, conf, cls=0):
    return dets([box], [cls], conf)


def many(boxes, confs, classes=None):
    out = dets(boxes, classes)
    out["confidence"] = np.asarray(confs, dtype=np.float32)
    return out


def hand_cases() -> List[Case]:
    c: List[Case] = []
    add = lambda name, tiles, frames, want, metric=IOU, thr=0.5, cap=8, n_kept=None, n_groups=1: c.append(
        Case(name, cap, metric, np.float32(thr), tiles, frames, n_kept, n_groups, want))
    # an object wholly inside the overlap (columns 80..112): both tiles see it whole, the mapped boxes are identical, IoU = 1
    obj = (96, 128, 32, 64)
    add("seam_duplicate_removed_by_iou", [A, B], [one(in_tile(A, *obj), .8), one(in_tile(B, *obj), .9)], [[(1, 0)]])
    # an object at columns 120..152: B sees it whole, A sees the 8 columns 120..128.  IoU = 8/32 = .25, IoS = 8/8 = 1
    whole, cut = (136, 128, 32, 64), (124, 128, 8, 64)
    half = [one(in_tile(A, *cut), .6), one(in_tile(B, *whole), .9)]
    add("cut_box_kept_by_iou", [A, B], half, [[(1, 0), (0, 0)]], metric=IOU, thr=0.5)
    add("cut_box_removed_by_ios", [A, B], half, [[(1, 0)]], metric=IOS, thr=0.5)
    # columns 112..144 whole in B, its left half 112..128 in A: IoU = 16/32 = .5 exactly
    eq = [one(in_tile(A, 120, 128, 16, 64), .6), one(in_tile(B, 128, 128, 32, 64), .9)]
    add("iou_equal_to_threshold_kept", [A, B], eq, [[(1, 0), (0, 0)]], metric=IOU, thr=0.5)
    add("iou_one_ulp_above_threshold_removed", [A, B], eq, [[(1, 0)]], metric=IOU, thr=np.nextafter(np.float32(.5), np.float32(0)))
    # two boxes of 32 columns, 16 apart: IoS = 16/32 = .5 exactly (IoU = 1/3)
    eqs = [one(in_tile(A, 96, 128, 32, 64), .9), one(in_tile(B, 112, 128, 32, 64), .6)]
    add("ios_equal_to_threshold_kept", [A, B], eqs, [[(0, 0), (1, 0)]], metric=IOS, thr=0.5)
    add("ios_one_ulp_above_threshold_removed", [A, B], eqs, [[(0, 0)]], metric=IOS, thr=np.nextafter(np.float32(.5), np.float32(0)))
    # identical boxes of two classes: the order is class ascending, nothing is suppressed
    add("different_classes_never_suppress", [A, B], [one(in_tile(A, *obj), .8, cls=1), one(in_tile(B, *obj), .9, cls=0)], [[(1, 0), (0, 0)]], metric=IOS, thr=0.0)
    # exact confidence ties: the boxes differ (columns 80..112 and 84..116, IoU = 28/36), so who survives shows in the bytes
    o2 = (100, 128, 32, 64)
    add("tie_broken_by_slab_index", [A, B], [one(in_tile(A, *o2), .75), one(in_tile(B, *obj), .75)], [[(0, 0)]])
    add("tie_broken_by_slab_index_swapped", [A, B], [one(in_tile(A, *obj), .75), one(in_tile(B, *o2), .75)], [[(0, 0)]])
    add("tie_broken_by_position", [A, B], [many([in_tile(A, *o2), in_tile(A, *obj)], [.75, .75]), one(in_tile(B, 160, 128, 16, 16), .9)], [[(1, 0), (0, 0)]])
    add("tie_of_signed_zeros", [A, B], [one(in_tile(A, *o2), -0.0), one(in_tile(B, *obj), 0.0)], [[(0, 0)]])
    # a chain: boxes of 32 columns at 80.., 88.., 96..: IoU(a, b) = IoU(b, c) = 24/40 = .6, IoU(a, c) = 16/48 = 1/3.  a removes b; c lives because b is dead
    chain = [one(in_tile(A, 96, 128, 32, 64), .9), many([in_tile(B, 104, 128, 32, 64), in_tile(B, 112, 128, 32, 64)], [.8, .7])]
    add("chain_b_dies_c_lives", [A, B], chain, [[(0, 0), (1, 1)]])
    # eleven disjoint boxes in a source of capacity 8: only 8 enter; its overflow flag propagates though the merged count fits
    row11 = dets([in_tile(A, 6 + 11 * j, 128, 8, 64) for j in range(11)])
    row11["confidence"] = np.float32(.9) - np.arange(11, dtype=np.float32) / np.float32(64)
    add("source_n_kept_above_cap", [A, B], [row11, dets([])], [[(0, j) for j in range(8)]], n_kept=[11, None])
    add("source_n_kept_negative_is_empty", [A, B], [row11[:3], one(in_tile(B, 160, 128, 16, 16), .5)], [[(1, 0)]], n_kept=[-3, None])
    # six disjoint boxes in each of two tiles, A's at columns 0..60 and B's at 130..190: twelve survivors, eight stored, overflow
    six = lambda t, x: many([in_tile(t, x + 10 * j + 4, 128, 8, 64) for j in range(6)], [.9 - j / 64 for j in range(6)])
    add("merged_count_above_cap", [A, B], [six(A, 0), six(B, 130)], [[(0, 0), (1, 0), (0, 1), (1, 1), (0, 2), (1, 2), (0, 3), (1, 3), (0, 4), (1, 4), (0, 5), (1, 5)]])
    add("empty_group", [grp(A, 1), grp(B, 1)], [one(in_tile(A, *obj), .8), one(in_tile(B, *obj), .9)], [[], [(1, 0)]], n_groups=2)
    add("group_minus_1_left_out", [A, grp(B, -1), B], [one(in_tile(A, *o2), .6), one(in_tile(B, *obj), .9), one(in_tile(B, *obj), .7)], [[(2, 0)]])
    # three groups interleaved in one call; group 1's surface is another size
    S2 = (1, 0, 0, 64, 64, 64, 64)
    add("interleaved_groups", [A, S2, grp(A, 2), B, S2, grp(B, 2)],
        [one(in_tile(A, *obj), .8), one((.5, .5, .25, .25), .7), one(in_tile(A, *cut), .9), one(in_tile(B, *obj), .9), one((.5, .5, .25, .25), .7),
         one(in_tile(B, *whole), .6)], [[(3, 0)], [(1, 0)], [(2, 0), (5, 0)]], n_groups=3)
    # zero-area boxes overlap nothing, not even themselves: inter = 0, m = 0
    flat = (96, 128, 0, 64)
    add("zero_area_boxes_survive", [A, B], [one(in_tile(A, *flat), .8), many([in_tile(B, *flat), in_tile(B, *obj)], [.9, .5])], [[(1, 0), (0, 0), (1, 1)]], metric=IOS, thr=0.0)
    # a whole-surface pass beside four quarters: an object inside quarter 0 comes back twice; an object on the vertical seam of the upper quarters is cut in two
    # halves (columns 112..128 and 128..144), each with IoS = 1 against the whole pass's box
    inside, seam = (40, 40, 32, 32), (128, 64, 32, 32)
    add("whole_surface_beside_quarters", QUARTERS + [WHOLE],
        [many([in_tile(QUARTERS[0], *inside), in_tile(QUARTERS[0], 120, 64, 16, 32)], [.9, .6]), one(in_tile(QUARTERS[1], 136, 64, 16, 32), .65), dets([]), dets([]),
         many([in_tile(WHOLE, *inside), in_tile(WHOLE, *seam)], [.7, .8])], [[(0, 0), (4, 1)]], metric=IOS, thr=0.5)
    return c


def case_raw(case: Case) -> np.ndarray:
    return build_slabs(case.frames, case.cap, case.n_kept, tag0=TAG0)


def poison(n_slabs: int, cap: int, extra: int = 64) -> np.ndarray:
    """a flat output buffer of n_slabs slabs and `extra` bytes behind them, all POISON"""
    return np.full(n_slabs * slab_bytes(cap) + extra, POISON, dtype=np.uint8)


def hand_expected(case: Case, tag0: int = TAG0) -> np.ndarray:
    """u8 [n_groups][slab_bytes]: the output that case.want describes on a poisoned buffer -- built with the map alone, no order, no suppression"""
    sb = slab_bytes(case.cap)
    out = np.full((case.n_groups, sb), POISON, dtype=np.uint8)
    for g in range(case.n_groups):
        src = [i for i, t in enumerate(case.tiles) if t[0] == g]
        kept = lambda i: len(case.frames[i]) if case.n_kept is None or case.n_kept[i] is None else case.n_kept[i]
        n_cand = sum(max(0, min(kept(i), case.cap)) for i in src)
        over = any(kept(i) > case.cap for i in src) or len(case.want[g]) > case.cap
        hdr = out[g, :16].view(SLAB_HDR_DTYPE)
        hdr["n_kept"], hdr["n_candidates"], hdr["flags"], hdr["frame_tag"] = len(case.want[g]), n_cand, SLAB_OVERFLOW if over else 0, (tag0 + g) & 0xFFFFFFFF
        recs = np.zeros(min(len(case.want[g]), case.cap), dtype=DET_DTYPE)
        for k, (i, pos) in enumerate(case.want[g][:case.cap]):
            d = case.frames[i][pos]
            recs[k]["x"], recs[k]["y"], recs[k]["w"], recs[k]["h"] = merge_ref.map_box(d, case.tiles[i])
            recs[k]["confidence"], recs[k]["class_id"] = d["confidence"], d["class_id"]
        out[g, 16:16 + 40 * len(recs)] = recs.view(np.uint8)
    return out


# ---- seeded random scenes ----------------------------------------------------------------------------------------------------------
# Objects on a W x H surface, cut into tile_grid tiles: a tile reports the part of an object it sees (if that is at least `min_vis` of the object),
# in NMS's output order, at most cap per tile.  targets: the scene is also cut down to exactly these candidate counts M (the last sources lose
# records) -- 0, the sizes around every block of 64 sorted positions and every power of two the sort pads to, and the scene's own size (None).
Scene = namedtuple("Scene", "name W H tw th ov n_tiles cap objects classes seed metric thr targets")
SCENES = [
    Scene("cap8_8tiles", 128, 64, 40, 40, 8, 8, 8, 150, 2, 21, IOS, 0.5, (None, 0, 1, 2, 63, 64)),                       # 8 tiles x 8 = 64 slots: the one-wave launch
    Scene("cap8_9tiles", 128, 96, 48, 40, 8, 9, 8, 200, 2, 22, IOU, 0.45, (None, 64, 65)),                               # 72 slots
    Scene("dozens_cap64_8tiles", 224, 128, 80, 80, 24, 8, 64, 40, 3, 23, IOS, 0.5, (None,)),                             # the common case: a few dozen candidates
    Scene("crowd_cap64_8tiles", 224, 128, 80, 80, 24, 8, 64, 600, 3, 24, IOS, 0.5, (127, 128, 129, 255, 256, 257, 511, 512)),
    Scene("crowd_cap64_9tiles", 192, 192, 80, 80, 24, 9, 64, 800, 4, 25, IOU, 0.5, (513, 575, 576)),                     # 576 slots: the wide launch
    Scene("one_class_cap64_16tiles", 248, 248, 80, 80, 24, 16, 64, 1600, 1, 26, IOS, 0.6, (1023, 1024)),                 # every pair is a same-class pair
    Scene("deep_cap1024_4tiles", 136, 136, 80, 80, 24, 4, 1024, 6000, 4, 28, IOS, 0.5, (3000, 4096)),                   # the capacity holds every survivor: the whole order shows
    Scene("full_cap64_64tiles", 509, 509, 96, 96, 37, 64, 64, 5000, 5, 27, IOS, 0.5, (1025, 2047, 2048, 2049, 4095, 4096)),   # ZLY_MERGE_MAX_CANDIDATES
]


def scene_tiles(sc: Scene):
    tiles = merge_ref.tile_grid(sc.W, sc.H, sc.tw, sc.th, sc.ov, sc.ov)
    assert len(tiles) == sc.n_tiles, (sc.name, len(tiles))
    return tiles


def scene_frames(sc: Scene, min_vis: float = 0.2) -> List[np.ndarray]:
    rng = np.random.default_rng(sc.seed)
    tiles = scene_tiles(sc)
    cx, cy = rng.uniform(0, sc.W, sc.objects), rng.uniform(0, sc.H, sc.objects)
    bw, bh = rng.uniform(6, sc.tw * .6, sc.objects), rng.uniform(6, sc.th * .6, sc.objects)
    cls = rng.integers(0, sc.classes, sc.objects)
    x0, x1, y0, y1 = np.clip(cx - bw / 2, 0, sc.W), np.clip(cx + bw / 2, 0, sc.W), np.clip(cy - bh / 2, 0, sc.H), np.clip(cy + bh / 2, 0, sc.H)
    frames = []
    for (_, tx, ty, tw, th, _, _) in tiles:
        vx0, vx1, vy0, vy1 = np.maximum(x0, tx), np.minimum(x1, tx + tw), np.maximum(y0, ty), np.minimum(y1, ty + th)
        area = np.maximum(vx1 - vx0, 0) * np.maximum(vy1 - vy0, 0)
        vis = np.flatnonzero(area >= min_vis * (x1 - x0) * (y1 - y0) + 1e-9)
        # a tile sees an object a little differently every time; a quarter of the confidences are rounded to sixteenths, so that exact ties occur
        conf = rng.uniform(.3, .99, len(vis))
        conf = np.where(rng.random(len(vis)) < .25, np.round(conf * 16) / 16, conf)
        jit = rng.normal(0, .4, (len(vis), 4))
        order = sorted(range(len(vis)), key=lambda i: (cls[vis[i]], -conf[i]))[:sc.cap]
        f = np.zeros(len(order), dtype=DET_DTYPE)
        for k, i in enumerate(order):
            o = vis[i]
            f[k]["x"] = ((vx0[o] + vx1[o]) / 2 + jit[i, 0] - tx) / tw
            f[k]["y"] = ((vy0[o] + vy1[o]) / 2 + jit[i, 1] - ty) / th
            f[k]["w"] = max(vx1[o] - vx0[o] + jit[i, 2], 0) / tw
            f[k]["h"] = max(vy1[o] - vy0[o] + jit[i, 3], 0) / th
            f[k]["confidence"], f[k]["class_id"] = conf[i], cls[o]
        frames.append(f)
    return frames


def cut_to(frames: Sequence[np.ndarray], target: Optional[int]) -> List[np.ndarray]:
    """the same sources holding exactly `target` records in all (None: as they are): the last sources lose records"""
    if target is None:
        return list(frames)
    out, left = [], target
    for f in frames:
        out.append(f[:min(len(f), left)])
        left -= len(out[-1])
    assert left == 0, f"the scene holds {target - left} candidates, fewer than the {target} asked for"
    return out


_SCENE_CACHE: Dict[tuple, tuple] = {}
SCENE_PARAMS = [(sc, t) for sc in SCENES for t in sc.targets]
SCENE_IDS = [f"{sc.name}-M{'all' if t is None else t}" for sc, t in SCENE_PARAMS]


def scene(sc: Scene, target: Optional[int]):
    """(tiles, raw source slabs, the oracle's output on a poisoned buffer as u8 [1][slab_bytes]); computed once, never modified"""
    key = (sc.name, target)
    if key not in _SCENE_CACHE:
        tiles = scene_tiles(sc)
        frames = cut_to(scene_frames(sc), target)
        raw = build_slabs(frames, sc.cap, tag0=TAG0)
        raw.setflags(write=False)
        want = merge_ref.merge_slabs(raw, tiles, 1, sc.cap, sc.metric, sc.thr, TAG0, np.full((1, slab_bytes(sc.cap)), POISON, dtype=np.uint8))
        want.setflags(write=False)
        _SCENE_CACHE[key] = (tiles, raw, want)
    return _SCENE_CACHE[key]


def scene_stats(sc: Scene, target: Optional[int]) -> Dict[str, int]:
    tiles, raw, want = scene(sc, target)
    hdr = want[0, :16].view(SLAB_HDR_DTYPE)[0]
    kept = want[0, 16:].view(DET_DTYPE)[:min(int(hdr["n_kept"]), sc.cap)]
    return dict(M=int(hdr["n_candidates"]), kept=int(hdr["n_kept"]), classes=len(set(kept["class_id"].tolist())))
