"""The exact numpy oracle of the tracking step (include/zly.h, "tracking"): float32 scalars, one rounding per operation, the sequential
greedy match.  One Tracker is one stream's state; step() takes a frame's stored detections (zly.DET_DTYPE records, slab order) and returns
their track ids.  It also counts, per stream, matches, births, expiries, evictions and re-acquisitions (a match with frame_no - last_seen > 1).

run_streams() drives a dict of trackers over frames tagged with stream indices (-1 = untracked) in the given order: the harness the tests use
for the oracle side of every batch composition.
"""
from typing import Dict, List, Optional, Sequence

import numpy as np

F = np.float32
U32 = 0xFFFFFFFF


def iou(a, b) -> np.float32:
    """calculateIoU as iou_cxcywh (csrc/kernels_post.hip) computes it: a, b = (x, y, w, h) float32 quadruples"""
    ax, ay, aw, ah = (F(v) for v in a)
    bx, by, bw, bh = (F(v) for v in b)
    two = F(2)
    ax0, ay0, ax1, ay1 = F(ax - F(aw / two)), F(ay - F(ah / two)), F(ax + F(aw / two)), F(ay + F(ah / two))
    bx0, by0, bx1, by1 = F(bx - F(bw / two)), F(by - F(bh / two)), F(bx + F(bw / two)), F(by + F(bh / two))
    lo_x = bx0 if ax0 < bx0 else ax0
    hi_x = bx1 if bx1 < ax1 else ax1
    lo_y = by0 if ay0 < by0 else ay0
    hi_y = by1 if by1 < ay1 else ay1
    dx, dy = F(hi_x - lo_x), F(hi_y - lo_y)
    ox = dx if F(0) < dx else F(0)
    oy = dy if F(0) < dy else F(0)
    inter = F(ox * oy)
    uni = F(F(F(aw * ah) + F(bw * bh)) - inter)
    return F(inter / uni) if uni > 0 else F(0)


class Tracker:
    def __init__(self, max_tracks: int, cap: int, match_iou: float = 0.3, max_lost: int = 6, first_id: int = 1):
        assert cap <= max_tracks <= 64
        self.T, self.cap = max_tracks, cap
        self.match_iou, self.max_lost = F(match_iou), int(max_lost)
        self.next_id = first_id
        self.reset(0)
        self.counts = dict(matches=0, births=0, expiries=0, evictions=0, reacquisitions=0)

    def reset(self, first_id: int = 0):
        """zly_track_reset: every slot free, frame_no = 0, evictions = 0; first_id = 0 keeps next_id"""
        self.frame_no = 0
        self.evictions = 0
        self.live = [False] * self.T
        self.box = [(F(0), F(0), F(0), F(0))] * self.T
        self.cls = [0] * self.T
        self.id = [0] * self.T
        self.last_seen = [0] * self.T
        if first_id:
            self.next_id = first_id

    def state(self) -> dict:
        """what zly_track_state_at reports"""
        return dict(frame_no=self.frame_no, next_id=self.next_id, n_live=sum(self.live), evictions=self.evictions)

    def step(self, dets: np.ndarray, n_kept: Optional[int] = None) -> np.ndarray:
        """dets: the slab's detection records; n_kept: the header's count (default len(dets)) -> uint32 ids of the first K = clamp(n_kept, 0, cap)"""
        n_kept = len(dets) if n_kept is None else n_kept
        K = max(0, min(n_kept, self.cap))
        D = [(F(d["x"]), F(d["y"]), F(d["w"]), F(d["h"])) for d in dets[:K]]
        C = [int(d["class_id"]) for d in dets[:K]]
        self.frame_no = (self.frame_no + 1) & U32
        pairs = []
        for d in range(K):
            for t in range(self.T):
                if self.live[t] and C[d] == self.cls[t]:
                    v = iou(D[d], self.box[t])
                    if v > self.match_iou:
                        pairs.append((-float(v), d, t))          # float32 -> float64 is exact: the order is the fp32 values'
        pairs.sort()
        ids = np.zeros(K, dtype=np.uint32)
        det_done, slot_done = [False] * K, [False] * self.T
        for _, d, t in pairs:
            if det_done[d] or slot_done[t]:
                continue
            det_done[d] = slot_done[t] = True
            if (self.frame_no - self.last_seen[t]) & U32 > 1:
                self.counts["reacquisitions"] += 1
            self.counts["matches"] += 1
            self.box[t] = D[d]
            self.last_seen[t] = self.frame_no
            ids[d] = self.id[t]
        for t in range(self.T):
            if self.live[t] and not slot_done[t] and ((self.frame_no - self.last_seen[t]) & U32) > self.max_lost:
                self.live[t] = False
                self.counts["expiries"] += 1
        born = [False] * self.T
        for d in range(K):
            if det_done[d]:
                continue
            free = [t for t in range(self.T) if not self.live[t]]
            if free:
                t = free[0]
            else:
                t = min((t for t in range(self.T) if not slot_done[t] and not born[t]), key=lambda t: (self.last_seen[t], t))
                self.evictions += 1
                self.counts["evictions"] += 1
            self.live[t], self.box[t], self.cls[t], self.id[t], self.last_seen[t] = True, D[d], C[d], self.next_id, self.frame_no
            born[t] = True
            ids[d] = self.next_id
            self.next_id = (self.next_id + 1) & U32 or 1
            self.counts["births"] += 1
        return ids


def run_streams(trackers: Dict[int, Tracker], frames: Sequence[np.ndarray], streams: Sequence[int],
                n_kept: Optional[Sequence[int]] = None) -> List[Optional[np.ndarray]]:
    """frames[i] (detection records) belongs to stream streams[i] (-1: untracked -> None); taken in the given order"""
    out: List[Optional[np.ndarray]] = []
    for i, (f, s) in enumerate(zip(frames, streams)):
        out.append(None if s < 0 else trackers[s].step(f, None if n_kept is None else n_kept[i]))
    return out
