"""The exact numpy oracle of the tracking step WITH the constant-velocity motion model (include/zly.h, "tracking": steps P, 2', 4'): float32
scalars, one rounding per operation, the sequential greedy match.  It has the shape of track_ref.Tracker -- step(), reset(), state() -- plus read(),
which returns what zly_track_read returns, and it reuses track_ref.iou.

Beside track_ref's counts it counts, per stream: `rescued` matches (accepted pairs whose IoU against the slot's STORED box is not above match_iou:
the plain tracker could not have made them), matches with dt > 1 (`coasted`) and updates where the clamp changed a velocity (`clamped`).
"""
from typing import Optional

import numpy as np

from track_ref import F, U32, iou, run_streams        # noqa: F401  (run_streams: the same harness drives either oracle)
from zly import TRACK_DTYPE


def clamp(v: np.float32, v_max: np.float32) -> np.float32:
    """v < -v_max ? -v_max : (v > v_max ? v_max : v)"""
    lo = F(-v_max)
    return lo if v < lo else (v_max if v > v_max else v)


class MotionTracker:
    def __init__(self, max_tracks: int, cap: int, match_iou: float = 0.3, max_lost: int = 6, beta: float = 0.5, v_max: float = 0.25, first_id: int = 1):
        assert cap <= max_tracks <= 64
        self.T, self.cap = max_tracks, cap
        self.match_iou, self.max_lost = F(match_iou), int(max_lost)
        self.beta, self.v_max = F(beta), F(v_max)
        self.next_id = first_id
        self.reset(0)
        self.counts = dict(matches=0, births=0, expiries=0, evictions=0, reacquisitions=0, rescued=0, coasted=0, clamped=0)

    def reset(self, first_id: int = 0):
        """zly_track_reset on a motion engine: every slot free, velocities and hits 0, frame_no = 0, evictions = 0; first_id = 0 keeps next_id"""
        self.frame_no = 0
        self.evictions = 0
        self.live = [False] * self.T
        self.box = [(F(0), F(0), F(0), F(0))] * self.T
        self.cls = [0] * self.T
        self.id = [0] * self.T
        self.last_seen = [0] * self.T
        self.vx = [F(0)] * self.T
        self.vy = [F(0)] * self.T
        self.hits = [0] * self.T
        if first_id:
            self.next_id = first_id

    def state(self) -> dict:
        """what zly_track_state_at reports"""
        return dict(frame_no=self.frame_no, next_id=self.next_id, n_live=sum(self.live), evictions=self.evictions)

    def read(self) -> np.ndarray:
        """what zly_track_read reports: the live slots in ascending slot order; x, y, w, h = the last matched box, not the prediction"""
        out = np.zeros(sum(self.live), dtype=TRACK_DTYPE)
        for i, t in enumerate(t for t in range(self.T) if self.live[t]):
            out[i]["x"], out[i]["y"], out[i]["w"], out[i]["h"] = self.box[t]
            out[i]["vx"], out[i]["vy"] = self.vx[t], self.vy[t]
            out[i]["class_id"], out[i]["id"], out[i]["hits"], out[i]["last_seen"] = self.cls[t], self.id[t], self.hits[t], self.last_seen[t]
        return out

    def step(self, dets: np.ndarray, n_kept: Optional[int] = None) -> np.ndarray:
        """dets: the slab's detection records; n_kept: the header's count (default len(dets)) -> uint32 ids of the first K = clamp(n_kept, 0, cap)"""
        n_kept = len(dets) if n_kept is None else n_kept
        K = max(0, min(n_kept, self.cap))
        D = [(F(d["x"]), F(d["y"]), F(d["w"]), F(d["h"])) for d in dets[:K]]
        C = [int(d["class_id"]) for d in dets[:K]]
        self.frame_no = (self.frame_no + 1) & U32
        # P. predict every live slot to this frame
        dtf = [F(0)] * self.T
        pred = [None] * self.T
        for t in range(self.T):
            if self.live[t]:
                dtf[t] = F((self.frame_no - self.last_seen[t]) & U32)                     # u32 -> fp32, round to nearest even
                x, y, w, h = self.box[t]
                pred[t] = (F(x + F(self.vx[t] * dtf[t])), F(y + F(self.vy[t] * dtf[t])), w, h)
        # 2'. candidates against the predicted box; 3. greedy, unchanged
        pairs = []
        for d in range(K):
            for t in range(self.T):
                if self.live[t] and C[d] == self.cls[t]:
                    v = iou(D[d], pred[t])
                    if v > self.match_iou:
                        pairs.append((-float(v), d, t))
        pairs.sort()
        ids = np.zeros(K, dtype=np.uint32)
        det_done, slot_done = [False] * K, [False] * self.T
        for _, d, t in pairs:
            if det_done[d] or slot_done[t]:
                continue
            det_done[d] = slot_done[t] = True
            dt = (self.frame_no - self.last_seen[t]) & U32
            if dt > 1:
                self.counts["reacquisitions"] += 1
                self.counts["coasted"] += 1
            if not iou(D[d], self.box[t]) > self.match_iou:
                self.counts["rescued"] += 1
            self.counts["matches"] += 1
            # 4'. the velocity takes the residual against the prediction
            rx, ry = F(D[d][0] - pred[t][0]), F(D[d][1] - pred[t][1])
            g = F(1) if self.hits[t] == 1 else self.beta
            ux, uy = F(self.vx[t] + F(g * F(rx / dtf[t]))), F(self.vy[t] + F(g * F(ry / dtf[t])))
            self.vx[t], self.vy[t] = clamp(ux, self.v_max), clamp(uy, self.v_max)
            if self.vx[t].view(np.uint32) != ux.view(np.uint32) or self.vy[t].view(np.uint32) != uy.view(np.uint32):
                self.counts["clamped"] += 1
            self.hits[t] = min(self.hits[t] + 1, U32)
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
            self.vx[t], self.vy[t], self.hits[t] = F(0), F(0), 1
            born[t] = True
            ids[d] = self.next_id
            self.next_id = (self.next_id + 1) & U32 or 1
            self.counts["births"] += 1
        return ids
