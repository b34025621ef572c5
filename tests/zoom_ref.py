"""The exact numpy oracle of the zoom regions' plan (include/zly.h, "Zoom regions", steps 1-6): float32 scalars, one rounding per operation, the
sequential greedy choice.

A Table is a stream's track table as the plan reads it; table_of() takes it from a track_ref.Tracker or a track_motion_ref.MotionTracker (whose
vx, vy it carries; the plain tracker's are 0), so the oracle composes with the tracking oracles that produce the tables.  plan() returns the K
regions of one frame as REGION_DTYPE records (the layout of zly_zoom_region) and, for tests that want to know what happened, the slots it skipped
as covered.
"""
from dataclasses import dataclass, field
from typing import List, Tuple

import numpy as np

F = np.float32
U32 = 0xFFFFFFFF

REGION_DTYPE = np.dtype([("x0", "<i4"), ("y0", "<i4"), ("w", "<i4"), ("h", "<i4"), ("slot", "<i4"), ("track_id", "<u4")])


@dataclass
class Config:
    """zly_zoom_config"""
    regions: int = 3
    region_w: int = 416
    region_h: int = 416
    max_age: int = 2
    class_id: int = -1


@dataclass
class Table:
    frame_no: int = 0
    live: List[bool] = field(default_factory=list)
    box: List[Tuple[np.float32, np.float32, np.float32, np.float32]] = field(default_factory=list)      # x, y, w, h
    cls: List[int] = field(default_factory=list)
    id: List[int] = field(default_factory=list)
    last_seen: List[int] = field(default_factory=list)
    vx: List[np.float32] = field(default_factory=list)
    vy: List[np.float32] = field(default_factory=list)

    @property
    def T(self) -> int:
        return len(self.live)

    def add(self, x, y, w, h, cls=0, id=1, last_seen=0, vx=0.0, vy=0.0, live=True):
        """appends a slot (hand cases); returns its index"""
        self.live.append(bool(live)); self.box.append((F(x), F(y), F(w), F(h))); self.cls.append(int(cls)); self.id.append(int(id))
        self.last_seen.append(int(last_seen) & U32); self.vx.append(F(vx)); self.vy.append(F(vy))
        return len(self.live) - 1


def table_of(tracker) -> Table:
    """the table a Tracker / MotionTracker holds now"""
    T = tracker.T
    vx = list(getattr(tracker, "vx", [F(0)] * T))
    vy = list(getattr(tracker, "vy", [F(0)] * T))
    return Table(frame_no=tracker.frame_no, live=list(tracker.live), box=list(tracker.box), cls=list(tracker.cls), id=list(tracker.id),
                 last_seen=list(tracker.last_seen), vx=vx, vy=vy)


def size(cfg: Config, W: int, H: int) -> Tuple[int, int, int, int]:
    """step 1 -> rw, rh, xmax, ymax"""
    rw, rh = min(cfg.region_w, W & ~1), min(cfg.region_h, H & ~1)
    return rw, rh, (W - rw) & ~1, (H - rh) & ~1


def fallback(cfg: Config, W: int, H: int) -> Tuple[int, int]:
    """step 6: the centred window's origin"""
    rw, rh, _, _ = size(cfg, W, H)
    return ((W - rw) // 2) & ~1, ((H - rh) // 2) & ~1


def _area_key(w: np.float32, h: np.float32) -> int:
    """the fp32 area as an integer whose order is the values' (-0 and +0 tie)"""
    a = F(w * h)
    if a == 0:
        a = F(0)
    u = int(np.array(a, dtype=np.float32).view(np.uint32))
    return (~u) & U32 if u & 0x80000000 else u | 0x80000000


def _covered_axis(p: np.float32, s: np.float32, o: int, r: int, E: int) -> bool:
    half = F(s * F(0.5))
    lo, hi = F(p - half), F(p + half)
    a, b = F(F(o) / F(E)), F(F(o + r) / F(E))
    return bool(lo >= a) and bool(hi <= b)


def _origin(p: np.float32, E: int, r: int, omax: int) -> int:
    pc = (p if p < 1 else F(1)) if p > 0 else F(0)
    c = int(F(pc * F(E)))                      # truncation; pc is in [0, 1]
    return min(max(c - r // 2, 0), omax) & ~1


def plan(t: Table, cfg: Config, W: int, H: int, with_covered: bool = False):
    """-> REGION_DTYPE[K] (and, with_covered, the list of slots skipped as covered)"""
    assert 2 <= W < (1 << 24) and 2 <= H < (1 << 24)
    rw, rh, xmax, ymax = size(cfg, W, H)
    Fn = t.frame_no & U32
    elig = []
    with np.errstate(all="ignore"):
        for s in range(t.T):
            x, y, w, h = t.box[s]
            if not t.live[s]:
                continue
            if cfg.class_id != -1 and t.cls[s] != cfg.class_id:
                continue
            age = (Fn - t.last_seen[s]) & U32
            if age > cfg.max_age:
                continue
            if not (F(w * F(W)) <= F(rw) and F(h * F(H)) <= F(rh)):
                continue
            elig.append((age, _area_key(w, h), s))
        elig.sort()
        out = np.zeros(cfg.regions, dtype=REGION_DTYPE)
        chosen, covered = 0, []
        for _, _, s in elig:
            if chosen >= cfg.regions:
                break
            x, y, w, h = t.box[s]
            dtf = F((Fn + 1 - t.last_seen[s]) & U32)
            px, py = F(x + F(t.vx[s] * dtf)), F(y + F(t.vy[s] * dtf))
            if any(_covered_axis(px, w, int(out[j]["x0"]), rw, W) and _covered_axis(py, h, int(out[j]["y0"]), rh, H) for j in range(chosen)):
                covered.append(s)
                continue
            out[chosen] = (_origin(px, W, rw, xmax), _origin(py, H, rh, ymax), rw, rh, s, t.id[s])
            chosen += 1
        fx, fy = fallback(cfg, W, H)
        for j in range(chosen, cfg.regions):
            out[j] = (fx, fy, rw, rh, -1, 0)
    return (out, covered) if with_covered else out
