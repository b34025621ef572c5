"""The exact numpy oracle of the camera motion estimate (include/zly.h, "Camera motion"), written from the header alone: the grid (the change map's
luma and cell sums, reused from tests/change_ref.py), FIRST, the SAD table over the window, the ordered best candidate, the sub-cell fit, the shift,
LOST, the pending shift, the record -- including what it must NOT write -- the reset, and step A on a track table.

Stream.frame() is steps 1-9 for one frame of one stream on a record buffer of the caller's; Stream.apply() is step A on arrays of x, y and live flags.
All of it is Python integers and numpy u64 except the two fp32 operations of step A."""
from dataclasses import dataclass

import numpy as np

import change_ref

FIRST, LOST, CLIPPED = 1, 2, 4
MAX_RADIUS, SIDE_MAX, SAD_ROOM = 8, 17, 289
MAX_CELLS, MAX_DIM, CELLS = change_ref.MAX_CELLS, change_ref.MAX_DIM, change_ref.CELLS
F = np.float32

HDR_DTYPE = np.dtype([("flags", "<u4"), ("step", "<u4"), ("gw", "<i4"), ("gh", "<i4"), ("dx", "<i4"), ("dy", "<i4"), ("fx", "<i4"), ("fy", "<i4"),
                      ("sx_q4", "<i4"), ("sy_q4", "<i4"), ("n_lost", "<u4"), ("n_applied", "<u4"), ("sad_min", "<u8"), ("sad_zero", "<u8"),
                      ("pend_x_q4", "<i8"), ("pend_y_q4", "<i8"), ("pad", "<u4", (4,))])
assert HDR_DTYPE.itemsize == 96
HDR_BYTES, REC_BYTES = 96, 96 + 8 * SAD_ROOM


@dataclass
class Config:
    """zly_camera_config"""
    cell: int = 16
    radius: int = 4
    max_residual_q4: int = 64


def layout():
    """step 9 -> (rec_bytes, sad_off, sad_room)"""
    return REC_BYTES, HDR_BYTES, SAD_ROOM


def grid_ok(W, H, cfg):
    """step 1: what a call accepts"""
    gw, gh = change_ref.grid(W, H, cfg.cell)
    return 1 <= W <= MAX_DIM and 1 <= H <= MAX_DIM and gw * gh <= MAX_CELLS and gw >= 2 * cfg.radius + 1 and gh >= 2 * cfg.radius + 1


def sad_table(S, P, R):
    """step 3: u64 [2R+1][2R+1], rows dy = -R..R, columns dx = -R..R, of the grids S (this frame) and P (the previous one), both [gh][gw]"""
    gh, gw = S.shape
    win = S[R:gh - R, R:gw - R].astype(np.int64)
    tab = np.zeros((2 * R + 1, 2 * R + 1), dtype=np.uint64)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            prev = P[R - dy:gh - R - dy, R - dx:gw - R - dx].astype(np.int64)
            tab[dy + R, dx + R] = int(np.abs(win - prev).sum(dtype=np.int64))
    return tab


def best(tab, R):
    """step 4 -> (dx, dy): least in (SAD, |dx| + |dy|, dy, dx)"""
    _, _, dy, dx = min((int(tab[dy + R, dx + R]), abs(dx) + abs(dy), dy, dx) for dy in range(-R, R + 1) for dx in range(-R, R + 1))
    return dx, dy


def fit(d, R, s0, sm, sp):
    """step 5 for one axis -> f; sm, sp are callables so that they are only asked for inside the table"""
    if abs(d) == R:
        return 0
    sm, sp = sm(), sp()
    hi = max(sm, sp)
    if s0 == 0 or hi == s0:
        return 0
    num, den = 16 * (sm - sp), 2 * (hi - s0)
    q = min(abs(num) // den, 8)
    return q if num >= 0 else -q


def estimate(S, P, cfg):
    """steps 3-7 -> dict(tab, dx, dy, fx, fy, sx_q4, sy_q4, sad_min, sad_zero, lost, clipped)"""
    R, C = cfg.radius, cfg.cell
    gh, gw = S.shape
    tab = sad_table(S, P, R)
    dx, dy = best(tab, R)
    at = lambda x, y: int(tab[y + R, x + R])           # noqa: E731
    s0 = at(dx, dy)
    fx = fit(dx, R, s0, lambda: at(dx - 1, dy), lambda: at(dx + 1, dy))
    fy = fit(dy, R, s0, lambda: at(dx, dy - 1), lambda: at(dx, dy + 1))
    npix = (gw - 2 * R) * (gh - 2 * R) * C * C
    return dict(tab=tab, dx=dx, dy=dy, fx=fx, fy=fy, sx_q4=(16 * dx + fx) * C, sy_q4=(16 * dy + fy) * C, sad_min=s0, sad_zero=at(0, 0),
                lost=16 * s0 > cfg.max_residual_q4 * npix, clipped=abs(dx) == R or abs(dy) == R)


def norm(pend_q4, E):
    """step A: (float)pend / (float)(16 * E), each conversion rounded to nearest even, one fp32 division"""
    return F(F(np.int64(pend_q4)) / F(np.int64(16 * E)))


class Stream:
    """a stream's state: geometry, previous grid, counters, pending shift"""

    def __init__(self):
        self.geom, self.prev, self.step = None, None, 0
        self.pend = [0, 0]
        self.n_lost = self.n_applied = 0

    def reset(self, record=None):
        """zly_camera_reset: no grid, no geometry, counter 0, pending shift 0 (the record's two fields too); n_lost and n_applied stay"""
        self.geom, self.prev, self.step = None, None, 0
        self.pend = [0, 0]
        if record is not None:
            h = record[:HDR_BYTES].view(HDR_DTYPE)
            h["pend_x_q4"], h["pend_y_q4"] = 0, 0

    def frame_sums(self, S, W, H, cfg, record):
        """steps 2-9 on the grid S [gh][gw] of a W x H frame; record: u8 [REC_BYTES], changed in place and only where the rule writes -> header"""
        assert grid_ok(W, H, cfg) and cfg.cell in CELLS and 1 <= cfg.radius <= MAX_RADIUS and 0 <= cfg.max_residual_q4 <= 4080
        assert record.dtype == np.uint8 and record.shape == (REC_BYTES,)
        gh, gw = S.shape
        R = cfg.radius
        first = self.prev is None or self.geom != (W, H, cfg.cell)
        hdr = np.zeros(1, dtype=HDR_DTYPE)
        if first:
            hdr["flags"] = FIRST
            self.pend = [0, 0]
        else:
            e = estimate(S, self.prev, cfg)
            hdr["flags"] = (LOST if e["lost"] else 0) | (CLIPPED if e["clipped"] else 0)
            for k in ("dx", "dy", "fx", "fy", "sx_q4", "sy_q4", "sad_min", "sad_zero"):
                hdr[k] = e[k]
            if e["lost"]:
                self.n_lost += 1
            else:
                self.pend[0] += e["sx_q4"]
                self.pend[1] += e["sy_q4"]
            side = 2 * R + 1
            record[HDR_BYTES:HDR_BYTES + 8 * side * side] = e["tab"].reshape(-1).view(np.uint8)
        self.geom, self.prev, self.step = (W, H, cfg.cell), S.copy(), self.step + 1
        hdr["step"], hdr["gw"], hdr["gh"], hdr["n_lost"], hdr["n_applied"] = self.step, gw, gh, self.n_lost, self.n_applied
        hdr["pend_x_q4"], hdr["pend_y_q4"] = self.pend
        record[:HDR_BYTES] = hdr.view(np.uint8)
        return hdr[0]

    def frame(self, bgr, cfg, record):
        """steps 1-9 for the frame with the BGR image bgr"""
        H, W = bgr.shape[:2]
        return self.frame_sums(change_ref.sums(bgr, cfg.cell)[0], W, H, cfg, record)

    def shift(self):
        """step A's (nx, ny), or None for a stream without a geometry"""
        if self.geom is None:
            return None
        return norm(self.pend[0], self.geom[0]), norm(self.pend[1], self.geom[1])

    def apply(self, x, y, live, record=None):
        """step A on float32 arrays x, y and the live flags of one track table (changed in place); the record's three fields"""
        sh = self.shift()
        if sh is None:
            return None
        for t in range(len(live)):
            if live[t]:
                x[t], y[t] = F(F(x[t]) + sh[0]), F(F(y[t]) + sh[1])
        self.pend = [0, 0]
        self.n_applied += 1
        if record is not None:
            h = record[:HDR_BYTES].view(HDR_DTYPE)
            h["pend_x_q4"], h["pend_y_q4"], h["n_applied"] = 0, 0, self.n_applied
        return sh

    def apply_tracker(self, tracker):
        """step A on a tests/track_ref.py Tracker (or MotionTracker): every live slot's box moves"""
        sh = self.shift()
        if sh is None:
            return None
        for t in range(tracker.T):
            if tracker.live[t]:
                x, y, w, h = tracker.box[t]
                tracker.box[t] = (F(F(x) + sh[0]), F(F(y) + sh[1]), w, h)
        self.pend = [0, 0]
        self.n_applied += 1
        return sh
