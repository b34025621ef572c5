"""The exact numpy oracle of the change map (include/zly.h, "Change map"), written from the header alone: the luma of the frame's BGR image, the
cells' sums, the stream's state with FIRST, the ACTIVE and GLOBAL decisions, the greedy peaks with the initial suppression, the record -- including
what it must NOT write -- and the fill of a zoom call's fallback regions.

luma() and sums() are steps 1-2, Stream.frame() steps 3-8 for one frame of one stream on a record buffer of the caller's, fill() the zoom fill.
Frames of other formats are first converted to BGR by their own references (chip_ref.bgr_of)."""
from dataclasses import dataclass

import numpy as np

import chip_ref

FIRST, GLOBAL = 1, 2
MAX_CELLS, MAX_DIM, MAX_PEAKS = 8192, chip_ref.MAX_DIM, 15
CELLS = (8, 16, 32, 64)

HDR_DTYPE = np.dtype([("n_cells", "<i4"), ("n_active", "<i4"), ("n_peaks", "<i4"), ("flags", "<u4"), ("gw", "<i4"), ("gh", "<i4"), ("step", "<u4"), ("pad", "<u4")])
PEAK_DTYPE = np.dtype([("x0", "<i4"), ("y0", "<i4"), ("w", "<i4"), ("h", "<i4"), ("cx", "<i4"), ("cy", "<i4"), ("activity", "<u4"), ("pad", "<u4")])
assert HDR_DTYPE.itemsize == 32 and PEAK_DTYPE.itemsize == 32


@dataclass
class Config:
    """zly_change_config"""
    cell: int = 32
    threshold_q4: int = 32
    max_active_permille: int = 250
    max_peaks: int = 3
    window_w: int = 416
    window_h: int = 416


def layout(cfg):
    """step 8 -> (rec_bytes, peaks_off, activity_off)"""
    peaks_off = HDR_DTYPE.itemsize
    activity_off = peaks_off + cfg.max_peaks * PEAK_DTYPE.itemsize
    return activity_off + 4 * MAX_CELLS, peaks_off, activity_off


def luma(bgr):
    """step 1: u32 [H][W]"""
    b = np.asarray(bgr, dtype=np.uint8).astype(np.uint32)
    return (29 * b[..., 0] + 150 * b[..., 1] + 77 * b[..., 2] + 128) >> 8


def grid(W, H, C):
    return -(-W // C), -(-H // C)


def sums(bgr, C):
    """step 2: u32 [gh][gw], and the cells' pixel counts"""
    Y = luma(bgr)
    H, W = Y.shape
    gw, gh = grid(W, H, C)
    S, npix = np.zeros((gh, gw), dtype=np.uint32), np.zeros((gh, gw), dtype=np.uint32)
    for cy in range(gh):
        for cx in range(gw):
            cell = Y[cy * C:min((cy + 1) * C, H), cx * C:min((cx + 1) * C, W)]
            S[cy, cx], npix[cy, cx] = cell.sum(dtype=np.uint64), cell.size
    return S, npix


def window(W, H, cfg):
    """step 6 -> (rw, rh, xmax, ymax)"""
    rw, rh = min(cfg.window_w, W & ~1), min(cfg.window_h, H & ~1)
    return rw, rh, (W - rw) & ~1, (H - rh) & ~1


def centre(c, C, E):
    return min(c * C + C // 2, E - 1)


def origin(pc, r, omax):
    return min(max(pc - r // 2, 0), omax) & ~1


def pick(A, npix, W, H, cfg, suppress=()):
    """steps 4-7 on an activity grid -> (n_active, is_global, [(x0, y0, rw, rh, cx, cy, A)]); suppress: rectangles (x0, y0, rw, rh)"""
    gh, gw = A.shape
    C = cfg.cell
    active = 16 * A.astype(np.int64) > cfg.threshold_q4 * npix.astype(np.int64)
    n_active = int(active.sum())
    is_global = n_active * 1000 > cfg.max_active_permille * gw * gh
    peaks = []
    if is_global or W < 2 or H < 2:
        return n_active, is_global, peaks
    rw, rh, xmax, ymax = window(W, H, cfg)
    pcx = np.array([centre(cx, C, W) for cx in range(gw)])
    pcy = np.array([centre(cy, C, H) for cy in range(gh)])

    def inside(x0, y0, w, h):
        return ((pcy >= y0) & (pcy < y0 + h))[:, None] & ((pcx >= x0) & (pcx < x0 + w))[None, :]
    live = active.copy()
    for (x0, y0, w, h) in suppress:
        live &= ~inside(x0, y0, w, h)
    while len(peaks) < cfg.max_peaks and live.any():
        flat = np.where(live, A, 0).reshape(-1)
        i = int(np.argmax(flat))                       # the first of the largest: the lowest index
        cx, cy = i % gw, i // gw
        x0, y0 = origin(int(pcx[cx]), rw, xmax), origin(int(pcy[cy]), rh, ymax)
        peaks.append((x0, y0, rw, rh, cx, cy, int(A[cy, cx])))
        live[cy, cx] = False
        live &= ~inside(x0, y0, rw, rh)
    return n_active, is_global, peaks


class Stream:
    """a stream's state: geometry, previous grid, counter"""

    def __init__(self):
        self.reset()

    def reset(self):
        self.geom, self.prev, self.step = None, None, 0

    def frame(self, bgr, cfg, record, suppress=()):
        """steps 3-8 for the frame with the BGR image bgr; record: u8 [rec_bytes], what the stream's record held -- changed in place, and only where
        the rule writes.  -> (header, peaks list, activity grid)"""
        H, W = bgr.shape[:2]
        assert 1 <= W <= MAX_DIM and 1 <= H <= MAX_DIM and cfg.cell in CELLS
        gw, gh = grid(W, H, cfg.cell)
        assert gw * gh <= MAX_CELLS
        S, npix = sums(bgr, cfg.cell)
        first = self.prev is None or self.geom != (W, H, cfg.cell)
        if first:
            A, n_active, is_global, peaks = np.zeros((gh, gw), dtype=np.uint32), 0, False, []
        else:
            A = np.abs(S.astype(np.int64) - self.prev.astype(np.int64)).astype(np.uint32)
            n_active, is_global, peaks = pick(A, npix, W, H, cfg, suppress)
        self.geom, self.prev, self.step = (W, H, cfg.cell), S, self.step + 1
        rec_bytes, peaks_off, activity_off = layout(cfg)
        assert record.dtype == np.uint8 and record.shape == (rec_bytes,)
        hdr = np.zeros(1, dtype=HDR_DTYPE)
        hdr["n_cells"], hdr["n_active"], hdr["n_peaks"], hdr["gw"], hdr["gh"], hdr["step"] = gw * gh, n_active, len(peaks), gw, gh, self.step
        hdr["flags"] = (FIRST if first else 0) | (GLOBAL if is_global else 0)
        record[:32] = hdr.view(np.uint8)
        for p, pk in enumerate(peaks):
            rec = np.zeros(1, dtype=PEAK_DTYPE)
            rec["x0"], rec["y0"], rec["w"], rec["h"], rec["cx"], rec["cy"], rec["activity"] = pk
            record[peaks_off + 32 * p:peaks_off + 32 * (p + 1)] = rec.view(np.uint8)
        record[activity_off:activity_off + 4 * gw * gh] = A.reshape(-1).view(np.uint8)
        return hdr[0], peaks, A


def fill(plan, peaks):
    """the zoom fill: plan a structured array with x0, y0, w, h, slot, track_id (K regions of one frame); peak p goes to the p-th region with
    slot == -1, which becomes {x0, y0 of the peak, slot = -2, track_id = 0}.  -> a copy"""
    out = plan.copy()
    p = 0
    for j in range(len(out)):
        if p >= len(peaks):
            break
        if int(out[j]["slot"]) != -1:
            continue
        out[j]["x0"], out[j]["y0"], out[j]["slot"], out[j]["track_id"] = peaks[p][0], peaks[p][1], -2, 0
        p += 1
    return out


def track_rects(plan):
    """the initial suppression of a zoom call: the plan's regions with slot >= 0"""
    return [(int(r["x0"]), int(r["y0"]), int(r["w"]), int(r["h"])) for r in plan if int(r["slot"]) >= 0]
