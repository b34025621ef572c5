"""The exact numpy oracle of the tile merge (include/zly.h, "Tiles"): float32 scalars, one rounding per operation, the sequential greedy loop.

merge_group() takes the sources of one group -- (header n_kept, header flags, detection records, tile) in ascending slab index -- and returns the
group's output (n_kept, n_candidates, flags, the stored records).  merge_slabs() is zly_merge_slabs on raw slab bytes: it returns the bytes that
the output buffer must hold, given what it held before (records at or beyond the stored count are not written).  tile_grid() is zly_tile_grid
in plain integers.  Written from the header alone: it shares no code with the kernel.

`strict` and `tie_break` exist for tests/test_merge_ref.py only, which perturbs the rule to show that the hand cases notice.
"""
from typing import List, Optional, Sequence, Tuple

import numpy as np

from zly import DET_DTYPE, SLAB_HDR_DTYPE, SLAB_OVERFLOW

F = np.float32
IOU, IOS = 0, 1
MAX_CANDIDATES = 4096
Tile = Tuple[int, int, int, int, int, int, int]          # group, x0, y0, w, h, W, H


def map_box(d, t: Tile):
    """step 2: (x, y, bw, bh) of a tile -> surface fractions"""
    _, x0, y0, w, h, W, H = t
    x = F(F(F(F(d["x"]) * F(w)) + F(x0)) / F(W))
    y = F(F(F(F(d["y"]) * F(h)) + F(y0)) / F(H))
    bw = F(F(F(d["w"]) * F(w)) / F(W))
    bh = F(F(F(d["h"]) * F(h)) / F(H))
    return x, y, bw, bh


def measure(a, b, metric: int) -> np.float32:
    """step 4: m for the mapped boxes a (earlier) and b (later)"""
    ax, ay, aw, ah = a
    bx, by, bw, bh = b
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
    area_a, area_b = F(aw * ah), F(bw * bh)
    if metric == IOU:
        uni = F(F(area_a + area_b) - inter)
        return F(inter / uni) if uni > 0 else F(0)
    mn = area_a if area_a < area_b else area_b
    return F(inter / mn) if mn > 0 else F(0)


def measure_many(a, b, metric: int) -> np.ndarray:
    """measure(a, b[k]) for every k: b = (x, y, w, h) float32 arrays"""
    ax, ay, aw, ah = a
    bx, by, bw, bh = b
    two = F(2)
    ax0, ay0, ax1, ay1 = F(ax - F(aw / two)), F(ay - F(ah / two)), F(ax + F(aw / two)), F(ay + F(ah / two))
    bx0, by0, bx1, by1 = bx - bw / two, by - bh / two, bx + bw / two, by + bh / two
    lo_x = np.where(ax0 < bx0, bx0, ax0)
    hi_x = np.where(bx1 < ax1, bx1, ax1)
    lo_y = np.where(ay0 < by0, by0, ay0)
    hi_y = np.where(by1 < ay1, by1, ay1)
    dx, dy = hi_x - lo_x, hi_y - lo_y
    ox = np.where(F(0) < dx, dx, F(0))
    oy = np.where(F(0) < dy, dy, F(0))
    inter = ox * oy
    area_a, area_b = F(aw * ah), bw * bh
    with np.errstate(divide="ignore", invalid="ignore"):
        if metric == IOU:
            uni = (area_a + area_b) - inter
            m = np.where(uni > 0, inter / uni, F(0))
        else:
            mn = np.where(area_a < area_b, area_a, area_b)
            m = np.where(mn > 0, inter / mn, F(0))
    assert m.dtype == F
    return m


def merge_group(sources: Sequence[tuple], cap: int, metric: int, thr: float, strict: bool = True, tie_break: bool = True):
    """sources: (n_kept, flags, records, tile) per source, ascending slab index -> (n_kept, n_candidates, flags, records[min(n_kept, cap)])"""
    thr = F(thr)
    cands = []
    flags = 0
    for si, (n_kept, fl, recs, t) in enumerate(sources):
        flags |= int(fl) & SLAB_OVERFLOW
        for pos in range(max(0, min(int(n_kept), cap))):
            d = recs[pos]
            cands.append((int(d["class_id"]), float(F(d["confidence"])), si, pos, map_box(d, t), d))
    # step 3: class ascending, confidence descending as value (float64 of a float32 is exact; -0.0 == 0.0 ties), slab, position
    if tie_break:
        cands.sort(key=lambda c: (c[0], -c[1], c[2], c[3]))
    else:
        cands.sort(key=lambda c: (c[0], -c[1], -c[2], -c[3]))
    # step 4 with the inner loop over numpy float32 arrays: element-wise IEEE single operations, one rounding each, the same sequence as
    # measure() (tests/test_merge_ref.py holds the two against each other bit for bit)
    n = len(cands)
    cls = np.array([c[0] for c in cands], dtype=np.int64)
    B = tuple(np.array([c[4][k] for c in cands], dtype=F) for k in range(4))
    alive = np.ones(n, dtype=bool)
    seg_end = np.searchsorted(cls, cls, side="right")      # classes ascend: nothing of a's class lies beyond its segment
    for i in range(n):
        if not alive[i] or i + 1 >= seg_end[i]:
            continue
        r = slice(i + 1, int(seg_end[i]))
        m = measure_many(cands[i][4], tuple(b[r] for b in B), metric)
        alive[r] &= ~((m > thr) if strict else (m >= thr))
    keep = [c for c, al in zip(cands, alive) if al]
    out = np.zeros(min(len(keep), cap), dtype=DET_DTYPE)
    for k, c in enumerate(keep[:cap]):
        out[k]["x"], out[k]["y"], out[k]["w"], out[k]["h"] = c[4]
        out[k]["confidence"], out[k]["class_id"] = c[5]["confidence"], c[5]["class_id"]
    if len(keep) > cap:
        flags |= SLAB_OVERFLOW
    return len(keep), len(cands), flags, out


def merge_slabs(raw: np.ndarray, tiles: Sequence[Tile], n_groups: int, cap: int, metric: int, thr: float, tag0: int, before: np.ndarray, **perturb) -> np.ndarray:
    """raw: u8 [n][slab_bytes] sources; before: u8 [>= n_groups][slab_bytes], what the output buffer held -> what it must hold afterwards"""
    out = before.copy()
    for g in range(n_groups):
        src = []
        for i, t in enumerate(tiles):
            if t[0] != g:
                continue
            hdr = raw[i, :16].view(SLAB_HDR_DTYPE)[0]
            src.append((int(hdr["n_kept"]), int(hdr["flags"]), raw[i, 16:].view(DET_DTYPE), t))
        assert len(src) * cap <= MAX_CANDIDATES
        n_kept, n_cand, flags, recs = merge_group(src, cap, metric, thr, **perturb)
        hdr = out[g, :16].view(SLAB_HDR_DTYPE)
        hdr["n_kept"], hdr["n_candidates"], hdr["flags"], hdr["frame_tag"] = n_kept, n_cand, flags, (tag0 + g) & 0xFFFFFFFF
        out[g, 16:16 + 40 * len(recs)] = recs.view(np.uint8)
    return out


def _axis(extent: int, tile: int, overlap: int, even: bool) -> Optional[List[Tuple[int, int]]]:
    """(origin, size) of one axis' tiles, None when the arguments are refused"""
    if not (1 <= extent < 1 << 24) or tile < 1 or overlap < 0 or overlap >= tile:
        return None
    if even and (extent % 2 or tile % 2):
        return None
    step = tile - overlap
    if tile >= extent:
        return [(0, extent)]
    count = -(-(extent - tile) // step) + 1
    out = []
    for i in range(count):
        o = min(i * step, extent - tile)
        out.append((o - o % 2 if even else o, tile))
    return out


def tile_grid(W: int, H: int, tile_w: int, tile_h: int, overlap_x: int = 0, overlap_y: int = 0, even: bool = False) -> Optional[List[Tile]]:
    """zly_tile_grid: row-major tiles with group 0, or None where it answers ZLY_ERR_INVALID_ARGUMENT"""
    xs, ys = _axis(W, tile_w, overlap_x, even), _axis(H, tile_h, overlap_y, even)
    if xs is None or ys is None:
        return None
    return [(0, x0, y0, w, h, W, H) for y0, h in ys for x0, w in xs]
