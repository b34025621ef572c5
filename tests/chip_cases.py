"""Shared case builders of the chips' tests (tests/test_chip_rules.py on the CPU, tests/test_gpu_chips.py on the GPU): frames of all twelve pixel
formats as tight buffers or as pitched views inside a poisoned buffer, and boxes that step 4 of include/zly.h's "Chips" turns into a wanted rectangle."""
import numpy as np

import chip_ref as cr
import pixfmt_ref as pr
import yuv422_ref as y2
import yuv_ref as yr

PIX_BGR = 0
F420, F422, FPK = tuple(yr.YUV_FORMATS), tuple(y2.FORMATS), (PIX_BGR,) + tuple(pr.PACKED)
ALL_FORMATS = FPK + F420 + F422
assert len(ALL_FORMATS) == 12
POISON = 0xA5


def is_nv12(fmt):
    return fmt in F420 and yr.is_nv12(fmt)


def plane_shapes(fmt, w, h):
    """[(rows, row_bytes)] per plane of a tight w x h frame"""
    if fmt in FPK:
        return [(h, pr.BPP[fmt] * w)]
    if fmt in F422:
        return [(h, 2 * w)]
    if is_nv12(fmt):
        return [(h, w), (h // 2, w)]
    return [(h, w), (h // 2, w // 2), (h // 2, w // 2)]


def smallest(fmt):
    """the smallest legal frame of the format"""
    return (2, 2) if fmt in F420 else (2, 1) if fmt in F422 else (1, 1)


def legal(fmt, w, h):
    """the size rounded up to what the format allows"""
    if fmt in F420:
        return w + (w & 1), h + (h & 1)
    if fmt in F422:
        return w + (w & 1), h
    return w, h


def frame(fmt, w, h, seed):
    """(tight frame as a flat u8 array, its BGR image): every byte random -- any byte is a legal sample"""
    n = sum(r * rb for r, rb in plane_shapes(fmt, w, h))
    f = np.random.default_rng(seed * 1000 + fmt).integers(0, 256, n, dtype=np.uint8)
    return f, np.ascontiguousarray(cr.bgr_of(fmt, f if fmt not in FPK else f.reshape(h, w, pr.BPP[fmt]), w, h))


def constant_frame(fmt, w, h, value):
    """a tight frame whose every byte is `value` (a constant image in every format)"""
    n = sum(r * rb for r, rb in plane_shapes(fmt, w, h))
    f = np.full(n, value, dtype=np.uint8)
    return f, np.ascontiguousarray(cr.bgr_of(fmt, f if fmt not in FPK else f.reshape(h, w, pr.BPP[fmt]), w, h))


def tight_view(fmt, w, h, base=0):
    """(fmt, w, h, off[3], pitch[3]) of a tight frame that starts `base` bytes into its buffer"""
    off, pitch, o = [0, 0, 0], [0, 0, 0], base
    for p, (rows, rb) in enumerate(plane_shapes(fmt, w, h)):
        off[p], pitch[p] = o, rb
        o += rows * rb
    return fmt, w, h, off, pitch


def pitched(frame_flat, fmt, w, h, pad=7, lead=5, fill=POISON):
    """the frame's samples inside a buffer of `fill` bytes: `lead` bytes in front of every plane, every row `pad` (+ the plane's index) bytes longer
    than its samples, and the last row of a plane NOT padded -- a plane ends with its last sample.  -> (buffer, view tuple as tight_view's)"""
    parts, off, pitch, o, pos = [], [0, 0, 0], [0, 0, 0], 0, 0
    for p, (rows, rb) in enumerate(plane_shapes(fmt, w, h)):
        pt = rb + pad + p
        plane = np.full(lead + (rows - 1) * pt + rb, fill, dtype=np.uint8)
        for r in range(rows):
            plane[lead + r * pt:lead + r * pt + rb] = frame_flat[pos + r * rb:pos + (r + 1) * rb]
        pos += rows * rb
        off[p], pitch[p] = o + lead, pt
        o += plane.size
        parts.append(plane)
    assert pos == frame_flat.size
    return np.concatenate(parts), (fmt, w, h, off, pitch)


def to_c(view):
    """view tuple -> zly.FrameView"""
    import zly
    fmt, w, h, off, pitch = view
    c = zly.FrameView()
    c.fmt, c.w, c.h = fmt, w, h
    for p in range(3):
        c.off[p], c.pitch[p] = off[p], pitch[p]
    return c


def shifted(view, delta):
    fmt, w, h, off, pitch = view
    n = len(plane_shapes(fmt, w, h))
    return fmt, w, h, [o + delta if p < n else 0 for p, o in enumerate(off)], pitch


def box_axis(o, n, E, scale):
    """(centre, size) of a box that step 4 turns into origin o, length n on an extent of E pixels: its scaled edges aim at the middle of the pixels
    o and o + n, half a pixel away from where truncation would change the result"""
    lo, hi = (o + 0.5) / E, (o + n + 0.5) / E
    x, w = np.float32((lo + hi) / 2), np.float32((hi - lo) / scale)
    assert cr.rect_axis(x, w, scale, E) == (o, n), (o, n, E, scale, cr.rect_axis(x, w, scale, E))
    return x, w


def box(x0, y0, rw, rh, W, H, scale, conf=0.9, cls=0, track=0):
    """a detection (x, y, w, h, confidence, class_id, track_id) whose rectangle is (x0, y0, rw, rh)"""
    x, w = box_axis(x0, rw, W, scale)
    y, h = box_axis(y0, rh, H, scale)
    return float(x), float(y), float(w), float(h), conf, cls, track
