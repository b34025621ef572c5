"""numpy reference of frame views (include/zly.h zly_frame_view): where a request's samples lie inside a larger, possibly pitched buffer.

Written from the header's definition with numpy slicing, independently of the library's helpers: View / surface / crop / nbytes mirror
zly_view_tight / zly_view_crop / zly_view_bytes, extract() makes the tight frame a view denotes -- the frame the engine must treat the view as,
bit for bit -- and embed() builds a surface around a frame."""
from collections import namedtuple

import numpy as np

PIX_BGR, PIX_NV12_BT601, PIX_I420_BT601, PIX_NV12_BT709, PIX_I420_BT709 = 0, 1, 2, 3, 4
ALL_FORMATS = (PIX_BGR, PIX_NV12_BT601, PIX_I420_BT601, PIX_NV12_BT709, PIX_I420_BT709)

View = namedtuple("View", "fmt w h off pitch")          # off, pitch: tuples, one entry per plane the format has


def is_nv12(fmt):
    return fmt in (PIX_NV12_BT601, PIX_NV12_BT709)


def plane_shapes(fmt, w, h):
    """[(rows, row_bytes)] per plane of a w x h frame"""
    if fmt == PIX_BGR:
        return [(h, 3 * w)]
    assert w % 2 == 0 and h % 2 == 0 and w >= 2 and h >= 2
    if is_nv12(fmt):
        return [(h, w), (h // 2, w)]
    return [(h, w), (h // 2, w // 2), (h // 2, w // 2)]


def tight_pitches(fmt, w):
    return [rb for _, rb in plane_shapes(fmt, w, 2)]


def surface(fmt, w, h, pitches=None):
    """the view of a whole surface whose planes follow each other, each of rows * pitch bytes; pitches None = tight"""
    shapes = plane_shapes(fmt, w, h)
    pitches = list(pitches) if pitches is not None else [rb for _, rb in shapes]
    off, o = [], 0
    for (rows, _), p in zip(shapes, pitches):
        off.append(o)
        o += rows * p
    return View(fmt, w, h, tuple(off), tuple(pitches))


def crop(v, x0, y0, w, h):
    assert 0 <= x0 and 0 <= y0 and w >= 1 and h >= 1 and x0 + w <= v.w and y0 + h <= v.h
    if v.fmt == PIX_BGR:
        off = (v.off[0] + y0 * v.pitch[0] + 3 * x0,)
    else:
        assert x0 % 2 == 0 and y0 % 2 == 0 and w % 2 == 0 and h % 2 == 0
        off = [v.off[0] + y0 * v.pitch[0] + x0]
        if is_nv12(v.fmt):
            off.append(v.off[1] + (y0 // 2) * v.pitch[1] + (x0 // 2) * 2)
        else:
            off += [v.off[p] + (y0 // 2) * v.pitch[p] + x0 // 2 for p in (1, 2)]
        off = tuple(off)
    return View(v.fmt, w, h, off, v.pitch)


def extents(v):
    return [(rows - 1) * p + rb for (rows, rb), p in zip(plane_shapes(v.fmt, v.w, v.h), v.pitch)]


def nbytes(v):
    """the smallest buffer that holds the view"""
    return max(o + e for o, e in zip(v.off, extents(v)))


def _plane(buf, off, pitch, rows, rb):
    """rows x rb window of a pitched plane as a strided numpy view"""
    return np.lib.stride_tricks.as_strided(buf[off:], shape=(rows, rb), strides=(pitch, 1), writeable=True)


def extract(buf, v):
    """the tight frame of the view's samples: u8 [h][w][3] for BGR, the packed 1-D buffer for YUV 4:2:0"""
    buf = np.asarray(buf, dtype=np.uint8).reshape(-1)
    assert nbytes(v) <= buf.size
    parts = [np.array(_plane(buf, o, p, rows, rb)) for (rows, rb), o, p in zip(plane_shapes(v.fmt, v.w, v.h), v.off, v.pitch)]
    if v.fmt == PIX_BGR:
        return np.ascontiguousarray(parts[0].reshape(v.h, v.w, 3))
    return np.ascontiguousarray(np.concatenate([q.reshape(-1) for q in parts]))


def embed(frame, fmt, surf_w, surf_h, pitches, x0, y0, fill, w=None, h=None):
    """a surf_w x surf_h surface with the given pitches (None = tight) whose bytes are all `fill` (a byte, or "noise" for seeded random
    bytes), except that the rectangle at (x0, y0) holds `frame` (BGR [h][w][3], or a packed YUV buffer with explicit w, h).
    -> (buffer, the view of the rectangle)"""
    frame = np.asarray(frame, dtype=np.uint8)
    if fmt == PIX_BGR:
        h, w = frame.shape[:2]
    s = surface(fmt, surf_w, surf_h, pitches)
    total = sum(rows * p for (rows, _), p in zip(plane_shapes(fmt, surf_w, surf_h), s.pitch))
    if isinstance(fill, str):
        buf = np.random.default_rng(surf_w * 31 + surf_h).integers(0, 256, total, dtype=np.uint8)
    else:
        buf = np.full(total, fill, dtype=np.uint8)
    v = crop(s, x0, y0, w, h)
    flat = frame.reshape(-1)
    pos = 0
    for (rows, rb), o, p in zip(plane_shapes(fmt, w, h), v.off, v.pitch):
        _plane(buf, o, p, rows, rb)[...] = flat[pos:pos + rows * rb].reshape(rows, rb)
        pos += rows * rb
    assert pos == flat.size
    return buf, v


def shift(v, delta):
    """the same view in a buffer that starts `delta` bytes earlier (surfaces packed one behind the other)"""
    return View(v.fmt, v.w, v.h, tuple(o + delta for o in v.off), v.pitch)


def to_c(v):
    """-> zly.FrameView"""
    import zly
    c = zly.FrameView()
    c.fmt, c.w, c.h = v.fmt, v.w, v.h
    for p, (o, pi) in enumerate(zip(v.off, v.pitch)):
        c.off[p] = o
        c.pitch[p] = pi
    return c


def from_c(c):
    n = len(plane_shapes(c.fmt, c.w, c.h))
    return View(c.fmt, c.w, c.h, tuple(int(c.off[p]) for p in range(n)), tuple(int(c.pitch[p]) for p in range(n)))
