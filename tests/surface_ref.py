"""numpy oracle of the resident surfaces (include/zly.h "Resident surfaces").

A surface is a 1-D u8 array in tight layout (zly_view_tight): the planes one behind the other, rows without pitch.  apply() writes a rectangle's
tight bytes into it, plane by plane, from a format table of its own -- written from the header, independently of csrc/frame_rules.h.  legal() is
zly_view_crop's rule for a destination rectangle.  tests/test_surface_ref.py holds apply() against per-pixel assignment."""
import numpy as np

PIX_BGR, PIX_NV12_BT601, PIX_I420_BT601, PIX_NV12_BT709, PIX_I420_BT709 = 0, 1, 2, 3, 4
PIX_YUY2_BT601, PIX_UYVY_BT601, PIX_YUY2_BT709, PIX_UYVY_BT709 = 10, 11, 12, 13
PIX_RGB, PIX_BGRA, PIX_RGBA = 16, 17, 18

# fmt -> (kind, bytes per pixel of plane 0, x must be even, y must be even); kind: "packed" (one plane), "nv12", "i420"
FORMATS = {
    PIX_BGR: ("packed", 3, False, False), PIX_RGB: ("packed", 3, False, False), PIX_BGRA: ("packed", 4, False, False), PIX_RGBA: ("packed", 4, False, False),
    PIX_YUY2_BT601: ("packed", 2, True, False), PIX_UYVY_BT601: ("packed", 2, True, False), PIX_YUY2_BT709: ("packed", 2, True, False), PIX_UYVY_BT709: ("packed", 2, True, False),
    PIX_NV12_BT601: ("nv12", 1, True, True), PIX_NV12_BT709: ("nv12", 1, True, True), PIX_I420_BT601: ("i420", 1, True, True), PIX_I420_BT709: ("i420", 1, True, True),
}
ALL_FORMATS = tuple(sorted(FORMATS))


def planes(fmt, w, h):
    """[(rows, row_bytes, x divisor, y divisor, bytes per x unit)] per plane of a w x h frame: a rectangle at (x0, y0) starts in the plane at row
    y0 / ydiv, byte (x0 / xdiv) * unit"""
    kind, bpp, _, _ = FORMATS[fmt]
    if kind == "packed":
        return [(h, bpp * w, 1, 1, bpp)]
    if kind == "nv12":
        return [(h, w, 1, 1, 1), (h // 2, w, 2, 2, 2)]
    return [(h, w, 1, 1, 1), (h // 2, w // 2, 2, 2, 1), (h // 2, w // 2, 2, 2, 1)]


def size_ok(fmt, w, h):
    if fmt not in FORMATS or w < 1 or h < 1:
        return False
    _, _, ex, ey = FORMATS[fmt]
    return not (ex and w % 2) and not (ey and h % 2)


def frame_bytes(fmt, w, h):
    return sum(rows * rb for rows, rb, *_ in planes(fmt, w, h)) if size_ok(fmt, w, h) else 0


def legal(fmt, W, H, x0, y0, w, h):
    """may the rectangle (x0, y0, w, h) be written into a W x H surface of format fmt?  (zly_view_crop's rule)"""
    if not size_ok(fmt, W, H) or x0 < 0 or y0 < 0 or w < 1 or h < 1 or x0 + w > W or y0 + h > H:
        return False
    _, _, ex, ey = FORMATS[fmt]
    return not (ex and (x0 % 2 or w % 2)) and not (ey and (y0 % 2 or h % 2))


def apply(surface, fmt, w, h, x0, y0, rect_bytes, rw=None, rh=None):
    """writes, in place, the tight rw x rh rectangle rect_bytes (1-D u8; for the one-plane formats rw, rh may be left out when rect_bytes is
    [rh][rw * bpp] or [rh][rw][bpp]) at (x0, y0) into the tight w x h surface; returns the surface"""
    rect = np.asarray(rect_bytes, dtype=np.uint8)
    if rw is None:
        assert FORMATS[fmt][0] == "packed" and rect.ndim >= 2
        rh, rw = rect.shape[0], rect.size // rect.shape[0] // FORMATS[fmt][1]
    rect = rect.reshape(-1)
    assert surface.dtype == np.uint8 and surface.ndim == 1 and surface.size >= frame_bytes(fmt, w, h)
    assert legal(fmt, w, h, x0, y0, rw, rh), (fmt, w, h, x0, y0, rw, rh)
    assert rect.size == frame_bytes(fmt, rw, rh)
    soff = roff = 0
    for (srows, srb, xd, yd, unit), (rrows, rrb, *_) in zip(planes(fmt, w, h), planes(fmt, rw, rh)):
        dst = surface[soff:soff + srows * srb].reshape(srows, srb)
        b0 = (x0 // xd) * unit
        dst[y0 // yd:y0 // yd + rrows, b0:b0 + rrb] = rect[roff:roff + rrows * rrb].reshape(rrows, rrb)
        soff += srows * srb
        roff += rrows * rrb
    return surface


def cut(surface, fmt, w, h, x0, y0, rw, rh):
    """the tight rw x rh rectangle at (x0, y0) of the tight w x h surface, as a 1-D u8 array (the inverse of apply)"""
    assert legal(fmt, w, h, x0, y0, rw, rh), (fmt, w, h, x0, y0, rw, rh)
    out, soff = [], 0
    for (srows, srb, xd, yd, unit), (rrows, rrb, *_) in zip(planes(fmt, w, h), planes(fmt, rw, rh)):
        src = surface[soff:soff + srows * srb].reshape(srows, srb)
        b0 = (x0 // xd) * unit
        out.append(src[y0 // yd:y0 // yd + rrows, b0:b0 + rrb].reshape(-1))
        soff += srows * srb
    return np.ascontiguousarray(np.concatenate(out))


def covers(w, h, x0, y0, rw, rh):
    """a keyframe: the rectangle is the whole surface"""
    return x0 == 0 and y0 == 0 and rw == w and rh == h


def disjoint(a, b):
    """two rectangles (x0, y0, w, h) of one surface"""
    return a[0] + a[2] <= b[0] or b[0] + b[2] <= a[0] or a[1] + a[3] <= b[1] or b[1] + b[3] <= a[1]
