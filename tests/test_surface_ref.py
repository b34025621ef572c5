"""tests/surface_ref.py against the definition it abbreviates: a surface after a rectangle is the frame in which every PIXEL of the rectangle has
been assigned, sample by sample, at the addresses include/zly.h gives for a tight frame of the format -- for every format, at legal rectangles of
every parity, and for sequences of rectangles in call order."""
import numpy as np
import pytest

import surface_ref as sr


def _samples(fmt, w, h, x, y):
    """the byte addresses of pixel (x, y)'s samples in a tight w x h frame of format fmt (include/zly.h "Pixel formats")"""
    kind, bpp, _, _ = sr.FORMATS[fmt]
    if kind == "packed" and bpp != 2:
        return [(y * w + x) * bpp + k for k in range(bpp)]
    if kind == "packed":                                   # 4:2:2: the pixel's whole macropixel Y0 U Y1 V / U Y0 V Y1
        return [(y * w + (x & ~1)) * 2 + k for k in range(4)]
    ci = (y >> 1) * (w // 2) + (x >> 1)
    if kind == "nv12":
        return [y * w + x, w * h + 2 * ci, w * h + 2 * ci + 1]
    return [y * w + x, w * h + ci, w * h + (w // 2) * (h // 2) + ci]


def _by_pixels(surface, fmt, w, h, x0, y0, rect, rw, rh):
    out = surface.copy()
    for y in range(rh):
        for x in range(rw):
            for d, s in zip(_samples(fmt, w, h, x0 + x, y0 + y), _samples(fmt, rw, rh, x, y)):
                out[d] = rect[s]
    return out


def _rects(fmt, w, h, rng, count):
    _, _, ex, ey = sr.FORMATS[fmt]
    sx, sy = (2 if ex else 1), (2 if ey else 1)
    out = [(0, 0, w, h), (0, 0, sx, sy), (w - sx, h - sy, sx, sy), (w - sx, 0, sx, sy), (0, h - sy, sx, sy)]
    while len(out) < count:
        rw, rh = int(rng.integers(1, w // sx + 1)) * sx, int(rng.integers(1, h // sy + 1)) * sy
        out.append((int(rng.integers(0, (w - rw) // sx + 1)) * sx, int(rng.integers(0, (h - rh) // sy + 1)) * sy, rw, rh))
    return out


@pytest.mark.parametrize("fmt", sr.ALL_FORMATS)
def test_apply_is_per_pixel_assignment(fmt):
    rng = np.random.default_rng(100 + fmt)
    _, _, ex, ey = sr.FORMATS[fmt]
    for w, h in ((38 if ex else 37, 30 if ey else 29), (2, 2), (16, 6)):
        assert sr.frame_bytes(fmt, w, h) == len({a for y in range(h) for x in range(w) for a in _samples(fmt, w, h, x, y)})
        surface = rng.integers(0, 256, sr.frame_bytes(fmt, w, h), dtype=np.uint8)
        for x0, y0, rw, rh in _rects(fmt, w, h, rng, 24):
            rect = rng.integers(0, 256, sr.frame_bytes(fmt, rw, rh), dtype=np.uint8)
            want = _by_pixels(surface, fmt, w, h, x0, y0, rect, rw, rh)
            got = sr.apply(surface.copy(), fmt, w, h, x0, y0, rect, rw, rh)
            assert np.array_equal(got, want), (fmt, w, h, x0, y0, rw, rh)
            assert np.array_equal(sr.cut(got, fmt, w, h, x0, y0, rw, rh), rect)
            surface = got                                   # the next rectangle lands on this one: call order


def test_a_keyframe_replaces_every_byte_and_a_rectangle_touches_only_its_own():
    for fmt in sr.ALL_FORMATS:
        _, bpp, ex, ey = sr.FORMATS[fmt]
        w, h = 12, 8
        frame = np.arange(sr.frame_bytes(fmt, w, h), dtype=np.uint8) | 1
        assert np.array_equal(sr.apply(np.zeros(frame.size, np.uint8), fmt, w, h, 0, 0, frame, w, h), frame)
        rect = np.full(sr.frame_bytes(fmt, 2, 2), 255, dtype=np.uint8)
        after = sr.apply(np.zeros(frame.size, np.uint8), fmt, w, h, 4, 2, rect, 2, 2)
        assert int((after == 255).sum()) == rect.size and int((after != 0).sum()) == rect.size


def test_apply_accepts_shaped_rectangles_of_the_one_plane_formats():
    s = np.zeros(sr.frame_bytes(sr.PIX_BGR, 5, 4), dtype=np.uint8)
    r = np.arange(2 * 3 * 3, dtype=np.uint8).reshape(2, 3, 3) + 1
    a = sr.apply(s.copy(), sr.PIX_BGR, 5, 4, 1, 2, r)
    assert np.array_equal(a.reshape(4, 5, 3)[2:4, 1:4], r) and int((a != 0).sum()) == r.size


def test_legal_is_the_crop_rule():
    assert sr.legal(sr.PIX_BGR, 37, 29, 36, 28, 1, 1) and not sr.legal(sr.PIX_BGR, 37, 29, 36, 28, 2, 1) and not sr.legal(sr.PIX_BGR, 37, 29, -1, 0, 1, 1)
    assert not sr.legal(sr.PIX_BGR, 37, 29, 0, 0, 0, 1)
    for fmt in (sr.PIX_NV12_BT601, sr.PIX_I420_BT709):
        assert sr.legal(fmt, 38, 30, 2, 4, 2, 2)
        for bad in ((1, 4, 2, 2), (2, 3, 2, 2), (2, 4, 3, 2), (2, 4, 2, 1)):
            assert not sr.legal(fmt, 38, 30, *bad), bad
    for fmt in (sr.PIX_YUY2_BT601, sr.PIX_UYVY_BT709):
        assert sr.legal(fmt, 38, 29, 2, 3, 2, 1) and not sr.legal(fmt, 38, 29, 1, 3, 2, 1) and not sr.legal(fmt, 38, 29, 2, 3, 1, 1)
    assert sr.covers(37, 29, 0, 0, 37, 29) and not sr.covers(37, 29, 0, 0, 37, 28)
    assert sr.disjoint((0, 0, 2, 2), (2, 0, 2, 2)) and not sr.disjoint((0, 0, 3, 2), (2, 1, 2, 2))
