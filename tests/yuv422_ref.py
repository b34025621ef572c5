"""numpy reference of the packed YUV 4:2:2 input formats ZLY_PIX_YUY2_* / ZLY_PIX_UYVY_* (include/zly.h).

A row holds w/2 macropixels of four bytes, two pixels each: YUY2 = Y0 U Y1 V, UYVY = U Y0 V Y1.  Pixel (x, y) takes its own Y and the U, V
of its macropixel (no interpolation between macropixels), then the header's integer conversion (yuv_ref.convert_yuv).  to_bgr() makes the BGR
frame a 4:2:2 frame stands for -- engine(frame) must equal engine(to_bgr(frame)) bit for bit --, from_bgr() makes 4:2:2 inputs from BGR pictures
(a float transform: only its output's content matters), embed() / cut() a pitched surface around a tight frame and a region out of one.  Written
from the header's definition with numpy indexing, independently of the library."""
import numpy as np

import yuv_ref as yr

PIX_YUY2_BT601, PIX_UYVY_BT601, PIX_YUY2_BT709, PIX_UYVY_BT709 = 10, 11, 12, 13
FORMATS = (PIX_YUY2_BT601, PIX_UYVY_BT601, PIX_YUY2_BT709, PIX_UYVY_BT709)
# position of Y0, U, Y1, V inside a macropixel
ORDER = {PIX_YUY2_BT601: (0, 1, 2, 3), PIX_YUY2_BT709: (0, 1, 2, 3), PIX_UYVY_BT601: (1, 0, 3, 2), PIX_UYVY_BT709: (1, 0, 3, 2)}


def matrix(fmt):
    return 709 if fmt in (PIX_YUY2_BT709, PIX_UYVY_BT709) else 601


def samples(buf, w, h, fmt):
    """(Y [h][w], U [h][w/2], V [h][w/2]) of a tight 4:2:2 frame (any shape holding 2*w*h bytes)"""
    buf = np.asarray(buf, dtype=np.uint8).reshape(-1)
    assert w >= 2 and w % 2 == 0 and h >= 1 and buf.size == 2 * w * h
    m = buf.reshape(h, w // 2, 4)
    y0, u, y1, v = (m[:, :, p] for p in ORDER[fmt])
    return np.stack([y0, y1], axis=-1).reshape(h, w), u, v


def pack(y, u, v, fmt):
    """Y [h][w], U, V [h][w/2] -> the tight frame of format fmt (1-D u8)"""
    h, w = y.shape
    m = np.empty((h, w // 2, 4), dtype=np.uint8)
    for a, p in zip((y[:, 0::2], u, y[:, 1::2], v), ORDER[fmt]):
        m[:, :, p] = a
    return np.ascontiguousarray(m.reshape(-1))


def to_bgr(buf, w, h, fmt):
    """tight 4:2:2 frame -> u8 [h][w][3] BGR: pixel (x, y) takes Y[y][x] and the U, V of macropixel x >> 1 of its row"""
    y, u, v = samples(buf, w, h, fmt)
    b, g, r = yr.convert_yuv(y, np.repeat(u, 2, axis=1), np.repeat(v, 2, axis=1), matrix(fmt))
    return np.ascontiguousarray(np.stack([b, g, r], axis=-1))


def from_bgr(bgr, fmt):
    """u8 [h][w][3] BGR (even w) -> tight 4:2:2 frame of format fmt (float limited-range transform, chroma = mean of each pixel pair)"""
    kr, kb = yr.KR_KB[matrix(fmt)]
    kg = 1.0 - kr - kb
    f = np.asarray(bgr, dtype=np.float64)
    b, g, r = f[..., 0], f[..., 1], f[..., 2]
    luma = kr * r + kg * g + kb * b
    y = 16.0 + 219.0 / 255.0 * luma
    cb = 128.0 + 224.0 / 255.0 * (b - luma) / (2.0 * (1.0 - kb))
    cr = 128.0 + 224.0 / 255.0 * (r - luma) / (2.0 * (1.0 - kr))
    h, w = y.shape
    assert w >= 2 and w % 2 == 0
    sub = lambda c: c.reshape(h, w // 2, 2).mean(axis=2)
    q = lambda c: np.clip(np.rint(c), 0, 255).astype(np.uint8)
    return pack(q(y), q(sub(cb)), q(sub(cr)), fmt)


def embed(frame, w, h, pitch, off, tail=0, fill=None, seed=0):
    """a buffer of off + (h-1)*pitch + 2*w + tail bytes holding the tight frame's rows pitch bytes apart from byte off on; every other byte is
    fill (None: random).  -> (buffer, mask of the bytes that belong to the frame)"""
    rows = np.asarray(frame, dtype=np.uint8).reshape(h, 2 * w)
    rb = 2 * w
    assert pitch >= rb
    n = off + (h - 1) * pitch + rb + tail
    buf = np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8) if fill is None else np.full(n, fill, dtype=np.uint8)
    mask = np.zeros(n, dtype=bool)
    for y in range(h):
        buf[off + y * pitch: off + y * pitch + rb] = rows[y]
        mask[off + y * pitch: off + y * pitch + rb] = True
    return buf, mask


def cut(buf, pitch, off, x0, y0, w, h):
    """the tight frame (1-D u8, 2*w*h bytes) of the rectangle (x0, y0, w, h), x0 and w even, of a surface that starts at byte off of buf"""
    assert x0 % 2 == 0 and w % 2 == 0
    buf = np.asarray(buf, dtype=np.uint8).reshape(-1)
    out = np.empty((h, 2 * w), dtype=np.uint8)
    for y in range(h):
        s = off + (y0 + y) * pitch + 2 * x0
        out[y] = buf[s: s + 2 * w]
    return np.ascontiguousarray(out.reshape(-1))


def region_mask(n, pitch, off, x0, y0, w, h):
    """mask over a buffer of n bytes of the bytes that belong to the rectangle"""
    mask = np.zeros(n, dtype=bool)
    for y in range(h):
        s = off + (y0 + y) * pitch + 2 * x0
        mask[s: s + 2 * w] = True
    return mask
