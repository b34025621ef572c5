"""numpy reference of the packed pixel formats ZLY_PIX_RGB / ZLY_PIX_BGRA / ZLY_PIX_RGBA (include/zly.h).

The rule they follow: a frame of one of these formats gives, bit for bit, what the BGR frame made of its B, G, R bytes gives.  to_bgr() makes
that BGR frame, from_bgr() the inverse (with a chosen fourth byte), embed() a pitched surface around a tight frame.  Written from the header's
definition with numpy indexing, independently of the library."""
import numpy as np

PIX_BGR, PIX_RGB, PIX_BGRA, PIX_RGBA = 0, 16, 17, 18
PACKED = (PIX_RGB, PIX_BGRA, PIX_RGBA)
BPP = {PIX_BGR: 3, PIX_RGB: 3, PIX_BGRA: 4, PIX_RGBA: 4}
# position of B, G, R inside a pixel
ORDER = {PIX_BGR: (0, 1, 2), PIX_RGB: (2, 1, 0), PIX_BGRA: (0, 1, 2), PIX_RGBA: (2, 1, 0)}


def to_bgr(frame, w, h, fmt):
    """u8 [h][w][3] BGR frame made of the B, G, R bytes of a packed frame (any shape holding h*w*bpp bytes)"""
    px = np.asarray(frame, dtype=np.uint8).reshape(h, w, BPP[fmt])
    return np.ascontiguousarray(px[:, :, list(ORDER[fmt])])


def from_bgr(bgr, fmt, x=0):
    """u8 [h][w][bpp] frame of format fmt whose B, G, R bytes are bgr's; x: the fourth byte of BGRA / RGBA, a scalar or an [h][w] array"""
    bgr = np.asarray(bgr, dtype=np.uint8)
    h, w = bgr.shape[:2]
    out = np.empty((h, w, BPP[fmt]), dtype=np.uint8)
    for c, pos in enumerate(ORDER[fmt]):
        out[:, :, pos] = bgr[:, :, c]
    if BPP[fmt] == 4:
        out[:, :, 3] = x
    return out


def embed(frame, fmt, pitch, off, tail=0, fill=None, seed=0):
    """a buffer of off + (h-1)*pitch + bpp*w + tail bytes holding the tight frame's rows pitch bytes apart from byte off on; every other byte is
    fill (None: random).  -> (buffer, mask of the bytes that belong to the frame)"""
    frame = np.asarray(frame, dtype=np.uint8)
    h, w = frame.shape[:2]
    rb = BPP[fmt] * w
    assert pitch >= rb
    n = off + (h - 1) * pitch + rb + tail
    buf = np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8) if fill is None else np.full(n, fill, dtype=np.uint8)
    mask = np.zeros(n, dtype=bool)
    rows = frame.reshape(h, rb)
    for y in range(h):
        buf[off + y * pitch: off + y * pitch + rb] = rows[y]
        mask[off + y * pitch: off + y * pitch + rb] = True
    return buf, mask


def cut(buf, fmt, pitch, off, x0, y0, w, h):
    """the tight [h][w][bpp] frame of the rectangle (x0, y0, w, h) of a surface that starts at byte off of buf with the given pitch"""
    bpp = BPP[fmt]
    buf = np.asarray(buf, dtype=np.uint8).reshape(-1)
    out = np.empty((h, w, bpp), dtype=np.uint8)
    for y in range(h):
        s = off + (y0 + y) * pitch + x0 * bpp
        out[y] = buf[s: s + w * bpp].reshape(w, bpp)
    return out
