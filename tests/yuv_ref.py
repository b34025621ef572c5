"""numpy reference of the YUV 4:2:0 input formats (include/zly.h, ZLY_PIX_*).

yuv420_to_bgr is the engine's integer conversion written out literally: every pixel of a YUV frame becomes the B, G, R bytes the
front kernels compute for it, so that engine(yuv) must equal engine(yuv420_to_bgr(yuv)) bit for bit.  bgr_to_yuv420 makes YUV
inputs from the synthetic BGR frames (a float transform: only its output's content matters, not its exactness)."""
import numpy as np

PIX_BGR, PIX_NV12_BT601, PIX_I420_BT601, PIX_NV12_BT709, PIX_I420_BT709 = 0, 1, 2, 3, 4
YUV_FORMATS = (PIX_NV12_BT601, PIX_I420_BT601, PIX_NV12_BT709, PIX_I420_BT709)

# (CY, CVR, CVG, CUG, CUB), 20 fractional bits
COEFFS = {601: (1220542, 1673527, -852492, -409993, 2116026),
          709: (1220945, 1879825, -558796, -223607, 2215014)}
KR_KB = {601: (0.299, 0.114), 709: (0.2126, 0.0722)}


def is_nv12(fmt):
    return fmt in (PIX_NV12_BT601, PIX_NV12_BT709)


def matrix(fmt):
    return 709 if fmt in (PIX_NV12_BT709, PIX_I420_BT709) else 601


def convert_yuv(y, u, v, mat):
    """integer Y, U, V arrays (any shape) -> (B, G, R) uint8 arrays: the formula of include/zly.h"""
    cy, cvr, cvg, cug, cub = COEFFS[mat]
    yy = np.maximum(np.asarray(y, np.int64) - 16, 0) * cy
    u = np.asarray(u, np.int64) - 128
    v = np.asarray(v, np.int64) - 128
    r = np.clip((yy + cvr * v + (1 << 19)) >> 20, 0, 255)
    g = np.clip((yy + cvg * v + cug * u + (1 << 19)) >> 20, 0, 255)
    b = np.clip((yy + cub * u + (1 << 19)) >> 20, 0, 255)
    return b.astype(np.uint8), g.astype(np.uint8), r.astype(np.uint8)


def planes(buf, w, h, fmt):
    """(Y [h][w], U [h/2][w/2], V [h/2][w/2]) of a packed NV12 / I420 buffer"""
    buf = np.asarray(buf, dtype=np.uint8).reshape(-1)
    assert w % 2 == 0 and h % 2 == 0 and buf.size == w * h * 3 // 2
    y = buf[:w * h].reshape(h, w)
    c = buf[w * h:]
    if is_nv12(fmt):
        uv = c.reshape(h // 2, w // 2, 2)
        return y, uv[..., 0], uv[..., 1]
    q = (w // 2) * (h // 2)
    return y, c[:q].reshape(h // 2, w // 2), c[q:].reshape(h // 2, w // 2)


def yuv420_to_bgr(buf, w, h, fmt):
    """packed YUV 4:2:0 frame -> u8 [h][w][3] BGR: pixel (x, y) takes Y[y][x] and the chroma sample of its 2 x 2 block"""
    y, u, v = planes(buf, w, h, fmt)
    uu = np.repeat(np.repeat(u, 2, axis=0), 2, axis=1)
    vv = np.repeat(np.repeat(v, 2, axis=0), 2, axis=1)
    b, g, r = convert_yuv(y, uu, vv, matrix(fmt))
    return np.ascontiguousarray(np.stack([b, g, r], axis=-1))


def pack(y, u, v, fmt):
    """Y [h][w], U, V [h/2][w/2] -> the packed buffer of format fmt (1-D u8)"""
    if is_nv12(fmt):
        c = np.stack([u, v], axis=-1).reshape(-1)
    else:
        c = np.concatenate([u.reshape(-1), v.reshape(-1)])
    return np.ascontiguousarray(np.concatenate([y.reshape(-1), c]).astype(np.uint8))


def bgr_to_yuv420(bgr, fmt):
    """u8 [h][w][3] BGR (even w, h) -> packed YUV 4:2:0 of format fmt (float limited-range transform, chroma = mean of each 2 x 2 block)"""
    kr, kb = KR_KB[matrix(fmt)]
    kg = 1.0 - kr - kb
    f = np.asarray(bgr, dtype=np.float64)
    b, g, r = f[..., 0], f[..., 1], f[..., 2]
    luma = kr * r + kg * g + kb * b
    y = 16.0 + 219.0 / 255.0 * luma
    cb = 128.0 + 224.0 / 255.0 * (b - luma) / (2.0 * (1.0 - kb))
    cr = 128.0 + 224.0 / 255.0 * (r - luma) / (2.0 * (1.0 - kr))
    h, w = y.shape
    sub = lambda c: c.reshape(h // 2, 2, w // 2, 2).mean(axis=(1, 3))
    q = lambda c: np.clip(np.rint(c), 0, 255).astype(np.uint8)
    return pack(q(y), q(sub(cb)), q(sub(cr)), fmt)


def float_reference(y, u, v, mat):
    """independent float conversion from Kr / Kb (luma x 255/219, chroma x 255/224; luma below 16 counts as 16, as in the
    integer formula) -> float R, G, B before rounding / clamping"""
    kr, kb = KR_KB[mat]
    kg = 1.0 - kr - kb
    ys = 255.0 / 219.0 * np.maximum(np.asarray(y, np.float64) - 16.0, 0.0)
    cs = 255.0 / 224.0
    u = (np.asarray(u, np.float64) - 128.0) * cs
    v = (np.asarray(v, np.float64) - 128.0) * cs
    r = ys + 2.0 * (1.0 - kr) * v
    b = ys + 2.0 * (1.0 - kb) * u
    g = ys - (2.0 * (1.0 - kb) * kb / kg) * u - (2.0 * (1.0 - kr) * kr / kg) * v
    return r, g, b
