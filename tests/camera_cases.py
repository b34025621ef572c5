"""Shared case builders of the camera motion's tests (tests/test_camera_ref.py and tests/test_camera_rules.py on the CPU, tests/test_gpu_camera.py on
the GPU): a seeded texture CANVAS -- block noise plus 40 random rectangles -- from which frames are cut at offsets that differ by a known shift, and
the frames of a pan as tight buffers of a pixel format with the BGR image the format's rules give them."""
import numpy as np

import chip_cases as cc
import chip_ref
import yuv422_ref
import yuv_ref

BGR, BGRA, NV12, I420, YUY2 = 0, 17, 1, 4, 10           # ZLY_PIX_BGR, _BGRA, _NV12_BT601, _I420_BT709, _YUY2_BT601
FORMATS = (BGR, BGRA, NV12, I420, YUY2)


def canvas(W, H, margin, block=1, seed=0):
    """a (H + 2*margin) x (W + 2*margin) BGR picture: noise in blocks of block x block pixels, then 40 rectangles of random place, size and colour"""
    rng = np.random.default_rng(seed)
    ch, cw = H + 2 * margin, W + 2 * margin
    nb = rng.integers(0, 256, (-(-ch // block), -(-cw // block), 3), dtype=np.uint8)
    pic = np.repeat(np.repeat(nb, block, axis=0), block, axis=1)[:ch, :cw].copy()
    for _ in range(40):
        rh, rw = int(rng.integers(4, max(ch // 4, 5))), int(rng.integers(4, max(cw // 4, 5)))
        y, x = int(rng.integers(0, ch - rh + 1)), int(rng.integers(0, cw - rw + 1))
        pic[y:y + rh, x:x + rw] = rng.integers(0, 256, 3, dtype=np.uint8)
    return pic


def cut(pic, W, H, margin, X, Y):
    """the W x H frame in which the canvas's content stands displaced by (X, Y) pixels against the frame cut at (0, 0); |X|, |Y| <= margin"""
    assert abs(X) <= margin and abs(Y) <= margin
    return np.ascontiguousarray(pic[margin - Y:margin - Y + H, margin - X:margin - X + W])


def pan(W, H, shifts, block=1, seed=0):
    """frames of a pan: frame 0 at rest, frame k displaced by shifts[k-1] against frame k-1 -> [BGR image] * (len(shifts) + 1)"""
    X = np.concatenate([[0], np.cumsum([s[0] for s in shifts])]).astype(int)
    Y = np.concatenate([[0], np.cumsum([s[1] for s in shifts])]).astype(int)
    margin = int(max(np.abs(X).max(), np.abs(Y).max(), 1))
    pic = canvas(W, H, margin, block, seed)
    return [cut(pic, W, H, margin, int(x), int(y)) for x, y in zip(X, Y)]


def as_format(fmt, bgr):
    """a BGR picture (of a size legal for the format) as a tight frame of the format -> (flat u8 frame, the BGR image the format's rules give it)"""
    h, w = bgr.shape[:2]
    assert cc.legal(fmt, w, h) == (w, h)
    if fmt == BGR:
        f = np.ascontiguousarray(bgr).reshape(-1)
    elif fmt == BGRA:
        f = np.ascontiguousarray(np.concatenate([bgr, np.full((h, w, 1), 0x3C, np.uint8)], axis=2)).reshape(-1)
    elif fmt in cc.F420:
        f = np.ascontiguousarray(yuv_ref.bgr_to_yuv420(bgr, fmt)).reshape(-1)
    else:
        f = np.ascontiguousarray(yuv422_ref.from_bgr(bgr, fmt)).reshape(-1)
    img = chip_ref.bgr_of(fmt, f if fmt not in cc.FPK else f.reshape(h, w, cc.pr.BPP[fmt]), w, h)
    return f, np.ascontiguousarray(img)


def gray(w, h, value=0):
    """a constant BGR image: its luma is `value`"""
    return np.full((h, w, 3), value, dtype=np.uint8)
