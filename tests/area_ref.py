"""numpy reference of the area-average resize filter (include/zly.h, ZLY_FLAG_AREA), written from the header's text.

axis_weights() is one axis' footprints and weights, area_bgr() the exact (int64) average of a BGR frame at a content size, area_resize() the
model-sized u8 image the pre-pass must produce for a BGR request -- the whole tensor of a stretch engine, the content inside 114 padding of a
letterbox engine --, preprocess_planar() the parity entry point's layout.  It is the exact oracle: an area engine must equal it bit for bit.
Frames of other formats are first converted to BGR by their own references (yuv_ref, yuv422_ref, pixfmt_ref): the header's rule."""
import numpy as np

import letterbox_ref as lb

PAD = lb.PAD
MAX_DIM = 16384
# the (S, D) pairs the CPU tests hold the arithmetic to, beside every pair with S, D <= 12
PAIRS = [(1920, 416), (1080, 416), (16384, 416), (2, 416), (417, 416), (415, 416), (1000, 37)]


def footprint(S, D, d):
    """(i0, i1, w(i0), w(i1)) of content index d: Python ints"""
    lo, hi = d * S, (d + 1) * S
    i0, i1 = lo // D, (hi - 1) // D
    w = lambda i: min(hi, (i + 1) * D) - max(lo, i * D)
    return i0, i1, w(i0), w(i1)


def axis_weights(S, D):
    """the D x S int64 matrix of w(d, i): zero outside a footprint"""
    d = np.arange(D, dtype=np.int64)[:, None]
    i = np.arange(S, dtype=np.int64)[None, :]
    lo, hi = d * S, (d + 1) * S
    return np.maximum(np.minimum(hi, (i + 1) * D) - np.maximum(lo, i * D), 0)


def axis_sums(a, axis, D):
    """int64 array with source length S on `axis` -> the same with length D: out[d] = sum over i of w(d, i) * a[i].
    The weights are overlaps of [d*S, (d+1)*S) with the source pixels' [i*D, (i+1)*D), so the sum is the integral of the step function a over
    the content pixel's interval: F(hi) - F(lo) with F(t) = D * (a[0] + ... + a[t//D - 1]) + (t % D) * a[t//D].  Exact in int64, and linear in S
    where the weight matrix (axis_weights, which tests/test_area_ref.py holds this against) is quadratic."""
    a = np.moveaxis(np.asarray(a, dtype=np.int64), axis, 0)
    S = a.shape[0]
    c = np.concatenate([np.zeros_like(a[:1]), np.cumsum(a, axis=0)])       # c[k] = a[0] + ... + a[k-1]
    t = np.arange(D + 1, dtype=np.int64) * S                               # lo of d = t[d], hi of d = t[d + 1]
    q, r = t // D, t % D
    shape = (-1,) + (1,) * (a.ndim - 1)
    F = D * c[q] + r.reshape(shape) * a[np.minimum(q, S - 1)]              # (t = S*D: q = S, r = 0)
    return np.moveaxis(F[1:] - F[:-1], 0, axis)


def area_bgr(frame, D_w, D_h):
    """u8 [h][w][c] -> u8 [D_h][D_w][c]: acc = sum wy * sum wx * p, v = (acc + (T >> 1)) // T with T = w * h, all in int64"""
    f = np.asarray(frame, dtype=np.int64)
    h, w = f.shape[:2]
    acc = axis_sums(axis_sums(f, 1, D_w), 0, D_h)
    T = w * h
    assert acc.max() < 255 * (1 << 28) + 1 and T <= 1 << 28
    v = (acc + (T >> 1)) // T
    assert v.min() >= 0 and v.max() <= 255
    return v.astype(np.uint8)


def area_resize(frame, tw, th, letterbox):
    """u8 [h][w][3] BGR request -> u8 [th][tw][3]: what the model sees, as bytes (before /255 and BGR->RGB)"""
    frame = np.asarray(frame, dtype=np.uint8)
    h, w = frame.shape[:2]
    if not letterbox:
        return np.ascontiguousarray(area_bgr(frame, tw, th))
    nw, nh, px, py = lb.geometry(w, h, tw, th)
    out = np.full((th, tw, 3), PAD, dtype=np.uint8)
    out[py:py + nh, px:px + nw] = area_bgr(frame, nw, nh)
    return np.ascontiguousarray(out)


def preprocess_planar(frame, tw, th, letterbox):
    """the parity entry point's layout: fp32 [3][th][tw], R, G, B planes, byte / 255 in fp32"""
    a = area_resize(frame, tw, th, letterbox)
    return np.ascontiguousarray(np.stack([a[..., 2], a[..., 1], a[..., 0]]).astype(np.float32) / np.float32(255.0))
