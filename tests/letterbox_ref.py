"""numpy reference of the letterbox resize mode (include/zly.h, ZLY_FLAG_LETTERBOX), written from the header's text.

geometry() is the integer content size and padding, letterbox_bgr() the model-sized u8 image the front kernels must produce for a BGR
request (114 padding, 16.16 fixed-point bilinear taps with 8-bit weights, all in int32 range), map_boxes() the box mapping of the
decode.  It is the exact oracle: a letterbox engine must equal it bit for bit.  float_bilinear() is an independent float64 half-pixel
bilinear of the same geometry, for the error bound of the fixed-point scheme."""
import numpy as np

PAD = 114
MAX_DIM = 16384


def geometry(w, h, tw, th):
    """(nw, nh, pad_x, pad_y) -- Python ints are unbounded: the header's 64-bit products"""
    w, h, tw, th = int(w), int(h), int(tw), int(th)
    if tw * h <= th * w:
        nw, nh = tw, max(1, (2 * h * tw + w) // (2 * w))
    else:
        nh, nw = th, max(1, (2 * w * th + h) // (2 * h))
    return nw, nh, (tw - nw) >> 1, (th - nh) >> 1


def axis_taps(S, D, track=None):
    """per content index d of an axis with source length S and content length D: (i0, i1, a) as int64 arrays.
    track: a list that receives the largest magnitude of every intermediate (the int32 claim)"""
    step = ((S << 16) + (D >> 1)) // D
    d = np.arange(D, dtype=np.int64)
    raw = d * step + (step >> 1) - 32768
    s = np.clip(raw, 0, (S - 1) << 16)
    if track is not None:
        track += [step, int(np.abs(d * step).max()), int(np.abs(d * step + (step >> 1)).max()), int(np.abs(raw).max()), (S << 16) + (D >> 1)]
    i0 = s >> 16
    return i0, np.minimum(i0 + 1, S - 1), (s >> 8) & 255


def resize_bgr(frame, nw, nh, track=None):
    """u8 [h][w][3] -> u8 [nh][nw][3]: the header's sampling"""
    f = np.asarray(frame, dtype=np.int64)
    h, w = f.shape[:2]
    x0, x1, ax = axis_taps(w, nw, track)
    y0, y1, ay = axis_taps(h, nh, track)
    ax = ax[None, :, None]
    ay = ay[:, None, None]
    p00, p01 = f[y0][:, x0], f[y0][:, x1]
    p10, p11 = f[y1][:, x0], f[y1][:, x1]
    acc = p00 * (256 - ax) * (256 - ay) + p01 * ax * (256 - ay) + p10 * (256 - ax) * ay + p11 * ax * ay + 32768
    if track is not None:
        track.append(int(acc.max()))
    v = acc >> 16
    assert v.min() >= 0 and v.max() <= 255
    return v.astype(np.uint8)


def letterbox_bgr(frame, tw, th, track=None):
    """u8 [h][w][3] BGR request -> u8 [th][tw][3]: what the model sees, as bytes (before /255 and BGR->RGB)"""
    frame = np.asarray(frame, dtype=np.uint8)
    h, w = frame.shape[:2]
    nw, nh, px, py = geometry(w, h, tw, th)
    out = np.full((th, tw, 3), PAD, dtype=np.uint8)
    out[py:py + nh, px:px + nw] = resize_bgr(frame, nw, nh, track)
    return np.ascontiguousarray(out)


def preprocess_planar(frame, tw, th):
    """the parity entry point's layout: fp32 [3][th][tw], R, G, B planes, byte / 255 in fp32"""
    lb = letterbox_bgr(frame, tw, th)
    return np.ascontiguousarray(np.stack([lb[..., 2], lb[..., 1], lb[..., 0]]).astype(np.float32) / np.float32(255.0))


def map_boxes(cx, cy, bw, bh, w, h, tw, th):
    """head boxes (model pixels, fp32) -> normalised boxes of the w x h request: single fp32 operations in the decode's order"""
    nw, nh, px, py = geometry(w, h, tw, th)
    f = np.float32
    cx, cy, bw, bh = (np.asarray(v, dtype=np.float32) for v in (cx, cy, bw, bh))
    return (cx - f(px)) / f(nw), (cy - f(py)) / f(nh), bw / f(nw), bh / f(nh)


def unpad_head(head, w, h, tw, th):
    """a head tensor [4+nc][N] with pad_x / pad_y subtracted from rows 0 / 1 in fp32: fed to the stretch oracle's post-processing with
    (nw, nh) as the image size, it performs exactly map_boxes' operations"""
    nw, nh, px, py = geometry(w, h, tw, th)
    out = np.array(head, dtype=np.float32, copy=True)
    out[0] = out[0] - np.float32(px)
    out[1] = out[1] - np.float32(py)
    return out, nw, nh


def float_bilinear(frame, nw, nh):
    """float64 half-pixel-centre bilinear resize (edge-clamped) of u8 [h][w][3] to [nh][nw][3], unrounded"""
    f = np.asarray(frame, dtype=np.float64)
    h, w = f.shape[:2]

    def axis(S, D):
        c = (np.arange(D, dtype=np.float64) + 0.5) * (S / D) - 0.5
        c = np.clip(c, 0.0, S - 1.0)
        i0 = np.floor(c).astype(np.int64)
        return i0, np.minimum(i0 + 1, S - 1), c - i0

    x0, x1, fx = axis(w, nw)
    y0, y1, fy = axis(h, nh)
    fx = fx[None, :, None]
    fy = fy[:, None, None]
    top = f[y0][:, x0] * (1 - fx) + f[y0][:, x1] * fx
    bot = f[y1][:, x0] * (1 - fx) + f[y1][:, x1] * fx
    return top * (1 - fy) + bot * fy
