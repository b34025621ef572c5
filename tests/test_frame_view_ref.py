"""Frame views on the host (include/zly.h zly_frame_view): zly_view_tight / zly_view_crop / zly_view_bytes against tests/view_ref.py's numpy
slicing, for BGR, NV12 and I420, tight and padded pitches, crops at the origin, in the interior and flush against the bottom-right corner,
composed crops, and every invalid case with its code.  No engine, no GPU."""
import ctypes as C

import numpy as np
import pytest

import view_ref as vr
import zly

FMTS = (zly.PIX_BGR, zly.PIX_NV12_BT601, zly.PIX_I420_BT601, zly.PIX_NV12_BT709, zly.PIX_I420_BT709)
PITCH_KINDS = (0, 1, 64)             # tight, tight + 1 (odd), tight + 64
SURF_W, SURF_H = 64, 48


def _surface(fmt, extra):
    """(buffer of distinct bytes, numpy view, C view) of a SURF_W x SURF_H surface whose pitches are tight + extra"""
    pitches = [p + extra for p in vr.tight_pitches(fmt, SURF_W)]
    s = vr.surface(fmt, SURF_W, SURF_H, pitches)
    total = sum(rows * p for (rows, _), p in zip(vr.plane_shapes(fmt, SURF_W, SURF_H), pitches))
    buf = (np.arange(total, dtype=np.uint64) * 2654435761 >> 7).astype(np.uint8)
    return buf, s, vr.to_c(s)


def _tight_frame_of(buf, s):
    """the whole surface as its tight frame"""
    return vr.extract(buf, s)


def _slice_frame(frame, fmt, W, H, x0, y0, w, h):
    """numpy slicing of a tight W x H frame: its (x0, y0, w, h) rectangle as a tight frame"""
    if fmt == zly.PIX_BGR:
        return np.ascontiguousarray(frame.reshape(H, W, 3)[y0:y0 + h, x0:x0 + w])
    y = frame[:W * H].reshape(H, W)[y0:y0 + h, x0:x0 + w]
    c = frame[W * H:]
    if vr.is_nv12(fmt):
        uv = c.reshape(H // 2, W // 2, 2)[y0 // 2:(y0 + h) // 2, x0 // 2:(x0 + w) // 2]
        return np.concatenate([y.reshape(-1), uv.reshape(-1)])
    q = (W // 2) * (H // 2)
    u = c[:q].reshape(H // 2, W // 2)[y0 // 2:(y0 + h) // 2, x0 // 2:(x0 + w) // 2]
    v = c[q:].reshape(H // 2, W // 2)[y0 // 2:(y0 + h) // 2, x0 // 2:(x0 + w) // 2]
    return np.concatenate([y.reshape(-1), u.reshape(-1), v.reshape(-1)])


def test_frame_view_struct_layout():
    assert C.sizeof(zly.FrameView) == 56
    assert zly.FrameView.off.offset == 16 and zly.FrameView.pitch.offset == 40


@pytest.mark.parametrize("fmt", FMTS)
def test_view_tight_is_the_tight_frame(fmt):
    for w, h in ((416, 416), (2, 2), (100, 62), (1920, 1080)):
        c = zly.view_tight(fmt, w, h)
        assert vr.from_c(c) == vr.surface(fmt, w, h)
        assert zly.view_bytes(c) == zly.frame_bytes(fmt, w, h) == vr.nbytes(vr.surface(fmt, w, h))
    if fmt == zly.PIX_BGR:
        assert zly.view_bytes(zly.view_tight(fmt, 1, 1)) == 3
        assert zly.view_bytes(zly.view_tight(fmt, 417, 3)) == 417 * 3 * 3


@pytest.mark.parametrize("extra", PITCH_KINDS)
@pytest.mark.parametrize("fmt", FMTS)
def test_crop_and_bytes_equal_numpy_slicing(fmt, extra):
    buf, s, cs = _surface(fmt, extra)
    assert zly.view_bytes(cs) == vr.nbytes(s) <= buf.size
    whole = _tight_frame_of(buf, s)
    rects = [(0, 0, 16, 12),                               # at the origin
             (10, 6, 30, 20),                              # interior
             (SURF_W - 22, SURF_H - 14, 22, 14),           # flush against the bottom-right corner
             (0, 0, SURF_W, SURF_H)]                       # the whole surface
    if fmt == zly.PIX_BGR:
        rects += [(7, 5, 9, 3), (SURF_W - 1, SURF_H - 1, 1, 1)]      # BGR has no parity rule
    for x0, y0, w, h in rects:
        cc = zly.view_crop(cs, x0, y0, w, h)
        want = vr.crop(s, x0, y0, w, h)
        assert vr.from_c(cc) == want, (x0, y0, w, h)
        assert zly.view_bytes(cc) == vr.nbytes(want) <= buf.size
        got = vr.extract(buf, vr.from_c(cc))
        assert np.array_equal(got.reshape(-1), _slice_frame(whole, fmt, SURF_W, SURF_H, x0, y0, w, h).reshape(-1)), (x0, y0, w, h)
    # the corner crop ends exactly where the surface's samples end: not one byte of row padding behind the last row is needed
    last = zly.view_crop(cs, SURF_W - 22, SURF_H - 14, 22, 14)
    assert zly.view_bytes(last) == zly.view_bytes(cs)


@pytest.mark.parametrize("fmt", FMTS)
def test_crops_compose(fmt):
    buf, s, cs = _surface(fmt, 64)
    a = zly.view_crop(cs, 8, 4, 40, 30)
    b = zly.view_crop(a, 6, 10, 20, 12)
    assert vr.from_c(b) == vr.from_c(zly.view_crop(cs, 14, 14, 20, 12)) == vr.crop(vr.crop(s, 8, 4, 40, 30), 6, 10, 20, 12)
    # in place: out may be the surface itself
    lib = zly.load_library()
    assert lib.zly_view_crop(C.byref(a), 6, 10, 20, 12, C.byref(a)) == zly.OK
    assert vr.from_c(a) == vr.from_c(b)


def _view(fmt, w, h, off=(0, 0, 0), pitch=(0, 0, 0)):
    c = zly.FrameView()
    c.fmt, c.w, c.h = fmt, w, h
    for p in range(3):
        c.off[p], c.pitch[p] = off[p], pitch[p]
    return c


def test_invalid_views_have_zero_bytes():
    B, N, I = zly.PIX_BGR, zly.PIX_NV12_BT601, zly.PIX_I420_BT709
    lib = zly.load_library()
    assert lib.zly_view_bytes(None) == 0
    bad = [_view(9, 16, 16, pitch=(48, 16, 16)),                 # unknown format
           _view(-1, 16, 16, pitch=(48, 16, 16)),
           _view(B, 0, 16, pitch=(48, 0, 0)),                    # w, h >= 1
           _view(B, 16, 0, pitch=(48, 0, 0)),
           _view(B, 16, 16, pitch=(47, 0, 0)),                   # pitch below the row's bytes
           _view(B, 16, 16, pitch=(-48, 0, 0)),                  # negative pitch
           _view(N, 15, 16, pitch=(16, 16, 0)),                  # YUV: even
           _view(N, 16, 15, pitch=(16, 16, 0)),
           _view(I, 0, 0, pitch=(16, 8, 8)),
           _view(N, 16, 16, pitch=(16, 15, 0)),                  # UV row is 2 * (w/2) bytes
           _view(I, 16, 16, pitch=(16, 8, 7)),                   # V row is w/2 bytes
           _view(I, 16, 16, pitch=(15, 8, 8)),
           _view(B, 16, 1 << 20, pitch=(1 << 12, 0, 0)),         # extent 2^32: not below 2^31
           _view(B, 1, 2, pitch=((1 << 31) - 3, 0, 0)),          # extent exactly 2^31
           _view(N, 16, 4, pitch=(16, (1 << 31) - 16, 0))]       # the UV plane's extent is 2^31
    for v in bad:
        assert zly.view_bytes(v) == 0, (v.fmt, v.w, v.h, list(v.pitch))
    # the largest valid extent, and planes that a format does not have are ignored
    assert zly.view_bytes(_view(B, 1, 2, pitch=((1 << 31) - 4, 0, 0))) == (1 << 31) - 1
    assert zly.view_bytes(_view(B, 16, 16, off=(5, 1 << 40, 1 << 50), pitch=(48, -1, -1))) == 5 + 16 * 48
    assert zly.view_bytes(_view(N, 16, 16, off=(0, 1000, 1 << 50), pitch=(16, 16, -1))) == 1000 + 8 * 16
    # offsets count: the maximum over the used planes
    assert zly.view_bytes(_view(I, 16, 16, off=(700, 0, 300), pitch=(20, 9, 8))) == max(700 + 15 * 20 + 16, 7 * 9 + 8, 300 + 7 * 8 + 8)


def test_view_tight_and_crop_errors():
    lib = zly.load_library()
    out = zly.FrameView()
    E = zly.ERR_INVALID_ARGUMENT
    for fmt, w, h in ((9, 16, 16), (zly.PIX_BGR, 0, 4), (zly.PIX_BGR, 4, -1), (zly.PIX_NV12_BT601, 15, 16), (zly.PIX_I420_BT601, 16, 2 + 1), (zly.PIX_NV12_BT709, 0, 0)):
        assert lib.zly_view_tight(fmt, w, h, C.byref(out)) == E, (fmt, w, h)
    assert lib.zly_view_tight(zly.PIX_BGR, 4, 4, None) == E
    s = zly.view_tight(zly.PIX_BGR, 64, 48)
    for x0, y0, w, h in ((-1, 0, 4, 4), (0, -2, 4, 4), (0, 0, 0, 4), (0, 0, 4, 0), (61, 0, 4, 4), (0, 45, 4, 4), (0, 0, 65, 48), (64, 0, 1, 1),
                         (2 ** 31 - 1, 0, 2, 2)):
        assert lib.zly_view_crop(C.byref(s), x0, y0, w, h, C.byref(out)) == E, (x0, y0, w, h)
    assert lib.zly_view_crop(None, 0, 0, 4, 4, C.byref(out)) == E and lib.zly_view_crop(C.byref(s), 0, 0, 4, 4, None) == E
    for fmt in (zly.PIX_NV12_BT601, zly.PIX_I420_BT709):
        y = zly.view_tight(fmt, 64, 48)
        for x0, y0, w, h in ((1, 0, 4, 4), (0, 1, 4, 4), (0, 0, 3, 4), (0, 0, 4, 5), (62, 0, 4, 4)):
            assert lib.zly_view_crop(C.byref(y), x0, y0, w, h, C.byref(out)) == E, (fmt, x0, y0, w, h)
        assert lib.zly_view_crop(C.byref(y), 2, 4, 8, 6, C.byref(out)) == zly.OK
    invalid = _view(zly.PIX_BGR, 16, 16, pitch=(47, 0, 0))
    assert lib.zly_view_crop(C.byref(invalid), 0, 0, 4, 4, C.byref(out)) == E
    with pytest.raises(zly.ZlyError):
        zly.view_crop(s, 0, 0, 65, 48)


def test_embed_and_extract_round_trip():
    rng = np.random.default_rng(3)
    for fmt in FMTS:
        w, h = 20, 12
        frame = rng.integers(0, 256, (h, w, 3), dtype=np.uint8) if fmt == zly.PIX_BGR else rng.integers(0, 256, w * h * 3 // 2, dtype=np.uint8)
        for extra in PITCH_KINDS:
            pitches = [p + extra for p in vr.tight_pitches(fmt, SURF_W)]
            for fill in (0, 255):
                buf, v = vr.embed(frame, fmt, SURF_W, SURF_H, pitches, 30, 20, fill, w=w, h=h)
                assert np.array_equal(vr.extract(buf, v), frame)
                assert vr.from_c(zly.view_crop(vr.to_c(vr.surface(fmt, SURF_W, SURF_H, pitches)), 30, 20, w, h)) == v
                assert int((buf != fill).sum()) <= frame.size
