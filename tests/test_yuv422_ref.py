"""Packed YUV 4:2:2 input formats (include/zly.h ZLY_PIX_YUY2_* / ZLY_PIX_UYVY_*), the parts that need no GPU: the constants, the size and view
rules of the library (loaded on the CPU, as tests/test_abi.py does), and the numpy oracle tests/yuv422_ref.py tied to the existing 4:2:0 one."""
import numpy as np
import pytest

import yuv422_ref as y2
import yuv_ref as yr
import zly
import zly_model as zm

FMTS = (zly.PIX_YUY2_BT601, zly.PIX_UYVY_BT601, zly.PIX_YUY2_BT709, zly.PIX_UYVY_BT709)


def _view(fmt, w, h, off, pitch):
    v = zly.FrameView()
    v.fmt, v.w, v.h = fmt, w, h
    v.off[0], v.pitch[0] = off, pitch
    return v


def test_constants():
    assert FMTS == (10, 11, 12, 13) and FMTS == y2.FORMATS


@pytest.mark.parametrize("fmt", FMTS)
def test_frame_bytes(fmt):
    for w, h in [(2, 1), (2, 3), (416, 416), (1920, 1081)]:
        assert zly.frame_bytes(fmt, w, h) == w * h * 2
        t = zly.view_tight(fmt, w, h)
        assert zly.view_bytes(t) == w * h * 2 and t.pitch[0] == 2 * w and t.off[0] == 0
    for w, h in [(3, 2), (417, 416), (1, 1), (0, 4), (-2, 4), (2, 0), (416, -1)]:      # odd w, w < 2, h < 1
        assert zly.frame_bytes(fmt, w, h) == 0, (w, h)
        with pytest.raises(zly.ZlyError) as ei:
            zly.view_tight(fmt, w, h)
        assert ei.value.code == zly.ERR_INVALID_ARGUMENT


def test_values_between_the_families_stay_unknown():
    for fmt in (5, 6, 7, 8, 9, 14, 15):
        assert zly.frame_bytes(fmt, 416, 416) == 0
        assert zly.view_bytes(_view(fmt, 416, 416, 0, 4 * 416)) == 0


@pytest.mark.parametrize("slack", [0, 64, 7])
@pytest.mark.parametrize("fmt", FMTS)
def test_view_crop_matches_numpy_slicing(fmt, slack):
    W, H, off = 64, 37, 13
    pitch = 2 * W + slack
    frame = np.random.default_rng(fmt * 10 + slack).integers(0, 256, 2 * W * H, dtype=np.uint8)
    buf, _ = y2.embed(frame, W, H, pitch, off, seed=3)
    whole = _view(fmt, W, H, off, pitch)
    assert zly.view_bytes(whole) == buf.size
    for x0, y0, w, h in [(0, 0, W, H), (2, 1, 10, 3), (62, 36, 2, 1), (20, 7, 30, 29), (0, 35, 64, 2)]:      # odd y0 and h are fine
        v = zly.view_crop(whole, x0, y0, w, h)
        assert (v.fmt, v.w, v.h, v.pitch[0]) == (fmt, w, h, pitch)
        assert v.off[0] == off + y0 * pitch + x0 * 2
        got = np.concatenate([buf[v.off[0] + y * pitch: v.off[0] + y * pitch + 2 * w] for y in range(h)])
        assert np.array_equal(got, y2.cut(buf, pitch, off, x0, y0, w, h))
        assert np.array_equal(y2.to_bgr(got, w, h, fmt), y2.to_bgr(frame, W, H, fmt)[y0:y0 + h, x0:x0 + w])
        assert zly.view_bytes(v) == v.off[0] + (h - 1) * pitch + 2 * w <= buf.size
    # crops compose
    a = zly.view_crop(zly.view_crop(whole, 4, 3, 40, 20), 6, 5, 10, 11)
    b = zly.view_crop(whole, 10, 8, 10, 11)
    assert (a.off[0], a.w, a.h, a.pitch[0]) == (b.off[0], b.w, b.h, b.pitch[0])
    for x0, y0, w, h in [(1, 0, 10, 3), (2, 0, 9, 3), (3, 1, 5, 5), (0, 0, W + 2, 2), (0, 30, 2, 8)]:       # odd x0 / w; outside the surface
        with pytest.raises(zly.ZlyError) as ei:
            zly.view_crop(whole, x0, y0, w, h)
        assert ei.value.code == zly.ERR_INVALID_ARGUMENT, (x0, y0, w, h)


@pytest.mark.parametrize("fmt", FMTS)
def test_view_validity(fmt):
    assert zly.view_bytes(_view(fmt, 64, 5, 3, 128)) == 3 + 4 * 128 + 128
    assert zly.view_bytes(_view(fmt, 64, 5, 3, 127)) == 0                       # pitch < 2 * w
    assert zly.view_bytes(_view(fmt, 63, 5, 0, 128)) == 0                       # odd w
    assert zly.view_bytes(_view(fmt, 0, 5, 0, 128)) == 0
    assert zly.view_bytes(_view(fmt, 64, 0, 0, 128)) == 0
    assert zly.view_bytes(_view(fmt, 2, 1, 5, 4)) == 9                          # the smallest frame, at an odd address
    big = 1 << 20
    assert zly.view_bytes(_view(fmt, 2, 2048, 0, big)) == 2047 * big + 4        # extent just below 2^31 ...
    assert zly.view_bytes(_view(fmt, 2, 2049, 0, big)) == 0                     # ... and at it


@pytest.mark.parametrize("mat", [601, 709])
def test_oracle_agrees_with_the_420_oracle_where_chroma_rows_are_pairwise_equal(mat):
    """a 4:2:2 frame whose chroma rows 2k and 2k + 1 are equal holds exactly the samples of an I420 frame: both oracles must convert them alike"""
    w, h = 66, 38
    rng = np.random.default_rng(mat)
    y = rng.integers(0, 256, (h, w), dtype=np.uint8)
    u = rng.integers(0, 256, (h // 2, w // 2), dtype=np.uint8)
    v = rng.integers(0, 256, (h // 2, w // 2), dtype=np.uint8)
    i420 = yr.PIX_I420_BT601 if mat == 601 else yr.PIX_I420_BT709
    want = yr.yuv420_to_bgr(yr.pack(y, u, v, i420), w, h, i420)
    for fmt in (f for f in FMTS if y2.matrix(f) == mat):
        frame = y2.pack(y, np.repeat(u, 2, axis=0), np.repeat(v, 2, axis=0), fmt)
        assert frame.size == zly.frame_bytes(fmt, w, h)
        assert np.array_equal(y2.to_bgr(frame, w, h, fmt), want)


def test_swapping_the_bytes_of_every_pair_turns_yuy2_into_uyvy():
    w, h = 34, 5
    frame = np.random.default_rng(1).integers(0, 256, 2 * w * h, dtype=np.uint8)
    swapped = np.ascontiguousarray(frame.reshape(-1, 2)[:, ::-1]).reshape(-1)
    assert not np.array_equal(frame, swapped)
    for yuy2, uyvy in [(zly.PIX_YUY2_BT601, zly.PIX_UYVY_BT601), (zly.PIX_YUY2_BT709, zly.PIX_UYVY_BT709)]:
        assert np.array_equal(y2.to_bgr(frame, w, h, yuy2), y2.to_bgr(swapped, w, h, uyvy))
        ya, ua, va = y2.samples(frame, w, h, yuy2)
        yb, ub, vb = y2.samples(swapped, w, h, uyvy)
        assert np.array_equal(ya, yb) and np.array_equal(ua, ub) and np.array_equal(va, vb)
    assert not np.array_equal(y2.to_bgr(frame, w, h, zly.PIX_YUY2_BT601), y2.to_bgr(frame, w, h, zly.PIX_YUY2_BT709))


def test_chroma_comes_from_the_pixels_own_macropixel():
    w, h = 8, 3
    y = np.full((h, w), 128, np.uint8)
    u = (np.arange(12, dtype=np.uint8).reshape(3, 4) * 20)
    v = 255 - u
    for fmt in FMTS:
        out = y2.to_bgr(y2.pack(y, u, v, fmt), w, h, fmt)
        for r in range(h):
            for m in range(w // 2):
                b, g, rr = yr.convert_yuv(np.array([128]), np.array([u[r, m]]), np.array([v[r, m]]), y2.matrix(fmt))
                assert tuple(out[r, 2 * m]) == tuple(out[r, 2 * m + 1]) == (b[0], g[0], rr[0])


@pytest.mark.parametrize("fmt", FMTS)
def test_round_trip_stays_close_to_the_picture(fmt):
    """the bound tests/test_yuv_ref.py holds the 4:2:0 round trip to, on the same flat picture (the forward transform is only a test-input generator)"""
    back = y2.to_bgr(y2.from_bgr(np.full((4, 4, 3), 100, np.uint8), fmt), 4, 4, fmt)
    assert np.abs(back.astype(int) - 100).max() <= 2
    pic = zm.synth_frames(1, 66, 37, seed=3)[0]
    f = y2.from_bgr(pic, fmt)
    assert f.size == 2 * 66 * 37 and f.dtype == np.uint8
