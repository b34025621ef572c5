"""The packed pixel formats ZLY_PIX_RGB / ZLY_PIX_BGRA / ZLY_PIX_RGBA on the host (no GPU): frame sizes, views of surfaces of 3- and 4-byte
pixels against numpy slicing, and the numpy reference's own round trip (tests/pixfmt_ref.py)."""
import numpy as np
import pytest

import pixfmt_ref as pr
import zly

FMTS = (zly.PIX_RGB, zly.PIX_BGRA, zly.PIX_RGBA)
BPP = {zly.PIX_RGB: 3, zly.PIX_BGRA: 4, zly.PIX_RGBA: 4}


def test_constants_match_the_reference_module():
    assert (zly.PIX_RGB, zly.PIX_BGRA, zly.PIX_RGBA) == (16, 17, 18) == pr.PACKED
    assert BPP == {f: pr.BPP[f] for f in FMTS}


def test_frame_bytes():
    for fmt in FMTS:
        for w, h in ((1, 1), (3, 5), (416, 416)):
            assert zly.frame_bytes(fmt, w, h) == w * h * BPP[fmt], (fmt, w, h)
        for w, h in ((0, 4), (4, 0), (-1, 4), (4, -3), (0, 0)):
            assert zly.frame_bytes(fmt, w, h) == 0, (fmt, w, h)
    for fmt in (5, 7, 9, 15, 19, -1):                        # between the YUV layouts and the packed family, and beyond it: unknown
        assert zly.frame_bytes(fmt, 416, 416) == 0, fmt


def test_view_tight_equals_frame_bytes():
    for fmt in FMTS:
        for w, h in ((1, 1), (3, 5), (416, 416), (1921, 1081)):
            v = zly.view_tight(fmt, w, h)
            assert zly.view_bytes(v) == zly.frame_bytes(fmt, w, h) == w * h * BPP[fmt]
            assert (v.off[0], v.pitch[0]) == (0, BPP[fmt] * w)


def _view(fmt, w, h, off, pitch):
    c = zly.FrameView()
    c.fmt, c.w, c.h = fmt, w, h
    c.off[0], c.pitch[0] = off, pitch
    return c


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("slack", [0, 64, 7])              # tight pitch, padded pitch, a pitch that is no multiple of 4
def test_view_crop_equals_numpy_slicing(fmt, slack):
    bpp = BPP[fmt]
    W, H, off = 37, 23, 13
    pitch = bpp * W + slack
    if slack == 7:
        assert pitch % 4
    rng = np.random.default_rng(fmt * 10 + slack)
    surface = rng.integers(0, 256, (H, W, bpp), dtype=np.uint8)
    buf, _ = pr.embed(surface, fmt, pitch, off, seed=1)
    s = _view(fmt, W, H, off, pitch)
    assert zly.view_bytes(s) == buf.size == off + (H - 1) * pitch + bpp * W
    for x0, y0, w, h in ((5, 3, 9, 7), (1, 1, 1, 1), (0, 0, W, H), (W - 3, H - 5, 3, 5), (11, 0, 25, 1), (W - 1, H - 1, 1, 1)):
        c = zly.view_crop(s, x0, y0, w, h)
        assert (c.fmt, c.w, c.h, c.pitch[0]) == (fmt, w, h, pitch)
        assert c.off[0] == off + y0 * pitch + x0 * bpp
        assert zly.view_bytes(c) == c.off[0] + (h - 1) * pitch + bpp * w
        want = surface[y0:y0 + h, x0:x0 + w]
        assert np.array_equal(pr.cut(buf, fmt, pitch, off, x0, y0, w, h), want)
        rows = np.lib.stride_tricks.as_strided(buf[c.off[0]:], shape=(h, w * bpp), strides=(pitch, 1))
        assert np.array_equal(rows.reshape(h, w, bpp), want)
    # crops compose, also in place
    a = zly.view_crop(zly.view_crop(s, 5, 3, 21, 15), 3, 5, 7, 3)
    b = zly.view_crop(s, 8, 8, 7, 3)
    assert (a.off[0], a.pitch[0], a.w, a.h) == (b.off[0], b.pitch[0], b.w, b.h)


def test_invalid_views_have_zero_bytes():
    for fmt in FMTS:
        bpp = BPP[fmt]
        assert zly.view_bytes(_view(fmt, 16, 16, 0, bpp * 16 - 1)) == 0            # pitch below bpp * w
        assert zly.view_bytes(_view(fmt, 16, 16, 0, bpp * 16)) == 16 * 16 * bpp
        assert zly.view_bytes(_view(fmt, 0, 16, 0, 64)) == 0
        assert zly.view_bytes(_view(fmt, 16, 0, 0, 64)) == 0
        assert zly.view_bytes(_view(fmt, 16, 1 << 20, 0, 1 << 12)) == 0            # extent 2^32
        assert zly.view_bytes(_view(fmt, 1, 2, 0, (1 << 31) - bpp)) == 0           # extent exactly 2^31
        assert zly.view_bytes(_view(fmt, 1, 2, 0, (1 << 31) - bpp - 1)) == (1 << 31) - 1
        assert zly.view_bytes(_view(fmt, 1, 1, 5, bpp)) == 5 + bpp                 # odd sizes and offsets are fine: no evenness rule
    for fmt in (5, 15):
        assert zly.view_bytes(_view(fmt, 16, 16, 0, 64)) == 0


def test_reference_round_trip():
    rng = np.random.default_rng(3)
    for w, h in ((1, 1), (2, 1), (3, 5), (31, 17)):
        b = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        x = rng.integers(0, 256, (h, w), dtype=np.uint8)
        for fmt in FMTS:
            f = pr.from_bgr(b, fmt, x=x)
            assert f.shape == (h, w, BPP[fmt]) and f.nbytes == zly.frame_bytes(fmt, w, h)
            assert np.array_equal(pr.to_bgr(f, w, h, fmt), b)
            assert np.array_equal(pr.to_bgr(f.reshape(-1), w, h, fmt), b)
            if BPP[fmt] == 4:
                assert np.array_equal(f[:, :, 3], x)
        # the byte orders themselves
        assert np.array_equal(pr.from_bgr(b, zly.PIX_RGB)[:, :, 0], b[:, :, 2])
        assert np.array_equal(pr.from_bgr(b, zly.PIX_BGRA, x=9)[:, :, :3], b)
        assert np.array_equal(pr.from_bgr(b, zly.PIX_RGBA, x=9)[:, :, :3], b[:, :, ::-1])


def test_binding_infers_sizes_from_packed_arrays():
    assert zly._dims(np.zeros((5, 3, 4), np.uint8), zly.PIX_BGRA, None, None) == (3, 5)
    assert zly._dims(np.zeros((5, 3, 3), np.uint8), zly.PIX_RGB, None, None) == (3, 5)
    assert zly._dims(np.zeros(60, np.uint8), zly.PIX_RGBA, 3, 5) == (3, 5)
    with pytest.raises(ValueError):
        zly._dims(np.zeros((5, 3, 3), np.uint8), zly.PIX_BGRA, None, None)
    with pytest.raises(ValueError):
        zly._dims(np.zeros(60, np.uint8), zly.PIX_RGBA, None, None)
