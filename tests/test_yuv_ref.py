"""CPU tests of the YUV 4:2:0 input formats (include/zly.h ZLY_PIX_*): the integer conversion the front kernels implement
(tests/yuv_ref.py) against an independent float reference, the two layouts, the chroma sharing, and zly_frame_bytes."""
import numpy as np
import pytest

import yuv_ref as yr
import zly
import zly_model as zm


@pytest.mark.parametrize("mat", [601, 709])
def test_integer_conversion_within_one_of_float_reference_for_all_yuv(mat):
    u, v = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    worst = 0
    for y in range(256):
        b, g, r = yr.convert_yuv(np.full_like(u, y), u, v, mat)
        fr, fg, fb = yr.float_reference(np.full(u.shape, y), u, v, mat)
        for got, want in ((r, fr), (g, fg), (b, fb)):
            d = np.abs(got.astype(np.float64) - np.clip(want, 0.0, 255.0))
            worst = max(worst, float(d.max()))
    assert worst <= 1.0, worst


def test_coefficients_are_the_documented_fixed_point_values():
    assert yr.COEFFS[601] == tuple(int(round(c * 2 ** 20)) * s for c, s in ((1.164, 1), (1.596, 1), (0.813, -1), (0.391, -1), (2.018, 1)))
    kr, kb = yr.KR_KB[709]
    kg = 1 - kr - kb
    ys, cs = 255 / 219, 255 / 224
    exact = (ys, 2 * (1 - kr) * cs, -2 * (1 - kr) * kr / kg * cs, -2 * (1 - kb) * kb / kg * cs, 2 * (1 - kb) * cs)
    assert yr.COEFFS[709] == tuple(int(round(c * 2 ** 20)) for c in exact)
    # every product of the formula fits the 24-bit multiplier's operands and the sums fit int32
    for c in yr.COEFFS[601] + yr.COEFFS[709]:
        assert -(1 << 23) <= c < (1 << 23)
    assert 239 * max(yr.COEFFS[601][0], yr.COEFFS[709][0]) + 128 * 2215014 + (1 << 19) < 2 ** 31


@pytest.mark.parametrize("mat", [601, 709])
def test_known_answers(mat):
    def bgr(y, u, v):
        return tuple(int(c[0]) for c in yr.convert_yuv(np.array([y]), np.array([u]), np.array([v]), mat))
    assert bgr(16, 128, 128) == (0, 0, 0)                    # limited-range black
    assert bgr(235, 128, 128) == (255, 255, 255)             # limited-range white
    assert bgr(0, 128, 128) == (0, 0, 0)                     # below black: luma floor
    assert bgr(255, 128, 128) == (255, 255, 255)             # above white: clamp
    # saturation corners: each channel clamps at both ends
    assert bgr(235, 128, 255)[2] == 255 and bgr(16, 128, 0)[2] == 0            # R from V
    assert bgr(235, 255, 128)[0] == 255 and bgr(16, 0, 128)[0] == 0            # B from U
    assert bgr(235, 0, 0)[1] == 255 and bgr(16, 255, 255)[1] == 0              # G from both
    assert bgr(255, 255, 255) == (255, 125 if mat == 601 else 184, 255)      # G = (yy + CVG*127 + CUG*127 + 2^19) >> 20
    assert bgr(0, 0, 0) == (0, 154 if mat == 601 else 96, 0)              # G = (-CVG*128 - CUG*128 + 2^19) >> 20


@pytest.mark.parametrize("mat", [601, 709])
def test_nv12_and_i420_of_one_picture_convert_identically(mat):
    bgr = zm.synth_frames(1, 66, 38, seed=3)[0]
    nv12, i420 = (yr.PIX_NV12_BT601, yr.PIX_I420_BT601) if mat == 601 else (yr.PIX_NV12_BT709, yr.PIX_I420_BT709)
    a, b = yr.bgr_to_yuv420(bgr, nv12), yr.bgr_to_yuv420(bgr, i420)
    assert not np.array_equal(a, b)                                 # the layouts differ ...
    for p, q in zip(yr.planes(a, 66, 38, nv12), yr.planes(b, 66, 38, i420)):
        assert np.array_equal(p, q)                                 # ... the planes do not
    assert np.array_equal(yr.yuv420_to_bgr(a, 66, 38, nv12), yr.yuv420_to_bgr(b, 66, 38, i420))
    # and the round trip stays close to the picture (the forward transform is only a test-input generator)
    back = yr.yuv420_to_bgr(yr.bgr_to_yuv420(np.full((4, 4, 3), 100, np.uint8), nv12), 4, 4, nv12)
    assert np.abs(back.astype(int) - 100).max() <= 2


def test_one_chroma_sample_covers_each_2x2_block():
    w, h = 8, 6
    y = np.full((h, w), 128, np.uint8)
    u = np.arange(12, dtype=np.uint8).reshape(3, 4) * 20
    v = 255 - u
    for fmt in yr.YUV_FORMATS:
        out = yr.yuv420_to_bgr(yr.pack(y, u, v, fmt), w, h, fmt)
        for by in range(3):
            for bx in range(4):
                blk = out[2 * by:2 * by + 2, 2 * bx:2 * bx + 2].reshape(4, 3)
                assert (blk == blk[0]).all()
                b, g, r = yr.convert_yuv(np.array([128]), np.array([u[by, bx]]), np.array([v[by, bx]]), yr.matrix(fmt))
                assert tuple(blk[0]) == (b[0], g[0], r[0])


def test_frame_bytes_of_the_library():
    """zly_frame_bytes needs neither an engine nor a GPU (the library is loaded on the CPU, as test_abi.py does)"""
    assert zly.frame_bytes(zly.PIX_BGR, 416, 416) == 416 * 416 * 3
    assert zly.frame_bytes(zly.PIX_BGR, 5, 3) == 45
    for fmt in (zly.PIX_NV12_BT601, zly.PIX_I420_BT601, zly.PIX_NV12_BT709, zly.PIX_I420_BT709):
        assert zly.frame_bytes(fmt, 416, 416) == 416 * 416 * 3 // 2
        assert zly.frame_bytes(fmt, 1920, 1080) == 1920 * 1080 * 3 // 2
        assert zly.frame_bytes(fmt, 2, 2) == 6
        assert zly.frame_bytes(fmt, 417, 416) == 0 and zly.frame_bytes(fmt, 416, 415) == 0      # odd sizes
        assert zly.frame_bytes(fmt, 0, 2) == 0 and zly.frame_bytes(fmt, 2, -2) == 0
    for bad in (-1, 5, 99):
        assert zly.frame_bytes(bad, 416, 416) == 0
    assert zly.frame_bytes(zly.PIX_BGR, 0, 4) == 0
