"""CPU tests of the letterbox resize mode (include/zly.h ZLY_FLAG_LETTERBOX): the host-only geometry export against the numpy reference
(tests/letterbox_ref.py), and the reference against itself -- identity, padding, int32 range, and the error of the fixed-point scheme
against a float64 bilinear."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import letterbox_ref as lb
import zly

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = [(416, 416), (640, 640), (640, 384)]
EDGE_SIZES = [(1, 1), (2, 2), (3, 1001), (4000, 3), (416, 416), (640, 640), (640, 384), (832, 832), (1280, 768), (896, 182), (182, 896), (1, 16384),
              (16384, 1), (16384, 16384), (1920, 1080), (1280, 720), (233, 416), (100, 62)]


def test_header_defines_the_flag_and_the_binding_carries_the_symbol():
    h = open(os.path.join(ROOT, "include", "zly.h")).read()
    assert re.search(r"#define\s+ZLY_FLAG_LETTERBOX\s+32\b", h)
    assert re.search(r"#define\s+ZLY_LETTERBOX_MAX_DIM\s+16384\b", h)
    assert zly.FLAG_LETTERBOX == 32 and zly.LETTERBOX_MAX_DIM == lb.MAX_DIM == 16384
    assert "zly_letterbox_geometry" in zly.SYMBOLS
    assert hasattr(zly.load_library(), "zly_letterbox_geometry")


def test_geometry_export_equals_reference_on_random_and_edge_sizes():
    rng = np.random.default_rng(20240)
    for tw, th in MODELS:
        sizes = [tuple(int(v) for v in rng.integers(1, 16385, size=2)) for _ in range(2000)] + EDGE_SIZES
        for w, h in sizes:
            got = zly.letterbox_geometry(w, h, tw, th)
            want = lb.geometry(w, h, tw, th)
            assert got == want, (w, h, tw, th, got, want)
            nw, nh, px, py = got
            assert 1 <= nw <= tw and 1 <= nh <= th and (nw == tw or nh == th)
            assert 0 <= px and px + nw <= tw and 0 <= py and py + nh <= th


def test_geometry_known_values():
    assert lb.geometry(1920, 1080, 416, 416) == (416, 234, 0, 91)
    assert lb.geometry(233, 416, 416, 416) == (233, 416, 91, 0)
    assert lb.geometry(416, 416, 416, 416) == (416, 416, 0, 0)
    assert lb.geometry(896, 182, 416, 416) == (416, 85, 0, 165)        # 182 * 416 / 896 = 84.5 exactly: half rounds up
    assert lb.geometry(182, 896, 416, 416) == (85, 416, 165, 0)
    assert lb.geometry(4000, 3, 416, 416) == (416, 1, 0, 207)          # never below one row
    assert lb.geometry(1, 1, 640, 384) == (384, 384, 128, 0)


def test_geometry_differs_from_python_rounding_only_at_exact_halves():
    """the header's claim: Ultralytics' round() (half to even) differs from round-half-up only where the scaled side is exactly k + 1/2"""
    rng = np.random.default_rng(7)
    diff = 0
    for _ in range(20000):
        w, h = (int(v) for v in rng.integers(1, 4097, size=2))
        nw, nh, _, _ = lb.geometry(w, h, 416, 416)
        r = min(416 / h, 416 / w)
        uw, uh = max(1, round(w * r)), max(1, round(h * r))
        if (nw, nh) != (uw, uh):
            diff += 1
            assert abs(nw - uw) <= 1 and abs(nh - uh) <= 1, (w, h)
    assert diff <= 40                                                    # a few in ten thousand


def test_geometry_refuses_bad_sizes():
    lib = zly.load_library()
    o = [C.c_int32(77) for _ in range(4)]
    refs = [C.byref(x) for x in o]
    for w, h, tw, th in [(0, 10, 416, 416), (10, 0, 416, 416), (-3, 10, 416, 416), (10, 10, 0, 416), (10, 10, 416, -1)]:
        assert lib.zly_letterbox_geometry(w, h, tw, th, *refs) == zly.ERR_INVALID_ARGUMENT
        assert all(x.value == 77 for x in o)
    assert lib.zly_letterbox_geometry(10, 10, 416, 416, None, refs[1], refs[2], refs[3]) == zly.ERR_INVALID_ARGUMENT
    with pytest.raises(zly.ZlyError):
        zly.letterbox_geometry(0, 0, 416, 416)


def test_model_sized_frame_is_unchanged():
    rng = np.random.default_rng(1)
    for tw, th in MODELS:
        f = rng.integers(0, 256, size=(th, tw, 3), dtype=np.uint8)
        assert np.array_equal(lb.letterbox_bgr(f, tw, th), f)


def test_padding_value_and_extent():
    rng = np.random.default_rng(2)
    for (w, h) in [(1920, 1080), (233, 416), (100, 62), (3, 1001), (4000, 3), (2, 2)]:
        f = np.full((h, w, 3), 255, dtype=np.uint8) if w * h > 16 else rng.integers(200, 256, size=(h, w, 3), dtype=np.uint8)
        out = lb.letterbox_bgr(f, 416, 416)
        nw, nh, px, py = lb.geometry(w, h, 416, 416)
        inside = np.zeros((416, 416), bool)
        inside[py:py + nh, px:px + nw] = True
        assert (out[~inside] == 114).all()
        assert (out[inside] >= 200).all()                                # content of a bright frame stays bright: 255 stays 255
        if w * h > 16:
            assert (out[inside] == 255).all()


def test_every_intermediate_fits_int32_at_the_size_limit():
    lim = (1 << 31) - 1
    for S in (16384, 16383, 9999):
        for D in (1, 2, 3, 5, 233, 415, 416, 640, 4096, 16384):
            t = []
            i0, i1, a = lb.axis_taps(S, D, t)
            assert max(t) <= lim, (S, D, max(t))
            assert i0.min() >= 0 and i1.max() <= S - 1 and a.min() >= 0 and a.max() <= 255
    t = []
    lb.resize_bgr(np.full((3, 5, 3), 255, np.uint8), 7, 9, t)
    assert max(t) <= 255 * 65536 + 32768 <= lim


@pytest.mark.parametrize("size", [(1920, 1080), (1280, 720), (640, 480), (100, 62), (418, 330), (233, 416), (3, 1001), (4000, 3)])
def test_fixed_point_error_against_float64_bilinear(size):
    """weight truncation (1/256 per axis) plus step rounding (D * 2^-17 source pixels per axis), times the largest step between
    neighbours (255), plus the final rounding: the derived bound.  Black / white noise is the worst case for both terms."""
    w, h = size
    rng = np.random.default_rng(w * 31 + h)
    frame = (rng.integers(0, 2, size=(h, w, 3), dtype=np.uint8) * 255).astype(np.uint8)
    nw, nh, _, _ = lb.geometry(w, h, 416, 416)
    got = lb.resize_bgr(frame, nw, nh).astype(np.float64)
    ref = lb.float_bilinear(frame, nw, nh)
    bound = 0.5 + 255.0 * ((1 / 256 + nw * 2.0 ** -17) + (1 / 256 + nh * 2.0 ** -17))
    err = float(np.abs(got - ref).max())
    print(f"{w}x{h} -> {nw}x{nh}: max error {err:.3f} grey levels, bound {bound:.3f}")
    assert err <= bound, (err, bound)


def test_map_boxes_and_unpad_head_are_the_same_operations():
    rng = np.random.default_rng(3)
    head = rng.uniform(0, 416, size=(8, 50)).astype(np.float32)
    w, h = 1920, 1080
    x, y, bw, bh = lb.map_boxes(head[0], head[1], head[2], head[3], w, h, 416, 416)
    hp, nw, nh = lb.unpad_head(head, w, h, 416, 416)
    f = np.float32
    assert np.array_equal(x, hp[0] / f(nw)) and np.array_equal(y, hp[1] / f(nh))
    assert np.array_equal(bw, hp[2] / f(nw)) and np.array_equal(bh, hp[3] / f(nh))
    # a box centred in the letterbox maps to the frame's centre
    cx, cy, _, _ = lb.map_boxes(f(208.0), f(208.0), f(10), f(10), w, h, 416, 416)
    assert abs(float(cx) - 0.5) < 1e-6 and abs(float(cy) - 0.5) < 1e-6
