"""The chips' oracle (tests/chip_ref.py) held to include/zly.h's "Chips" by hand: the rectangle of step 4 on cases whose integers are written out
here, the rule's stated consequences, the selection of steps 1-3, "nothing else is written", and perturbations of the rule that these cases must
notice -- an oracle that agreed with a perturbed rule on all of them could not tell the kernel from a wrong one.  No GPU."""
import numpy as np
import pytest

import area_ref as ar
import chip_ref as cr
import yuv422_ref as y2
import yuv_ref as yr

F = np.float32
NAN, INF = float("nan"), float("inf")


def _f(bits):
    return np.array(bits, dtype=np.uint32).view(np.float32)[()]


# (x, w, scale, E) -> (origin, length): every number worked out by hand from the header's step 4
AXIS_CASES = [
    ((0.5, 0.25, 1.0, 100), (37, 25)),          # the middle: lo = .375 -> 37.5 -> 37, hi = .625 -> 62.5 -> 62
    ((0.5, 0.125, 4.0, 100), (25, 50)),         # scale 4: e = .5
    ((0.125, 0.25, 1.0, 100), (0, 25)),         # touching the left border: lo = 0
    ((0.0625, 0.25, 1.0, 100), (0, 18)),        # crossing it: lo = -.0625 -> 0, hi = .1875 -> 18.75 -> 18
    ((0.875, 0.25, 1.0, 100), (75, 25)),        # touching the right border: hi = 1
    ((0.9375, 0.25, 1.0, 100), (81, 19)),       # crossing it: lo = .8125 -> 81.25 -> 81, hi -> 1 -> 100
    ((1.5, 0.25, 1.0, 100), (99, 1)),           # wholly outside on the right: a = 100 -> 99, b = 100
    ((-0.5, 0.25, 1.0, 100), (0, 1)),           # wholly outside on the left: a = b = 0 -> b = 1
    ((0.5, 0.0, 1.0, 100), (50, 1)),            # w = 0: a = b = 50 -> b = 51
    ((NAN, 0.25, 1.0, 100), (0, 1)),            # NaN in x: lo, hi NaN -> 0
    ((0.5, NAN, 1.0, 100), (0, 1)),             # NaN in w
    ((INF, 0.25, 1.0, 100), (99, 1)),           # +inf in x: lo = hi = inf -> 1
    ((-INF, 0.25, 1.0, 100), (0, 1)),
    ((0.5, INF, 1.0, 100), (0, 100)),           # +inf in w: lo = -inf -> 0, hi = inf -> 1: the whole extent
    ((0.5, -INF, 1.0, 100), (99, 1)),           # -inf in w: lo = +inf -> 1 -> 99, hi = -inf -> 0 -> max(0, 100) = 100
    ((INF, INF, 1.0, 100), (0, 100)),           # inf - inf = NaN -> 0; inf + inf -> 1
    ((0.5, 0.25, 1.0, 1), (0, 1)),              # W = 1
    ((1.0, 0.0, 1.0, 100), (99, 1)),            # x = 1.0 exactly: a = W is clamped to W - 1
    ((0.5, 0.5, 1.0, 16384), (4096, 8192)),
    # an e = w * scale whose rounding decides: found by search, the integers are the rule's (one rounding per operation)
    ((_f(1058274016), _f(1050864689), 1.25, 1920), (728, 763)),
]


@pytest.mark.parametrize("args,want", AXIS_CASES)
def test_rect_axis_hand_cases(args, want):
    assert cr.rect_axis(*args) == want
    o, n = cr.rect_axis(*args)
    assert 0 <= o and 1 <= n and o + n <= args[3]


def test_rect_takes_both_axes_and_is_always_legal():
    assert cr.rect((0.5, 0.9375, 0.25, 0.25), 100, 100, 1.0) == (37, 81, 25, 19)
    d = np.zeros(1, dtype=cr.DET_DTYPE)[0]
    d["x"], d["y"], d["w"], d["h"] = 0.5, 0.5, 0.125, 0.0
    assert cr.rect(d, 100, 1, 4.0) == (25, 0, 50, 1)
    rng = np.random.default_rng(3)
    vals = np.concatenate([rng.uniform(-1, 2, 500).astype(np.float32), np.array([NAN, INF, -INF, 0, 1, -0.0], dtype=np.float32)])
    for k in range(2000):
        x, y, w, h = rng.choice(vals, 4)
        W, H = int(rng.integers(1, 300)), int(rng.integers(1, 300))
        x0, y0, rw, rh = cr.rect((x, y, w, h), W, H, [1.0, 1.25, 4.0][k % 3])
        assert 0 <= x0 and 0 <= y0 and rw >= 1 and rh >= 1 and x0 + rw <= W and y0 + rh <= H


# ---- perturbations of the rule: each must change at least one hand case ------------------------------------------------------------------
def _axis_variant(x, w, scale, E, ceil=False, fma=False):
    with np.errstate(all="ignore"):
        x, w, scale = F(x), F(w), F(scale)
        if fma:                                 # lo = fma(-e, 0.5, x) with e unrounded: the product is not rounded before the sum
            lo = F(np.float64(x) - np.float64(w) * np.float64(scale) * 0.5)
            hi = F(np.float64(x) + np.float64(w) * np.float64(scale) * 0.5)
        else:
            half = F(F(w * scale) * F(0.5))
            lo, hi = F(x - half), F(x + half)
        pa, pb = F(cr._c(lo) * F(E)), F(cr._c(hi) * F(E))
        a, b = (int(np.ceil(pa)), int(np.ceil(pb))) if ceil else (int(pa), int(pb))
    a = min(a, E - 1)
    b = min(max(b, a + 1), E)
    return a, b - a


def test_the_variant_without_perturbation_is_the_oracle():
    for args, want in AXIS_CASES:
        assert _axis_variant(*args) == want


@pytest.mark.parametrize("kw", [dict(ceil=True), dict(fma=True)], ids=["ceil", "fma"])
def test_hand_cases_notice_a_perturbed_rectangle(kw):
    assert any(_axis_variant(*args, **kw) != want for args, want in AXIS_CASES)


def test_hand_cases_notice_selection_by_confidence():
    # slab order is class ascending, confidence descending: the first eligible detection is not the most confident one
    slab = cr.make_slab([(0.2, 0.2, 0.1, 0.1, 0.6, 0, 0), (0.7, 0.7, 0.1, 0.1, 0.9, 1, 0)], cap=4)
    n_elig, chosen = cr.select(slab, 4, cr.Config(max_chips=1))
    assert (n_elig, chosen) == (2, [0])
    _, dets = cr.parse_slab(slab, 4)
    by_conf = sorted(range(2), key=lambda d: -float(dets[d]["confidence"]))[:1]
    assert by_conf != chosen


@pytest.mark.parametrize("fmt", list(yr.YUV_FORMATS) + list(y2.FORMATS))
def test_hand_cases_notice_chroma_relative_to_the_rectangle(fmt):
    """a chip of a rectangle with an odd origin uses every pixel's own chroma sample; converting the cropped planes as a frame of their own --
    chroma indexed from the rectangle's corner -- gives other pixels"""
    W, H = 8, 6
    rng = np.random.default_rng(fmt)
    is420 = fmt in yr.YUV_FORMATS
    frame = rng.integers(0, 256, W * H * 3 // 2 if is420 else W * H * 2, dtype=np.uint8)
    bgr = cr.bgr_of(fmt, frame, W, H)
    x0, y0, rw, rh = 1, (1 if is420 else 0), 4, 4
    want = cr.chip_bgr(bgr, (x0, y0, rw, rh), cr.Config(chip_w=4, chip_h=4))
    assert np.array_equal(want, bgr[y0:y0 + rh, x0:x0 + rw])                 # the identity consequence
    if is420:
        y, u, v = yr.planes(frame, W, H, fmt)
        yy = y[y0:y0 + rh, x0:x0 + rw]
        cu = u[y0 // 2:y0 // 2 + rh // 2, x0 // 2:x0 // 2 + rw // 2]          # the rectangle's "own" chroma grid, phase lost
        cv = v[y0 // 2:y0 // 2 + rh // 2, x0 // 2:x0 // 2 + rw // 2]
        wrong = yr.yuv420_to_bgr(yr.pack(yy, cu, cv, fmt), rw, rh, fmt)
    else:
        yv, u, v = y2.samples(frame, W, H, fmt)
        wrong = y2.to_bgr(y2.pack(yv[y0:y0 + rh, x0:x0 + rw], u[y0:y0 + rh, x0 // 2:x0 // 2 + rw // 2], v[y0:y0 + rh, x0 // 2:x0 // 2 + rw // 2], fmt), rw, rh, fmt)
    assert not np.array_equal(wrong, want)


# ---- the consequences the header states ---------------------------------------------------------------------------------------------------
def test_a_rectangle_of_the_chips_size_returns_the_source_pixels():
    rng = np.random.default_rng(5)
    bgr = rng.integers(0, 256, (40, 50, 3), dtype=np.uint8)
    for layout in (cr.BGR8, cr.RGB_F32):
        cfg = cr.Config(chip_w=17, chip_h=9, layout=layout)
        got = cr.chip(bgr, (3, 5, 17, 9), cfg)
        src = bgr[5:14, 3:20]
        if layout == cr.BGR8:
            assert np.array_equal(got.reshape(9, 17, 3), src)
        else:
            want = np.stack([src[..., 2], src[..., 1], src[..., 0]]).astype(np.float32) / np.float32(255)
            assert np.array_equal(got.view(np.float32).reshape(3, 9, 17), want)


def test_a_constant_frame_gives_constant_chips():
    bgr = np.empty((33, 47, 3), dtype=np.uint8)
    bgr[...] = (7, 130, 255)
    for r in [(0, 0, 47, 33), (5, 6, 1, 1), (10, 3, 13, 29), (46, 32, 1, 1)]:
        c = cr.chip_bgr(bgr, r, cr.Config(chip_w=8, chip_h=5))
        assert c.shape == (5, 8, 3) and (c == np.array([7, 130, 255], dtype=np.uint8)).all()


def test_upscale_from_one_pixel_replicates_it():
    rng = np.random.default_rng(6)
    bgr = rng.integers(0, 256, (4, 4, 3), dtype=np.uint8)
    c = cr.chip_bgr(bgr, (2, 1, 1, 1), cr.Config(chip_w=64, chip_h=64))
    assert (c == bgr[1, 2]).all()


def test_chip_is_the_area_resize_of_the_crop():
    rng = np.random.default_rng(7)
    bgr = rng.integers(0, 256, (30, 41, 3), dtype=np.uint8)
    c = cr.chip_bgr(bgr, (4, 2, 20, 10), cr.Config(chip_w=10, chip_h=5))
    blocks = bgr[2:12, 4:24].astype(np.int64).reshape(5, 2, 10, 2, 3).sum(axis=(1, 3))
    assert np.array_equal(c, ((blocks + 2) // 4).astype(np.uint8))            # S = 2D: the 2 x 2 block mean, rounded half up
    assert np.array_equal(c, ar.area_bgr(bgr[2:12, 4:24], 10, 5))


# ---- selection ------------------------------------------------------------------------------------------------------------------------------
def _dets(classes):
    return [(0.1 + 0.05 * k, 0.5, 0.1, 0.1, 0.9 - 0.01 * k, c, 100 + k) for k, c in enumerate(classes)]


def test_selection_class_filter_and_counts():
    slab = cr.make_slab(_dets([0, 0, 1, 2, 2, 2]), cap=8)
    assert cr.select(slab, 8, cr.Config(max_chips=4, class_id=-1)) == (6, [0, 1, 2, 3])      # n_eligible above max_chips
    assert cr.select(slab, 8, cr.Config(max_chips=3, class_id=2)) == (3, [3, 4, 5])          # equal to it
    assert cr.select(slab, 8, cr.Config(max_chips=2, class_id=2)) == (3, [3, 4])
    assert cr.select(slab, 8, cr.Config(max_chips=4, class_id=1)) == (1, [2])
    assert cr.select(slab, 8, cr.Config(max_chips=4, class_id=7)) == (0, [])                 # none eligible
    assert cr.select(cr.make_slab([], cap=8), 8, cr.Config()) == (0, [])


def test_selection_clamps_n_kept():
    over = cr.make_slab(_dets([0, 1, 1, 1]), cap=4, n_kept=9, flags=1)                       # n_kept above cap, with the overflow flag: K = cap
    assert cr.select(over, 4, cr.Config(max_chips=8)) == (4, [0, 1, 2, 3])
    neg = cr.make_slab(_dets([0, 1]), cap=4, n_kept=-3)                                      # negative n_kept: K = 0
    assert cr.select(neg, 4, cr.Config(max_chips=8)) == (0, [])
    part = cr.make_slab(_dets([0, 1, 1]), cap=4, n_kept=2)                                   # records behind n_kept are not detections
    assert cr.select(part, 4, cr.Config(max_chips=8)) == (2, [0, 1])


# ---- the chip slab ----------------------------------------------------------------------------------------------------------------------------
def test_layout_numbers():
    sb, po, st, cb = cr.layout(cr.Config(chip_w=64, chip_h=64, max_chips=16))
    assert (po, st, cb, sb) == (768, 12288, 12288, 768 + 16 * 12288)                         # 16 + 16 * 32 = 528 -> 768
    sb, po, st, cb = cr.layout(cr.Config(chip_w=33, chip_h=17, max_chips=7))
    assert (po, st, cb, sb) == (256, 1696, 1683, 256 + 7 * 1696)                             # 16 + 224 = 240 -> 256; 1683 -> 1696
    sb, po, st, cb = cr.layout(cr.Config(chip_w=1, chip_h=1, max_chips=1, layout=cr.RGB_F32))
    assert (po, st, cb, sb) == (256, 16, 12, 272)


@pytest.mark.parametrize("layout", [cr.BGR8, cr.RGB_F32])
def test_nothing_else_is_written(layout):
    cfg = cr.Config(chip_w=5, chip_h=3, max_chips=4, class_id=1, scale=1.25, layout=layout)
    rng = np.random.default_rng(8)
    frames = [rng.integers(0, 256, (20, 30, 3), dtype=np.uint8), rng.integers(0, 256, (7, 9, 3), dtype=np.uint8)]
    slabs = np.stack([cr.make_slab(_dets([0, 1, 1, 2]), cap=6, frame_tag=41, fill=0xEE), cr.make_slab(_dets([0]), cap=6, frame_tag=42, fill=0xEE)])
    sb, po, st, cb = cr.layout(cfg)
    before = np.full((2, sb), 0xA5, dtype=np.uint8)
    out = cr.chip_slabs(slabs, frames, cfg, before)
    written = np.zeros((2, sb), dtype=bool)
    written[:, :16] = True
    for j in range(2):                                                                        # frame 0: two chips; frame 1: none
        written[0, 16 + 32 * j:48 + 32 * j] = True
        written[0, po + j * st:po + j * st + cb] = True
    assert (out[~written] == 0xA5).all()
    h0, h1 = out[0, :16].view(cr.HDR_DTYPE)[0], out[1, :16].view(cr.HDR_DTYPE)[0]
    assert (int(h0["n_chips"]), int(h0["n_eligible"]), int(h0["frame_tag"]), int(h0["flags"])) == (2, 2, 41, 0)
    assert (int(h1["n_chips"]), int(h1["n_eligible"]), int(h1["frame_tag"]), int(h1["flags"])) == (0, 0, 42, 0)
    recs = out[0, 16:16 + 64].view(cr.REC_DTYPE)
    assert [int(r["det"]) for r in recs] == [1, 2] and [int(r["track_id"]) for r in recs] == [101, 102] and [int(r["class_id"]) for r in recs] == [1, 1]
    for j, r in enumerate(recs):
        rc = (int(r["x0"]), int(r["y0"]), int(r["w"]), int(r["h"]))
        assert rc == cr.rect(_dets([0, 1, 1, 2])[1 + j], 30, 20, 1.25)
        assert np.array_equal(out[0, po + j * st:po + j * st + cb], cr.chip(frames[0], rc, cfg))
    assert np.array_equal(before, np.full((2, sb), 0xA5, dtype=np.uint8))                     # the caller's array is not modified
