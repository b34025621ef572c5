"""The area resize oracle (tests/area_ref.py) against an independent exact implementation, and the properties include/zly.h states.

The independent implementation knows no weight formula: a content pixel is the interval [d*S/D, (d+1)*S/D) of the source axis as
fractions.Fraction, a source pixel the interval [i, i+1), and the mean is the overlap-weighted sum divided by the content pixel's area, rounded
half up -- every source pixel is tried against every content pixel."""
from fractions import Fraction

import numpy as np
import pytest

import area_ref as ar
import letterbox_ref as lb

PAIRS = ar.PAIRS


def _overlap(a0, a1, b0, b1):
    lo, hi = max(a0, b0), min(a1, b1)
    return hi - lo if hi > lo else Fraction(0)


def _axis_overlaps(S, D, ds):
    """{d: [(i, overlap length as a Fraction)]} by trying every source pixel"""
    out = {}
    for d in ds:
        a0, a1 = Fraction(d * S, D), Fraction((d + 1) * S, D)
        out[d] = [(i, _overlap(a0, a1, Fraction(i), Fraction(i + 1))) for i in range(S)]
        out[d] = [(i, o) for i, o in out[d] if o > 0]
    return out


def _fraction_area(frame, D_w, D_h):
    h, w = frame.shape[:2]
    ox, oy = _axis_overlaps(w, D_w, range(D_w)), _axis_overlaps(h, D_h, range(D_h))
    out = np.zeros((D_h, D_w, frame.shape[2]), dtype=np.uint8)
    cell = Fraction(w, D_w) * Fraction(h, D_h)
    for y in range(D_h):
        for x in range(D_w):
            for c in range(frame.shape[2]):
                s = sum(wy * wx * int(frame[iy, ix, c]) for iy, wy in oy[y] for ix, wx in ox[x])
                mean = s / cell
                out[y, x, c] = int(mean + Fraction(1, 2))           # floor(mean + 1/2): round half up (int() truncates, the value is positive)
    return out


def test_every_small_pair_equals_the_fraction_implementation():
    rng = np.random.default_rng(7)
    for S in range(1, 13):
        for D in range(1, 13):
            # S x 3 -> D x 2 and 3 x S -> 2 x D: the pair on the x axis and on the y axis
            f = rng.integers(0, 256, (3, S, 3), dtype=np.uint8)
            assert np.array_equal(ar.area_bgr(f, D, 2), _fraction_area(f, D, 2)), (S, D, "x")
            g = rng.integers(0, 256, (S, 3, 3), dtype=np.uint8)
            assert np.array_equal(ar.area_bgr(g, 2, D), _fraction_area(g, 2, D)), (S, D, "y")


def _some_d(D, seed):
    return sorted({0, D - 1, *np.random.default_rng(seed).integers(0, D, 50).tolist()})


@pytest.mark.parametrize("S,D", PAIRS)
def test_large_pairs_footprints_and_weights(S, D):
    """the weight matrix and the footprints against interval overlaps, at d = 0, D - 1 and 50 seeded d"""
    ds = _some_d(D, S * 31 + D)
    W = ar.axis_weights(S, D)
    assert np.array_equal(W.sum(axis=1), np.full(D, S))                     # the weights of one d sum to S
    assert W.max() <= D and W.min() >= 0
    for d in ds:
        a0, a1 = Fraction(d * S, D), Fraction((d + 1) * S, D)
        i0, i1, w0, w1 = ar.footprint(S, D, d)
        lo_i, hi_i = int(a0), int(a1) if a1 != int(a1) else int(a1) - 1    # first and last source pixel the interval touches
        assert (i0, i1) == (lo_i, hi_i), (S, D, d)
        nz = np.nonzero(W[d])[0]
        assert nz[0] == i0 and nz[-1] == i1 and len(nz) == i1 - i0 + 1
        for i in {i0, i1, (i0 + i1) // 2}:
            assert Fraction(int(W[d, i]), D) == _overlap(a0, a1, Fraction(i), Fraction(i + 1)), (S, D, d, i)
        assert (w0, w1) == (int(W[d, i0]), int(W[d, i1]))
        assert all(int(W[d, i]) == D for i in range(i0 + 1, i1))            # interior weights equal D


@pytest.mark.parametrize("S,D", PAIRS)
def test_large_pairs_values(S, D):
    """area_bgr on a random strip against the literal weighted sum with the weight matrix (int64) and, at seeded d, against Fractions"""
    rng = np.random.default_rng(S + D)
    f = rng.integers(0, 256, (2, S, 3), dtype=np.uint8)
    got = ar.area_bgr(f, D, 1)                                              # x: S -> D, y: 2 -> 1 (the mean of the two rows)
    W = ar.axis_weights(S, D)
    acc = np.einsum("di,ic->dc", W, f.astype(np.int64).sum(axis=0))         # wy = 1 for both rows
    T = 2 * S
    assert np.array_equal(got[0], ((acc + (T >> 1)) // T).astype(np.uint8))
    for d in _some_d(D, S)[:12]:
        a0, a1 = Fraction(d * S, D), Fraction((d + 1) * S, D)
        for c in range(3):
            s = sum(_overlap(a0, a1, Fraction(i), Fraction(i + 1)) * (int(f[0, i, c]) + int(f[1, i, c])) for i in range(int(a0), min(S, int(a1) + 1)))
            assert int(got[0, d, c]) == int(s / (2 * Fraction(S, D)) + Fraction(1, 2)), (S, D, d, c)
    # the same strip on the y axis
    assert np.array_equal(ar.area_bgr(np.ascontiguousarray(f.transpose(1, 0, 2)), 1, D)[:, 0], got[0])


def test_identity_at_equal_size():
    f = np.random.default_rng(1).integers(0, 256, (37, 53, 3), dtype=np.uint8)
    assert np.array_equal(ar.area_bgr(f, 53, 37), f)
    assert np.array_equal(ar.area_resize(f, 53, 37, False), f)
    g = np.random.default_rng(2).integers(0, 256, (64, 96, 3), dtype=np.uint8)
    assert np.array_equal(ar.area_resize(g, 96, 64, True), g)               # a model-sized request: no padding, the identity


def test_block_mean_at_integer_ratios():
    rng = np.random.default_rng(3)
    for kx, ky, D_w, D_h in [(2, 2, 8, 5), (3, 1, 7, 4), (1, 4, 5, 3), (5, 3, 4, 6)]:
        f = rng.integers(0, 256, (D_h * ky, D_w * kx, 3), dtype=np.uint8)
        s = f.astype(np.int64).reshape(D_h, ky, D_w, kx, 3).sum(axis=(1, 3))
        n = kx * ky
        want = np.floor(s / n + 0.5).astype(np.uint8)                       # round half up (small integers: exact in float64)
        assert np.array_equal(ar.area_bgr(f, D_w, D_h), want), (kx, ky)


def test_constants_stay_constant_and_255_stays_255():
    for v in (0, 1, 114, 254, 255):
        for (h, w, D_w, D_h) in [(7, 13, 5, 3), (3, 5, 11, 9), (1080, 1920, 416, 416), (1, 1, 416, 416), (2, 16384, 416, 416)]:
            f = np.full((h, w, 3), v, dtype=np.uint8)
            assert (ar.area_bgr(f, D_w, D_h) == v).all(), (v, h, w)


def test_checkerboard_at_half_size_is_128():
    yy, xx = np.mgrid[0:64, 0:96]
    f = np.repeat((((xx + yy) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)
    assert (ar.area_bgr(f, 48, 32) == 128).all()                            # (2 * 255 + 2) // 4 = 128: 127.5 rounds up


def test_upscale_replicates_with_blended_seams():
    f = np.array([[[0, 0, 0], [200, 100, 50]]], dtype=np.uint8)             # 2 x 1 -> 3 x 1: [p0, (p0 + p1) / 2, p1]
    assert ar.area_bgr(f, 3, 1)[0].tolist() == [[0, 0, 0], [100, 50, 25], [200, 100, 50]]


def test_letterbox_places_the_content_in_padding():
    f = np.random.default_rng(5).integers(0, 256, (270, 480, 3), dtype=np.uint8)
    tw, th = 64, 64
    nw, nh, px, py = lb.geometry(480, 270, tw, th)
    out = ar.area_resize(f, tw, th, True)
    assert (nw, nh, px, py) == (64, 36, 0, 14)
    assert (out[:py] == ar.PAD).all() and (out[py + nh:] == ar.PAD).all()
    assert np.array_equal(out[py:py + nh, px:px + nw], ar.area_bgr(f, nw, nh))
    p = ar.preprocess_planar(f, tw, th, True)
    assert p.shape == (3, th, tw) and p.dtype == np.float32
    assert np.array_equal(p[0], out[..., 2].astype(np.float32) / np.float32(255.0))
