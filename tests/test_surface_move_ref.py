"""tests/surface_move_ref.py against the definition it abbreviates: after a move every PIXEL of the destination rectangle holds, sample by sample,
what the corresponding pixel of the source rectangle held BEFORE the move -- a naive loop that reads from a snapshot.  Hand cases: a shift by one
pixel in each of the eight directions, a move onto itself, chroma following luma, and two dependent moves whose result tells index order from its
alternatives."""
import numpy as np
import pytest

import surface_move_ref as mr
import surface_ref as sr
from test_surface_ref import _samples


def _naive(surface, fmt, w, h, moves):
    out = surface.copy()
    for sx, sy, dx, dy, mw, mh in moves:
        before = out.copy()
        for y in range(mh):
            for x in range(mw):
                for d, s in zip(_samples(fmt, w, h, dx + x, dy + y), _samples(fmt, w, h, sx + x, sy + y)):
                    out[d] = before[s]
    return out


def _frame(fmt, w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, sr.frame_bytes(fmt, w, h), dtype=np.uint8)


EIGHT = [(-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1)]


@pytest.mark.parametrize("fmt", sr.ALL_FORMATS)
def test_a_shift_by_one_step_in_each_of_the_eight_directions(fmt):
    _, _, ex, ey = sr.FORMATS[fmt]
    w, h = (38 if ex else 37), (30 if ey else 29)
    stx, sty = (2 if ex else 1), (2 if ey else 1)
    f = _frame(fmt, w, h, 10 + fmt)
    for ux, uy in EIGHT:
        m = (8, 6, 8 + ux * stx, 6 + uy * sty, 12, 10)
        assert mr.legal(fmt, w, h, m) and mr.self_overlaps(m) and not mr.identity(m)
        got = mr.apply_moves(f.copy(), fmt, w, h, [m])
        assert np.array_equal(got, _naive(f, fmt, w, h, [m])), (fmt, m)
        assert not np.array_equal(got, f)
        # the destination holds the old source, and nothing else changed
        assert np.array_equal(sr.cut(got, fmt, w, h, m[2], m[3], 12, 10), sr.cut(f, fmt, w, h, 8, 6, 12, 10))
        rest = sr.apply(got.copy(), fmt, w, h, m[2], m[3], sr.cut(f, fmt, w, h, m[2], m[3], 12, 10), 12, 10)
        assert np.array_equal(rest, f)


def test_a_shift_by_one_pixel_in_bgr_is_three_bytes():
    w, h = 7, 5
    f = _frame(sr.PIX_BGR, w, h, 1)
    for ux, uy in EIGHT:
        got = mr.apply_moves(f.copy(), sr.PIX_BGR, w, h, [(1, 1, 1 + ux, 1 + uy, 5, 3)]).reshape(h, w, 3)
        assert np.array_equal(got[1 + uy:4 + uy, 1 + ux:6 + ux], f.reshape(h, w, 3)[1:4, 1:6])


@pytest.mark.parametrize("fmt", sr.ALL_FORMATS)
def test_a_move_onto_itself_changes_nothing(fmt):
    f = _frame(fmt, 38, 30, 20 + fmt)
    m = (4, 6, 4, 6, 10, 8)
    assert mr.identity(m) and mr.self_overlaps(m)
    assert np.array_equal(mr.apply_moves(f.copy(), fmt, 38, 30, [m]), f)


@pytest.mark.parametrize("fmt", [sr.PIX_NV12_BT601, sr.PIX_I420_BT709, sr.PIX_YUY2_BT601])
def test_chroma_follows_luma(fmt):
    kind = sr.FORMATS[fmt][0]
    w, h = 16, 12
    f = _frame(fmt, w, h, 30 + fmt)
    m = (2, 2, 8, 6, 6, 4)
    got = mr.apply_moves(f.copy(), fmt, w, h, [m])
    assert np.array_equal(got, _naive(f, fmt, w, h, [m]))
    if kind == "packed":                                    # YUY2: the macropixels Y0 U Y1 V travel whole
        a, b = got.reshape(h, w * 2), f.reshape(h, w * 2)
        assert np.array_equal(a[6:10, 16:28], b[2:6, 4:16])
    else:
        ya, yb = got[:w * h].reshape(h, w), f[:w * h].reshape(h, w)
        assert np.array_equal(ya[6:10, 8:14], yb[2:6, 2:8])
        if kind == "nv12":
            ca, cb = got[w * h:].reshape(h // 2, w), f[w * h:].reshape(h // 2, w)
            assert np.array_equal(ca[3:5, 8:14], cb[1:3, 2:8]) and int((ca != cb).sum()) <= 2 * 6
        else:
            q = (w // 2) * (h // 2)
            for k in (0, 1):
                ca, cb = got[w * h + k * q:w * h + (k + 1) * q].reshape(h // 2, w // 2), f[w * h + k * q:w * h + (k + 1) * q].reshape(h // 2, w // 2)
                assert np.array_equal(ca[3:5, 4:7], cb[1:3, 1:4]) and int((ca != cb).sum()) <= 2 * 3


def test_two_dependent_moves_are_applied_in_index_order():
    """move 1 reads what move 0 wrote: the result differs from "all sources read first" and from the reverse order"""
    fmt, w, h = sr.PIX_BGR, 12, 6
    f = np.arange(sr.frame_bytes(fmt, w, h), dtype=np.uint8)
    a, b = (0, 0, 4, 0, 4, 4), (4, 0, 8, 2, 4, 4)
    assert mr.conflicts(a, b) and mr.conflicts(b, a) and not mr.self_overlaps(a) and not mr.self_overlaps(b)
    in_order = mr.apply_moves(f.copy(), fmt, w, h, [a, b])
    assert np.array_equal(in_order, _naive(f, fmt, w, h, [a, b]))
    reverse = mr.apply_moves(f.copy(), fmt, w, h, [b, a])
    sources_first = f.copy()
    for m in (a, b):
        sr.apply(sources_first, fmt, w, h, m[2], m[3], sr.cut(f, fmt, w, h, m[0], m[1], 4, 4), 4, 4)
    assert not np.array_equal(in_order, reverse) and not np.array_equal(in_order, sources_first)
    # in order, the block at (8, 2) is the ORIGINAL block at (0, 0)
    assert np.array_equal(sr.cut(in_order, fmt, w, h, 8, 2, 4, 4), sr.cut(f, fmt, w, h, 0, 0, 4, 4))


def test_random_sequences_against_the_naive_loop():
    for fmt in sr.ALL_FORMATS:
        _, _, ex, ey = sr.FORMATS[fmt]
        w, h = (14 if ex else 13), (10 if ey else 9)
        stx, sty = (2 if ex else 1), (2 if ey else 1)
        rng = np.random.default_rng(40 + fmt)
        f = _frame(fmt, w, h, 50 + fmt)
        moves = []
        while len(moves) < 12:
            mw, mh = int(rng.integers(1, w // stx)) * stx, int(rng.integers(1, h // sty)) * sty
            p = lambda lim, st: int(rng.integers(0, lim // st + 1)) * st
            moves.append((p(w - mw, stx), p(h - mh, sty), p(w - mw, stx), p(h - mh, sty), mw, mh))
        assert np.array_equal(mr.apply_moves(f.copy(), fmt, w, h, moves), _naive(f, fmt, w, h, moves)), fmt


def test_conflicts_and_self_overlaps_are_the_headers_definitions():
    assert mr.self_overlaps((0, 0, 3, 3, 4, 4)) and not mr.self_overlaps((0, 0, 4, 0, 4, 4)) and not mr.self_overlaps((0, 0, 0, 4, 4, 4))
    a = (0, 0, 10, 0, 4, 4)
    assert mr.conflicts(a, (10, 0, 20, 0, 4, 4))            # reads what a wrote
    assert mr.conflicts(a, (20, 0, 3, 3, 4, 4))             # writes what a reads
    assert mr.conflicts(a, (20, 0, 13, 3, 4, 4))            # writes what a wrote
    assert not mr.conflicts(a, (0, 0, 20, 0, 4, 4))         # two readers of one source
    assert not mr.conflicts(a, (4, 0, 14, 0, 4, 4))         # touching
