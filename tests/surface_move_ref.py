"""numpy oracle of the moves of the resident surfaces (include/zly.h "Resident surfaces", MOVES), on the plane helpers of tests/surface_ref.py.

A move is (sx, sy, dx, dy, w, h) on one tight surface (a 1-D u8 array): every plane's source rectangle is copied out whole, then written to the
destination rectangle -- memmove semantics.  apply_moves() applies a list of them in index order.  conflicts() and self_overlaps() are the header's
definitions, in surface pixels; tests/test_surface_move_ref.py holds apply_moves() against a per-pixel loop."""
import numpy as np

import surface_ref as sr


def legal(fmt, W, H, m):
    """both rectangles of the move are legal for zly_view_crop on the W x H surface"""
    sx, sy, dx, dy, w, h = m
    return sr.legal(fmt, W, H, sx, sy, w, h) and sr.legal(fmt, W, H, dx, dy, w, h)


def apply_moves(frame_bytes, fmt, w, h, moves):
    """applies, in place and in index order, the moves (sx, sy, dx, dy, mw, mh) to the tight w x h surface; returns the surface"""
    for m in moves:
        sx, sy, dx, dy, mw, mh = m
        assert legal(fmt, w, h, m), (fmt, w, h, m)
        tmp = sr.cut(frame_bytes, fmt, w, h, sx, sy, mw, mh).copy()          # the source, whole, before the destination is written
        sr.apply(frame_bytes, fmt, w, h, dx, dy, tmp, mw, mh)
    return frame_bytes


def _meet(ax, ay, bx, by, wa, ha, wb, hb):
    return ax < bx + wb and bx < ax + wa and ay < by + hb and by < ay + ha


def self_overlaps(m):
    """source and destination of the move (sx, sy, dx, dy, w, h) intersect"""
    sx, sy, dx, dy, w, h = m
    return _meet(sx, sy, dx, dy, w, h, w, h)


def identity(m):
    return m[0] == m[2] and m[1] == m[3]


def conflicts(a, b):
    """two moves (sx, sy, dx, dy, w, h) of ONE surface: a source meets the other's destination, or the destinations meet"""
    asx, asy, adx, ady, aw, ah = a
    bsx, bsy, bdx, bdy, bw, bh = b
    return (_meet(asx, asy, bdx, bdy, aw, ah, bw, bh) or _meet(adx, ady, bsx, bsy, aw, ah, bw, bh) or _meet(adx, ady, bdx, bdy, aw, ah, bw, bh))
