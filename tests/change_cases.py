"""Shared case builders of the change map's tests (tests/test_change_ref.py and tests/test_change_rules.py on the CPU, tests/test_gpu_change.py on the
GPU): frame sequences of all twelve pixel formats whose steps differ in known ways, on top of tests/chip_cases.py's frames and views."""
import numpy as np

import chip_cases as cc
import change_ref as chr_

SIZES = ((1, 1), (2, 2), (7, 5), (33, 31), (101, 77), (641, 479), (640, 480))
CELLS = chr_.CELLS


def legal_size(fmt, w, h):
    """the size rounded up to what the format allows"""
    return cc.legal(fmt, w, h)


def film(fmt, w, h, kinds, seed):
    """a sequence of tight frames of one stream -> [(frame flat u8, BGR image)].  kinds, one per step:
         "new"    every byte random (the first step, or a change of the whole scene)
         "same"   the previous frame again
         "blocks" the previous frame with up to three random rectangles of plane 0 overwritten by random bytes
         "flat"   the previous frame with one rectangle of plane 0 set to its bytes' complement: a large, certain change"""
    rng = np.random.default_rng(seed * 7919 + fmt * 31 + w * 3 + h)
    shapes = cc.plane_shapes(fmt, w, h)
    total = sum(r * rb for r, rb in shapes)
    rows, rb = shapes[0]
    out, cur = [], None
    for kind in kinds:
        if kind == "new" or cur is None:
            cur = rng.integers(0, 256, total, dtype=np.uint8)
        elif kind == "same":
            cur = cur.copy()
        else:
            cur = cur.copy()
            plane = cur[:rows * rb].reshape(rows, rb)
            for _ in range(1 if kind == "flat" else int(rng.integers(1, 4))):
                rh_, rw_ = int(rng.integers(1, max(rows // 3, 1) + 1)), int(rng.integers(1, max(rb // 3, 1) + 1))
                r0, c0 = int(rng.integers(0, rows - rh_ + 1)), int(rng.integers(0, rb - rw_ + 1))
                if kind == "flat":
                    plane[r0:r0 + rh_, c0:c0 + rw_] = 255 - plane[r0:r0 + rh_, c0:c0 + rw_]
                else:
                    plane[r0:r0 + rh_, c0:c0 + rw_] = rng.integers(0, 256, (rh_, rw_), dtype=np.uint8)
        f = cur
        out.append((f, np.ascontiguousarray(chr_.chip_ref.bgr_of(fmt, f if fmt not in cc.FPK else f.reshape(h, w, cc.pr.BPP[fmt]), w, h))))
    return out


def gray(w, h, value=0):
    """a constant BGR image: its luma is `value`"""
    return np.full((h, w, 3), value, dtype=np.uint8)
