"""The change map's oracle (tests/change_ref.py) against cases computed by hand from include/zly.h "Change map": the oracle is what the host twin
(tests/test_change_rules.py) and the kernels (tests/test_gpu_change.py) are compared with, so it is checked first.  No GPU, no library."""
import numpy as np
import pytest

import change_cases as cs
import change_ref as chr_

Config = chr_.Config


def _rec(cfg, fill=0):
    return np.full(chr_.layout(cfg)[0], fill, dtype=np.uint8)


def _run(frames, cfg, suppress=()):
    s, rec, out = chr_.Stream(), _rec(cfg), []
    for f in frames:
        out.append(s.frame(f, cfg, rec, suppress))
    return out, rec, s


def test_luma_of_gray_is_the_gray_and_the_weights_sum_to_256():
    for v in (0, 1, 127, 128, 255):
        assert int(chr_.luma(cs.gray(3, 2, v))[0, 0]) == v
    px = np.zeros((1, 3, 3), np.uint8)
    px[0, 0, 0] = px[0, 1, 1] = px[0, 2, 2] = 255                      # pure B, G, R
    assert chr_.luma(px)[0].tolist() == [(29 * 255 + 128) >> 8, (150 * 255 + 128) >> 8, (77 * 255 + 128) >> 8] == [29, 149, 77]


def test_constant_frame_first_then_no_activity():
    cfg = Config(cell=32, window_w=64, window_h=64)
    out, rec, _ = _run([cs.gray(70, 40, 9)] * 2, cfg)
    (h0, p0, a0), (h1, p1, a1) = out
    assert (int(h0["n_cells"]), int(h0["gw"]), int(h0["gh"]), int(h0["flags"]), int(h0["step"]), int(h0["n_active"]), int(h0["n_peaks"])) == (6, 3, 2, chr_.FIRST, 1, 0, 0)
    assert (int(h1["flags"]), int(h1["step"]), int(h1["n_active"]), int(h1["n_peaks"])) == (0, 2, 0, 0) and not a0.any() and not a1.any()
    S, npix = chr_.sums(cs.gray(70, 40, 9), 32)
    assert npix.tolist() == [[1024, 1024, 192], [256, 256, 48]] and (S == 9 * npix).all()


def test_a_block_moved_gives_two_equal_peaks_lowest_index_first():
    cfg = Config(cell=32, threshold_q4=32, max_active_permille=500, max_peaks=3, window_w=20, window_h=20)
    f0, f1 = cs.gray(96, 64), cs.gray(96, 64)
    f0[10:22, 10:22] = 255                                             # 12 x 12 in cell (0, 0)
    f1[10:22, 40:52] = 255                                             # ... moved into cell (1, 0)
    (_, (h, peaks, A)), rec, _ = _run([f0, f1], cfg)
    assert A.tolist() == [[36720, 36720, 0], [0, 0, 0]] and int(h["n_active"]) == 2 and int(h["flags"]) == 0
    # cell 0: centre (16, 16), window origin 16 - 10 = 6; cell 1: centre (48, 16), origin 38
    assert peaks == [(6, 6, 20, 20, 0, 0, 36720), (38, 6, 20, 20, 1, 0, 36720)]
    got = rec[32:96].view(chr_.PEAK_DTYPE)
    assert [tuple(int(v) for v in r)[:7] for r in got] == peaks and not rec[96:128].any()        # the third peak record is untouched


def test_the_largest_activity_and_the_threshold_at_equality():
    # a whole cell of 64 x 64 going 0 -> 255: A = 4096 * 255, and 16 * A == 4080 * 4096 exactly: not active at the largest threshold
    frames = [cs.gray(64, 64, 0), cs.gray(64, 64, 255)]
    (_, (h, peaks, A)), _, _ = _run(frames, Config(cell=64, threshold_q4=4080, max_active_permille=1000, window_w=64, window_h=64))
    assert int(A[0, 0]) == 1044480 and int(h["n_active"]) == 0 and peaks == []
    (_, (h, peaks, A)), _, _ = _run(frames, Config(cell=64, threshold_q4=4079, max_active_permille=1000, window_w=64, window_h=64))
    assert int(h["n_active"]) == 1 and peaks == [(0, 0, 64, 64, 0, 0, 1044480)]
    # one pixel of an 8 x 8 cell: 16 * 128 == 32 * 64 is not active, 129 is
    for v, want in ((128, 0), (129, 1)):
        f1 = cs.gray(8, 8, 0)
        f1[3, 4] = v
        (_, (h, peaks, A)), _, _ = _run([cs.gray(8, 8, 0), f1], Config(cell=8, threshold_q4=32, max_active_permille=1000, window_w=8, window_h=8))
        assert int(A[0, 0]) == v and int(h["n_active"]) == want == len(peaks)


def test_global_at_equality_and_one_above():
    cfg = Config(cell=32, threshold_q4=0, max_active_permille=250, window_w=32, window_h=32)
    f0 = cs.gray(64, 64, 0)
    f1, f2 = f0.copy(), f0.copy()
    f1[0, 0] = 255                                                     # one of four cells: 1000 > 1000 is false
    f2[0, 0] = f2[0, 40] = 255                                         # two: 2000 > 1000
    (_, (h, peaks, A)), _, _ = _run([f0, f1], cfg)
    assert (int(h["n_active"]), int(h["flags"]), len(peaks)) == (1, 0, 1)
    (_, (h, peaks, A)), rec, _ = _run([f0, f2], cfg)
    assert (int(h["n_active"]), int(h["flags"]), len(peaks)) == (2, chr_.GLOBAL, 0)
    assert rec[chr_.layout(cfg)[2]:][:16].view(np.uint32).tolist() == [255, 255, 0, 0]            # the activity grid is still written


def test_first_geometry_change_and_reset():
    cfg = Config(cell=16, threshold_q4=0, max_active_permille=1000, window_w=16, window_h=16)
    s, rec = chr_.Stream(), _rec(cfg)
    a, b = cs.gray(32, 32, 0), cs.gray(32, 32, 200)
    flags = [int(s.frame(f, c, rec)[0]["flags"]) for f, c in ((a, cfg), (b, cfg), (cs.gray(33, 32, 0), cfg), (cs.gray(33, 32, 9), cfg),
                                                             (cs.gray(33, 32, 0), Config(cell=8, threshold_q4=0, max_active_permille=1000, window_w=16, window_h=16)))]
    assert flags == [chr_.FIRST, 0, chr_.FIRST, 0, chr_.FIRST] and s.step == 5
    s.reset()
    h, peaks, A = s.frame(a, cfg, rec)
    assert int(h["flags"]) == chr_.FIRST and int(h["step"]) == 1 and peaks == [] and not A.any()


def test_windows_of_two_pixels_leave_their_own_centre_outside_and_the_loop_ends():
    cfg = Config(cell=32, threshold_q4=0, max_active_permille=1000, max_peaks=15, window_w=2, window_h=2)
    f0, f1 = cs.gray(64, 64, 0), cs.gray(64, 64, 0)
    for k, (y, x) in enumerate(((1, 1), (1, 33), (33, 1), (33, 33))):
        f1[y, x] = 10 + k                                              # four active cells, A = 10, 11, 12, 13
    (_, (h, peaks, A)), _, _ = _run([f0, f1], cfg)
    # centre 16 -> origin 15 & ~1 = 14: the window [14, 16) does not hold pixel 16; each peak cell is removed all the same
    assert peaks == [(46, 46, 2, 2, 1, 1, 13), (14, 46, 2, 2, 0, 1, 12), (46, 14, 2, 2, 1, 0, 11), (14, 14, 2, 2, 0, 0, 10)]


def test_a_peak_in_the_last_column_with_an_odd_difference():
    cfg = Config(cell=32, threshold_q4=0, max_active_permille=1000, max_peaks=2, window_w=40, window_h=40)
    f0, f1 = cs.gray(101, 77, 0), cs.gray(101, 77, 0)
    f1[5, 100] = 50                                                    # cell (3, 0): centre min(112, 100) = 100; xmax = 61 & ~1 = 60: the window ends at 100
    (_, (h, peaks, A)), _, _ = _run([f0, f1], cfg)
    assert peaks == [(60, 0, 40, 40, 3, 0, 50)]


def test_fewer_and_more_peaks_than_max_peaks_and_the_suppression():
    f0, f1 = cs.gray(128, 32, 0), cs.gray(128, 32, 0)
    for cx, v in enumerate((40, 90, 20, 70)):
        f1[3, 32 * cx + 3] = v
    base = dict(cell=32, threshold_q4=0, max_active_permille=1000, window_w=32, window_h=32)
    (_, (h, peaks, A)), _, _ = _run([f0, f1], Config(max_peaks=2, **base))
    assert [(p[4], p[6]) for p in peaks] == [(1, 90), (3, 70)] and int(h["n_active"]) == 4
    (_, (h, peaks, A)), _, _ = _run([f0, f1], Config(max_peaks=9, **base))
    assert [(p[4], p[6]) for p in peaks] == [(1, 90), (3, 70), (0, 40), (2, 20)]
    # windows of 66: around cell 1 (centre 48 -> origin 15 & ~1 = 14) [14, 80) holds the centres 16 and 48; around cell 3 (centre 112 -> clamped to
    # xmax = 62) [62, 128) holds 80 and 112: two peaks remove all four cells
    (_, (h, peaks, A)), _, _ = _run([f0, f1], Config(max_peaks=9, **dict(base, window_w=66)))
    assert [(p[0], p[4]) for p in peaks] == [(14, 1), (62, 3)]
    # the initial suppression: a rectangle over the centres of cells 1 and 3
    (_, (h, peaks, A)), _, _ = _run([f0, f1], Config(max_peaks=9, **base), suppress=[(40, 0, 20, 32), (100, 10, 20, 10)])
    assert [p[4] for p in peaks] == [0, 2] and int(h["n_active"]) == 4


def test_the_fill_takes_fallbacks_in_region_order():
    plan = np.zeros(4, dtype=[("x0", "<i4"), ("y0", "<i4"), ("w", "<i4"), ("h", "<i4"), ("slot", "<i4"), ("track_id", "<u4")])
    plan["slot"], plan["track_id"], plan["x0"] = [5, -1, 9, -1], [7, 0, 8, 0], [1, 2, 3, 4]
    out = chr_.fill(plan, [(10, 20, 8, 8, 0, 0, 5)])
    assert out["slot"].tolist() == [5, -2, 9, -1] and out["x0"].tolist() == [1, 10, 3, 4] and out["y0"].tolist() == [0, 20, 0, 0]
    out = chr_.fill(plan, [(10, 20, 8, 8, 0, 0, 5), (30, 40, 8, 8, 1, 1, 4), (50, 60, 8, 8, 2, 2, 3)])
    assert out["slot"].tolist() == [5, -2, 9, -2] and out["x0"].tolist() == [1, 10, 3, 30]
    assert chr_.track_rects(plan) == [(1, 0, 0, 0), (3, 0, 0, 0)]


@pytest.mark.parametrize("w,h", cs.SIZES)
def test_every_size_and_cell(w, h):
    """the grid's shape and pixel counts, the sums against a per-pixel loop, and identical frames giving n_active = 0"""
    bgr = np.random.default_rng(w * 1000 + h).integers(0, 256, (h, w, 3), dtype=np.uint8)
    Y = chr_.luma(bgr)
    for C in cs.CELLS:
        S, npix = chr_.sums(bgr, C)
        gw, gh = chr_.grid(w, h, C)
        assert S.shape == (gh, gw) == ((h + C - 1) // C, (w + C - 1) // C) and int(npix.sum()) == w * h and int(S.sum()) == int(Y.sum())
        if w * h <= 101 * 77:
            want = np.zeros((gh, gw), dtype=np.int64)
            for y in range(h):
                for x in range(w):
                    want[y // C, x // C] += int(Y[y, x])
            assert (want == S).all()
        cfg = Config(cell=C, threshold_q4=0, max_active_permille=0, window_w=8, window_h=8)
        (_, (hd, peaks, A)), _, _ = _run([bgr, bgr], cfg)
        assert int(hd["n_active"]) == 0 and int(hd["flags"]) == 0 and not A.any()
