"""The camera motion oracle (tests/camera_ref.py) against ground truth: frames cut from one canvas at offsets that differ by a known shift
(tests/camera_cases.py), hand cases of every flag, and the composition with the tracking oracle (tests/track_ref.py) on a panning scene.  CPU only."""
import numpy as np
import pytest

import camera_cases as cs
import camera_ref as cam
import change_ref
import track_cases
import track_ref

NEVER_LOST = 4080            # 16 * SAD <= 16 * 255 * npix: no frame is LOST at this setting


def _rec():
    return np.zeros(cam.REC_BYTES, dtype=np.uint8)


def _pair(W, H, cfg, shift, block, seed):
    """the header of the second of two frames that differ by `shift`"""
    f0, f1 = cs.pan(W, H, [shift], block, seed)
    s, rec = cam.Stream(), _rec()
    assert int(s.frame(f0, cfg, rec)["flags"]) == cam.FIRST
    return s.frame(f1, cfg, rec), s, rec


@pytest.mark.parametrize("W,H,C", [(640, 360, 8), (320, 208, 16)])
def test_whole_cell_shifts_inside_the_radius_are_recovered_exactly(W, H, C):
    """sizes that are multiples of C: a partial last column or row of the PREVIOUS grid, which the candidates at -R reach, holds fewer pixels than
    the whole cell it is compared with, and the match there is not exact"""
    cfg = cam.Config(cell=C, radius=4, max_residual_q4=0)                 # an exact match has no residual at all
    for k, (dx, dy) in enumerate(((0, 0), (1, 0), (0, -1), (-3, 2), (3, 3), (-2, -3), (4, 0), (-4, 4), (2, -4))):
        h, s, _ = _pair(W, H, cfg, (dx * C, dy * C), 1 + 3 * (k % 2), seed=k)
        clipped = cam.CLIPPED if max(abs(dx), abs(dy)) == 4 else 0
        assert (int(h["dx"]), int(h["dy"]), int(h["fx"]), int(h["fy"]), int(h["flags"])) == (dx, dy, 0, 0, clipped), (dx, dy, h)
        assert (int(h["sx_q4"]), int(h["sy_q4"])) == (16 * dx * C, 16 * dy * C) and int(h["sad_min"]) == 0
        assert s.pend == [16 * dx * C, 16 * dy * C]


ERRORS = {}


@pytest.mark.parametrize("W,H,C,trials", [(1920, 1080, 16, 6), (640, 360, 8, 16)])
@pytest.mark.parametrize("block", [1, 4])
def test_arbitrary_integer_shifts_are_recovered_to_a_quarter_cell(W, H, C, trials, block):
    """|shift| <= (R - 1) * C per axis; the bound C / 4 is twice what a numpy prototype of the rule measured (C / 8 in 120 trials on such canvases).
    The maximum over this committed case set is printed, for DESIGN.md section 5"""
    cfg = cam.Config(cell=C, radius=4, max_residual_q4=NEVER_LOST)
    rng = np.random.default_rng(1000 * C + block)
    worst = 0.0
    for k in range(trials):
        sx, sy = (int(v) for v in rng.integers(-3 * C, 3 * C + 1, 2))
        h, _, _ = _pair(W, H, cfg, (sx, sy), block, seed=100 * C + 10 * block + k)
        ex, ey = abs(int(h["sx_q4"]) / 16 - sx), abs(int(h["sy_q4"]) / 16 - sy)
        worst = max(worst, ex / C, ey / C)
        assert ex <= C / 4 and ey <= C / 4 and not int(h["flags"]) & cam.LOST, (sx, sy, h)
    ERRORS[(W, H, C, block)] = worst
    print(f"camera shift error, {W} x {H}, C = {C}, block {block}: max {worst:.4f} cells over {trials} trials")


def test_a_flat_frame_and_an_unchanged_frame_give_zero():
    cfg = cam.Config(cell=8, radius=3, max_residual_q4=0)
    s, rec = cam.Stream(), _rec()
    s.frame(cs.gray(104, 96, 77), cfg, rec)                               # 13 x 12 whole cells: the previous grid has no partial cell to differ by
    h = s.frame(cs.gray(104, 96, 77), cfg, rec)
    assert (int(h["dx"]), int(h["dy"]), int(h["fx"]), int(h["fy"]), int(h["flags"]), int(h["sad_min"])) == (0, 0, 0, 0, 0, 0)
    h = s.frame(cs.gray(104, 96, 80), cfg, rec)                           # every candidate has the same SAD: (0, 0) is least in the order
    tab = rec[cam.HDR_BYTES:cam.HDR_BYTES + 8 * 49].view(np.uint64)
    assert (int(h["dx"]), int(h["dy"]), int(h["fx"]), int(h["fy"])) == (0, 0, 0, 0) and (tab == tab[0]).all() and tab[0] == 3 * 64 * 7 * 6
    assert int(h["flags"]) == cam.LOST and s.pend == [0, 0]               # three levels per pixel against a residual of none
    pic = cs.canvas(100, 90, 0, 1, seed=3)
    s.frame(pic, cfg, rec)
    h = s.frame(pic, cfg, rec)
    assert (int(h["dx"]), int(h["dy"]), int(h["sad_min"]), int(h["sad_zero"]), int(h["flags"])) == (0, 0, 0, 0, 0)


def test_unrelated_frames_are_lost_and_leave_the_pending_shift_alone():
    cfg = cam.Config(cell=8, radius=4, max_residual_q4=16)                # one luma level per pixel
    f0, f1 = cs.pan(640, 360, [(16, -8)], 4, seed=5)
    other = cs.canvas(640, 360, 0, 4, seed=6)
    s, rec = cam.Stream(), _rec()
    s.frame(f0, cfg, rec)
    s.frame(f1, cfg, rec)
    assert s.pend == [256, -128] and s.n_lost == 0
    h = s.frame(other, cfg, rec)
    assert int(h["flags"]) & cam.LOST and s.pend == [256, -128] and (int(h["pend_x_q4"]), int(h["pend_y_q4"]), int(h["n_lost"])) == (256, -128, 1)
    assert 16 * int(h["sad_min"]) > 16 * (80 - 8) * (45 - 8) * 64
    h = s.frame(other, cfg, rec)                                          # ... and the stream goes on from the new picture
    assert int(h["flags"]) == 0 and int(h["step"]) == 4 and s.pend == [256, -128]


def test_first_on_a_geometry_change_zeroes_the_pending_shift_and_leaves_the_table():
    cfg = cam.Config(cell=8, radius=2, max_residual_q4=NEVER_LOST)
    f0, f1 = cs.pan(96, 64, [(8, 8)], 1, seed=7)
    s, rec = cam.Stream(), _rec()
    rec[:] = 0xEE
    s.frame(f0, cfg, rec)
    assert (rec[cam.HDR_BYTES:] == 0xEE).all() and not rec[80:96].any()  # FIRST: no table; the padding is zero
    s.frame(f1, cfg, rec)
    assert s.pend == [128, 128] and (rec[cam.HDR_BYTES + 8 * 25:] == 0xEE).all()
    table = rec[cam.HDR_BYTES:].copy()
    h = s.frame(cs.canvas(104, 64, 0, 1, seed=8), cfg, rec)               # another width
    assert int(h["flags"]) == cam.FIRST and s.pend == [0, 0] and (int(h["pend_x_q4"]), int(h["step"]), int(h["gw"])) == (0, 3, 13)
    assert np.array_equal(rec[cam.HDR_BYTES:], table)
    h = s.frame(cs.canvas(104, 64, 0, 1, seed=8), cam.Config(cell=16, radius=1, max_residual_q4=0), rec)      # another cell
    assert int(h["flags"]) == cam.FIRST
    s.reset(rec)
    assert int(s.frame(cs.canvas(104, 64, 0, 1, seed=8), cam.Config(cell=16, radius=1, max_residual_q4=0), rec)["step"]) == 1


def test_the_pending_shift_accumulates_over_three_frames_and_an_apply_takes_it():
    cfg = cam.Config(cell=8, radius=4, max_residual_q4=NEVER_LOST)
    shifts = [(8, 0), (-16, 24), (11, -5)]
    frames = cs.pan(640, 360, shifts, 1, seed=9)
    s, rec = cam.Stream(), _rec()
    total = [0, 0]
    for k, f in enumerate(frames):
        h = s.frame(f, cfg, rec)
        if k:
            total = [total[0] + int(h["sx_q4"]), total[1] + int(h["sy_q4"])]
        assert s.pend == total and (int(h["pend_x_q4"]), int(h["pend_y_q4"])) == tuple(total)
    assert abs(total[0] / 16 - 3) <= 2 and abs(total[1] / 16 - 19) <= 2
    x, y, live = np.array([0.5, 0.25], np.float32), np.array([0.5, 0.75], np.float32), [True, False]
    nx, ny = s.apply(x, y, live, rec)
    assert nx == np.float32(np.float32(total[0]) / np.float32(16 * 640)) and ny == np.float32(np.float32(total[1]) / np.float32(16 * 360))
    assert x[0] == np.float32(np.float32(0.5) + nx) and (x[1], y[1]) == (0.25, 0.75)
    h = rec[:96].view(cam.HDR_DTYPE)[0]
    assert s.pend == [0, 0] and (int(h["pend_x_q4"]), int(h["pend_y_q4"]), int(h["n_applied"])) == (0, 0, 1)
    assert cam.Stream().apply(x, y, live) is None                         # no geometry: skipped whole


def test_sads_above_two_to_the_32():
    """6144 x 4096 at C = 64, all white then all black: every cell differs by 64 * 64 * 255, every candidate's SAD is 88 * 56 times that"""
    cell = int(change_ref.sums(cs.gray(64, 64, 255), 64)[0][0, 0])
    assert cell == 64 * 64 * 255
    cfg = cam.Config(cell=64, radius=4, max_residual_q4=NEVER_LOST)
    s, rec = cam.Stream(), _rec()
    s.frame_sums(np.full((64, 96), cell, np.uint32), 6144, 4096, cfg, rec)
    h = s.frame_sums(np.zeros((64, 96), np.uint32), 6144, 4096, cfg, rec)
    tab = rec[cam.HDR_BYTES:cam.HDR_BYTES + 8 * 81].view(np.uint64)
    assert int(tab[0]) == cell * 88 * 56 > 1 << 32 and (tab == tab[0]).all()
    assert (int(h["dx"]), int(h["dy"]), int(h["fx"]), int(h["fy"]), int(h["flags"])) == (0, 0, 0, 0, 0) and int(h["sad_min"]) == cell * 88 * 56


# ---- composition with the tracking oracle ------------------------------------------------------------------------------------------
PAN_W, PAN_H, PAN = 640, 360, (24, 8)                 # 24 px = 0.0375 of the width per frame: more than the boxes are wide
PAN_CFG = cam.Config(cell=8, radius=4, max_residual_q4=NEVER_LOST)
PAN_BOXES = ((0.30, 0.40, 0.03, 0.05), (0.45, 0.55, 0.03, 0.05), (0.60, 0.30, 0.03, 0.05))


def pan_scene(steps=6):
    """-> (frames [BGR], detections per frame): three boxes that ride on the canvas"""
    frames = cs.pan(PAN_W, PAN_H, [PAN] * steps, 1, seed=11)
    dets = [track_cases.dets([(np.float32(x + k * PAN[0] / PAN_W), np.float32(y + k * PAN[1] / PAN_H), w, h) for x, y, w, h in PAN_BOXES]) for k in range(steps + 1)]
    return frames, dets


def pan_ids(frames, dets, apply, cap=8, max_tracks=8):
    """the CPU composition: per frame the camera oracle, the apply step (or not), the tracking oracle -> ids per frame"""
    s, rec, tr = cam.Stream(), _rec(), track_ref.Tracker(max_tracks, cap)
    out = []
    for f, d in zip(frames, dets):
        s.frame(f, PAN_CFG, rec)
        if apply:
            s.apply_tracker(tr)
        out.append(tr.step(d).tolist())
    return out


def test_ids_persist_under_a_pan_with_the_apply_step_and_not_without():
    frames, dets = pan_scene()
    with_apply, without = pan_ids(frames, dets, True), pan_ids(frames, dets, False)
    assert all(ids == [1, 2, 3] for ids in with_apply), with_apply
    assert without == [[3 * k + 1, 3 * k + 2, 3 * k + 3] for k in range(7)], without
