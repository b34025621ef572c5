"""Moves inside resident surfaces on the GPU (include/zly.h "Resident surfaces", MOVES; csrc/kernels_surface.hip: surface_move_kernel).

The store's bytes, bit for bit, against tests/surface_move_ref.py through zly_surface_read, in the mirror of the whole store that
tests/test_gpu_surface.py keeps -- every byte of every slot, slack and neighbours included: every source / destination alignment of a BGR row,
overlap in every direction by one step and by all but one, destinations that share 16-byte granules, every format family, heights on either side
of the kernel's band size and rows longer than a band, the most moves a call takes, a dependent chain, a call over several surfaces, one large
surface.  Then ordering against updates and against detect calls on callers' streams, and the detection rule: zly_detect_surfaces after moves
equals zly_detect_device_view on the oracle's frames uploaded whole."""
import numpy as np
import pytest
import torch            # before the first engine: the process then uses torch's HIP runtime throughout, as tests/test_gpu_parity.py does

import surface_move_ref as mr
import surface_ref as sr
import test_gpu_surface as tgs
import zly
import zly_model as zm
from oracle_lib import det_fields_equal

pytestmark = pytest.mark.gpu

BGR, BGRA, NV12, I420, YUY2 = zly.PIX_BGR, zly.PIX_BGRA, zly.PIX_NV12_BT601, zly.PIX_I420_BT709, zly.PIX_YUY2_BT601
BAND, SLOTS, EACH, BIG_W, BIG_H = tgs.BAND, tgs.SLOTS, tgs.EACH, tgs.BIG_W, tgs.BIG_H
MODES = {"stretch": 0, "letterbox": zly.FLAG_LETTERBOX}
_ENGINES = {}


@pytest.fixture(scope="module")
def engine_for(weights_path):
    """one engine per resize mode, shared by the module, with a store of test_gpu_surface's geometry (its Mirror reads whole slots) and moves enabled"""
    def get(mode):
        if mode not in _ENGINES:
            e = zly.Engine(weights_path, dtype=zly.DTYPE_BF16, max_batch=4, max_dets=64, conf_thr=0.05, warmup_runs=0, flags=MODES[mode])
            e.surfaces_enable(SLOTS, EACH if mode == "stretch" else 640 * 480 * 4)
            e.surface_moves_enable(0)
            _ENGINES[mode] = e
        return _ENGINES[mode]
    yield get
    for e in _ENGINES.values():
        e.close()
    _ENGINES.clear()


class Mirror(tgs.Mirror):
    def move(self, moves):
        """moves: (s, sx, sy, dx, dy, w, h), one call"""
        self.e.surface_move(moves)
        for s, *m in moves:
            fmt, w, h = self.shape[s]
            mr.apply_moves(self.full[s], fmt, w, h, [tuple(m)])


def _steps(fmt):
    _, _, ex, ey = sr.FORMATS[fmt]
    return (2 if ex else 1), (2 if ey else 1)


def _overlap_set(fmt):
    """a 12 x 10 block at (12, 10) moved up, down, left, right and diagonally, by one step of the format and by all but one"""
    stx, sty = _steps(fmt)
    out = []
    for far in (False, True):
        kx, ky = (12 - stx, 10 - sty) if far else (stx, sty)
        for ux, uy in ((-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1)):
            out.append((12, 10, 12 + ux * kx, 10 + uy * ky, 12, 10))
    assert all(mr.self_overlaps(m) and not mr.identity(m) for m in out)
    return out


def test_every_alignment_of_source_and_destination(engine_for):
    """BGR 37 x 29, a 5 x 3 block: every dx - sx from -16 to 16 at every dx mod 16.  A pixel is 3 bytes and a row 111, so this is every difference of
    source and destination alignment mod 16 at every destination alignment, and every head / body / tail shape of a 15-byte row"""
    e = engine_for("stretch")
    m = Mirror(e)
    m.define(1, BGR, 37, 29)
    m.keyframe(1, 100)
    seen = set()
    for delta in range(-16, 17):
        call = []
        for r in range(16):
            dx = r + 16 if delta >= 0 else r
            sx = dx - delta
            sy = (5 * r) % 27
            dy = sy if delta % 2 == 0 else (sy + 7) % 27
            call.append((1, sx, sy, dx, dy, 5, 3))
            seen.add((delta, dx % 16))
        m.move(call)
        m.check(1)
    assert len(seen) == 33 * 16
    m.check_all()


def test_overlap_in_every_direction_and_shared_granules(engine_for):
    e = engine_for("stretch")
    m = Mirror(e)
    m.define(1, BGR, 37, 29)
    m.keyframe(1, 200)
    for mv in _overlap_set(BGR):
        m.move([(1,) + mv])
        m.check(1)
    # destinations 1 to 5 pixels wide that tile [20, 36) x [1, 28): neighbours share 16-byte granules with each other and with the untouched columns
    # 19 and 36; the sources lie 19 pixels to the left, so no move depends on another: one launch.  Then every second one only
    board = tgs._checkerboard(37, 29, 20, 36, 1, 28)
    assert len(board) > 50 and {r[2] for r in board} == {1, 2, 3, 4, 5}
    moves = [(x - 19, y, x, y, rw, rh) for x, y, rw, rh in board]
    assert not any(mr.conflicts(a, b) for i, a in enumerate(moves) for b in moves[i + 1:]) and not any(mr.self_overlaps(a) for a in moves)
    m.keyframe(1, 201)
    m.move([(1,) + mv for mv in moves])
    m.check(1)
    for phase in (0, 1):
        m.keyframe(1, 202 + phase)
        m.move([(1,) + mv for mv in moves[phase::2]])
        m.check(1)
    # ... and overlapping moves side by side: both go through the bounce buffer and come back into neighbouring granules
    m.move([(1, 3, 3, 4, 4, 5, 9), (1, 9, 3, 10, 2, 5, 9), (1, 15, 3, 14, 4, 3, 9)])
    m.check(1)
    m.check_all()


@pytest.mark.parametrize("fmt,w,h", [(BGRA, 40, 30), (NV12, 38, 30), (I420, 38, 30), (YUY2, 38, 29)])
def test_formats(engine_for, fmt, w, h):
    e = engine_for("stretch")
    m = Mirror(e)
    m.define(2, fmt, w, h)
    m.keyframe(2, 300 + fmt)
    stx, sty = _steps(fmt)
    for mv in _overlap_set(fmt):
        m.move([(2,) + mv])
        m.check(2)
    m.move([(2, 0, 0, w - 6 * stx, h - 4 * sty, 6 * stx, 4 * sty), (2, w - 2 * stx, 0, 0, h - 2 * sty, 2 * stx, 2 * sty)])      # clear of themselves, corner to corner
    m.check(2)
    m.move([(2,) + mv for mv in _overlap_set(fmt)])                              # all sixteen in one call: a chain of phases
    m.check(2)
    m.check_all()


def test_heights_around_the_band_size_and_rows_longer_than_a_band(engine_for):
    e = engine_for("stretch")
    m = Mirror(e)
    for s, (fmt, w, bpp) in enumerate(((BGRA, 40, 4), (BGR, 37, 3), (BGRA, 64, 4)), start=1):
        per = BAND // (bpp * w)
        assert per >= 2
        m.define(s, fmt, w + 3, 2 * per + 4)
        m.keyframe(s, 400 + s)
        for rh in (per - 1, per, per + 1):
            m.move([(s, 1, 1, 2, 2, w, rh)])                                     # overlaps itself: gathered and scattered
            m.move([(s, 1, 0, 2, rh + 1, w, rh)])                                # clear of itself: store -> store
            m.check(s)
    wide, high = 4100, 12
    assert 4 * wide > BAND
    m.define(4, BGRA, wide, high)
    m.keyframe(4, 404)
    m.move([(4, 0, 0, 1, 1, wide - 1, high - 1)])
    m.check(4)
    m.move([(4, 0, 0, 0, 6, wide, 6), (4, 3, 2, 0, 5, wide - 3, 2)])
    m.check(4)
    m.check_all()


def test_call_sizes(engine_for):
    e = engine_for("stretch")
    m = Mirror(e)
    for s in range(SLOTS):
        m.define(s, BGR, 37, 29)
        m.keyframe(s, 500 + s)
    # the most a call takes, all independent: pixels of even rows go one row down
    cells = [(s, x, y, x, y + 1, 1, 1) for y in range(0, 28, 2) for x in range(37) for s in range(SLOTS)]
    assert len(cells) >= zly.SURFACE_MAX_MOVES + 1
    with pytest.raises(zly.ZlyError) as ei:
        e.surface_move(cells[:zly.SURFACE_MAX_MOVES + 1])
    assert ei.value.code == zly.ERR_INVALID_ARGUMENT
    m.check(*range(SLOTS))
    m.move(cells[:zly.SURFACE_MAX_MOVES])
    m.check(*range(SLOTS))
    # a chain of 64 moves of which each reads what the one before it wrote (and overlaps itself): a 3 x 3 block walks 64 pixels
    path = [(i, 0) for i in range(33)] + [(32, j) for j in range(1, 17)] + [(32 - k, 16) for k in range(1, 17)]
    assert len(path) == 65
    m.move([(3, ax, ay, bx, by, 3, 3) for (ax, ay), (bx, by) in zip(path, path[1:])])
    m.check(3)
    m.check_all()
    # one call over five surfaces of five formats
    for s, (fmt, w, h) in tgs.SMALL.items():
        m.define(s, fmt, w, h)
        m.keyframe(s, 510 + s)
    call = []
    for k, mv in enumerate(_overlap_set(NV12)):                                  # even everywhere: legal for every format
        call += [(s,) + mv for s in tgs.SMALL if (s + k) % 2]
    m.move(call)
    m.check(*tgs.SMALL)
    m.check_all()


def test_one_large_surface(engine_for):
    """1920 x 1080 BGRA: scrolled by one row and by 40 rows (8 MB through the bounce buffer), and a 640 x 480 block moved clear of itself"""
    e = engine_for("stretch")
    m = Mirror(e)
    m.define(2, BGRA, BIG_W, BIG_H)
    m.keyframe(2, 600)
    m.move([(2, 0, 1, 0, 0, BIG_W, BIG_H - 1)])
    m.check(2)
    m.move([(2, 0, 0, 0, 40, BIG_W, BIG_H - 40)])
    m.check(2)
    m.move([(2, 100, 100, 900, 500, 640, 480)])
    m.check(2)
    m.check_all()


def test_move_then_update_then_read_without_a_synchronise(engine_for):
    e = engine_for("stretch")
    m = Mirror(e)
    m.define(1, BGRA, 640, 480)
    m.keyframe(1, 700)
    rng = np.random.default_rng(7)
    for k in range(4):
        m.move([(1, 0, 40, 0, 0, 640, 440), (1, 10, 450, 300, 445, 100, 20)])      # the scroll, then a block that lands on rows the scroll read: two phases
        m.update([(1, 0, 440, 640, 40, tgs._rnd(rng, BGRA, 640, 40)), (1, 5, 5, 9, 9, tgs._rnd(rng, BGRA, 9, 9))])      # the dirty rectangles, on top of the moves
    m.check(1)
    m.check_all()


def _uploaded(e, frames, views_of, tag0):
    """zly_detect_device_view on the frames uploaded whole into one buffer; views_of(i, tight view with offsets) -> the view to detect"""
    offs = np.cumsum([0] + [(f.size + 255) // 256 * 256 for f, _ in frames])
    host = np.zeros(int(offs[-1]), dtype=np.uint8)
    views = []
    for i, (f, (fmt, w, h)) in enumerate(frames):
        host[offs[i]:offs[i] + f.size] = f
        v = zly.view_tight(fmt, w, h)
        for p in range(3):
            v.off[p] += int(offs[i])
        views.append(views_of(i, v))
    d_host = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    e.detect_device_view(d_host.data_ptr(), host.nbytes, views, tag0=tag0)
    return e.read_slabs(len(frames))


@pytest.mark.parametrize("mode", list(MODES))
def test_detecting_after_moves_is_detecting_on_the_oracles_frames_uploaded_whole(engine_for, mode):
    e = engine_for(mode)
    W, H = 640, 480
    streams = (BGR, NV12, YUY2) if mode == "stretch" else (BGRA,)
    n = len(streams)
    frames = []
    for i, fmt in enumerate(streams):
        bgr = zm.synth_frames(1, W, H, seed=800 + i)[0]
        f = np.ascontiguousarray(np.concatenate([bgr, np.full((H, W, 1), 255, np.uint8)], axis=2)).reshape(-1) if fmt == BGRA else tgs._as_format(fmt, bgr)
        frames.append(f.copy())
        e.surface_define(i, fmt, W, H)
    e.surface_update([(i, 0, 0, frames[i], zly.view_tight(fmt, W, H)) for i, fmt in enumerate(streams)])
    calls = [[(0, 24, 0, 0, W, H - 24)],                                          # a scroll up
             [(0, 0, 16, 0, W - 16, H), (32, 40, 330, 200, 240, 200)],            # a scroll right, then a window dragged clear of itself
             [(100, 60, 140, 90, 300, 260)]]                                      # a window dragged across itself
    rois = [(160, 120, 320, 240), (0, 0, 416, 416), (224, 64, 416, 416)]
    total_kept = 0
    for step, call in enumerate(calls if mode == "stretch" else calls[1:2]):
        e.surface_move([(i,) + mv for i in range(n) for mv in call])
        for i, fmt in enumerate(streams):
            mr.apply_moves(frames[i], fmt, W, H, call)
        e.detect_surfaces(list(range(n)), tag0=10 * step)
        got = e.read_slabs(n)
        described = [(frames[i], (fmt, W, H)) for i, fmt in enumerate(streams)]
        want = _uploaded(e, described, lambda i, v: v, 10 * step)
        assert tgs._slabs_equal(got, want), (mode, step)
        total_kept += sum(int(h["n_kept"]) for h, _ in want)
        e.detect_surfaces(list(range(n)), rois=[rois[(i + step) % 3] for i in range(n)], tag0=10 * step + 5)
        got = e.read_slabs(n)
        want = _uploaded(e, described, lambda i, v: zly.view_crop(v, *rois[(i + step) % 3]), 10 * step + 5)
        assert tgs._slabs_equal(got, want), (mode, step, "rois")
        for i in range(n):
            assert np.array_equal(e.surface_read(i, frames[i].size), frames[i]), (mode, step, i)
    assert total_kept >= 1, total_kept             # the comparison is not one of empty lists


def test_detect_move_detect_on_callers_streams_without_a_synchronise(engine_for):
    """detect k on a CALLER's stream, move k + 1 on the engine's, detect k + 1 on another caller's stream, ... with nothing but enqueues in between.
    A move kernel that overtook the detect call before it would hand that call the scrolled picture (or a torn one); a detect call that overtook
    the move kernel before it, the picture not yet scrolled.  Each step's slab must be the slab of its own picture uploaded whole."""
    e = engine_for("stretch")
    W, H, steps = 960, 540, 6
    bgr = zm.synth_frames(1, W, H, seed=900)[0]
    frame = np.ascontiguousarray(np.concatenate([bgr, np.full((H, W, 1), 255, np.uint8)], axis=2)).reshape(-1)
    whole = zly.view_tight(BGRA, W, H)
    sb = e.slab_bytes
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    d_slabs = torch.zeros(steps * sb, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    e.surface_define(0, BGRA, W, H)
    e.surface_update([(0, 0, 0, frame, whole)])
    pictures = []
    for k in range(steps):
        if k:
            mv = (0, 36, 48, 0, W - 48, H - 36)                                   # the picture slides right and up, across itself
            e.surface_move([(0,) + mv])
            mr.apply_moves(frame, BGRA, W, H, [mv])
        pictures.append(frame.copy())
        e.detect_surfaces([0], d_slabs_ptr=d_slabs.data_ptr() + k * sb, tag0=k, stream=streams[k % 2].cuda_stream)
    for s in streams:
        s.synchronize()
    e.sync()
    got = zly.parse_slabs(d_slabs.cpu().numpy(), steps, e.max_dets)
    want = []
    for k in range(steps):
        d = torch.from_numpy(pictures[k]).cuda()
        torch.cuda.synchronize()
        e.detect_device_view(d.data_ptr(), pictures[k].nbytes, [whole], tag0=k)
        want.append(e.read_slabs(1)[0])
    assert tgs._slabs_equal(got, want)
    # the pictures tell each other apart: a call that saw its neighbour's picture would have failed above
    assert all(len(want[k][1]) > 0 and not (len(want[k][1]) == len(want[k + 1][1]) and det_fields_equal(want[k][1], want[k + 1][1])) for k in range(steps - 1))
    assert np.array_equal(e.surface_read(0, frame.size), frame)


def test_refusals_on_a_live_engine(weights_path):
    e = zly.Engine(weights_path, dtype=zly.DTYPE_BF16, max_batch=1, warmup_runs=0)

    def code(f, *a):
        with pytest.raises(zly.ZlyError) as ei:
            f(*a)
        return ei.value.code, ei.value.message

    assert code(e.surface_moves_enable, 0)[0] == zly.ERR_INVALID_ARGUMENT       # no store yet
    assert code(e.surface_move, [(0, 0, 0, 1, 1, 2, 2)])[0] == zly.ERR_INVALID_ARGUMENT
    fb = 37 * 29 * 3
    e.surfaces_enable(2, fb)
    e.surface_define(0, BGR, 37, 29)
    e.surface_define(1, BGR, 37, 29)
    key = np.random.default_rng(9).integers(0, 256, fb, dtype=np.uint8)
    e.surface_update([(0, 0, 0, key, zly.view_tight(BGR, 37, 29))])
    rc, msg = code(e.surface_move, [(0, 0, 0, 1, 1, 8, 8)])                      # before zly_surface_moves_enable
    assert rc == zly.ERR_INVALID_ARGUMENT and "zly_surface_moves_enable" in msg
    e.surface_moves_enable(1024)
    assert code(e.surface_moves_enable, 1024)[0] == zly.ERR_INVALID_ARGUMENT    # twice
    assert code(e.surface_move, [(0, 0, 0, 1, 1, 8, 8), (1, 0, 0, 1, 1, 8, 8)])[0] == zly.ERR_INVALID_INPUT        # slot 1 has no keyframe
    assert code(e.surface_move, [(0, 0, 0, 1, 1, 8, 8), (0, 30, 0, 0, 0, 8, 8)])[0] == zly.ERR_INVALID_ARGUMENT    # an illegal source
    assert code(e.surface_move, [(0, 0, 0, 1, 0, 36, 29)])[0] == zly.ERR_INVALID_ARGUMENT                          # 3132 bytes across itself, a bounce buffer of 1024
    assert code(e.surface_move, [])[0] == zly.ERR_INVALID_ARGUMENT
    assert np.array_equal(e.surface_read(0, fb), key)                            # nothing was enqueued: the store is unchanged
    assert not e.surface_read(1, fb).any()
    e.surface_move([(0, 0, 0, 1, 1, 8, 8)])
    assert np.array_equal(e.surface_read(0, fb), mr.apply_moves(key.copy(), BGR, 37, 29, [(0, 0, 1, 1, 8, 8)]))
    e.close()
