"""Resident surfaces on the GPU (include/zly.h "Resident surfaces"; csrc/kernels_surface.hip).

The store's bytes, bit for bit, against tests/surface_ref.py through zly_surface_read: single pixels at the corners, every destination alignment
and head / body / tail combination of a BGR row, heights on either side of the kernel's band size, rectangles that share a 16-byte granule, the
most rectangles a call takes, one large frame -- and the neighbouring slots and the slack behind a frame untouched.  Then the detection rule:
zly_detect_surfaces on patched surfaces equals zly_detect_device_view on the oracle's frames uploaded whole, on a stretch, a letterbox and an area
engine, through zly_detect_delta too, composed with the tile merge and the tracker."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch            # before the first engine: the process then uses torch's HIP runtime throughout, as tests/test_gpu_parity.py does

import surface_ref as sr
import yuv422_ref
import yuv_ref
import zly
import zly_model as zm
from oracle_lib import det_fields_equal

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAND = int(re.search(r"#define\s+ZLY_SURFACE_BAND_BYTES\s+(\d+)", open(os.path.join(ROOT, "zero-latency-yolo_amd", "csrc", "surface_device.h")).read()).group(1))
BGR, BGRA, NV12, I420, YUY2 = zly.PIX_BGR, zly.PIX_BGRA, zly.PIX_NV12_BT601, zly.PIX_I420_BT709, zly.PIX_YUY2_BT601
BIG_W, BIG_H = 1920, 1080
EACH = BIG_W * BIG_H * 4            # max_bytes_each of the stretch engine's store: one 1920 x 1080 BGRA frame, exactly
SLOTS = 8
MODES = {"stretch": 0, "letterbox": zly.FLAG_LETTERBOX, "area": zly.FLAG_AREA}
_ENGINES = {}


@pytest.fixture(scope="module")
def engine_for(weights_path):
    """one engine per resize mode, shared by the module; the stretch engine carries the large store and the byte tests"""
    def get(mode):
        if mode not in _ENGINES:
            e = zly.Engine(weights_path, dtype=zly.DTYPE_BF16, max_batch=16 if mode == "stretch" else 4, max_dets=64, conf_thr=0.05, warmup_runs=0, flags=MODES[mode])
            e.surfaces_enable(SLOTS, EACH if mode == "stretch" else 640 * 480 * 4)
            _ENGINES[mode] = e
        return _ENGINES[mode]
    yield get
    for e in _ENGINES.values():
        e.close()
    _ENGINES.clear()


def _raw_slot(e, s):
    """all max_bytes_each bytes of slot s: the slot is defined as the largest frame for the read (a define enqueues nothing and changes no byte)"""
    e.surface_define(s, BGRA, BIG_W, BIG_H)
    return e.surface_read(s, EACH)


class Mirror:
    """the store as the oracle says it is: every slot's max_bytes_each bytes, starting from what the store holds now"""

    def __init__(self, e):
        self.e = e
        self.full = [_raw_slot(e, s) for s in range(SLOTS)]
        self.shape = [None] * SLOTS

    def define(self, s, fmt, w, h):
        self.e.surface_define(s, fmt, w, h)
        self.shape[s] = (fmt, w, h)

    def keyframe(self, s, seed):
        fmt, w, h = self.shape[s]
        px = np.random.default_rng(seed).integers(0, 256, sr.frame_bytes(fmt, w, h), dtype=np.uint8)
        self.update([(s, 0, 0, w, h, px)])

    def update(self, rects, call=None):
        """rects: (s, x0, y0, rw, rh, tight bytes).  Odd-numbered rectangles go in as crops of a larger host buffer, the others as tight frames."""
        args = []
        for i, (s, x0, y0, rw, rh, px) in enumerate(rects):
            fmt = self.shape[s][0]
            px = np.ascontiguousarray(px, dtype=np.uint8).reshape(-1)
            if i % 2 and rw + 4 <= 4096:
                host = np.full(sr.frame_bytes(fmt, rw + 4, rh + 2), 0xA5, dtype=np.uint8)
                sr.apply(host, fmt, rw + 4, rh + 2, 2, 2, px, rw, rh)
                args.append((s, x0, y0, host, zly.view_crop(zly.view_tight(fmt, rw + 4, rh + 2), 2, 2, rw, rh)))
            else:
                args.append((s, x0, y0, px, zly.view_tight(fmt, rw, rh)))
        (call or self.e.surface_update)(args)
        for s, x0, y0, rw, rh, px in rects:
            fmt, w, h = self.shape[s]
            sr.apply(self.full[s], fmt, w, h, x0, y0, px, rw, rh)

    def check(self, *slots):
        for s in slots:
            fmt, w, h = self.shape[s]
            fb = sr.frame_bytes(fmt, w, h)
            got = self.e.surface_read(s, fb)
            assert np.array_equal(got, self.full[s][:fb]), (s, self.shape[s], np.flatnonzero(got != self.full[s][:fb])[:8])

    def check_all(self):
        """every byte of every slot, the slack behind the frames included (this redefines the slots)"""
        for s in range(SLOTS):
            got = _raw_slot(self.e, s)
            assert np.array_equal(got, self.full[s]), (s, np.flatnonzero(got != self.full[s])[:8])
            self.shape[s] = None


def _rnd(rng, fmt, rw, rh):
    return rng.integers(0, 256, sr.frame_bytes(fmt, rw, rh), dtype=np.uint8)


SMALL = {1: (BGR, 37, 29), 2: (BGRA, 40, 30), 3: (NV12, 38, 30), 4: (I420, 38, 30), 5: (YUY2, 38, 29)}


def _small_store(e):
    m = Mirror(e)
    for s, (fmt, w, h) in SMALL.items():
        m.define(s, fmt, w, h)
        m.keyframe(s, 1000 + s)                              # the poison pattern
    m.check(*SMALL)
    return m


def test_store_bytes_single_pixels_alignments_and_the_full_surface(engine_for):
    e = engine_for("stretch")
    m = _small_store(e)
    rng = np.random.default_rng(1)
    # the smallest legal rectangle at every corner and in the middle of every surface, all in one call
    rects = []
    for s, (fmt, w, h) in SMALL.items():
        _, _, ex, ey = sr.FORMATS[fmt]
        rw, rh = (2 if ex else 1), (2 if ey else 1)
        for x0, y0 in ((0, 0), (w - rw, 0), (0, h - rh), (w - rw, h - rh), ((w // 2) & ~1, (h // 2) & ~1)):
            rects.append((s, x0, y0, rw, rh, _rnd(rng, fmt, rw, rh)))
    m.update(rects)
    m.check(*SMALL)
    # every BGR x0 in 0..16 with widths 1..17: the row pitch is 111 bytes, so rows y and y + 1 differ in alignment too -- all destination
    # alignments mod 16, all head / body / tail combinations
    for rw in range(1, 18):
        m.update([(1, x0, (x0 + rw) % 29, rw, 1, _rnd(rng, BGR, rw, 1)) for x0 in range(17)])
        m.check(1)
    seen = {(111 * ((x0 + rw) % 29) + 3 * x0) % 16 for rw in range(1, 18) for x0 in range(17)}
    assert seen == set(range(16))
    # ... and two rows high at every x0, widths that end inside, at and beyond a granule
    for rw in (5, 6, 11):
        m.update([(1, x0, (2 * x0 + rw) % 28, rw, 2, _rnd(rng, BGR, rw, 2)) for x0 in range(14)])
        m.check(1)
    # the full surface again: a keyframe replaces every byte
    for s in SMALL:
        m.keyframe(s, 2000 + s)
    m.check(*SMALL)
    m.check_all()


def test_store_bytes_around_the_band_size(engine_for):
    """a job is cut into bands of max(1, BAND // row_bytes) rows: heights one below, at and one above one and two bands, for rows of 160 and 111
    bytes, and for rows of 256 bytes, whose bands are exactly BAND bytes, so that the rectangles' bytes lie on either side of a multiple of it"""
    e = engine_for("stretch")
    m = Mirror(e)
    rng = np.random.default_rng(2)
    for s, (fmt, w, bpp) in enumerate(((BGRA, 40, 4), (BGR, 37, 3), (BGRA, 64, 4)), start=1):
        per = BAND // (bpp * w)
        assert per >= 2 and (w != 64 or per * bpp * w == BAND)
        m.define(s, fmt, w + 3, 2 * per + 2)
        m.keyframe(s, 3000 + s)
        for rh in (per - 1, per, per + 1, 2 * per - 1, 2 * per, 2 * per + 1):
            m.update([(s, 1, 1, w, rh, _rnd(rng, fmt, w, rh))])
            m.check(s)
    # rows longer than a band: one row per band
    wide = BAND // 4 + 5
    m.define(4, BGRA, wide, 3)
    m.keyframe(4, 3004)
    m.update([(4, 0, 1, wide, 2, _rnd(rng, BGRA, wide, 2)), (4, 3, 0, wide - 3, 1, _rnd(rng, BGRA, wide - 3, 1))])
    m.check(4)
    m.check_all()


def _checkerboard(w, h, x_lo, x_hi, y_lo, y_hi):
    """disjoint rectangles 1 to 5 pixels wide and 1 to 3 high that tile [x_lo, x_hi) x [y_lo, y_hi) completely"""
    out, y, k = [], y_lo, 0
    while y < y_hi:
        rh = min(1 + k % 3, y_hi - y)
        x = x_lo
        while x < x_hi:
            rw = min(1 + (k * 3 + k // 5) % 5, x_hi - x)
            out.append((x, y, rw, rh))
            x += rw
            k += 1
        y += rh
    return out


def test_rectangles_that_share_a_granule(engine_for):
    """BGR rectangles 1 to 5 pixels wide lie 3 to 15 bytes apart: neighbours share 16-byte granules.  First all of them in one call; then only every
    second one, so that the others' bytes must survive -- a read-modify-write at a rectangle's edge fails one of the two"""
    e = engine_for("stretch")
    m = Mirror(e)
    m.define(1, BGR, 37, 29)
    m.keyframe(1, 4000)
    board = _checkerboard(37, 29, 2, 35, 1, 28)
    assert len(board) > 100 and sum(r[2] * r[3] for r in board) == 33 * 27 and {r[2] for r in board} == {1, 2, 3, 4, 5}
    rng = np.random.default_rng(3)
    m.update([(1, x, y, rw, rh, _rnd(rng, BGR, rw, rh)) for x, y, rw, rh in board])
    m.check(1)
    for phase in (0, 1):
        m.update([(1, x, y, rw, rh, _rnd(rng, BGR, rw, rh)) for x, y, rw, rh in board[phase::2]])
        m.check(1)
    m.check_all()


def test_the_most_rectangles_a_call_takes(engine_for):
    e = engine_for("stretch")
    m = Mirror(e)
    for s in range(SLOTS):
        m.define(s, BGR, 37, 29)
        m.keyframe(s, 5000 + s)
    rng = np.random.default_rng(4)
    cell = lambda i: ((i // SLOTS * 5) % 37, (i // SLOTS * 5) // 37)
    rects = [(i % SLOTS, *cell(i), 1, 1, _rnd(rng, BGR, 1, 1)) for i in range(zly.SURFACE_MAX_RECTS + 1)]
    assert len({(r[0], r[1], r[2]) for r in rects}) == len(rects)
    with pytest.raises(zly.ZlyError) as ei:
        e.surface_update([(r[0], r[1], r[2], r[5], zly.view_tight(BGR, 1, 1)) for r in rects])      # one more than the most: refused ...
    assert ei.value.code == zly.ERR_INVALID_ARGUMENT
    m.check(*range(SLOTS))                                   # ... and the store is unchanged
    m.update(rects[:zly.SURFACE_MAX_RECTS])
    m.check(*range(SLOTS))
    m.check_all()


def test_one_large_surface(engine_for):
    """1920 x 1080 BGRA: a keyframe of 8.3 MB is some five hundred bands in one job; then 64 seeded rectangles in one call"""
    e = engine_for("stretch")
    m = Mirror(e)
    m.define(2, BGRA, BIG_W, BIG_H)
    m.keyframe(2, 6000)
    m.check(2)
    rng = np.random.default_rng(5)
    rects = []
    for cy in range(8):
        for cx in range(8):
            rw, rh = int(rng.integers(1, 241)), int(rng.integers(1, 136))
            x0, y0 = cx * 240 + int(rng.integers(0, 240 - rw + 1)), cy * 135 + int(rng.integers(0, 135 - rh + 1))
            rects.append((2, x0, y0, rw, rh, _rnd(rng, BGRA, rw, rh)))
    m.update(rects)
    m.check(2)
    m.check_all()


# ---- the detection rule ----------------------------------------------------------------------------------------------------------
STREAMS = ((BGR, 333, 251), (NV12, 640, 360), (YUY2, 418, 240))


def _as_format(fmt, bgr):
    if fmt == BGR:
        return np.ascontiguousarray(bgr).reshape(-1)
    if fmt in (zly.PIX_NV12_BT601, zly.PIX_I420_BT709):
        return yuv_ref.bgr_to_yuv420(bgr, fmt)
    return yuv422_ref.from_bgr(bgr, fmt)


def _step_rects(rng, fmt, w, h, count):
    _, _, ex, ey = sr.FORMATS[fmt]
    sx, sy = (2 if ex else 1), (2 if ey else 1)
    out = []
    while len(out) < count:
        rw, rh = int(rng.integers(8, w // 2)) // sx * sx, int(rng.integers(8, h // 2)) // sy * sy
        r = (int(rng.integers(0, w - rw + 1)) // sx * sx, int(rng.integers(0, h - rh + 1)) // sy * sy, rw, rh)
        if all(sr.disjoint(r, o) for o in out):
            out.append(r)
    return out


def _slabs_equal(a, b):
    return len(a) == len(b) and all(ha == hb and det_fields_equal(da, db) and np.array_equal(da["timestamp"], db["timestamp"]) for (ha, da), (hb, db) in zip(a, b))


@pytest.mark.parametrize("mode", list(MODES))
def test_detecting_on_patched_surfaces_is_detecting_on_the_frames_uploaded_whole(engine_for, mode):
    e = engine_for(mode)
    rng = np.random.default_rng(6)
    films = [[_as_format(fmt, f) for f in zm.synth_frames(6, w, h, seed=700 + i)] for i, (fmt, w, h) in enumerate(STREAMS)]
    n = len(STREAMS)
    for i, (fmt, w, h) in enumerate(STREAMS):
        e.surface_define(i, fmt, w, h)                       # the streams through zly_surface_update + zly_detect_surfaces
        e.surface_define(n + i, fmt, w, h)                   # and again through zly_detect_delta
    frames = [None] * n
    total_kept = 0
    for step in range(6):
        rects = []
        for i, (fmt, w, h) in enumerate(STREAMS):
            new = films[i][step]
            if step == 0:
                frames[i] = new.copy()
                rects.append((i, 0, 0, new, zly.view_tight(fmt, w, h)))
                continue
            for x0, y0, rw, rh in _step_rects(rng, fmt, w, h, 4):       # "these rectangles changed": cut from the stream's next picture
                sr.apply(frames[i], fmt, w, h, x0, y0, sr.cut(new, fmt, w, h, x0, y0, rw, rh), rw, rh)
                rects.append((i, x0, y0, new, zly.view_crop(zly.view_tight(fmt, w, h), x0, y0, rw, rh)))
        e.surface_update(rects)
        e.detect_surfaces(list(range(n)), tag0=10 * step)
        got = e.read_slabs(n)
        for i, (fmt, w, h) in enumerate(STREAMS):
            assert np.array_equal(e.surface_read(i, frames[i].size), frames[i]), (mode, step, i)
        # the reference: the oracle's frames uploaded whole, one buffer, tight views, same n and order
        offs = np.cumsum([0] + [(f.size + 255) // 256 * 256 for f in frames])
        host = np.zeros(int(offs[-1]), dtype=np.uint8)
        views = []
        for i, (fmt, w, h) in enumerate(STREAMS):
            host[offs[i]:offs[i] + frames[i].size] = frames[i]
            v = zly.view_tight(fmt, w, h)
            for p in range(3):
                v.off[p] += int(offs[i])
            views.append(v)
        d_host = torch.from_numpy(host).cuda()
        torch.cuda.synchronize()
        e.detect_device_view(d_host.data_ptr(), host.nbytes, views, tag0=10 * step)
        want = e.read_slabs(n)
        assert _slabs_equal(got, want), (mode, step)
        total_kept += sum(int(h["n_kept"]) for h, _ in want)
        # the host-memory convenience on the second set of slots
        dets = e.detect_delta([(n + r[0],) + r[1:] for r in rects], [n + i for i in range(n)], cap=64)
        for (d, k), (hdr, wd) in zip(dets, want):
            assert k == int(hdr["n_kept"]) and det_fields_equal(d, wd) and (len(d) == 0 or (d["timestamp"] > 0).all()), (mode, step)
    assert total_kept >= 18, total_kept                     # the comparison is not one of empty lists
    # a call without rectangles: nothing changed, the same answer
    again = e.detect_delta([], [n + i for i in range(n)], cap=64)
    assert all(k == k2 and det_fields_equal(d, d2) for (d, k), (d2, k2) in zip(again, dets))


def test_update_detect_update_on_callers_streams_without_a_synchronise(engine_for):
    """The device-path loop as a server runs it: update k on the engine's stream, detect k on a CALLER's stream, update k + 1, ... with nothing but
    enqueues in between, the detections going to two streams in turn.  Every step replaces the whole surface with another picture, so a patch kernel
    that overtook the detect call before it would hand that call the next picture (or a torn one).  Each step's slab must be the slab of its own picture
    uploaded whole; the store is ordered against the callers' streams in both directions by the engine."""
    e = engine_for("stretch")
    W, H, steps = 960, 540, 6
    films = [np.ascontiguousarray(np.concatenate([f, np.full((H, W, 1), 255, np.uint8)], axis=2)).reshape(-1) for f in zm.synth_frames(steps, W, H, seed=900)]
    whole = zly.view_tight(BGRA, W, H)
    sb = e.slab_bytes
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    d_slabs = torch.zeros(steps * sb, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    e.surface_define(0, BGRA, W, H)
    for k in range(steps):
        e.surface_update([(0, 0, 0, films[k], whole)])
        e.detect_surfaces([0], d_slabs_ptr=d_slabs.data_ptr() + k * sb, tag0=k, stream=streams[k % 2].cuda_stream)
    for s in streams:
        s.synchronize()
    e.sync()
    got = zly.parse_slabs(d_slabs.cpu().numpy(), steps, e.max_dets)
    want = []
    for k in range(steps):
        d = torch.from_numpy(films[k]).cuda()
        torch.cuda.synchronize()
        e.detect_device_view(d.data_ptr(), films[k].nbytes, [whole], tag0=k)
        want.append(e.read_slabs(1)[0])
    assert _slabs_equal(got, want)
    # the pictures tell each other apart: a call that saw its neighbour's picture would have failed above
    assert all(len(want[k][1]) > 0 and not (len(want[k][1]) == len(want[k + 1][1]) and det_fields_equal(want[k][1], want[k + 1][1])) for k in range(steps - 1))
    assert np.array_equal(e.surface_read(0, films[-1].size), films[-1])


def test_tiles_of_a_resident_surface_merge_and_track_as_the_uploaded_surface_does(engine_for):
    e = engine_for("stretch")
    W = H = 832
    tiles = zly.tile_grid(W, H, 416, 416, 32, 32)
    n = len(tiles)
    assert n == 9
    pictures = [np.ascontiguousarray(f).reshape(-1) for f in zm.synth_frames(2, W, H, seed=800)]
    surf = zly.view_tight(BGR, W, H)
    e.surface_define(0, BGR, W, H)
    e.surface_update([(0, 0, 0, pictures[0], surf)])
    e.detect_surfaces([0] * n, rois=[(t.x0, t.y0, t.w, t.h) for t in tiles])
    e.merge_slabs(tiles, 1)
    (hdr, dets), = e.read_merged(1)
    tdets, tn = e.detect_tiled(pictures[0], surf, tiles, cap=64)
    assert tn == int(hdr["n_kept"]) > 0 and det_fields_equal(dets, tdets)
    # the tracker: ids on the resident surface's slabs over two pictures = ids on the whole uploads' slabs
    e.track_enable(max_streams=2, max_tracks=64)
    second = pictures[0].copy()
    patch = (208, 104, 416, 520)
    sr.apply(second, BGR, W, H, patch[0], patch[1], sr.cut(pictures[1], BGR, W, H, *patch), patch[2], patch[3])
    ids = []
    for k in range(2):
        if k:
            e.surface_update([(0, patch[0], patch[1], pictures[1], zly.view_crop(surf, *patch))])
        e.detect_surfaces([0])
        e.track_slabs([1])
        ids.append(e.read_slabs(1)[0])
    e.track_reset(1, 1)
    for k, pic in enumerate((pictures[0], second)):
        d = torch.from_numpy(pic).cuda()
        torch.cuda.synchronize()
        e.detect_device_view(d.data_ptr(), pic.nbytes, [surf])
        e.track_slabs([1])
        (whdr, wd), = e.read_slabs(1)
        assert whdr == ids[k][0] and det_fields_equal(wd, ids[k][1]) and len(wd) > 0 and (wd["track_id"] > 0).all(), k


def test_state_keyframes_redefinition_and_refusals(engine_for):
    e = engine_for("stretch")
    lib = e.lib
    m = Mirror(e)
    m.define(1, BGR, 37, 29)
    rng = np.random.default_rng(7)

    def code(f, *a, **k):
        with pytest.raises(zly.ZlyError) as ei:
            f(*a, **k)
        return ei.value.code

    assert code(e.detect_surfaces, [1]) == zly.ERR_INVALID_INPUT                     # defined, no keyframe yet
    m.update([(1, 0, 0, 37, 28, _rnd(rng, BGR, 37, 28))])                            # all but one row is not a keyframe
    assert code(e.detect_surfaces, [1]) == zly.ERR_INVALID_INPUT
    m.keyframe(1, 7000)
    e.detect_surfaces([1])
    e.detect_surfaces([1, 1], rois=[(0, 0, 20, 20), (17, 9, 20, 20)])
    assert code(e.detect_surfaces, [1], rois=[(30, 0, 8, 8)]) == zly.ERR_INVALID_ARGUMENT
    assert code(e.detect_surfaces, [SLOTS]) == zly.ERR_INVALID_ARGUMENT
    assert code(e.detect_surfaces, [3]) == zly.ERR_INVALID_INPUT                     # defined (by the mirror's read), never keyframed
    m.define(1, BGR, 37, 29)                                                         # redefining invalidates, and changes no byte
    assert code(e.detect_surfaces, [1]) == zly.ERR_INVALID_INPUT
    m.check(1)
    # refused updates enqueue nothing: an overlap, a rectangle outside, another format, a source view beyond its buffer
    px = _rnd(rng, BGR, 4, 4)
    t44 = zly.view_tight(BGR, 4, 4)
    assert code(e.surface_update, [(1, 0, 0, px, t44), (1, 3, 3, px, t44)]) == zly.ERR_INVALID_ARGUMENT
    assert code(e.surface_update, [(1, 5, 5, px, t44), (1, 34, 0, px, t44)]) == zly.ERR_INVALID_ARGUMENT
    assert code(e.surface_update, [(1, 5, 5, px, t44), (1, 10, 10, _rnd(rng, BGRA, 4, 4), zly.view_tight(BGRA, 4, 4))]) == zly.ERR_INVALID_ARGUMENT
    assert code(e.surface_update, [(1, 5, 5, px, t44), (1, 10, 10, px[:-1], t44)]) == zly.ERR_INVALID_INPUT
    assert code(e.detect_delta, [(1, 5, 5, px, t44)], [1]) == zly.ERR_INVALID_INPUT  # the update is legal, the surface is not valid: nothing is enqueued
    m.check(1)
    assert code(e.surface_define, 1, 9, 8, 8) == zly.ERR_INVALID_ARGUMENT
    assert code(e.surface_define, 1, NV12, 9, 8) == zly.ERR_INVALID_INPUT
    assert code(e.surface_define, 1, BGRA, BIG_W, BIG_H + 1) == zly.ERR_INVALID_INPUT
    assert code(e.surfaces_enable, 2, 4096) == zly.ERR_INVALID_ARGUMENT              # twice
    assert code(e.surface_read, 3, 16) == zly.ERR_INVALID_ARGUMENT
    assert lib.zly_surface_read(e.h, 1, None, 0) == zly.ERR_INVALID_ARGUMENT
    assert code(e.surface_read, 1, 37 * 29 * 3 - 1) == zly.ERR_INVALID_ARGUMENT
    m.check_all()


def test_an_engine_without_a_store_refuses_every_call(weights_path):
    e = zly.Engine(weights_path, dtype=zly.DTYPE_BF16, max_batch=1, warmup_runs=0)
    for f, a in ((e.surface_define, (0, BGR, 8, 8)), (e.surface_read, (0, 192)), (e.detect_surfaces, ([0],)), (e.detect_delta, ([], [0])),
                 (e.surface_update, ([(0, 0, 0, np.zeros(192, np.uint8), zly.view_tight(BGR, 8, 8))],))):
        with pytest.raises(zly.ZlyError) as ei:
            f(*a)
        assert ei.value.code == zly.ERR_INVALID_ARGUMENT and "zly_surfaces_enable" in ei.value.message
    for bad in ((0, 1024), (4, 0), (-1, 1024), (2, 1 << 56)):
        with pytest.raises(zly.ZlyError) as ei:
            e.surfaces_enable(*bad)
        assert ei.value.code == zly.ERR_INVALID_ARGUMENT
    e.close()
