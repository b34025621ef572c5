"""The change map on the GPU (include/zly.h "Change map"; csrc/kernels_change.hip), byte for byte against tests/change_ref.py: after every call the
WHOLE record of every stream -- header, peaks, activity grid and every byte the rule does not write -- must equal the oracle applied to the frames
the stream was given.  The records are the engine's own (zly_change_enable zeroes them), so the test cannot poison them; it keeps a mirror of each
from the zeroes on, and PRIMES every stream of the kernel tests with frames of the test's largest geometry that leave every peak record and nearly
every activity cell non-zero (_prime) before the frames under test, so that a kernel that wrote zeroes where it must not write would be seen.

1. The two kernels: all twelve formats, tight and through pitched views in a poisoned buffer, every size and cell of the issue, widths around the sums
   kernel's shape constants, sequences of 3-6 frames, several streams in one call and split over calls, in any batch position.
2. Resident surfaces with update -> change -> update and nothing but enqueues in between.  Refusals change nothing.
3. Zoom: the extended RULE against a twin engine driven through the explicit sequence."""
import os
import re

import numpy as np
import pytest
import torch            # before the first engine: the process then uses torch's HIP runtime throughout, as tests/test_gpu_parity.py does

import change_cases as cs
import change_ref as chr_
import chip_cases as cc
import test_gpu_zoom as tz
import zly
import zoom_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = cc.POISON
ARG, INPUT = zly.ERR_INVALID_ARGUMENT, zly.ERR_INVALID_INPUT
BGR, BGRA, NV12, I420, YUY2 = zly.PIX_BGR, zly.PIX_BGRA, zly.PIX_NV12_BT601, zly.PIX_I420_BT709, zly.PIX_YUY2_BT601


def _kernel_constants():
    """the sums kernel's shape constants, parsed from its header: sizes around them are where it changes path"""
    text = open(os.path.join(ROOT, "zero-latency-yolo_amd", "csrc", "change_device.h")).read()
    c = {k: int(v) for k, v in re.findall(r"#define\s+(ZLY_CHANGE_(?:THREADS|TILE_PX|GRANULE_PX))\s+(\d+)", text)}
    assert set(c) == {"ZLY_CHANGE_THREADS", "ZLY_CHANGE_TILE_PX", "ZLY_CHANGE_GRANULE_PX"}, c
    return c


CONSTS = _kernel_constants()


def _engine(weights_path, cfg, max_streams=8, flags=0, enable=True, surfaces=0):
    """the 416 x 416 engine of tests/test_gpu_zoom.py, max_batch 16"""
    e = zly.Engine(weights_path, dtype=zly.DTYPE_BF16, max_batch=16, max_dets=tz.CAP, conf_thr=tz.CONF, iou_thr=tz.IOU, warmup_runs=0, flags=flags)
    if enable:
        e.change_enable(max_streams, cell=cfg.cell, threshold_q4=cfg.threshold_q4, max_active_permille=cfg.max_active_permille, max_peaks=cfg.max_peaks,
                        window_w=cfg.window_w, window_h=cfg.window_h)
        assert e.change_layout() == chr_.layout(cfg)
    if surfaces:
        e.surfaces_enable(surfaces, 640 * 480 * 4)
    return e


def _pack(items):
    """[(buffer, view tuple)] -> (one host buffer with every item at a multiple of 256 behind 3 poisoned bytes, the views in it)"""
    parts, views, o = [], [], 0
    for buf, view in items:
        lead = 3
        size = -(-(lead + buf.size) // 256) * 256
        p = np.full(size, POISON, dtype=np.uint8)
        p[lead:lead + buf.size] = buf
        parts.append(p)
        views.append(cc.to_c(cc.shifted(view, o + lead)))
        o += size
    return np.concatenate(parts), views


class Mirror:
    """the oracle's streams and the bytes their records must hold"""

    def __init__(self, cfg, n=8):
        self.cfg = cfg
        self.streams = [chr_.Stream() for _ in range(n)]
        self.recs = [np.zeros(chr_.layout(cfg)[0], dtype=np.uint8) for _ in range(n)]
        self.flags, self.peaks = set(), 0

    def frame(self, s, bgr, suppress=()):
        h, peaks, _ = self.streams[s].frame(bgr, self.cfg, self.recs[s], suppress)
        self.flags.add(int(h["flags"]))
        self.peaks += len(peaks)
        return h, peaks

    def check(self, e, streams, what=""):
        for s in streams:
            got = e.change_read(s)
            if not np.array_equal(got, self.recs[s]):
                bad = np.flatnonzero(got != self.recs[s])
                raise AssertionError(f"{what}: stream {s}: {len(bad)} bytes differ, first at {bad[:6].tolist()}; header {got[:32].view(chr_.HDR_DTYPE)[0]} "
                                     f"want {self.recs[s][:32].view(chr_.HDR_DTYPE)[0]}")


def _call(e, mirror, items, streams, what=""):
    """one zly_change_device_view call: items = [(buffer, view tuple, BGR image)]; every stream's whole record against the oracle"""
    host, views = _pack([(b, v) for b, v, _ in items])
    d = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    e.change_device_view(d.data_ptr(), host.nbytes, views, streams)
    for s, (_, _, bgr) in zip(streams, items):
        mirror.frame(s, bgr)
    mirror.check(e, streams, what)


KINDS = ["new", "blocks", "flat", "same", "blocks", "new"]


def _prime(e, m, streams, w=0, h=0, seed=90):
    """The records are zero after zly_change_enable, and a kernel that wrote zeroes where it must not write would go unseen while they are.  So
    every stream first takes three BGR frames of a geometry at least as large as the test's largest and at least 10 x 7 cells: a random one, the
    same with a white block of a cell's size in every corner and in the middle (five separate peaks: no test asks for more), and another random one
    (nearly every cell changes: new peaks, or GLOBAL, which leaves the peaks alone).
    After that every peak record and nearly every activity cell of that grid is non-zero -- asserted here on the mirror -- and whatever the later,
    smaller frames must not write can be told from a zero"""
    rng = np.random.default_rng(seed)
    b = m.cfg.cell
    w, h = max(w, 10 * b), max(h, 7 * b)
    assert m.cfg.max_peaks <= 5 and w <= 642 and h <= 480
    f0 = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    f1 = f0.copy()
    for (x, y) in ((1, 1), (w - b - 1, 1), (1, h - b - 1), (w - b - 1, h - b - 1), ((w - b) // 2, (h - b) // 2)):
        f1[y:y + b, x:x + b] = 255
    f2 = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    for k, bgr in enumerate((f0, f1, f2)):
        _call(e, m, [(bgr.reshape(-1), cc.tight_view(BGR, w, h), bgr)] * len(streams), streams, ("prime", k))
    po, ao = chr_.layout(m.cfg)[1:]
    nc = chr_.grid(w, h, m.cfg.cell)[0] * chr_.grid(w, h, m.cfg.cell)[1]
    for s_ in streams:
        peaks = m.recs[s_][po:ao].view(chr_.PEAK_DTYPE)
        assert (peaks["w"] != 0).all() and (peaks["activity"] != 0).all(), (s_, peaks)
        assert np.count_nonzero(m.recs[s_][ao:ao + 4 * nc].view(np.uint32)) >= 0.9 * nc


# ---- 1. the kernels -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", cs.CELLS)
def test_every_format_tight_and_pitched(weights_path, C):
    """per format a film of five frames at 70 x 50 (rounded up to what the format allows: odd sizes where it allows them) and three at its smallest
    size; streams 0 and 2 take them tight, 1 and 3 through pitched views with odd plane origins, all four in one call"""
    cfg = chr_.Config(cell=C, threshold_q4=8, max_active_permille=600, max_peaks=4, window_w=24, window_h=16)
    e, m = _engine(weights_path, cfg), Mirror(cfg)
    _prime(e, m, [0, 1, 2, 3], 70, 50)
    for fmt in cc.ALL_FORMATS:
        (w, h), (ws, hs) = cs.legal_size(fmt, 69, 49), cc.smallest(fmt)
        big, small = cs.film(fmt, w, h, KINDS[:5], seed=3), cs.film(fmt, ws, hs, KINDS[:5], seed=4)
        for k in range(5):
            (f, bgr), (g, sbgr) = big[k], small[k]
            items = [(f, cc.tight_view(fmt, w, h), bgr), cc.pitched(f, fmt, w, h) + (bgr,), (g, cc.tight_view(fmt, ws, hs), sbgr), cc.pitched(g, fmt, ws, hs) + (sbgr,)]
            _call(e, m, items if k < 3 else items[:2], [0, 1, 2, 3] if k < 3 else [0, 1], (fmt, k))
    assert m.peaks >= 12 and m.flags >= {0, chr_.FIRST}, (m.peaks, m.flags)
    e.close()


@pytest.mark.parametrize("C", cs.CELLS)
def test_the_sizes_of_the_issue(weights_path, C):
    """1 x 1 ... 641 x 479 as BGR (every size is legal) and, rounded up, as NV12: three frames each, the stream changing geometry from size to size
    (FIRST each time) with the larger sizes first, so that the records keep cells and peaks of the larger grids"""
    cfg = chr_.Config(cell=C, threshold_q4=16, max_active_permille=500, max_peaks=3, window_w=208, window_h=208)
    e, m = _engine(weights_path, cfg), Mirror(cfg)
    _prime(e, m, [0, 1], 642, 480)
    for (w0, h0) in cs.SIZES[::-1]:
        if -(-w0 // C) * -(-h0 // C) > chr_.MAX_CELLS:
            continue
        for s, fmt in ((0, BGR), (1, NV12)):
            w, h = cs.legal_size(fmt, w0, h0)
            for k, (f, bgr) in enumerate(cs.film(fmt, w, h, ["new", "flat", "blocks"], seed=11)):
                _call(e, m, [(f, cc.tight_view(fmt, w, h), bgr)], [s], (fmt, w, h, k))
    assert m.peaks >= 4, m.peaks
    e.close()


@pytest.mark.parametrize("fmt", [BGR, BGRA, NV12, I420, YUY2])
def test_sizes_around_the_sums_kernels_shape_constants(weights_path, fmt):
    """widths one below, at and one above the granule, the tile and two tiles, heights around the tile, through pitched views; cells of 8 (a granule
    spans two cells) and of 64 (a tile is one cell) on two engines"""
    g, t = CONSTS["ZLY_CHANGE_GRANULE_PX"], CONSTS["ZLY_CHANGE_TILE_PX"]
    for C in (8, 64):
        cfg = chr_.Config(cell=C, threshold_q4=8, max_active_permille=700, max_peaks=2, window_w=32, window_h=32)
        e, m = _engine(weights_path, cfg), Mirror(cfg)
        _prime(e, m, list(range(8)), 2 * t + 2, t + 2)
        sizes = [(w, t + d) for d, ws in ((-1, (g - 1, g, g + 1)), (0, (t - 1, t, t + 1)), (1, (2 * t - 1, 2 * t, 2 * t + 1))) for w in ws]
        for k in range(3):
            items = []
            for i, (w0, h0) in enumerate(sizes[:8]):
                w, h = cs.legal_size(fmt, w0, h0)
                f, bgr = cs.film(fmt, w, h, ["new", "flat", "blocks"], seed=20 + i)[k]
                items.append(cc.pitched(f, fmt, w, h, pad=3, lead=1) + (bgr,))
            _call(e, m, items, list(range(8)), (fmt, C, k))
        # the ninth size on a stream that has held another geometry
        w, h = cs.legal_size(fmt, *sizes[8])
        for f, bgr in cs.film(fmt, w, h, ["new", "flat"], seed=29):
            _call(e, m, [cc.pitched(f, fmt, w, h, pad=3, lead=1) + (bgr,)], [5], (fmt, C, "ninth"))
        e.close()


def test_streams_in_one_call_split_over_calls_and_in_any_batch_position(weights_path):
    """four streams of four formats and sizes over five steps: engine A takes each step in one call, engine B in two calls with the streams in
    another order.  Both must hold the oracle's records: a stream's result does not depend on its batch position or on its neighbours"""
    cfg = chr_.Config(cell=16, threshold_q4=8, max_active_permille=600, max_peaks=5, window_w=48, window_h=32)
    a, b, ma, mb = _engine(weights_path, cfg), _engine(weights_path, cfg), Mirror(cfg), Mirror(cfg)
    shapes = ((BGR, 101, 77), (NV12, 128, 64), (YUY2, 66, 31), (zly.PIX_RGBA, 33, 31))
    _prime(a, ma, [0, 1, 2, 3], 128, 77)
    _prime(b, mb, [3, 2, 1, 0], 128, 77)
    films = [cs.film(fmt, w, h, KINDS[:5], seed=40 + i) for i, (fmt, w, h) in enumerate(shapes)]
    for k in range(5):
        items = [(films[i][k][0], cc.tight_view(fmt, w, h), films[i][k][1]) for i, (fmt, w, h) in enumerate(shapes)]
        _call(a, ma, items, [0, 1, 2, 3], ("A", k))
        _call(b, mb, [items[3], items[1]], [3, 1], ("B1", k))
        _call(b, mb, [items[2], items[0]], [2, 0], ("B2", k))
    for s in range(4):
        assert np.array_equal(ma.recs[s], mb.recs[s])
    assert ma.peaks >= 6
    a.close()
    b.close()


def test_reset(weights_path):
    cfg = chr_.Config(cell=32, threshold_q4=8, max_active_permille=1000, max_peaks=2, window_w=32, window_h=32)
    e, m = _engine(weights_path, cfg), Mirror(cfg)
    film = cs.film(BGR, 96, 64, ["new", "flat", "flat", "flat"], seed=50)
    items = lambda k: [(film[k][0], cc.tight_view(BGR, 96, 64), film[k][1])] * 2          # noqa: E731
    _call(e, m, items(0), [0, 1])
    _call(e, m, items(1), [0, 1])
    e.change_reset(1)
    m.streams[1].reset()
    _call(e, m, items(2), [0, 1])
    assert int(m.recs[0][:32].view(chr_.HDR_DTYPE)[0]["flags"]) == 0 and int(m.recs[1][:32].view(chr_.HDR_DTYPE)[0]["flags"]) == chr_.FIRST
    assert int(m.recs[1][:32].view(chr_.HDR_DTYPE)[0]["step"]) == 1
    e.change_reset(-1)
    for s in m.streams:
        s.reset()
    _call(e, m, items(3), [0, 1])
    e.close()


# ---- 2. resident surfaces, refusals -----------------------------------------------------------------------------------------------------------
def test_update_change_update_with_nothing_but_enqueues(weights_path):
    """update k on the engine's stream, zly_change_surfaces k on a caller's stream, update k + 1, ... over six whole new pictures.  Step k gives
    picture k to stream k (its second frame) and to stream k + 1 (its first), so that after the loop stream k's record is the difference of pictures
    k - 1 and k for every k: a patch kernel that overtook a sums kernel would have handed it the next picture"""
    cfg = chr_.Config(cell=32, threshold_q4=8, max_active_permille=1000, max_peaks=3, window_w=64, window_h=64)
    e, m = _engine(weights_path, cfg, surfaces=1), Mirror(cfg)
    W, H, steps = 320, 200, 6
    film = cs.film(BGRA, W, H, ["new"] + ["flat", "blocks"] * 3, seed=60)[:steps + 1]
    whole = zly.view_tight(BGRA, W, H)
    callers = [torch.cuda.Stream(), torch.cuda.Stream()]
    e.surface_define(0, BGRA, W, H)
    for k in range(steps):
        e.surface_update([(0, 0, 0, film[k][0], whole)])
        e.change_surfaces([0, 0], [k, k + 1], stream=callers[k % 2].cuda_stream)
        m.frame(k, film[k][1])
        m.frame(k + 1, film[k][1])
    for c in callers:
        c.synchronize()
    m.check(e, list(range(steps + 1)), "surfaces")
    assert m.peaks >= 3
    e.close()


def _code(f, *a, **k):
    with pytest.raises(zly.ZlyError) as ei:
        f(*a, **k)
    return ei.value.code


def test_refusals_change_nothing(weights_path):
    cfg = chr_.Config(cell=8, threshold_q4=8, max_active_permille=1000, max_peaks=2, window_w=16, window_h=16)
    plain = _engine(weights_path, cfg, enable=False)
    f, bgr = cc.frame(BGR, 16, 8, seed=1)
    d = torch.from_numpy(np.concatenate([f, np.zeros(64, np.uint8)])).cuda()
    torch.cuda.synchronize()
    v = zly.view_tight(BGR, 16, 8)
    assert _code(plain.change_device_view, d.data_ptr(), f.size, [v], [0]) == ARG and _code(plain.change_surfaces, [0], [0]) == ARG
    assert _code(plain.change_read, 0) == ARG and _code(plain.change_layout) == ARG and _code(plain.change_reset, 0) == ARG and _code(plain.zoom_use_change) == ARG
    for bad in (dict(cell=0), dict(cell=24), dict(cell=128), dict(threshold_q4=-1), dict(threshold_q4=4081), dict(max_active_permille=-1), dict(max_active_permille=1001),
                dict(max_peaks=0), dict(max_peaks=16), dict(window_w=0), dict(window_w=207), dict(window_h=16386), dict(max_streams=0)):
        assert _code(plain.change_enable, **bad) == ARG, bad
    assert plain.lib.zly_change_enable(plain.h, None, 4) == ARG
    c = zly.ChangeConfig()
    plain.lib.zly_default_change_config(plain.h, c)
    assert (c.cell, c.threshold_q4, c.max_active_permille, c.max_peaks, c.window_w, c.window_h) == (32, 32, 250, 3, 416, 416)
    e = plain
    e.change_enable(4, cell=8, threshold_q4=8, max_active_permille=1000, max_peaks=2, window_w=16, window_h=16)
    assert _code(e.change_enable, 4) == ARG                                                          # twice
    assert _code(e.zoom_use_change) == ARG                                                           # no zoom regions
    m = Mirror(cfg, 4)
    _call(e, m, [(f, cc.tight_view(BGR, 16, 8), bgr)] * 2, [0, 1])                                   # a good call first: states to disturb
    call = lambda vs, ss, nbytes=f.size: e.change_device_view(d.data_ptr(), nbytes, vs, ss)          # noqa: E731
    assert _code(call, [], []) == ARG                                                                # n = 0
    assert _code(call, [v] * 17, list(range(17))) == ARG                                             # n above max_batch
    assert e.lib.zly_change_device_view(e.h, 1, d.data_ptr(), f.size, None, (zly.C.c_int32 * 1)(0), None) == ARG
    assert e.lib.zly_change_device_view(e.h, 1, d.data_ptr(), f.size, (zly.FrameView * 1)(v), None, None) == ARG
    assert _code(call, [v, v], [1, 1]) == ARG and _code(call, [v, v], [0, 4]) == ARG and _code(call, [v, v], [0, -1]) == ARG
    bad_fmt, odd, short, wide, many = (zly.view_tight(BGR, 16, 8) for _ in range(5))
    bad_fmt.fmt = 5
    odd.fmt, odd.w = NV12, 15
    short.pitch[0] = 47
    wide.w, wide.h = 16385, 1
    wide.pitch[0] = 3 * 16385
    many.w, many.h = 1024, 520                                                                       # 128 x 65 cells of 8
    many.pitch[0] = 3 * 1024
    assert _code(call, [v, bad_fmt], [0, 1]) == ARG
    assert _code(call, [v, odd], [0, 1]) == INPUT and _code(call, [v, short], [0, 1]) == INPUT and _code(call, [v, v], [0, 1], f.size - 1) == INPUT
    assert _code(call, [v, wide], [0, 1], 1 << 20) == INPUT and _code(call, [v, many], [0, 1], 1 << 22) == INPUT
    assert _code(e.change_read, 4) == ARG and _code(e.change_reset, 4) == ARG and _code(e.change_surfaces, [0], [0]) == ARG          # no store
    raw = np.zeros(8, np.uint8)
    assert e.lib.zly_change_read(e.h, 0, raw.ctypes.data, 8) == ARG
    e.surfaces_enable(2, 16 * 8 * 3)
    assert _code(e.change_surfaces, [0], [0]) == ARG and _code(e.change_surfaces, [2], [0]) == ARG   # undefined, out of range
    e.surface_define(0, BGR, 16, 8)
    assert _code(e.change_surfaces, [0], [0]) == INPUT                                               # defined, no keyframe
    m.check(e, [0, 1, 2, 3], "after the refusals")                                                   # no record changed ...
    g, gbgr = cc.frame(BGR, 16, 8, seed=2)
    e.surface_update([(0, 0, 0, g, v)])
    e.change_surfaces([0, 0], [0, 2])                                                                # ... and no state: stream 0 is on its second frame
    m.frame(0, gbgr)
    m.frame(2, gbgr)
    m.check(e, [0, 1, 2, 3], "the accepted call")
    assert [int(m.recs[s][:32].view(chr_.HDR_DTYPE)[0]["step"]) for s in (0, 2)] == [2, 1]
    e.close()


# ---- 3. zoom: the extended RULE ---------------------------------------------------------------------------------------------------------------
def _scene(w, h, k, i, jump=False):
    """a static background per stream with two small patches that move from step to step; jump: another background (the whole scene moves)"""
    pic = tz._picture(w, h, 31 * i + (77 if jump else 0), 17 * i + (40 if jump else 0), i).copy()
    f = tz.G["frames_64"]
    for j, (px, py) in enumerate((((40 + 90 * k) % (w - 72), (30 + 50 * k) % (h - 72)), ((w - 80 - 70 * k) % (w - 72), (h - 90 + 40 * k) % (h - 72)))):
        pic[py:py + 48, px:px + 48] = 255 - f[(i + j) % 2][:48, :48]
    return np.ascontiguousarray(pic)


class Counts:
    """what a run of the extended rule met"""

    def __init__(self):
        self.filled, self.flags = 0, set()


def _zoom_pair(weights_path, flags, zcfg, ccfg, **kw):
    e1, e2 = tz._engine(weights_path, flags, cfg=zcfg, **kw), tz._engine(weights_path, flags, zoom=False, **kw)
    for e in (e1, e2):
        e.change_enable(8, cell=ccfg.cell, threshold_q4=ccfg.threshold_q4, max_active_permille=ccfg.max_active_permille, max_peaks=ccfg.max_peaks,
                        window_w=ccfg.window_w, window_h=ccfg.window_h)
    e1.zoom_use_change(True)
    return e1, e2


def _run_extended_rule(e1, e2, steps, zcfg, ccfg, what):
    """steps: lists of (fmt, w, h, tight bytes, pitch), one surface per stream.  e1 takes the zoom call, e2 the explicit sequence: zly_change_device_view
    on the surfaces, the old plan (the oracle's, from zly_track_read), the fill -- step 7 of the oracle on the activity grid e2's record holds, with
    the plan's track regions as initial suppression -- then crops, detect, merge and track as tests/test_gpu_zoom.py's twin makes them"""
    twin = Counts()
    sb = e1.slab_bytes

    def frame(d_ptr, nbytes, views, streams, d_out_ptr, tag0):
        e2.change_device_view(d_ptr, nbytes, views, streams)
        tiles, call_views, plans, all_peaks = [], [], [], []
        for i, (v, s) in enumerate(zip(views, streams)):
            plan = zoom_ref.plan(tz._table_from_engine(e2, s), zcfg, v.w, v.h)
            hdr, _, act = zly.parse_change_record(e2.change_read(s), ccfg.max_peaks)
            twin.flags.add(int(hdr["flags"]))
            peaks = []
            if not int(hdr["flags"]):
                _, npix = chr_.sums(np.zeros((v.h, v.w, 3), np.uint8), ccfg.cell)
                _, _, peaks = chr_.pick(act, npix, v.w, v.h, ccfg, chr_.track_rects(plan))
            plan = chr_.fill(plan, peaks)
            twin.filled += int((plan["slot"] == -2).sum())
            plans.append(plan)
            all_peaks.append(peaks)
            call_views.append(v)
            tiles.append(zly.tile(0, 0, v.w, v.h, v.w, v.h, group=i))
            for r in plan:
                call_views.append(zly.view_crop(v, int(r["x0"]), int(r["y0"]), int(r["w"]), int(r["h"])))
                tiles.append(zly.tile(int(r["x0"]), int(r["y0"]), int(r["w"]), int(r["h"]), v.w, v.h, group=i))
        e2.detect_device_view(d_ptr, nbytes, call_views)
        e2.merge_slabs(tiles, len(views), d_out_ptr=d_out_ptr, tag0=tag0)
        e2.track_slabs(list(streams), d_out_ptr)
        return plans, all_peaks

    track_regions = 0
    for k, surfaces in enumerate(steps):
        n = len(surfaces)
        streams = list(range(1, n + 1))
        host, views = tz._pack(surfaces)
        d_host = torch.from_numpy(host).cuda()
        d1 = torch.full((n * sb + 64,), tz.POISON, dtype=torch.uint8, device="cuda")
        d2 = torch.full((n * sb + 64,), tz.POISON, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        e1.detect_device_zoom(d_host.data_ptr(), host.nbytes, views, streams, d_out_ptr=d1.data_ptr(), tag0=100 * k)
        plans, all_peaks = frame(d_host.data_ptr(), host.nbytes, views, streams, d2.data_ptr(), 100 * k)
        e1.sync()
        e2.sync()
        got, want = d1.cpu().numpy(), d2.cpu().numpy()
        assert np.array_equal(got, want), (what, k, np.flatnonzero(got != want)[:8])
        assert (got[n * sb:] == tz.POISON).all()
        plan1 = e1.zoom_read_plan(n)
        for i, s in enumerate(streams):
            assert all(np.array_equal(plan1[i][f], plans[i][f]) for f in ("x0", "y0", "w", "h", "track_id")), (what, k, i, plan1[i], plans[i])
            assert np.array_equal(np.minimum(plan1[i]["slot"], 0), np.minimum(plans[i]["slot"], 0)), (what, k, i, plan1[i], plans[i])
            assert e1.track_state(s) == e2.track_state(s) and e1.track_read(s).tobytes() == e2.track_read(s).tobytes(), (what, k, s)
            # the streams' change records: the zoom call's peaks are the suppressed ones, everything else is the plain call's
            r1, r2 = e1.change_read(s), e2.change_read(s)
            ao = chr_.layout(ccfg)[2]
            h1, h2 = r1[:32].view(chr_.HDR_DTYPE).copy(), r2[:32].view(chr_.HDR_DTYPE).copy()
            assert [tuple(int(x) for x in p)[:7] for p in zly.parse_change_record(r1, ccfg.max_peaks)[1]] == all_peaks[i], (what, k, s)
            h1["n_peaks"] = h2["n_peaks"] = 0
            assert h1.tobytes() == h2.tobytes() and np.array_equal(r1[ao:], r2[ao:]), (what, k, s)
            track_regions += int((plans[i]["slot"] >= 0).sum())
    return twin, track_regions


CCFG = chr_.Config(cell=32, threshold_q4=32, max_active_permille=250, max_peaks=3, window_w=208, window_h=208)
# tests/test_gpu_zoom.py's plan config with a class no detection has: tracks take NONE of the K regions, every region is a fallback for the fill.
# (With CFG0 itself the golden pictures' tracks take all three regions of every frame after the first -- measured on an MI355X: 36 of 36.)
NO_TRACK_REGIONS = zoom_ref.Config(regions=3, region_w=208, region_h=208, max_age=2, class_id=10000)


def _steps(sizes, fmt_of, n_steps, jump_at=None):
    return [[(fmt_of(i), w, h, tz._as_format(fmt_of(i), _scene(w, h, k, i, jump=(k == jump_at))), None) for i, (w, h) in enumerate(sizes)] for k in range(n_steps)]


@pytest.mark.parametrize("flags", [0, zly.FLAG_ASYNC_NMS], ids=["in_stream_order", "deferred_nms"])
@pytest.mark.parametrize("mode", list(tz.MODES))
def test_the_extended_rule(weights_path, mode, flags):
    """K = 3 on BGR surfaces over six steps, tracks taking none of the regions: step 0 is FIRST (nothing filled), step 3 moves the whole scene
    and step 4 moves it back (GLOBAL: nothing filled), steps 1, 2 and 5 fill the fallbacks.  With the flag a fourth stream rides along: 16 views, the batch size from which the
    engine defers its NMS"""
    e1, e2 = _zoom_pair(weights_path, tz.MODES[mode] | flags, NO_TRACK_REGIONS, CCFG)
    sizes = tz.SIZES + (((334, 250),) if flags else ())
    twin, track_regions = _run_extended_rule(e1, e2, _steps(sizes, lambda i: BGR, 6, jump_at=3), NO_TRACK_REGIONS, CCFG, (mode, flags))
    assert twin.filled >= 6 and track_regions == 0 and twin.flags >= {0, chr_.FIRST, chr_.GLOBAL}, (twin.filled, track_regions, twin.flags)
    e1.close()
    e2.close()


def test_the_extended_rule_when_tracks_take_every_region(weights_path):
    """tests/test_gpu_zoom.py's own plan config: from the second step on the tracks take the regions, and the peaks inside them are suppressed"""
    e1, e2 = _zoom_pair(weights_path, 0, tz.CFG0, CCFG)
    twin, track_regions = _run_extended_rule(e1, e2, _steps(tz.SIZES, lambda i: BGR, 4), tz.CFG0, CCFG, "tracks")
    print("regions taken by tracks:", track_regions, "filled:", twin.filled)
    assert track_regions >= 9, (track_regions, twin.filled)
    e1.close()
    e2.close()


def test_the_extended_rule_on_five_formats(weights_path):
    """the plane offsets the pick kernel computes: a pitched BGRA surface, NV12 and I420 in one call, YUY2 and tight BGR in another; three steps each"""
    e1, e2 = _zoom_pair(weights_path, 0, NO_TRACK_REGIONS, CCFG)
    filled = 0
    for group in (((BGRA, 418, 240, 4 * 418 + 72), (NV12, 640, 480, None), (I420, 590, 432, None)), ((YUY2, 418, 241, None), (BGR, 333, 251, None))):
        steps = [[(fmt, w, h, tz._as_format(fmt, _scene(w, h, k, i)), pitch) for i, (fmt, w, h, pitch) in enumerate(group)] for k in range(3)]
        for e in (e1, e2):
            e.track_reset(-1, 1)
            e.change_reset(-1)
        twin, _ = _run_extended_rule(e1, e2, steps, NO_TRACK_REGIONS, CCFG, [g[0] for g in group])
        filled += twin.filled
    assert filled >= 5, filled
    e1.close()
    e2.close()


@pytest.mark.parametrize("regions", [1, 15])
def test_the_extended_rule_at_one_and_fifteen_regions(weights_path, regions):
    """K = 1 and K = 15 (sixteen views from one frame) on one 640 x 480 BGR stream.  Both engines' change maps take a frame before the first zoom call,
    so that step 0 -- whose track table is empty: tracks take 0 of the K regions -- is not FIRST and its fallbacks are filled"""
    zcfg = zoom_ref.Config(regions=regions, region_w=208, region_h=208, max_age=2, class_id=-1)
    ccfg = chr_.Config(cell=32, threshold_q4=32, max_active_permille=250, max_peaks=min(regions, 4), window_w=208, window_h=208)
    e1, e2 = _zoom_pair(weights_path, 0, zcfg, ccfg, max_batch=16 if regions == 15 else 2)
    steps = _steps(((640, 480),), lambda i: BGR, 4)
    host, views = tz._pack([(BGR, 640, 480, tz._as_format(BGR, _scene(640, 480, 7, 0)), None)])
    d = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    for e in (e1, e2):
        e.change_device_view(d.data_ptr(), host.nbytes, views, [1])
    e1.sync()
    e2.sync()
    twin, track_regions = _run_extended_rule(e1, e2, steps, zcfg, ccfg, regions)
    print("K", regions, "regions taken by tracks:", track_regions, "filled:", twin.filled)
    assert twin.filled >= 1 and chr_.FIRST not in twin.flags, (twin.filled, twin.flags)
    assert track_regions >= 1
    e1.close()
    e2.close()


def test_with_use_change_off_a_zoom_call_is_what_it_was(weights_path):
    """zly_zoom_use_change(e, 0): the zoom call's slabs and plans equal those of an engine that never enabled a change map, and its own change
    records stay as they were"""
    e1, e0 = _zoom_pair(weights_path, 0, tz.CFG0, CCFG)[0], tz._engine(weights_path)
    e1.zoom_use_change(False)
    sb = e1.slab_bytes
    before = [e1.change_read(s).copy() for s in range(8)]
    for k, surfaces in enumerate(_steps(tz.SIZES, lambda i: BGR, 3)):
        host, views = tz._pack(surfaces)
        d = torch.from_numpy(host).cuda()
        outs = [torch.full((3 * sb,), tz.POISON, dtype=torch.uint8, device="cuda") for _ in range(2)]
        torch.cuda.synchronize()
        for e, o in zip((e1, e0), outs):
            e.detect_device_zoom(d.data_ptr(), host.nbytes, views, [1, 2, 3], d_out_ptr=o.data_ptr(), tag0=k)
            e.sync()
        assert np.array_equal(outs[0].cpu().numpy(), outs[1].cpu().numpy()), k
        assert e1.zoom_read_plan(3).tobytes() == e0.zoom_read_plan(3).tobytes()
    assert all(np.array_equal(e1.change_read(s), before[s]) for s in range(8))
    # ... and the refusals of the switch and of a zoom call with it on
    e1.zoom_use_change(True)
    assert _code(e1.detect_device_zoom, d.data_ptr(), host.nbytes, views[:1], [8]) == ARG               # beyond both tables
    other = tz._engine(weights_path)
    other.change_enable(8, window_w=416, window_h=416)
    assert _code(other.zoom_use_change) == ARG                                                          # the window is not the region
    other.close()
    e1.close()
    e0.close()
