"""The chips on the GPU (include/zly.h "Chips"; csrc/kernels_chips.hip), byte for byte against tests/chip_ref.py: the whole output buffer of every
call -- headers, records, chips and every byte the rule does not write -- must equal the oracle applied to the slabs and frames the call was given.

First the two kernels alone, on hand-written slabs uploaded by the test (no inference): every format, tight and through pitched views in a poisoned
buffer, rectangles of every kind, five chip sizes, both layouts, the large frames where the staging chunks and the row bands meet, the selection.
Then end to end behind the detector, the tracker, the tile merge and the zoom call, and the ordering of zly_chips_surfaces against the updates of
resident surfaces with nothing but enqueues in between."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch            # before the first engine: the process then uses torch's HIP runtime throughout, as tests/test_gpu_parity.py does

import chip_cases as cc
import chip_ref as cr
import zly
import zly_model as zm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = cc.POISON
ARG, INPUT = zly.ERR_INVALID_ARGUMENT, zly.ERR_INVALID_INPUT
BGR, BGRA, NV12, I420, YUY2 = zly.PIX_BGR, zly.PIX_BGRA, zly.PIX_NV12_BT601, zly.PIX_I420_BT709, zly.PIX_YUY2_BT601


def _kernel_constants():
    """the cut kernel's shape constants, parsed from its header: rectangle sizes around them are where it changes path"""
    text = open(os.path.join(ROOT, "zero-latency-yolo_amd", "csrc", "chip_device.h")).read()
    c = {k: int(v) for k, v in re.findall(r"#define\s+(ZLY_CHIP_(?:THREADS|CHUNK_PX|BAND_ROWS))\s+(\d+)", text)}
    assert set(c) == {"ZLY_CHIP_THREADS", "ZLY_CHIP_CHUNK_PX", "ZLY_CHIP_BAND_ROWS"}, c
    return c


CONSTS = _kernel_constants()


def _engine(weights_path, cfg, max_batch=4, max_dets=16, flags=0, enable=True, **kw):
    e = zly.Engine(weights_path, dtype=zly.DTYPE_BF16, max_batch=max_batch, max_dets=max_dets, conf_thr=0.05, warmup_runs=0, flags=flags, **kw)
    if enable:
        e.chips_enable(chip_w=cfg.chip_w, chip_h=cfg.chip_h, max_chips=cfg.max_chips, class_id=cfg.class_id, scale=cfg.scale, layout=cfg.layout)
        assert e.chip_layout() == cr.layout(cfg)[:3]
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


def _cut(e, cfg, items, slabs, bgrs):
    """one zly_chips_device_view call on uploaded frames and slabs into a poisoned buffer of the test's; the whole buffer against the oracle"""
    n = len(items)
    host, views = _pack(items)
    slabs = np.ascontiguousarray(np.stack(slabs))
    sb = cr.layout(cfg)[0]
    before = np.full((n, sb), POISON, dtype=np.uint8)
    d_base, d_slabs, d_chips = torch.from_numpy(host).cuda(), torch.from_numpy(slabs).cuda(), torch.from_numpy(before).cuda()
    torch.cuda.synchronize()
    e.chips_device_view(d_base.data_ptr(), host.nbytes, views, d_slabs_ptr=d_slabs.data_ptr(), d_chips_ptr=d_chips.data_ptr())
    e.sync()
    torch.cuda.synchronize()
    got = d_chips.cpu().numpy()
    want = cr.chip_slabs(slabs, bgrs, cfg, before, cap=e.max_dets)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        hdrs = [got[i, :16].view(cr.HDR_DTYPE)[0] for i in range(n)]
        raise AssertionError(f"{len(bad)} bytes differ, first at (frame, byte) {bad[:4].tolist()}; headers {hdrs}; pixels_off {cr.layout(cfg)[1]}, stride {cr.layout(cfg)[2]}")
    return got


def _rects(W, H, cw, ch, odd):
    """the rectangles the issue lists, clipped to what a W x H frame holds: 1 x 1; the whole frame; exactly the chip's size; smaller than the chip
    in one axis and larger in the other; at all four borders; odd origins"""
    r = [(W // 2, H // 2, 1, 1), (0, 0, W, H)]
    if cw <= W and ch <= H:
        r.append((min(3, W - cw), min(5, H - ch), cw, ch))
    r += [(W // 4, H // 4, max(min(cw // 2, W // 2), 1), max(min(2 * ch + 1, H // 2), 1)), (W // 5, H // 5, max(min(2 * cw + 3, W // 2), 1), max(min(ch // 2, H // 2), 1))]
    r += [(0, H // 3, max(W // 3, 1), max(H // 3, 1)), (W - max(W // 3, 1), H // 3, max(W // 3, 1), max(H // 3, 1)),
          (W // 3, 0, max(W // 3, 1), max(H // 3, 1)), (W // 3, H - max(H // 3, 1), max(W // 3, 1), max(H // 3, 1))]
    if odd and W > 8 and H > 8:
        r += [(1, 1, W - 2, H - 2), (5, 3, 7, 5), (W - 4, H - 6, 3, 5)]
    return r


def _slab_for(rects, W, H, cfg, cap, tag):
    dets = [cc.box(x0, y0, rw, rh, W, H, cfg.scale, conf=0.95 - 0.01 * k, cls=k % 3, track=1000 + k) for k, (x0, y0, rw, rh) in enumerate(rects)]
    assert len(dets) <= cap
    return cr.make_slab(dets, cap=cap, frame_tag=tag, fill=0xEE)


# ---- 1. the kernels alone -------------------------------------------------------------------------------------------------------------------
CHIP_SHAPES = [(1, 1, cr.BGR8), (8, 8, cr.BGR8), (8, 8, cr.RGB_F32), (33, 17, cr.RGB_F32), (33, 17, cr.BGR8), (64, 64, cr.BGR8), (256, 256, cr.BGR8), (256, 256, cr.RGB_F32)]


@pytest.mark.parametrize("cw,ch,layout", CHIP_SHAPES)
def test_every_format_tight_and_pitched(weights_path, cw, ch, layout):
    """per format one call of four frames: 64 x 48 tight and as a pitched view between poisoned bytes, and the smallest legal frame likewise"""
    cfg = cr.Config(chip_w=cw, chip_h=ch, max_chips=16, class_id=-1, scale=1.25, layout=layout)
    e = _engine(weights_path, cfg)
    for fmt in cc.ALL_FORMATS:
        items, slabs, bgrs = [], [], []
        for (w, h) in ((64, 48), cc.smallest(fmt)):
            f, bgr = cc.frame(fmt, w, h, seed=3)
            slab = _slab_for(_rects(w, h, cw, ch, odd=True), w, h, cfg, 16, tag=fmt * 100 + w)
            items += [(f, cc.tight_view(fmt, w, h)), cc.pitched(f, fmt, w, h)]
            slabs += [slab, slab]
            bgrs += [bgr, bgr]
        got = _cut(e, cfg, items, slabs, bgrs)
        assert int(got[0, :16].view(cr.HDR_DTYPE)[0]["n_chips"]) >= 11
    e.close()


def test_large_frames_where_chunks_and_bands_meet(weights_path):
    """a 1000 x 1000 rectangle of a 1920 x 1080 BGRA frame (16 bands of 63 rows, one staging unit per row) and the full width of a 16384 x 2 BGR frame
    (17 staging units per row, every chip row from the same two source rows)"""
    cfg = cr.Config(chip_w=64, chip_h=64, max_chips=4, scale=1.0)
    e = _engine(weights_path, cfg, max_batch=2)
    f0, b0 = cc.frame(BGRA, 1920, 1080, seed=11)
    f1, b1 = cc.frame(BGR, 16384, 2, seed=12)
    s0 = _slab_for([(455, 37, 1000, 1000), (0, 0, 1920, 1080), (919, 79, 1001, 1001)], 1920, 1080, cfg, 16, tag=1)
    s1 = _slab_for([(0, 0, 16384, 2), (1, 1, 16383, 1)], 16384, 2, cfg, 16, tag=2)
    _cut(e, cfg, [(f0, cc.tight_view(BGRA, 1920, 1080)), (f1, cc.tight_view(BGR, 16384, 2))], [s0, s1], [b0, b1])
    e.close()


@pytest.mark.parametrize("fmt", [BGR, BGRA, NV12, I420, YUY2])
def test_rectangles_around_the_kernels_shape_constants(weights_path, fmt):
    """rectangle widths and heights one below, at and one above the workgroup's width, a staging chunk (and two of them) and the row band, from odd origins"""
    cfg = cr.Config(chip_w=33, chip_h=17, max_chips=16, scale=1.0)
    e = _engine(weights_path, cfg, max_batch=1)
    W, H = 2 * CONSTS["ZLY_CHIP_CHUNK_PX"] + 8, CONSTS["ZLY_CHIP_CHUNK_PX"] + 4
    f, bgr = cc.frame(fmt, W, H, seed=21)
    sizes = []
    for c in (CONSTS["ZLY_CHIP_BAND_ROWS"], CONSTS["ZLY_CHIP_THREADS"], CONSTS["ZLY_CHIP_CHUNK_PX"]):
        sizes += [c - 1, c, c + 1]
    rects = [(1 + (k & 1) * 2, 1 + (k % 3), s, sizes[(k + 4) % len(sizes)]) for k, s in enumerate(sizes)]
    rects += [(3, 2, 2 * CONSTS["ZLY_CHIP_CHUNK_PX"] + d, 5) for d in (-1, 0, 1)]                  # a second staging unit of one pixel, none, and two
    rects += [(1019, 0, 4, 3), (1020, 1, 2, 2)]                                                     # rectangles that begin at a chunk seam of the frame
    _cut(e, cfg, [cc.pitched(f, fmt, W, H, pad=3, lead=1)], [_slab_for(rects, W, H, cfg, 16, tag=7)], [bgr])
    e.close()


def test_upscale_identity_and_constant_frames(weights_path):
    """the rule's consequences on the device: a rectangle of the chip's size returns the source pixels, a one-pixel rectangle its pixel, a constant frame constant chips"""
    cfg = cr.Config(chip_w=8, chip_h=8, max_chips=8, scale=1.0)
    e = _engine(weights_path, cfg, max_batch=4)
    items, slabs, bgrs = [], [], []
    for fmt in (BGR, NV12, YUY2, zly.PIX_RGBA):
        f, bgr = cc.constant_frame(fmt, 40, 30, 90 + fmt) if fmt != BGR else cc.frame(fmt, 40, 30, seed=5)
        items.append((f, cc.tight_view(fmt, 40, 30)))
        slabs.append(_slab_for([(7, 9, 8, 8), (11, 4, 1, 1), (0, 0, 40, 30), (3, 3, 2, 17)], 40, 30, cfg, 16, tag=fmt))
        bgrs.append(bgr)
    got = _cut(e, cfg, items, slabs, bgrs)
    sb, po, st, cb = cr.layout(cfg)
    assert np.array_equal(got[0, po:po + cb].reshape(8, 8, 3), bgrs[0][9:17, 7:15])
    assert (got[0, po + st:po + st + cb].reshape(8, 8, 3) == bgrs[0][4, 11]).all()
    for i in (1, 2, 3):
        assert all((got[i, po + j * st:po + j * st + cb].reshape(64, 3) == bgrs[i][0, 0]).all() for j in range(4))
    e.close()


def test_rectangle_arithmetic_is_not_contracted(weights_path):
    """boxes whose rectangle an fma in lo / hi would move by a pixel (found by search against the oracle; tests/test_chip_ref.py holds the first by hand)"""
    cfg = cr.Config(chip_w=4, chip_h=2, max_chips=4, scale=1.25)
    e = _engine(weights_path, cfg, max_batch=1)
    f, bgr = cc.frame(BGR, 1920, 2, seed=9)
    bits = lambda u: float(np.array(u, dtype=np.uint32).view(np.float32))      # noqa: E731
    dets = [(bits(1058274016), 0.5, bits(1050864689), 0.5, 0.9, 0, 1), (bits(1064584439), 0.5, bits(1042313654), 0.5, 0.8, 0, 2)]
    got = _cut(e, cfg, [(f, cc.tight_view(BGR, 1920, 2))], [cr.make_slab(dets, cap=16)], [bgr])
    recs = got[0, 16:16 + 64].view(cr.REC_DTYPE)
    assert [(int(r["x0"]), int(r["w"])) for r in recs] == [(728, 763), (1643, 277)]
    e.close()


def test_selection_on_mixed_formats_at_max_batch(weights_path):
    """slabs of up to 80 detections walked 64 at a time, a class filter, n_eligible of 0, at and above max_chips, n_kept above cap and negative; six
    frames of six formats in one call (n = max_batch), then one alone (n = 1)"""
    cap = 80
    cfg = cr.Config(chip_w=2, chip_h=3, max_chips=40, class_id=1, scale=1.5, layout=cr.RGB_F32)
    e = _engine(weights_path, cfg, max_batch=6, max_dets=cap)
    rng = np.random.default_rng(31)

    def dets(classes):
        return [(float(rng.uniform(-0.1, 1.1)), float(rng.uniform(-0.1, 1.1)), float(rng.uniform(0, 0.6)), float(rng.uniform(0, 0.6)), 0.9 - 0.01 * k, c, 7 + k)
                for k, c in enumerate(classes)]
    specs = [dict(dets=dets([k % 2 for k in range(76)])),                                   # 38 eligible, some behind detection 64
             dict(dets=dets([1] * 80), n_kept=200, flags=zly.SLAB_OVERFLOW),                # n_kept above cap: K = 80, 80 eligible, 40 chips
             dict(dets=dets([0, 2, 3, 0])),                                                 # none eligible
             dict(dets=dets([1] * 40)),                                                     # exactly max_chips
             dict(dets=dets([1, 1, 1]), n_kept=-5),                                         # negative: K = 0
             dict(dets=dets([0] * 64 + [1] * 3))]                                           # the only eligible ones in the second round of 64
    fmts = (BGR, NV12, YUY2, BGRA, I420, zly.PIX_RGB)
    items, slabs, bgrs = [], [], []
    for i, (fmt, sp) in enumerate(zip(fmts, specs)):
        w, h = cc.legal(fmt, 37 + 2 * i, 21 + i)
        f, bgr = cc.frame(fmt, w, h, seed=60 + i)
        items.append(cc.pitched(f, fmt, w, h) if i % 2 else (f, cc.tight_view(fmt, w, h)))
        slabs.append(cr.make_slab(sp["dets"], cap=cap, n_kept=sp.get("n_kept"), flags=sp.get("flags", 0), frame_tag=500 + i, fill=0x11))
        bgrs.append(bgr)
    got = _cut(e, cfg, items, slabs, bgrs)
    heads = [tuple(int(v) for v in got[i, :16].view(np.int32)[:2]) for i in range(6)]
    assert heads == [(38, 38), (40, 80), (0, 0), (40, 40), (0, 0), (3, 3)]
    _cut(e, cfg, items[:1], slabs[:1], bgrs[:1])
    e.close()


# ---- 2. refusals ------------------------------------------------------------------------------------------------------------------------------
def _code(f, *a, **k):
    with pytest.raises(zly.ZlyError) as ei:
        f(*a, **k)
    return ei.value.code


def test_refusals(weights_path):
    cfg = cr.Config(chip_w=4, chip_h=4, max_chips=4)
    plain = _engine(weights_path, cfg, max_batch=2, enable=False)
    f, _ = cc.frame(BGR, 16, 8, seed=1)
    d = torch.from_numpy(np.concatenate([f, np.zeros(64, np.uint8)])).cuda()
    d_slabs = torch.zeros(2 * plain.slab_bytes, dtype=torch.uint8, device="cuda")
    d_chips = torch.full((1 << 16,), POISON, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    v = zly.view_tight(BGR, 16, 8)
    # an engine without chips refuses every call of the section
    assert _code(plain.chips_device_view, d.data_ptr(), f.size, [v], d_slabs_ptr=d_slabs.data_ptr(), d_chips_ptr=d_chips.data_ptr()) == ARG
    assert _code(plain.chips_surfaces, [0]) == ARG and _code(plain.read_chips, 1) == ARG and _code(plain.chip_layout) == ARG
    for bad in (dict(chip_w=0), dict(chip_h=257), dict(max_chips=0), dict(max_chips=17), dict(class_id=-2), dict(scale=0.5), dict(scale=4.01),
                dict(scale=float("nan")), dict(scale=float("inf")), dict(layout=2)):
        assert _code(plain.chips_enable, **bad) == ARG, bad
    assert plain.lib.zly_chips_enable(plain.h, None) == ARG
    c = zly.ChipConfig()
    plain.lib.zly_default_chip_config(plain.h, C.byref(c))
    assert (c.chip_w, c.chip_h, c.max_chips, c.class_id, c.scale, c.layout) == (64, 64, 16, -1, 1.25, zly.CHIP_BGR8)
    plain.chips_enable(chip_w=4, chip_h=4, max_chips=4)
    assert _code(plain.chips_enable) == ARG                                                           # twice
    e = plain
    kw = dict(d_slabs_ptr=d_slabs.data_ptr(), d_chips_ptr=d_chips.data_ptr())
    assert _code(e.chips_device_view, d.data_ptr(), f.size, [], **kw) == ARG                          # n = 0
    assert _code(e.chips_device_view, d.data_ptr(), f.size, [v, v, v], **kw) == ARG                   # n above max_batch
    assert e.lib.zly_chips_device_view(e.h, 1, d.data_ptr(), f.size, None, d_slabs.data_ptr(), 0, d_chips.data_ptr(), None) == ARG      # null views
    assert _code(e.chips_device_view, d.data_ptr(), f.size, [v], source=2, d_chips_ptr=d_chips.data_ptr()) == ARG
    assert _code(e.chips_device_view, d.data_ptr(), f.size, [v], source=zly.CHIPS_SRC_MERGED, **kw) == ARG        # a source beside d_slabs
    assert _code(e.chips_device_view, d.data_ptr(), f.size, [v], source=zly.CHIPS_SRC_MERGED, d_chips_ptr=d_chips.data_ptr()) == ARG     # no merge yet
    assert _code(e.chips_surfaces, [0], **kw) == ARG                                                  # no store
    bad_fmt, odd, short, wide = zly.view_tight(BGR, 16, 8), zly.view_tight(BGR, 16, 8), zly.view_tight(BGR, 16, 8), zly.FrameView()
    bad_fmt.fmt = 5
    odd.fmt = NV12
    odd.w = 15
    short.pitch[0] = 47
    wide.fmt, wide.w, wide.h = BGR, 16385, 1
    wide.pitch[0] = 3 * 16385
    assert _code(e.chips_device_view, d.data_ptr(), f.size, [bad_fmt], **kw) == ARG
    assert _code(e.chips_device_view, d.data_ptr(), f.size, [odd], **kw) == INPUT
    assert _code(e.chips_device_view, d.data_ptr(), f.size, [short], **kw) == INPUT
    assert _code(e.chips_device_view, d.data_ptr(), f.size - 1, [v], **kw) == INPUT                   # the view needs one byte more
    assert _code(e.chips_device_view, d.data_ptr(), 1 << 20, [wide], **kw) == INPUT                   # above ZLY_AREA_MAX_DIM (the size claimed would hold it)
    e.surfaces_enable(2, 16 * 8 * 3)
    assert _code(e.chips_surfaces, [0], **kw) == ARG                                                  # an undefined slot, as zly_detect_surfaces
    assert _code(e.chips_surfaces, [2], **kw) == ARG
    e.surface_define(0, BGR, 16, 8)
    assert _code(e.chips_surfaces, [0], **kw) == INPUT                                                # defined, no keyframe
    e.sync()
    torch.cuda.synchronize()
    assert (d_chips.cpu().numpy() == POISON).all()                                                    # a refused call enqueues nothing
    # ... and the same call, accepted, writes its header
    e.surface_update([(0, 0, 0, f, v)])
    e.chips_surfaces([0], **kw)
    e.sync()
    torch.cuda.synchronize()
    assert d_chips.cpu().numpy()[:16].view(np.int32).tolist() == [0, 0, 0, 0]
    e.close()


# ---- 3. end to end --------------------------------------------------------------------------------------------------------------------------
E2E_CFG = cr.Config(chip_w=32, chip_h=24, max_chips=8, class_id=-1, scale=1.25, layout=cr.BGR8)
MODES = {"stretch": 0, "letterbox": zly.FLAG_LETTERBOX, "area": zly.FLAG_AREA}


def _raw(e, fn, n):
    raw = np.zeros((n, e.slab_bytes), dtype=np.uint8)
    assert fn(e.h, n, raw.ctypes.data) == zly.OK
    return raw


def _expect_engine_chips(e, cfg, raw_slabs, bgrs, min_chips):
    """zly_read_chips of the engine-owned buffer against the oracle on the slabs read back: headers, records and chips (the buffer's other bytes are
    the engine's: zero, or an earlier call's)"""
    n = len(bgrs)
    got = e.read_chips(n)
    want = cr.chip_slabs(raw_slabs, bgrs, cfg, got, cap=e.max_dets)
    assert np.array_equal(got, want), np.argwhere(got != want)[:4].tolist()
    total = sum(int(got[i, :16].view(np.int32)[0]) for i in range(n))
    assert total >= min_chips, total                                   # the comparison is not one of empty slabs
    return got


def _three_frames(seed):
    out = []
    for i, (fmt, w, h) in enumerate(((BGR, 640, 480), (BGRA, 418, 330), (NV12, 800, 600))):
        bgr = np.ascontiguousarray(zm.synth_frames(1, w, h, seed=seed + i)[0])
        if fmt == BGRA:
            f = np.concatenate([bgr, np.full((h, w, 1), 200, np.uint8)], axis=2).reshape(-1)
        elif fmt == NV12:
            import yuv_ref as yr
            f = yr.bgr_to_yuv420(bgr, fmt)
        else:
            f = bgr.reshape(-1)
        out.append((fmt, w, h, np.ascontiguousarray(f), np.ascontiguousarray(cr.bgr_of(fmt, f, w, h))))
    return out


@pytest.mark.parametrize("mode", list(MODES))
def test_chips_behind_the_detector_and_the_tracker(weights_path, mode):
    """zly_detect_device_view on three frames of three formats, then chips from the engine's own slabs; the same with zly_track_slabs in between:
    the records carry the track ids"""
    e = _engine(weights_path, E2E_CFG, max_batch=4, max_dets=32, flags=MODES[mode])
    e.track_enable(max_streams=4, max_tracks=64)
    frames = _three_frames(700)
    host, views = _pack([(f, cc.tight_view(fmt, w, h)) for fmt, w, h, f, _ in frames])
    bgrs = [b for *_, b in frames]
    d = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    e.detect_device_view(d.data_ptr(), host.nbytes, views, tag0=40)
    e.chips_device_view(d.data_ptr(), host.nbytes, views)
    raw = _raw(e, e.lib.zly_read_slabs, 3)
    got = _expect_engine_chips(e, E2E_CFG, raw, bgrs, min_chips=6)
    assert all(int(r["track_id"]) == 0 for i in range(3) for r in zly.parse_chip_slab(got[i], 32, 24, 8, 0, *e.chip_layout()[1:])[1])
    e.detect_device_view(d.data_ptr(), host.nbytes, views, tag0=50)
    e.track_slabs([0, 1, 2])
    e.chips_device_view(d.data_ptr(), host.nbytes, views)
    raw = _raw(e, e.lib.zly_read_slabs, 3)
    got = _expect_engine_chips(e, E2E_CFG, raw, bgrs, min_chips=6)
    recs = [r for i in range(3) for r in zly.parse_chip_slab(got[i], 32, 24, 8, 0, *e.chip_layout()[1:])[1]]
    assert all(int(r["track_id"]) != 0 for r in recs) and [int(h) for h in got[:, 8:12].view(np.uint32).reshape(-1)] == [50, 51, 52]
    e.close()


def test_chips_of_merged_tiles_and_of_a_zoomed_surface(weights_path):
    """zly_merge_slabs on a tile grid, then ZLY_CHIPS_SRC_MERGED with the surface's view; zly_detect_surfaces_zoom, then zly_chips_surfaces"""
    e = _engine(weights_path, E2E_CFG, max_batch=12, max_dets=32)
    W = H = 832
    pic = np.ascontiguousarray(zm.synth_frames(1, W, H, seed=810)[0])
    tiles = zly.tile_grid(W, H, 416, 416, 32, 32)
    surf = zly.view_tight(BGR, W, H)
    d = torch.from_numpy(pic.reshape(-1)).cuda()
    torch.cuda.synchronize()
    e.detect_device_view(d.data_ptr(), pic.nbytes, [zly.view_crop(surf, t.x0, t.y0, t.w, t.h) for t in tiles])
    e.merge_slabs(tiles, tag0=77)
    e.chips_device_view(d.data_ptr(), pic.nbytes, [surf], source=zly.CHIPS_SRC_MERGED)
    raw = _raw(e, e.lib.zly_read_merged, 1)
    got = _expect_engine_chips(e, E2E_CFG, raw, [pic], min_chips=3)
    assert int(got[0, 8:12].view(np.uint32)[0]) == 77
    # the zoom call on a resident surface: its merged, tracked slab lies in the merge's buffer too
    e.track_enable(max_streams=2, max_tracks=64)
    e.zoom_enable(regions=2)
    e.surfaces_enable(1, W * H * 3)
    e.surface_define(0, BGR, W, H)
    for step in range(2):
        e.surface_update([(0, 0, 0, pic.reshape(-1), surf)])
        e.detect_surfaces_zoom([0], [1], tag0=90 + step)
        e.chips_surfaces([0], source=zly.CHIPS_SRC_MERGED)
    raw = _raw(e, e.lib.zly_read_merged, 1)
    got = _expect_engine_chips(e, E2E_CFG, raw, [pic], min_chips=3)
    recs = zly.parse_chip_slab(got[0], 32, 24, 8, 0, *e.chip_layout()[1:])[1]
    assert int(got[0, 8:12].view(np.uint32)[0]) == 91 and all(int(r["track_id"]) != 0 for r in recs)
    e.close()


# ---- 4. ordering ------------------------------------------------------------------------------------------------------------------------------
def test_update_detect_chips_update_with_nothing_but_enqueues(weights_path):
    """update k on the engine's stream, zly_detect_surfaces k on a CALLER's stream, zly_chips_surfaces k, update k + 1, ... over six steps and two
    streams, every step a whole new picture.  The chips of step k must be cut from picture k with the boxes of step k: a patch kernel that overtook
    the cut kernel would hand it the next picture, a cut kernel that overtook the NMS the boxes of the step before."""
    e = _engine(weights_path, E2E_CFG, max_batch=2, max_dets=32)
    W, Hh, steps = 960, 540, 6
    pics = [np.ascontiguousarray(f) for f in zm.synth_frames(steps, W, Hh, seed=900)]
    films = [np.ascontiguousarray(np.concatenate([p, np.full((Hh, W, 1), 255, np.uint8)], axis=2)).reshape(-1) for p in pics]
    whole = zly.view_tight(BGRA, W, Hh)
    sb, csb = e.slab_bytes, e.chip_layout()[0]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    d_slabs = torch.zeros(steps * sb, dtype=torch.uint8, device="cuda")
    d_chips = torch.full((steps * csb,), POISON, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    e.surfaces_enable(1, W * Hh * 4)
    e.surface_define(0, BGRA, W, Hh)
    for k in range(steps):
        s = streams[k % 2].cuda_stream
        e.surface_update([(0, 0, 0, films[k], whole)])
        e.detect_surfaces([0], d_slabs_ptr=d_slabs.data_ptr() + k * sb, tag0=k, stream=s)
        e.chips_surfaces([0], d_slabs_ptr=d_slabs.data_ptr() + k * sb, d_chips_ptr=d_chips.data_ptr() + k * csb, stream=s)
    for s in streams:
        s.synchronize()
    e.sync()
    raw = d_slabs.cpu().numpy().reshape(steps, sb)
    got = d_chips.cpu().numpy().reshape(steps, csb)
    want = cr.chip_slabs(raw, pics, E2E_CFG, np.full((steps, csb), POISON, dtype=np.uint8), cap=32)
    assert np.array_equal(got, want), np.argwhere(got != want)[:4].tolist()
    heads = [got[k, :16].view(np.int32) for k in range(steps)]
    assert all(int(h[0]) >= 1 for h in heads) and [int(h[2]) for h in heads] == list(range(steps))
    # the pictures tell each other apart: chips cut from a neighbour's picture would have failed above
    po, cb = cr.layout(E2E_CFG)[1], cr.layout(E2E_CFG)[3]
    assert all(not np.array_equal(got[k, po:po + cb], got[k + 1, po:po + cb]) for k in range(steps - 1))
    e.close()
