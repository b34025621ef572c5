"""The area-average resize filter (include/zly.h ZLY_FLAG_AREA) on the GPU, bit-exact throughout against tests/area_ref.py: the pre-pass of an
area engine must produce, for a request frame of any format, tight or through a view, exactly area_resize(its BGR conversion), so that the engine
gives what the engine without the flag gives for that model-sized frame -- and boxes come back mapped from the request's size, on every entry
point that takes frames.  Mirrors tests/test_gpu_letterbox.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch            # before the first engine: the process then uses torch's HIP runtime throughout, as tests/test_gpu_parity.py does

import area_ref as ar
import letterbox_ref as lb
import pixfmt_ref as pr
import view_ref as vr
import yuv422_ref as y2
import yuv_ref as yr
import zly
import zly_model as zm
from oracle_lib import det_fields_equal

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AREA, LBF = zly.FLAG_AREA, zly.FLAG_LETTERBOX
MODES = [pytest.param(AREA, id="area"), pytest.param(AREA | LBF, id="letterbox_area")]
CONF, IOU = 0.05, 0.45
POISON = 0xA5


def _kernel_constants():
    """the staging-chunk and row-band sizes of the pre-pass kernel, parsed from its header: sizes around them are where it changes path"""
    text = open(os.path.join(ROOT, "zero-latency-yolo_amd", "csrc", "area_device.h")).read()
    c = {k: int(v) for k, v in re.findall(r"#define\s+(ZLY_AREA_[A-Z_]+)\s+(\d+)", text)}
    assert set(c) == {"ZLY_AREA_THREADS", "ZLY_AREA_CHUNK_PX", "ZLY_AREA_BAND_ROWS", "ZLY_AREA_BAND_SMALL"}, c
    return sorted(set(c.values()))


CONSTS = _kernel_constants()
BASE_SIZES = [(416, 416), (832, 832), (1920, 1080), (417, 415), (100, 62), (233, 416),
              (1, 1), (2, 2), (3, 1001), (4000, 3), (16384, 2), (2, 16384)]
# one below, at and one above every constant, as a width and as a height
EDGE_SIZES = [s for c in CONSTS for s in ((c - 1, c + 1), (c, c), (c + 1, c - 1))]
SIZES = BASE_SIZES + [s for s in EDGE_SIZES if s not in BASE_SIZES]

F420 = yr.YUV_FORMATS
F422 = y2.FORMATS
FPK = pr.PACKED
# four sizes per format that are legal for it; 2 x 2 for 4:2:0 and 2 x 1 for 4:2:2 among them
FMT_SIZES = {**{f: [(2, 2), (100, 62), (418, 330), (1920, 1080)] for f in F420},
             **{f: [(2, 1), (100, 63), (418, 331), (1920, 1080)] for f in F422},
             **{f: [(1, 1), (100, 62), (417, 415), (1920, 1080)] for f in FPK}}
assert len(FMT_SIZES) == 11


def _bgr(w, h, seed):
    return np.ascontiguousarray(zm.synth_frames(1, w, h, seed=seed, rects=w >= 16 and h >= 16)[0])


_FRAMES = {}


def _any_frame(fmt, w, h, seed):
    """(frame as the engine takes it, the BGR frame it stands for): made once and shared (never modified)"""
    k = (fmt, w, h, seed)
    if k not in _FRAMES:
        _FRAMES[k] = _make_frame(fmt, w, h, seed)
        for a in _FRAMES[k]:
            a.setflags(write=False)
    return _FRAMES[k]


def _make_frame(fmt, w, h, seed):
    if fmt == zly.PIX_BGR:
        b = _bgr(w, h, seed)
        return b, b
    if fmt in F422:
        f = y2.from_bgr(_bgr(w, h, seed), fmt)
        return f, y2.to_bgr(f, w, h, fmt)
    if fmt in FPK:
        f = pr.from_bgr(_bgr(w, h, seed), fmt, x=np.random.default_rng(seed + 7).integers(0, 256, (h, w), dtype=np.uint8))
        return f, pr.to_bgr(f, w, h, fmt)
    y = yr.bgr_to_yuv420(_bgr(w, h, seed), fmt)
    return y, yr.yuv420_to_bgr(y, w, h, fmt)


_WANT = {}


def _want_planar(key, bgr, tw, th, letterbox):
    """the oracle's tensor for a frame, computed once per (frame key, model, geometry) and shared by the tests (never modified)"""
    k = (key, tw, th, bool(letterbox))
    if k not in _WANT:
        _WANT[k] = ar.preprocess_planar(bgr, tw, th, letterbox)
        _WANT[k].setflags(write=False)
    return _WANT[k]


def _same_results(a, b):
    return len(a) == len(b) and all(na == nb and det_fields_equal(da, db) for (da, na), (db, nb) in zip(a, b))


def _slab_results(e, n):
    return [(d, int(h["n_kept"])) for h, d in e.read_slabs(n)]


def _raw_slabs(e, n):
    raw = np.zeros(n * e.slab_bytes, dtype=np.uint8)
    assert e.lib.zly_read_slabs(e.h, n, raw.ctypes.data) == zly.OK
    return raw


def _eq_words(got, want):
    return np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ---- 1. preprocess equals the oracle, as uint32 words ----------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", MODES)
@pytest.mark.parametrize("dtype", [zly.DTYPE_FP32, zly.DTYPE_BF16])
def test_preprocess_bgr_every_size(weights_path, dtype, flags):
    e = zly.Engine(weights_path, dtype=dtype, max_batch=1, warmup_runs=0, flags=flags)
    for k, (w, h) in enumerate(SIZES):
        f = _bgr(w, h, seed=100 + k)
        got = e.preprocess(f)
        want = _want_planar(("bgr", w, h, 100 + k), f, 416, 416, flags & LBF)
        assert _eq_words(got, want), (w, h, int((got != want).sum()))
    e.close()


@pytest.mark.parametrize("flags", MODES)
@pytest.mark.parametrize("dtype", [zly.DTYPE_FP32, zly.DTYPE_BF16])
def test_preprocess_every_other_format(weights_path, dtype, flags):
    e = zly.Engine(weights_path, dtype=dtype, max_batch=1, warmup_runs=0, flags=flags)
    for fmt, sizes in FMT_SIZES.items():
        for k, (w, h) in enumerate(sizes):
            f, bgr = _any_frame(fmt, w, h, seed=200 + k)
            got = e.preprocess(f, fmt=fmt, w=w, h=h)
            want = _want_planar(("fmt", fmt, w, h, 200 + k), bgr, 416, 416, flags & LBF)
            assert _eq_words(got, want), (fmt, w, h, int((got != want).sum()))
    e.close()


def test_preprocess_non_square_model(weights_path):
    for flags in (AREA, AREA | LBF):
        e = zly.Engine(weights_path, dtype=zly.DTYPE_FP32, model_w=640, model_h=384, max_batch=1, warmup_runs=0, flags=flags)
        for k, (w, h) in enumerate([(1920, 1080), (384, 640), (640, 384), (100, 62), (1021, 17)]):
            f = _bgr(w, h, seed=150 + k)
            assert _eq_words(e.preprocess(f), _want_planar(("bgr", w, h, 150 + k), f, 640, 384, flags & LBF)), (w, h, flags)
        e.close()


def _packed_view(fmt, bgr_like, w, h, pitch_pad, base_off, x0, y0):
    """a frame of a one-plane format as the crop at (x0, y0) of a pitched surface that begins at the odd byte base_off of a poisoned buffer"""
    bpp = 2 if fmt in F422 else pr.BPP[fmt]
    pitch = (x0 + w) * bpp + pitch_pad
    off = base_off + y0 * pitch + x0 * bpp
    off += 1 - off % 2                                            # the region's first byte at an odd offset, whatever the origin's parity
    if fmt in F422:
        buf, _ = y2.embed(bgr_like, w, h, pitch, off, tail=3, fill=POISON)
    else:
        buf, _ = pr.embed(bgr_like, fmt, pitch, off, tail=3, fill=POISON)
    c = zly.FrameView()
    c.fmt, c.w, c.h = fmt, w, h
    c.off[0], c.pitch[0] = off, pitch
    return buf, c


def _view_cases():
    """three views per format family: pitch > row bytes, odd byte offsets, a crop origin != 0 (one of them wider than a staging chunk)"""
    geo = [(642, 360, 7, 3, 5, 2), (100, 62, 1, 1, 11, 9), (CONSTS[-1] * 2 + 6, 10, 13, 5, 3, 1)]
    cases = []
    for i, (w, h, pad, base, x0, y0) in enumerate(geo):
        # packed family (BGR, RGB, BGRA, RGBA in turn) and packed 4:2:2 (x0 even)
        for fmt in ((zly.PIX_BGR, zly.PIX_BGRA, zly.PIX_RGB)[i], (zly.PIX_RGBA, zly.PIX_BGR, zly.PIX_BGRA)[i], F422[i], F422[3 - i]):
            f, bgr = _any_frame(fmt, w, h, seed=300 + i)
            buf, c = _packed_view(fmt, f, w, h, pad, base, x0 & ~1 if fmt in F422 else x0, y0)
            cases.append((fmt, w, h, buf, c, bgr, ("view", fmt, i)))
        # 4:2:0: a crop at an even origin of a pitched surface, the buffer shifted by an odd number of bytes
        for fmt in (F420[i], F420[3 - i]):
            f, bgr = _any_frame(fmt, w, h, seed=300 + i)
            sw, sh = w + 2 * x0 + 4, h + 2 * y0 + 2
            pitches = [rb + pad + p for p, (_, rb) in enumerate(vr.plane_shapes(fmt, sw, sh))]
            buf, v = vr.embed(f, fmt, sw, sh, pitches, 2 * x0, 2 * y0, POISON, w=w, h=h)
            buf = np.concatenate([np.full(base, POISON, np.uint8), buf])
            cases.append((fmt, w, h, buf, vr.to_c(vr.shift(v, base)), bgr, ("view", fmt, i)))
    return cases


@pytest.mark.parametrize("flags", MODES)
def test_preprocess_views_in_a_poisoned_buffer(weights_path, flags):
    e = zly.Engine(weights_path, dtype=zly.DTYPE_FP32, max_batch=1, warmup_runs=0, flags=flags)
    cases = _view_cases()
    assert len(cases) == 18
    for fmt, w, h, buf, c, bgr, key in cases:
        assert c.pitch[0] > w * (1 if fmt in F420 else 2 if fmt in F422 else pr.BPP[fmt]) and c.off[0] % 2 == 1
        got = e.preprocess_view(buf, c)
        assert _eq_words(got, _want_planar(key, bgr, 416, 416, flags & LBF)), (fmt, w, h)
    e.close()


# ---- 2. the whole path ---------------------------------------------------------------------------------------------------------------
MIX = [(zly.PIX_BGRA, 1920, 1080), (zly.PIX_NV12_BT601, 640, 480), (zly.PIX_BGR, 233, 416), (zly.PIX_UYVY_BT709, 418, 331)]


def _mix(seed):
    pairs = [_any_frame(f, w, h, seed=seed + i) for i, (f, w, h) in enumerate(MIX)]
    return [p[0] for p in pairs], [p[1] for p in pairs]


def _detect_mix(e, frames):
    return e.detect_batch(frames, fmt=[m[0] for m in MIX], ws=[m[1] for m in MIX], hs=[m[2] for m in MIX])


def _whole_path_check(oracle, make_engine, flags):
    """detect_batch of mixed sizes and formats on an area engine: the head tensors are those of the engine without the flag fed the oracle's
    resized frames at the same n, the detections are the CPU post-processing oracle's on the engine's own head, mapped from the REQUEST's size,
    and the launch table names the plain engine's kernels"""
    n = len(MIX)
    frames, bgr = _mix(400)
    e = make_engine(flags)
    tw, th = e.model_w, e.model_h
    got = _detect_mix(e, frames)
    heads = [e.head_tensor(i) for i in range(n)]
    names = e.op_kernels(n)
    e.close()
    p = make_engine(flags & ~AREA)
    p.detect_batch([ar.area_resize(b, tw, th, flags & LBF) for b in bgr])
    for i in range(n):
        assert np.array_equal(heads[i], p.head_tensor(i)), (i, MIX[i])
    assert names == p.op_kernels(n)
    p.close()
    for i, (_, w, h) in enumerate(MIX):
        if flags & LBF:
            hp, nw, nh = lb.unpad_head(heads[i], w, h, tw, th)
            want = oracle.postprocess(hp, nw, nh, CONF, IOU)
        else:
            want = oracle.postprocess(heads[i], w, h, CONF, IOU)
        d, k = got[i]
        assert k == len(want) and det_fields_equal(d, want[:len(d)]), (i, MIX[i], k, len(want))
    assert sum(k for _, k in got) > 0                              # the comparison covered detections


@pytest.mark.parametrize("flags", MODES)
def test_whole_path_default_front(weights_path, oracle, flags):
    mk = lambda fl: zly.Engine(weights_path, dtype=zly.DTYPE_BF16, max_batch=4, max_dets=512, conf_thr=CONF, warmup_runs=0, flags=fl)
    _whole_path_check(oracle, mk, flags)


@pytest.mark.parametrize("flags", MODES)
def test_whole_path_no_stem1(weights_path, oracle, monkeypatch, flags):
    monkeypatch.setenv("ZLY_NO_STEM1", "1")                        # read at zly_create
    mk = lambda fl: zly.Engine(weights_path, dtype=zly.DTYPE_BF16, max_batch=4, max_dets=512, conf_thr=CONF, warmup_runs=0, flags=fl)
    _whole_path_check(oracle, mk, flags)


@pytest.mark.parametrize("flags", MODES)
def test_whole_path_no_fusion(weights_path, oracle, flags):
    mk = lambda fl: zly.Engine(weights_path, dtype=zly.DTYPE_BF16, max_batch=4, max_dets=512, conf_thr=CONF, warmup_runs=0, flags=fl | zly.FLAG_NO_FUSION)
    _whole_path_check(oracle, mk, flags)


# ---- 3. the mode does something, and nothing else changes --------------------------------------------------------------------------------
def test_checkerboard_differs_from_the_plain_engine_and_model_sized_requests_do_not(weights_path):
    yy, xx = np.mgrid[0:832, 0:832]
    board = np.ascontiguousarray(np.repeat((((xx + yy) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2))
    frames = np.ascontiguousarray(np.stack([_bgr(416, 416, seed=500 + i) for i in range(3)]))
    d = torch.from_numpy(frames).cuda()
    torch.cuda.synchronize()
    out = {}
    for fl in (AREA, 0):
        e = zly.Engine(weights_path, dtype=zly.DTYPE_BF16, max_batch=3, max_dets=128, conf_thr=CONF, warmup_runs=1, flags=fl)
        pre = e.preprocess(board)
        e.detect_device(d.data_ptr(), 3, 416, 416)
        out[fl] = (pre, _raw_slabs(e, 3), e.preprocess(frames[0]), _slab_results(e, 3))
        e.close()
    # a 1-pixel checkerboard at 2x: every block's mean is 127.5 -> 128; the nearest pick sees one colour only
    assert np.array_equal(out[AREA][0], np.full((3, 416, 416), np.float32(128) / np.float32(255.0), np.float32))
    assert not np.array_equal(out[AREA][0], out[0][0])
    # a model-sized request: slabs byte for byte, tensor word for word
    assert np.array_equal(out[AREA][1], out[0][1]) and _eq_words(out[AREA][2], out[0][2])
    assert sum(k for _, k in out[0][3]) > 0


def test_plain_engine_beside_an_area_engine_gives_its_golden_bytes(weights_path):
    G = np.load(os.path.join(ROOT, "tests", "golden", "zly_golden_64.npz"))
    frames = [G["frames_64"][0], G["frames_64"][1], G["frame_96x80"]]
    a = zly.Engine(weights_path, model_w=64, model_h=64, conf_thr=float(G["conf"]), iou_thr=float(G["iou"]), max_batch=3, max_dets=256,
                   dtype=zly.DTYPE_FP32, warmup_runs=0, flags=AREA)
    a.detect_batch(frames, cap=256)
    p = zly.Engine(weights_path, model_w=64, model_h=64, conf_thr=float(G["conf"]), iou_thr=float(G["iou"]), max_batch=3, max_dets=256,
                   dtype=zly.DTYPE_FP32, warmup_runs=0)
    for i, f in enumerate(frames):
        assert np.array_equal(p.preprocess(f), G["pre"][i])
        # the 64 x 64 frames are model-sized: the area engine's tensor is the golden one too; the 96 x 80 frame's is the oracle's
        want = G["pre"][i] if f.shape[:2] == (64, 64) else ar.preprocess_planar(f, 64, 64, False)
        assert _eq_words(a.preprocess(f), want), i
    a.close()
    p.close()


# ---- 4. paths ------------------------------------------------------------------------------------------------------------------------
def _surface(fmt, W, H, seed, pad, off):
    """a pitched BGRA / BGR surface at an odd offset of a poisoned buffer -> (buffer, its view, the tight frame)"""
    f, _ = _any_frame(fmt, W, H, seed)
    pitch = W * pr.BPP[fmt] + pad
    buf, _ = pr.embed(f, fmt, pitch, off, tail=0, fill=POISON)
    c = zly.FrameView()
    c.fmt, c.w, c.h = fmt, W, H
    c.off[0], c.pitch[0] = off, pitch
    return buf, c, f


@pytest.mark.parametrize("flags", MODES)
def test_device_view_two_views_of_one_surface_and_production_flags(weights_path, flags):
    fmt, W, H, off, pad = zly.PIX_BGRA, 1282, 722, 5, 9
    buf, whole, _ = _surface(fmt, W, H, 600, pad, off)
    regions = [(0, 0, W, H), (301, 111, 700, 500)]
    views = [zly.view_crop(whole, *r) for r in regions]
    tight = [pr.cut(buf, fmt, W * 4 + pad, off, *r) for r in regions]
    d = torch.from_numpy(buf).cuda()
    torch.cuda.synchronize()
    e = zly.Engine(weights_path, dtype=zly.DTYPE_BF16, max_batch=2, max_dets=256, conf_thr=CONF, warmup_runs=0, flags=flags)
    want = e.detect_batch(tight, fmt=fmt)
    e.detect_device_view(d.data_ptr(), buf.nbytes, views)
    assert _same_results(_slab_results(e, 2), want) and sum(k for _, k in want) > 0
    raw = _raw_slabs(e, 2)
    e.close()
    # the production flags give the dump engine's slab bytes
    q = zly.Engine(weights_path, dtype=zly.DTYPE_BF16, max_batch=2, max_dets=256, conf_thr=CONF, warmup_runs=0,
                   flags=flags | zly.FLAG_NO_HEAD_TENSOR | zly.FLAG_ASYNC_NMS)
    q.detect_device_view(d.data_ptr(), buf.nbytes, views)
    assert np.array_equal(_raw_slabs(q, 2), raw)
    q.close()


def test_production_flags_at_a_deferred_batch_size(weights_path):
    """16 frames: the smallest batch whose NMS ZLY_FLAG_ASYNC_NMS moves to its own stream"""
    n, w, h = 16, 640, 360
    base = zm.synth_frames(4, w, h, seed=650)
    frames = np.ascontiguousarray(np.stack([np.roll(base[i % 4], 8 * (i // 4), axis=1) for i in range(n)]))
    d = torch.from_numpy(frames).cuda()
    torch.cuda.synchronize()
    raws = []
    for extra in (0, zly.FLAG_NO_HEAD_TENSOR | zly.FLAG_ASYNC_NMS):
        e = zly.Engine(weights_path, dtype=zly.DTYPE_BF16, max_batch=n, max_dets=128, conf_thr=CONF, warmup_runs=0, flags=AREA | LBF | extra)
        for _ in range(2):
            e.detect_device(d.data_ptr(), n, w, h)
        raws.append(_raw_slabs(e, n))
        kept = sum(int(hd["n_kept"]) for hd, _ in zly.parse_slabs(raws[-1], n, 128))
        e.close()
    assert np.array_equal(raws[0], raws[1]) and kept > 0


@pytest.mark.parametrize("flags", MODES)
def test_submit_view_lone_frame_and_full_batch(weights_path, flags):
    """fp32 engine (exact however the ring batches the frames): every ticket equals the frame's result inside detect_batch"""
    n = 4
    e = zly.Engine(weights_path, dtype=zly.DTYPE_FP32, max_batch=n, max_dets=256, conf_thr=CONF, warmup_runs=0, flags=flags)
    surf = [_surface(zly.PIX_BGR if i % 2 else zly.PIX_BGRA, 700 + 31 * i, 400 + 17 * i, 700 + i, 3 + i, 1 + 2 * i) for i in range(n)]
    want = e.detect_batch([s[2] for s in surf], fmt=[s[1].fmt for s in surf])
    assert sum(k for _, k in want) > 0
    lone = e.wait(e.submit_view(surf[0][0], surf[0][1]))
    assert lone[1] == want[0][1] and det_fields_equal(lone[0], want[0][0])
    tickets = [e.submit_view(s[0], s[1]) for s in surf]
    assert _same_results([e.wait(t) for t in tickets], want)
    e.close()


@pytest.mark.parametrize("flags", MODES)
def test_detect_tiled_2x2_and_one_tracked_frame(weights_path, flags):
    fmt, W, H, off, pad = zly.PIX_BGRA, 1280, 960, 3, 5
    buf, whole, _ = _surface(fmt, W, H, 800, pad, off)
    tiles = zly.tile_grid(W, H, 704, 544, 128, 128)
    assert len(tiles) == 4
    e = zly.Engine(weights_path, dtype=zly.DTYPE_BF16, max_batch=4, max_dets=256, conf_thr=CONF, warmup_runs=0, flags=flags)
    tight = [pr.cut(buf, fmt, W * 4 + pad, off, t.x0, t.y0, t.w, t.h) for t in tiles]
    want = e.detect_batch(tight, fmt=fmt)                          # the four tiles as a batch of four
    assert sum(k for _, k in want) > 0
    d = torch.from_numpy(buf).cuda()
    torch.cuda.synchronize()
    e.detect_device_view(d.data_ptr(), buf.nbytes, [zly.view_crop(whole, t.x0, t.y0, t.w, t.h) for t in tiles])
    assert _same_results(_slab_results(e, 4), want)
    e.merge_slabs(tiles)
    hd, merged = e.read_merged(1)[0]
    got = e.detect_tiled(buf, whole, tiles)
    assert got[1] == int(hd["n_kept"]) and det_fields_equal(got[0], merged) and got[1] > 0
    e.close()
    # one tracked frame through the ring: the lone frame's result, with ids
    t = zly.Engine(weights_path, dtype=zly.DTYPE_BF16, max_batch=4, max_dets=64, conf_thr=CONF, warmup_runs=0, flags=flags)
    t.track_enable(max_streams=2, max_tracks=64)
    v0 = zly.view_crop(whole, tiles[0].x0, tiles[0].y0, tiles[0].w, tiles[0].h)
    lone = t.detect_batch(tight[:1], fmt=fmt)[0]
    tr = t.wait(t.submit_view_tracked(buf, v0, 1))
    assert tr[1] == lone[1] and lone[1] > 0 and (tr[0]["track_id"] != 0).all()
    for k in ("x", "y", "w", "h", "confidence", "class_id"):
        assert np.array_equal(tr[0][k].view(np.uint32), lone[0][k].view(np.uint32)), k
    t.close()


# ---- 5. errors -----------------------------------------------------------------------------------------------------------------------
def test_oversized_requests_and_models_are_refused(weights_path):
    e = zly.Engine(weights_path, dtype=zly.DTYPE_FP32, max_batch=2, max_dets=128, conf_thr=CONF, warmup_runs=0, flags=AREA)
    lib = e.lib
    out = np.zeros(128, dtype=zly.DET_DTYPE)
    n = C.c_int32(0)
    t = C.c_uint64(12345)
    pre = np.zeros((3, 416, 416), np.float32)
    batches0 = e.stats()["batches"]
    for f in (np.zeros((1, 16385, 3), np.uint8), np.zeros((16385, 1, 3), np.uint8)):
        h, w = f.shape[:2]
        assert lib.zly_detect(e.h, f.ctypes.data, f.nbytes, w, h, out.ctypes.data, 128, C.byref(n)) == zly.ERR_INVALID_INPUT
        assert b"area mode" in lib.zly_last_error()
        assert lib.zly_submit(e.h, f.ctypes.data, f.nbytes, w, h, C.byref(t)) == zly.ERR_INVALID_INPUT and t.value == 12345
        assert lib.zly_preprocess(e.h, f.ctypes.data, f.nbytes, w, h, pre.ctypes.data) == zly.ERR_INVALID_INPUT
        v = zly.view_tight(zly.PIX_BGR, w, h)
        assert lib.zly_detect_view(e.h, f.ctypes.data, f.nbytes, C.byref(v), out.ctypes.data, 128, C.byref(n)) == zly.ERR_INVALID_INPUT
    d = torch.zeros(16385 * 3, dtype=torch.uint8, device="cuda")
    assert lib.zly_detect_device(e.h, 1, d.data_ptr(), 16385, 1, None, 0, None) == zly.ERR_INVALID_INPUT
    assert e.stats()["batches"] == batches0                        # nothing was enqueued
    good = _bgr(640, 480, seed=900)
    want = e.detect(good, cap=128)
    assert want[1] > 0 and e.stats()["batches"] == batches0 + 1    # the engine still serves
    e.close()
    with pytest.raises(zly.ZlyError) as ex:
        zly.Engine(weights_path, dtype=zly.DTYPE_FP32, model_w=16416, model_h=416, max_batch=1, warmup_runs=0, flags=AREA)
    assert ex.value.code == zly.ERR_INVALID_ARGUMENT and "ZLY_FLAG_AREA" in str(ex.value)
    # a plain engine takes the wide frame as before
    s = zly.Engine(weights_path, dtype=zly.DTYPE_FP32, max_batch=1, max_dets=128, warmup_runs=0)
    s.detect(np.zeros((1, 16385, 3), np.uint8))
    s.close()
