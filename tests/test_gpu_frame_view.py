"""Frame views (include/zly.h zly_frame_view: pitched surfaces and regions of interest) on the GPU.  The defining rule: a view gives, bit for
bit, what the tight frame made of its samples (tests/view_ref.py: extract) gives through the _fmt entry point of the same name, on the same
engine with the same batch size and composition -- in every front-kernel configuration, stretch and letterbox.  All comparisons are exact:
two runs of one engine, no tolerance."""
import ctypes as C
import threading

import numpy as np
import pytest
import torch            # before the first engine: the process then uses torch's HIP runtime throughout, as tests/test_gpu_parity.py does

import view_ref as vr
import yuv_ref as yr
import zly
import zly_model as zm
from oracle_lib import det_fields_equal

pytestmark = pytest.mark.gpu

ALL_FMTS = (zly.PIX_BGR, zly.PIX_NV12_BT601, zly.PIX_I420_BT601, zly.PIX_NV12_BT709, zly.PIX_I420_BT709)
SIZES = [(416, 416), (640, 480), (1280, 720), (1920, 1080), (100, 62), (418, 330), (2, 2)]       # tests/test_gpu_yuv_input.py's
PITCH_KINDS = (0, 1, 64)             # tight, tight + 1 (odd), tight + 64


def _frame(w, h, fmt, seed):
    """a tight synthetic frame of format fmt: BGR [h][w][3], or the packed YUV buffer"""
    bgr = zm.synth_frames(1, w, h, seed=seed, rects=w >= 16 and h >= 16)[0]
    return np.ascontiguousarray(bgr) if fmt == zly.PIX_BGR else yr.bgr_to_yuv420(bgr, fmt)


def _pitches(fmt, surf_w, extra):
    return [p + extra for p in vr.tight_pitches(fmt, surf_w)]


def _embed(frame, fmt, w, h, surf_w, surf_h, extra, x0, y0, fill):
    return vr.embed(frame, fmt, surf_w, surf_h, _pitches(fmt, surf_w, extra), x0, y0, fill, w=w, h=h)


def _pack(surfaces):
    """[(buffer, view)] -> one buffer holding the surfaces one behind the other (16 bytes apart at least) and the views inside it"""
    bufs, views, pos = [], [], 0
    for buf, v in surfaces:
        views.append(vr.shift(v, pos))
        pad = (-buf.size) % 16 + 16
        bufs += [buf, np.full(pad, 0xA5, np.uint8)]
        pos += buf.size + pad
    return np.concatenate(bufs), views


def _tight_args(frames, views):
    return dict(fmt=[v.fmt for v in views], ws=[v.w for v in views], hs=[v.h for v in views])


def _same_results(a, b):
    return len(a) == len(b) and all(na == nb and det_fields_equal(da, db) for (da, na), (db, nb) in zip(a, b))


def _slab_results(e, n):
    return [(d, int(h["n_kept"])) for h, d in e.read_slabs(n)]


# ---- 1. tensor level ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lb", [False, True])
@pytest.mark.parametrize("dtype", [zly.DTYPE_FP32, zly.DTYPE_BF16])
def test_preprocess_view_equals_preprocess_of_the_extracted_frame(weights_path, dtype, lb):
    e = zly.Engine(weights_path, dtype=dtype, max_batch=1, warmup_runs=0, flags=zly.FLAG_LETTERBOX if lb else 0)
    for k, (w, h) in enumerate(SIZES):
        for fmt in ALL_FMTS:
            frame = _frame(w, h, fmt, seed=100 + k)
            want = e.preprocess(frame, fmt=fmt, w=w, h=h)
            for extra in PITCH_KINDS:
                # the region inside a surface with a margin on every side (even offsets: YUV), once more flush against the bottom-right corner
                for (x0, y0, mx, my) in ((6, 4, 10, 8), (6, 4, 0, 0)):
                    got = []
                    for fill in (0, 255):
                        buf, v = _embed(frame, fmt, w, h, x0 + w + mx, y0 + h + my, extra, x0, y0, fill)
                        assert np.array_equal(vr.extract(buf, v).reshape(-1), frame.reshape(-1))
                        got.append(e.preprocess_view(buf, vr.to_c(v)))
                    assert np.array_equal(got[0].view(np.uint32), want.view(np.uint32)), (w, h, fmt, extra, x0, y0, mx, my)
                    assert np.array_equal(got[1].view(np.uint32), want.view(np.uint32)), (w, h, fmt, extra, x0, y0, mx, my, "fill 255")
    e.close()


# ---- 2. / 3. the front kernels -----------------------------------------------------------------------------------------------
def _mixed_views(n, fill="noise"):
    """four views of four surfaces in one buffer: a model-sized BGR crop of a 1920 x 1080 surface, a resized BGR crop, an NV12 crop, an I420 crop"""
    spec = [(zly.PIX_BGR, 416, 416, 1920, 1080, 128, 752, 332),
            (zly.PIX_BGR, 640, 480, 800, 600, 1, 77, 53),
            (zly.PIX_NV12_BT601, 418, 330, 640, 480, 64, 100, 62),
            (zly.PIX_I420_BT709, 100, 62, 320, 240, 1, 220, 178)][:n]          # the I420 crop is flush against its surface's corner
    frames, surfaces = [], []
    for i, (fmt, w, h, sw, sh, extra, x0, y0) in enumerate(spec):
        f = _frame(w, h, fmt, seed=200 + i)
        frames.append(f)
        surfaces.append(_embed(f, fmt, w, h, sw, sh, extra, x0, y0, fill))
    buf, views = _pack(surfaces)
    for f, v in zip(frames, views):
        assert np.array_equal(vr.extract(buf, v).reshape(-1), f.reshape(-1))
    return buf, views, frames


def _front_check(e, n, want_kernel, kernel_index=1):
    """detect_device_view on mixed views against detect_batch of the extracted frames, same n: detections and head tensors identical"""
    buf, views, frames = _mixed_views(n)
    d_buf = torch.from_numpy(buf).cuda()
    torch.cuda.synchronize()
    e.detect_device_view(d_buf.data_ptr(), buf.nbytes, [vr.to_c(v) for v in views])
    got = _slab_results(e, n)
    got_heads = [e.head_tensor(i) for i in range(n)]
    want = e.detect_batch(frames, **_tight_args(frames, views))
    want_heads = [e.head_tensor(i) for i in range(n)]
    assert _same_results(got, want)
    for g, w_ in zip(got_heads, want_heads):
        assert np.array_equal(g, w_)
    assert sum(k for _, k in got) > 0                          # the comparison covered detections
    assert want_kernel in e.op_kernels(n)[kernel_index], e.op_kernels(n)[kernel_index]
    # bytes outside the regions do not reach a result
    buf2, views2, _ = _mixed_views(n, fill=255)
    assert views2 == views
    d_buf2 = torch.from_numpy(buf2).cuda()
    torch.cuda.synchronize()
    e.detect_device_view(d_buf2.data_ptr(), buf2.nbytes, [vr.to_c(v) for v in views2])
    assert _same_results(_slab_results(e, n), want)


LB = [pytest.param(0, id="stretch"), pytest.param(zly.FLAG_LETTERBOX, id="letterbox")]


@pytest.mark.parametrize("flags", LB)
@pytest.mark.parametrize("var", [None, "0", "2"])
def test_front_stem_model1_all_variants(weights_path, monkeypatch, var, flags):
    if var is not None:
        monkeypatch.setenv("ZLY_STEM1_VAR", var)               # read at zly_create
    e = zly.Engine(weights_path, dtype=zly.DTYPE_BF16, max_batch=4, max_dets=512, conf_thr=0.05, warmup_runs=0, flags=flags)
    _front_check(e, 4, "stem_model1_kernel")
    e.close()


@pytest.mark.parametrize("flags", LB)
def test_front_stem_fused_no_stem1(weights_path, monkeypatch, flags):
    monkeypatch.setenv("ZLY_NO_STEM1", "1")
    e = zly.Engine(weights_path, dtype=zly.DTYPE_BF16, max_batch=4, max_dets=512, conf_thr=0.05, warmup_runs=0, flags=flags)
    _front_check(e, 4, "stem_fused_kernel")
    e.close()


@pytest.mark.parametrize("flags", LB)
def test_front_no_fusion(weights_path, flags):
    e = zly.Engine(weights_path, dtype=zly.DTYPE_BF16, max_batch=4, max_dets=512, conf_thr=0.05, warmup_runs=0, flags=zly.FLAG_NO_FUSION | flags)
    _front_check(e, 4, "stem_fused_kernel")
    e.close()


@pytest.mark.parametrize("flags", LB)
def test_front_yolov8s_stem_fused_two_tiles(tmp_path, flags):
    spec = zm.build_spec("s")
    p = str(tmp_path / "yolov8s_synth.zlyw")
    zm.write_zlyw(p, spec, zm.synth_weights(spec, seed=9))
    e = zly.Engine(p, dtype=zly.DTYPE_BF16, max_batch=3, max_dets=512, conf_thr=0.05, warmup_runs=0, flags=flags)
    _front_check(e, 3, "stem_fused_kernel")
    e.close()


@pytest.mark.parametrize("flags", LB)
def test_front_fp32_preprocess_kernel(weights_path, flags):
    e = zly.Engine(weights_path, dtype=zly.DTYPE_FP32, max_batch=4, max_dets=512, conf_thr=0.05, warmup_runs=0, flags=flags)
    _front_check(e, 4, "preprocess_kernel", kernel_index=0)
    e.close()


# ---- 4. tiling ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [zly.PIX_BGR, zly.PIX_NV12_BT601])
def test_tiling_one_surface_eight_views_one_call(weights_path, fmt):
    """eight 416 x 416 tiles of one padded 1920 x 1080 surface -- tiles flush against the right and bottom edges among them -- in ONE call
    equal the eight tight crops"""
    W, H, T = 1920, 1080, 416
    pitches = [1920 * 3 + 128] if fmt == zly.PIX_BGR else [1920 + 64, 1920 + 192]
    surf = _frame(W, H, fmt, seed=210)
    buf, whole = vr.embed(surf, fmt, W, H, pitches, 0, 0, 0x5A, w=W, h=H)
    tiles = [(0, 0), (416, 0), (W - T, 0), (0, H - T), (W - T, H - T), (752, 332), (1000, H - T), (W - T, 300)]
    views = [vr.crop(whole, x0, y0, T, T) for x0, y0 in tiles]
    cs = zly.view_crop(zly.view_crop(vr.to_c(whole), 0, 0, W, H), W - T, H - T, T, T)
    assert vr.from_c(cs) == views[4] and zly.view_bytes(cs) == vr.nbytes(whole) <= buf.size
    frames = [vr.extract(buf, v) for v in views]
    e = zly.Engine(weights_path, dtype=zly.DTYPE_BF16, max_batch=8, max_dets=512, conf_thr=0.05, warmup_runs=0)
    d_buf = torch.from_numpy(buf).cuda()
    torch.cuda.synchronize()
    e.detect_device_view(d_buf.data_ptr(), buf.nbytes, [vr.to_c(v) for v in views], tag0=40)
    slabs = e.read_slabs(8)
    got = [(d, int(h["n_kept"])) for h, d in slabs]
    assert [int(h["frame_tag"]) for h, _ in slabs] == list(range(40, 48))
    heads = [e.head_tensor(i) for i in range(8)]
    want = e.detect_batch(frames, **_tight_args(frames, views))
    assert _same_results(got, want)
    for i in range(8):
        assert np.array_equal(heads[i], e.head_tensor(i)), i
    assert sum(k for _, k in got) > 0
    e.close()


# ---- 5. host paths -----------------------------------------------------------------------------------------------------------
def test_host_paths_equal_their_fmt_counterparts(weights_path):
    e = zly.Engine(weights_path, dtype=zly.DTYPE_BF16, max_batch=4, max_dets=512, conf_thr=0.05, warmup_runs=0)
    buf, views, frames = _mixed_views(4)
    cviews = [vr.to_c(v) for v in views]
    total = 0
    for f, v, cv in zip(frames, views, cviews):
        got = e.detect_view(buf, cv)
        want = e.detect(f, fmt=v.fmt, w=v.w, h=v.h)
        assert got[1] == want[1] and det_fields_equal(got[0], want[0]), v
        total += got[1]
    # batch: one buffer per frame, here the four surfaces' own buffers next to the packed one
    got = e.detect_batch_view([buf] * 4, cviews)
    got_heads = [e.head_tensor(i) for i in range(4)]
    want = e.detect_batch(frames, **_tight_args(frames, views))
    assert _same_results(got, want)
    for i in range(4):
        assert np.array_equal(got_heads[i], e.head_tensor(i))
    total += sum(k for _, k in got)
    assert total > 0
    e.close()


def test_submit_view_equals_submit_fmt_fp32(weights_path):
    """fp32 engine (exact however the frames are batched): 4 threads submit views; every ticket equals the synchronous detect of the extracted frame"""
    e = zly.Engine(weights_path, dtype=zly.DTYPE_FP32, max_batch=8, max_dets=128, conf_thr=0.05, warmup_runs=1)
    buf, views, frames = _mixed_views(4)
    cviews = [vr.to_c(v) for v in views]
    serial = [e.detect(f, fmt=v.fmt, w=v.w, h=v.h, cap=128) for f, v in zip(frames, views)]
    viafmt = [e.wait(e.submit(f, fmt=v.fmt, w=v.w, h=v.h), cap=128) for f, v in zip(frames, views)]
    for a, b in zip(serial, viafmt):
        assert a[1] == b[1] and det_fields_equal(a[0], b[0])
    errors, results = [], []
    lock = threading.Lock()

    def worker(tid):
        try:
            for k in range(16):
                j = (tid + k) % 4
                r = e.wait(e.submit_view(buf, cviews[j]), cap=128)
                with lock:
                    results.append((j, r))
        except Exception as ex:          # noqa: BLE001
            errors.append(ex)

    th = [threading.Thread(target=worker, args=(i,)) for i in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors
    assert len(results) == 64
    for j, (d, n) in results:
        assert n == serial[j][1] and det_fields_equal(d, serial[j][0]), j
    assert sum(s[1] for s in serial) > 0
    e.close()


# ---- 6. errors ---------------------------------------------------------------------------------------------------------------
def test_errors_make_no_ticket_and_engine_still_serves(weights_path):
    e = zly.Engine(weights_path, dtype=zly.DTYPE_FP32, max_batch=2, max_dets=128, conf_thr=0.05, warmup_runs=0)
    lib = e.lib
    frame = _frame(416, 416, zly.PIX_BGR, seed=600)
    buf, v = _embed(frame, zly.PIX_BGR, 416, 416, 640, 480, 64, 100, 30, 7)
    good = vr.to_c(v)

    def mod(**kw):
        c = vr.to_c(v)
        for k, val in kw.items():
            if k == "pitch0":
                c.pitch[0] = val
            elif k == "off0":
                c.off[0] = val
            else:
                setattr(c, k, val)
        return c

    nv = zly.view_tight(zly.PIX_NV12_BT601, 416, 416)
    odd = zly.view_tight(zly.PIX_NV12_BT601, 416, 416); odd.w = 415
    cases = [(mod(fmt=7), buf.nbytes, zly.ERR_INVALID_ARGUMENT),                     # unknown format
             (mod(w=0), buf.nbytes, zly.ERR_INVALID_INPUT),                           # w, h >= 1
             (mod(pitch0=416 * 3 - 1), buf.nbytes, zly.ERR_INVALID_INPUT),            # pitch below the row's bytes
             (mod(pitch0=-(640 * 3 + 64)), buf.nbytes, zly.ERR_INVALID_INPUT),        # negative pitch
             (mod(pitch0=1 << 23), 1 << 40, zly.ERR_INVALID_INPUT),                   # extent not below 2^31
             (odd, 416 * 416 * 3 // 2, zly.ERR_INVALID_INPUT),                        # odd YUV width
             (good, zly.view_bytes(good) - 1, zly.ERR_INVALID_INPUT),                 # the buffer is one byte short
             (mod(off0=int(good.off[0]) + 1 + buf.nbytes - zly.view_bytes(good)), buf.nbytes, zly.ERR_INVALID_INPUT)]   # the region ends one byte behind it
    out = np.zeros(128, dtype=zly.DET_DTYPE)
    n = C.c_int32(0)
    t = C.c_uint64(12345)
    out3 = np.zeros((3, 416, 416), np.float32)
    d_buf = torch.from_numpy(buf).cuda()
    torch.cuda.synchronize()
    stats0 = e.stats()
    for cv, nb, code in cases:
        tag = (cv.fmt, cv.w, cv.h, list(cv.pitch), nb)
        assert lib.zly_detect_view(e.h, buf.ctypes.data, nb, C.byref(cv), out.ctypes.data, 128, C.byref(n)) == code, tag
        assert lib.zly_submit_view(e.h, buf.ctypes.data, nb, C.byref(cv), C.byref(t)) == code and t.value == 12345, tag
        assert lib.zly_submit_try_view(e.h, buf.ctypes.data, nb, C.byref(cv), C.byref(t)) == code and t.value == 12345, tag
        assert lib.zly_preprocess_view(e.h, buf.ctypes.data, nb, C.byref(cv), out3.ctypes.data) == code, tag
        assert lib.zly_detect_device_view(e.h, 1, d_buf.data_ptr(), nb, C.byref(cv), None, 0, None) == code, tag
        ptrs = (C.c_void_p * 2)(buf.ctypes.data, buf.ctypes.data)
        nbs = (C.c_size_t * 2)(buf.nbytes, nb)
        two = (zly.FrameView * 2)(good, cv)
        n2 = (C.c_int32 * 2)()
        out2 = np.zeros((2, 128), dtype=zly.DET_DTYPE)
        assert lib.zly_detect_batch_view(e.h, 2, ptrs, nbs, two, out2.ctypes.data, 128, n2) == code, tag
    assert lib.zly_detect_view(e.h, buf.ctypes.data, buf.nbytes, None, out.ctypes.data, 128, C.byref(n)) == zly.ERR_INVALID_ARGUMENT
    assert lib.zly_detect_device_view(e.h, 3, d_buf.data_ptr(), buf.nbytes, C.byref(good), None, 0, None) == zly.ERR_INVALID_ARGUMENT      # n > max_batch
    assert e.stats()["inference_count"] == stats0["inference_count"]
    # exactly the bytes the view needs are enough
    need = zly.view_bytes(good)
    want = e.detect(frame, cap=128)
    got = e.detect_view(buf[:need], good, cap=128)
    assert got[1] == want[1] and det_fields_equal(got[0], want[0])
    d2 = e.wait(e.submit_view(buf, good), cap=128)
    assert d2[1] == want[1] and det_fields_equal(d2[0], want[0])
    assert nv.fmt == zly.PIX_NV12_BT601
    e.close()


def test_letterbox_engine_bounds_the_views_size(weights_path):
    e = zly.Engine(weights_path, dtype=zly.DTYPE_FP32, max_batch=1, max_dets=64, warmup_runs=0, flags=zly.FLAG_LETTERBOX)
    big = zly.view_tight(zly.PIX_BGR, zly.LETTERBOX_MAX_DIM + 1, 2)
    buf = np.zeros(zly.view_bytes(big), np.uint8)
    out = np.zeros(64, dtype=zly.DET_DTYPE)
    n = C.c_int32(0)
    t = C.c_uint64(777)
    assert e.lib.zly_detect_view(e.h, buf.ctypes.data, buf.nbytes, C.byref(big), out.ctypes.data, 64, C.byref(n)) == zly.ERR_INVALID_INPUT
    assert e.lib.zly_submit_view(e.h, buf.ctypes.data, buf.nbytes, C.byref(big), C.byref(t)) == zly.ERR_INVALID_INPUT and t.value == 777
    # ... the view's size, not the surface's: a small window of a surface wider than the limit is fine
    win = zly.view_crop(big, 16000, 0, 64, 2)
    e.detect_view(buf, win, cap=64)
    e.close()


# ---- 7. descriptor cache coherence -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [False, True])
def test_plain_and_view_calls_alternate(weights_path, graph):
    """plain detect_device, then detect_device_view with the SAME offsets and sizes but another pitch, then plain again, then view again: each
    call gives what it gave the first time (neither reuses the other's descriptors)"""
    n, w, h = 4, 416, 416
    e = zly.Engine(weights_path, dtype=zly.DTYPE_BF16, max_batch=n, max_dets=512, conf_thr=0.05, use_graph=graph, warmup_runs=1 if graph else 0)
    tight = np.stack([_frame(w, h, zly.PIX_BGR, seed=200 + i) for i in range(n)])
    fb = w * h * 3
    # the same buffer read through views whose first samples are the tight frames' (same src_off, w, h) and whose pitch is 3 w + 12: other samples
    pitch = 3 * w + 12
    views = [vr.View(zly.PIX_BGR, w, h - 8, (i * fb,), (pitch,)) for i in range(n)]
    views_same = [vr.View(zly.PIX_BGR, w, h, (i * fb,), (3 * w,)) for i in range(n)]
    flat = tight.reshape(-1)
    assert max(vr.nbytes(v) for v in views) <= flat.size
    d = torch.from_numpy(flat).cuda()
    torch.cuda.synchronize()
    want_plain = e.detect_batch(list(tight))
    want_view = e.detect_batch([vr.extract(flat, v) for v in views])
    first = {}
    for rnd in range(2):
        e.detect_device(d.data_ptr(), n, w, h)
        plain = _slab_results(e, n)
        e.detect_device_view(d.data_ptr(), flat.nbytes, [vr.to_c(v) for v in views_same])
        same = _slab_results(e, n)
        e.detect_device_view(d.data_ptr(), flat.nbytes, [vr.to_c(v) for v in views])
        view = _slab_results(e, n)
        for k, r in (("plain", plain), ("same", same), ("view", view)):
            if rnd == 0:
                first[k] = r
            assert _same_results(r, first[k]), (rnd, k)
    assert _same_results(first["plain"], want_plain) and _same_results(first["same"], want_plain)
    assert _same_results(first["view"], want_view)
    assert sum(k for _, k in first["plain"]) > 0 and sum(k for _, k in first["view"]) > 0
    # and with identical src_off, w, h: a view of pitch 3 w + 12 right after the plain call, then the plain call right after it
    v2 = [vr.View(zly.PIX_BGR, w, h, (i * fb,), (pitch,)) for i in range(n - 1)]
    assert max(vr.nbytes(v) for v in v2) <= flat.size
    want_v2 = e.detect_batch([vr.extract(flat, v) for v in v2])
    want_p3 = e.detect_batch(list(tight[:n - 1]))
    for rnd in range(2):
        e.detect_device(d.data_ptr(), n - 1, w, h)
        assert _same_results(_slab_results(e, n - 1), want_p3), rnd
        e.detect_device_view(d.data_ptr(), flat.nbytes, [vr.to_c(v) for v in v2])
        assert _same_results(_slab_results(e, n - 1), want_v2), rnd
    assert not _same_results(want_v2, want_p3)                 # the two really read different samples
    e.close()
