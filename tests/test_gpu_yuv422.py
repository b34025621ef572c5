"""Packed YUV 4:2:2 request frames (include/zly.h ZLY_PIX_YUY2_* / ZLY_PIX_UYVY_*: capture cards, UVC devices) on the GPU.  The front kernels
load a pixel's 4-byte macropixel, pick Y, U, V with one permute, convert with the header's integer formula and then take the BGR path, so
engine(frame) must equal, bit for bit, engine(to_bgr(frame)) on the same engine with the same batch composition -- through every entry point, in
every front-kernel configuration, stretch and letterbox, tight frames and views.  The oracle is tests/yuv422_ref.py's to_bgr."""
import ctypes as C

import numpy as np
import pytest
import torch            # before the first engine: the process then uses torch's HIP runtime throughout, as tests/test_gpu_parity.py does

import pixfmt_ref as pr
import yuv422_ref as y2
import yuv_ref as yr
import zly
import zly_model as zm
from oracle_lib import det_fields_equal

pytestmark = pytest.mark.gpu

FMTS = (zly.PIX_YUY2_BT601, zly.PIX_UYVY_BT601, zly.PIX_YUY2_BT709, zly.PIX_UYVY_BT709)
# each size is a place the fetch can go wrong: the w == 2 letterbox clamp (both taps in the frame's only macropixel), odd heights, sizes that are no
# multiple of a tile, a model-sized frame (it must take the general path, not the 12-byte BGR quads) and a common capture size
SIZES = [(2, 1), (2, 2), (2, 3), (4, 1), (6, 5), (100, 63), (418, 331), (416, 416), (640, 480)]
LB = [pytest.param(0, id="stretch"), pytest.param(zly.FLAG_LETTERBOX, id="letterbox")]


def _bgr(w, h, seed):
    return np.ascontiguousarray(zm.synth_frames(1, w, h, seed=seed, rects=w >= 16 and h >= 16)[0])


def _y422(w, h, fmt, seed):
    """a tight frame of format fmt (1-D u8) made from a synthetic picture, and the BGR frame it stands for"""
    f = y2.from_bgr(_bgr(w, h, seed), fmt)
    assert f.size == 2 * w * h
    return f, y2.to_bgr(f, w, h, fmt)


def _same_results(a, b):
    return len(a) == len(b) and all(na == nb and det_fields_equal(da, db) for (da, na), (db, nb) in zip(a, b))


def _slab_results(e, n):
    return [(d, int(h["n_kept"])) for h, d in e.read_slabs(n)]


def _c_view(fmt, w, h, off, pitch):
    c = zly.FrameView()
    c.fmt, c.w, c.h = fmt, w, h
    c.off[0], c.pitch[0] = off, pitch
    return c


# ---- 1. preprocess, bit-exact ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", LB)
@pytest.mark.parametrize("dtype", [zly.DTYPE_FP32, zly.DTYPE_BF16])
def test_preprocess_equals_preprocess_of_its_bgr(weights_path, dtype, flags):
    e = zly.Engine(weights_path, dtype=dtype, max_batch=1, warmup_runs=0, flags=flags)
    for k, (w, h) in enumerate(SIZES):
        want = {}
        for fmt in FMTS:
            f, b = _y422(w, h, fmt, seed=100 + k)
            got = e.preprocess(f, fmt=fmt, w=w, h=h)
            key = b.tobytes()
            if key not in want:
                want[key] = e.preprocess(b)
            assert np.array_equal(got.view(np.uint32), want[key].view(np.uint32)), (w, h, fmt)
            # ... and through a view of a pitched surface at an odd address
            buf, _ = y2.embed(f, w, h, 2 * w + 5, 3, seed=k)
            got = e.preprocess_view(buf, _c_view(fmt, w, h, 3, 2 * w + 5))
            assert np.array_equal(got.view(np.uint32), want[key].view(np.uint32)), (w, h, fmt, "view")
    e.close()


# ---- 2. every front-kernel configuration -----------------------------------------------------------------------------------------
def _front_check(e, n, want_kernel, kernel_index=1):
    """detect_batch on mixed-size frames of the four formats against their BGR conversions, same n: detections and head tensors identical"""
    sizes = [(416, 416), (640, 480), (100, 63), (418, 331)][:n]
    fmts = [FMTS[i % 4] for i in range(n)]
    pairs = [_y422(w, h, f, seed=200 + i) for i, ((w, h), f) in enumerate(zip(sizes, fmts))]
    got = e.detect_batch([p[0] for p in pairs], fmt=fmts, ws=[s[0] for s in sizes], hs=[s[1] for s in sizes])
    got_heads = [e.head_tensor(i) for i in range(n)]
    want = e.detect_batch([p[1] for p in pairs])
    want_heads = [e.head_tensor(i) for i in range(n)]
    assert _same_results(got, want)
    for g, w_ in zip(got_heads, want_heads):
        assert np.array_equal(g, w_)
    assert sum(k for _, k in got) > 0                          # the comparison covered detections
    assert want_kernel in e.op_kernels(n)[kernel_index], e.op_kernels(n)[kernel_index]


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
def test_front_yolov8s_stem_fused_two_tiles(tmp_path, flags):
    spec = zm.build_spec("s")
    p = str(tmp_path / "yolov8s_synth.zlyw")
    zm.write_zlyw(p, spec, zm.synth_weights(spec, seed=9))
    e = zly.Engine(p, dtype=zly.DTYPE_BF16, max_batch=3, max_dets=512, conf_thr=0.05, warmup_runs=0, flags=flags)
    _front_check(e, 3, "stem_fused_kernel")
    e.close()


@pytest.mark.parametrize("flags", LB)
@pytest.mark.parametrize("dtype", [zly.DTYPE_BF16, zly.DTYPE_FP32], ids=["bf16", "fp32"])
def test_front_no_fusion(weights_path, dtype, flags):
    """ZLY_FLAG_NO_FUSION: a bf16 engine still fuses preprocess into the stem conv (stem_fused_kernel); an fp32 engine runs preprocess_kernel alone"""
    e = zly.Engine(weights_path, dtype=dtype, max_batch=4, max_dets=512, conf_thr=0.05, warmup_runs=0, flags=zly.FLAG_NO_FUSION | flags)
    if dtype == zly.DTYPE_BF16:
        _front_check(e, 4, "stem_fused_kernel")
    else:
        _front_check(e, 4, "preprocess_kernel", kernel_index=0)
    e.close()


# ---- 3. one batch of every format family -------------------------------------------------------------------------------------------
def _any_frame(fmt, w, h, seed):
    """(frame as the engine takes it, its BGR conversion)"""
    if fmt == zly.PIX_BGR:
        b = _bgr(w, h, seed)
        return b, b
    if fmt in FMTS:
        return _y422(w, h, fmt, seed)
    if fmt in pr.PACKED:
        f = pr.from_bgr(_bgr(w, h, seed), fmt, x=np.random.default_rng(seed + 7).integers(0, 256, (h, w), dtype=np.uint8))
        return f, pr.to_bgr(f, w, h, fmt)
    y = yr.bgr_to_yuv420(_bgr(w, h, seed), fmt)
    return y, yr.yuv420_to_bgr(y, w, h, fmt)


@pytest.mark.parametrize("flags", LB)
def test_mixed_formats_in_one_batch(weights_path, flags):
    e = zly.Engine(weights_path, dtype=zly.DTYPE_BF16, max_batch=5, max_dets=512, conf_thr=0.05, warmup_runs=0, flags=flags)
    fmts = [zly.PIX_BGR, zly.PIX_NV12_BT601, zly.PIX_BGRA, zly.PIX_YUY2_BT601, zly.PIX_UYVY_BT709]
    sizes = [(416, 416), (640, 480), (333, 500), (418, 331), (100, 63)]
    pairs = [_any_frame(f, w, h, seed=300 + i) for i, (f, (w, h)) in enumerate(zip(fmts, sizes))]
    got = e.detect_batch([p[0] for p in pairs], fmt=fmts, ws=[s[0] for s in sizes], hs=[s[1] for s in sizes])
    heads = [e.head_tensor(i) for i in range(5)]
    want = e.detect_batch([p[1] for p in pairs])
    assert _same_results(got, want)
    for i in range(5):
        assert np.array_equal(heads[i], e.head_tensor(i))
    assert sum(k for _, k in got) > 0
    e.close()


# ---- 4. a batch without a 4:2:2 frame launches what it launched ---------------------------------------------------------------------
# The front group op_kernels(4)[:3] and the Detect tail of the parent commit's library (bf16 YOLOv8n, max_batch 4), recorded there: whatever the composition of a batch, the engine
# names the same launches as it did before the packed 4:2:2 level existed.  (That the kernels behind the names are the parent's code, symbol by
# symbol, is tools/isa_diff.py's check; that a batch's level is the highest of its frames' is what the bit-exact comparisons of this file and of
# tests/test_gpu_yuv_input.py / test_gpu_packed_formats.py rest on.)
PARENT_KERNELS = {
    0: ["(fused into stem_fused_kernel)", "stem_model1_kernel (preprocess+model.0+model.1)", "(fused into the previous launch)"],
    zly.FLAG_LETTERBOX: ["(fused into stem_fused_kernel)", "stem_model1_kernel<LB> (letterbox preprocess+model.0+model.1)", "(fused into the previous launch)"],
}
PARENT_HEAD = {0: "head_fused_kernel", zly.FLAG_LETTERBOX: "head_fused_kernel<LB> (letterbox box mapping)"}      # op_kernels(4)[-2]


@pytest.mark.parametrize("flags", LB)
def test_batches_without_a_422_frame_name_the_parents_kernels(weights_path, flags):
    e = zly.Engine(weights_path, dtype=zly.DTYPE_BF16, max_batch=4, max_dets=512, conf_thr=0.05, warmup_runs=0, flags=flags)
    sizes = [(416, 416), (640, 480), (100, 62), (418, 330)]
    batches = {"bgr": [zly.PIX_BGR] * 4,
               "yuv": [zly.PIX_BGR, zly.PIX_NV12_BT601, zly.PIX_I420_BT709, zly.PIX_NV12_BT709],
               "packed": [zly.PIX_RGB, zly.PIX_BGRA, zly.PIX_NV12_BT601, zly.PIX_RGBA]}
    covered = 0
    for name, fmts in batches.items():
        pairs = [_any_frame(f, w, h, seed=350 + i) for i, (f, (w, h)) in enumerate(zip(fmts, sizes))]
        got = e.detect_batch([p[0] for p in pairs], fmt=fmts, ws=[s[0] for s in sizes], hs=[s[1] for s in sizes])
        names = e.op_kernels(4)
        assert names[:3] == PARENT_KERNELS[flags] and names[-2] == PARENT_HEAD[flags] and len(names) == 60, (name, names)
        want = e.detect_batch([p[1] for p in pairs])
        assert _same_results(got, want), name
        covered += sum(k for _, k in got)
    assert covered > 0
    e.close()


# ---- 5. + 6. entry points; bytes outside the region are inert -----------------------------------------------------------------------
@pytest.mark.parametrize("flags", LB)
def test_fmt_entry_points(weights_path, flags):
    """detect_fmt, detect_batch_fmt, submit_fmt / wait with a partial batch, detect_device_fmt with n contiguous frames"""
    n, w, h = 3, 418, 331
    e = zly.Engine(weights_path, dtype=zly.DTYPE_BF16, max_batch=4, max_dets=512, conf_thr=0.05, warmup_runs=0, flags=flags)
    for fmt in (zly.PIX_YUY2_BT601, zly.PIX_UYVY_BT709):
        pairs = [_y422(w, h, fmt, seed=400 + fmt + i) for i in range(n)]
        want1 = [e.detect(b) for _, b in pairs]
        want_n = e.detect_batch([b for _, b in pairs])
        assert sum(k for _, k in want1) > 0 and sum(k for _, k in want_n) > 0
        assert _same_results([e.detect(f, fmt=fmt, w=w, h=h) for f, _ in pairs], want1)
        assert _same_results(e.detect_batch([f for f, _ in pairs], fmt=fmt, ws=[w] * n, hs=[h] * n), want_n)
        # one ticket at a time: a partial batch of one, as the lone detect runs
        assert _same_results([e.wait(e.submit(f, fmt=fmt, w=w, h=h)) for f, _ in pairs], want1)
        d = torch.from_numpy(np.concatenate([f for f, _ in pairs])).cuda()
        torch.cuda.synchronize()
        e.detect_device(d.data_ptr(), n, w, h, fmt=fmt)
        assert _same_results(_slab_results(e, n), want_n)
    e.close()


@pytest.mark.parametrize("flags", LB)
@pytest.mark.parametrize("fmt", [zly.PIX_YUY2_BT709, zly.PIX_UYVY_BT601])
def test_views_of_a_pitched_surface(weights_path, fmt, flags):
    """regions of one surface with row padding, a pitch that is no multiple of 4 and a base offset that is no multiple of 4, through zly_detect_view,
    zly_submit_view and zly_detect_device_view (four views of one device buffer in one call): each equals the _fmt call on the tight frame cut out
    with numpy; bytes outside the regions, randomised twice, never reach a result"""
    W, H, off = 480, 301, 3
    pitch = 2 * W + 7
    assert pitch % 4 and off % 4
    surface, _ = _y422(W, H, fmt, seed=450 + fmt)
    buf, _ = y2.embed(surface, W, H, pitch, off, tail=0, seed=5)
    # the whole surface; a crop at an odd y0 with an odd height; one that ends on the buffer's last byte; the smallest frame there is
    regions = [(0, 0, W, H), (36, 21, 302, 201), (W - 100, H - 63, 100, 63), (210, 151, 2, 1)]
    last = regions[2]
    assert off + (last[1] + last[3] - 1) * pitch + (last[0] + last[2]) * 2 == buf.size
    whole = _c_view(fmt, W, H, off, pitch)
    assert zly.view_bytes(whole) == buf.size
    views = [zly.view_crop(whole, *r) for r in regions]
    tight = [y2.cut(buf, pitch, off, *r) for r in regions]
    n = len(regions)
    e = zly.Engine(weights_path, dtype=zly.DTYPE_BF16, max_batch=n, max_dets=512, conf_thr=0.05, warmup_runs=0, flags=flags)
    bgr = [y2.to_bgr(t, r[2], r[3], fmt) for t, r in zip(tight, regions)]
    want1 = [e.detect(b) for b in bgr]                                             # batches of one, as detect_view / a lone submit_view run
    want_n = e.detect_batch(bgr)                                                   # the batch of n, as detect_device_view runs
    want_heads = [e.head_tensor(i) for i in range(n)]
    assert sum(k for _, k in want_n) > 0 and sum(k for _, k in want1) > 0

    def run_all(b):
        out1 = [e.detect_view(b, v) for v in views]
        out2 = [e.wait(e.submit_view(b, v)) for v in views]
        d = torch.from_numpy(b).cuda()
        torch.cuda.synchronize()
        e.detect_device_view(d.data_ptr(), b.nbytes, views)
        out3 = _slab_results(e, n)
        heads = [e.head_tensor(i) for i in range(n)]
        return out1, out2, out3, heads

    out1, out2, out3, heads = run_all(buf)
    assert _same_results(out1, want1)
    assert _same_results(out2, want1)
    assert _same_results(out3, want_n)
    for g, w_ in zip(heads, want_heads):
        assert np.array_equal(g, w_)
    # every byte outside a region takes other values, twice: per region for the single-view calls ...
    rng = np.random.default_rng(77)
    for rnd in range(2):
        noise = rng.integers(0, 256, buf.size, dtype=np.uint8)
        for v, r, w1 in zip(views, regions, want1):
            keep = y2.region_mask(buf.size, pitch, off, *r)
            b2 = np.where(keep, buf, noise).astype(np.uint8)
            g = e.detect_view(b2, v)
            assert g[1] == w1[1] and det_fields_equal(g[0], w1[0]), (r, rnd)
            g = e.wait(e.submit_view(b2, v))
            assert g[1] == w1[1] and det_fields_equal(g[0], w1[0]), (r, rnd)
        # ... and for the device call everything outside the surface's rows (row padding, the base offset)
        keep = y2.region_mask(buf.size, pitch, off, 0, 0, W, H)
        b3 = np.where(keep, buf, noise).astype(np.uint8)
        assert not np.array_equal(b3, buf)
        d3 = torch.from_numpy(b3).cuda()
        torch.cuda.synchronize()
        e.detect_device_view(d3.data_ptr(), b3.nbytes, views)
        assert _same_results(_slab_results(e, n), want_n)
    e.close()


# ---- 7. tiles ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", LB)
def test_detect_tiled_equals_detect_tiled_of_its_bgr(weights_path, flags):
    """four overlapping tiles of a pitched YUY2 surface, merged on the GPU: zly_tile_grid's even tiles are valid for 4:2:2 surfaces, and
    zly_detect_tiled, zly_merge_slabs need no change -- the result is that of the surface's BGR conversion"""
    fmt, W, H, off = zly.PIX_YUY2_BT601, 640, 480, 6
    pitch = 2 * W + 10
    surface, bgr = _y422(W, H, fmt, seed=500)
    buf, _ = y2.embed(surface, W, H, pitch, off, seed=6)
    tiles = zly.tile_grid(W, H, 416, 416, 32, 32, even=True)
    assert len(tiles) == 4
    e = zly.Engine(weights_path, dtype=zly.DTYPE_BF16, max_batch=4, max_dets=256, conf_thr=0.05, warmup_runs=0, flags=flags)
    got = e.detect_tiled(buf, _c_view(fmt, W, H, off, pitch), tiles)
    want = e.detect_tiled(bgr.reshape(-1), zly.view_tight(zly.PIX_BGR, W, H), tiles)
    assert got[1] == want[1] and det_fields_equal(got[0], want[0])
    assert got[1] > 0
    e.close()


# ---- 8. errors ---------------------------------------------------------------------------------------------------------------------
def test_errors_enqueue_nothing_and_engine_still_serves(weights_path):
    e = zly.Engine(weights_path, dtype=zly.DTYPE_FP32, max_batch=2, max_dets=128, conf_thr=0.05, warmup_runs=0)
    lib = e.lib
    out = np.zeros(128, dtype=zly.DET_DTYPE)
    out3 = np.zeros((3, 416, 416), np.float32)
    n = C.c_int32(0)
    t = C.c_uint64(12345)
    batches0 = e.stats()["batches"]
    cases = []                                                                     # (fmt, w, h, nbytes, code, expected size in the message)
    for fmt in FMTS:
        cases.append((fmt, 63, 48, 63 * 48 * 2, zly.ERR_INVALID_INPUT, 63 * 48 * 2))                  # odd w
        for nb in (64 * 48 * 2 - 1, 64 * 48 * 2 + 1, 64 * 48 * 3, 64 * 48 * 3 // 2, 0):              # a wrong byte count (BGR's and 4:2:0's among them)
            cases.append((fmt, 64, 48, nb, zly.ERR_INVALID_INPUT, 64 * 48 * 2))
    for fmt in (6, 8, 14):
        cases.append((fmt, 64, 48, 64 * 48 * 2, zly.ERR_INVALID_ARGUMENT, None))
    buf = np.zeros(64 * 48 * 4, np.uint8)
    for f, w, h, nb, code, expected in cases:
        assert lib.zly_detect_fmt(e.h, f, buf.ctypes.data, nb, w, h, out.ctypes.data, 128, C.byref(n)) == code, (f, w, nb)
        assert lib.zly_submit_fmt(e.h, f, buf.ctypes.data, nb, w, h, C.byref(t)) == code and t.value == 12345
        assert lib.zly_submit_try_fmt(e.h, f, buf.ctypes.data, nb, w, h, C.byref(t)) == code and t.value == 12345
        assert lib.zly_preprocess_fmt(e.h, f, buf.ctypes.data, nb, w, h, out3.ctypes.data) == code
        if code == zly.ERR_INVALID_INPUT:
            msg = lib.zly_last_error()
            assert ("Invalid image data size: expected %d, got %d" % (expected, nb)).encode() in msg, msg
            assert (b"even width" in msg) == (w % 2 == 1), msg
        assert lib.zly_detect_device_fmt(e.h, f, 1, None, w, h, None, 0, None) == (code if code == zly.ERR_INVALID_ARGUMENT else zly.ERR_INVALID_INPUT)
    # views: too small a pitch, an odd width, a view that needs more bytes than the buffer has; an unknown format
    for fmt in FMTS:
        good = _c_view(fmt, 64, 48, 3, 2 * 64 + 1)
        need = zly.view_bytes(good)
        assert need == 3 + 47 * 129 + 128
        bad_views = [(_c_view(fmt, 64, 48, 3, 2 * 64 - 1), buf.nbytes), (_c_view(fmt, 63, 48, 3, 2 * 64), buf.nbytes), (good, need - 1)]
        for v, nb in bad_views:
            assert lib.zly_detect_view(e.h, buf.ctypes.data, nb, C.byref(v), out.ctypes.data, 128, C.byref(n)) == zly.ERR_INVALID_INPUT
            assert lib.zly_submit_view(e.h, buf.ctypes.data, nb, C.byref(v), C.byref(t)) == zly.ERR_INVALID_INPUT and t.value == 12345
            assert lib.zly_preprocess_view(e.h, buf.ctypes.data, nb, C.byref(v), out3.ctypes.data) == zly.ERR_INVALID_INPUT
            assert lib.zly_detect_device_view(e.h, 1, buf.ctypes.data, nb, C.byref(v), None, 0, None) == zly.ERR_INVALID_INPUT
    for fmt in (6, 8, 14):
        v = _c_view(fmt, 64, 48, 0, 4 * 64)
        assert lib.zly_detect_view(e.h, buf.ctypes.data, buf.nbytes, C.byref(v), out.ctypes.data, 128, C.byref(n)) == zly.ERR_INVALID_ARGUMENT
        assert lib.zly_submit_view(e.h, buf.ctypes.data, buf.nbytes, C.byref(v), C.byref(t)) == zly.ERR_INVALID_ARGUMENT and t.value == 12345
        assert lib.zly_detect_device_view(e.h, 1, buf.ctypes.data, buf.nbytes, C.byref(v), None, 0, None) == zly.ERR_INVALID_ARGUMENT
    assert e.stats()["batches"] == batches0                                        # nothing was enqueued
    for fmt in FMTS:                                                               # the engine still serves good frames of every format
        f, b = _y422(416, 416, fmt, seed=700 + fmt)
        want = e.detect(b)
        got = e.detect(f, fmt=fmt, w=416, h=416)
        assert got[1] == want[1] and det_fields_equal(got[0], want[0])
        d2 = e.wait(e.submit(f, fmt=fmt, w=416, h=416))
        assert d2[1] == want[1] and det_fields_equal(d2[0], want[0])
        assert want[1] > 0
    e.close()
