"""Packed RGB / BGRA / RGBA request frames (include/zly.h ZLY_PIX_RGB / ZLY_PIX_BGRA / ZLY_PIX_RGBA) on the GPU.  The front kernels fetch such
a frame's pixel as the word B | G<<8 | R<<16 and then take the BGR path, so engine(frame) must equal, bit for bit, engine(to_bgr(frame)) on the
same engine with the same batch composition -- through every entry point, in every front-kernel configuration, stretch and letterbox -- and the
fourth byte of a 4-byte pixel must never reach a result.  The oracle is tests/pixfmt_ref.py's to_bgr."""
import ctypes as C
import json
import os
import struct
import subprocess
import threading

import numpy as np
import pytest
import torch            # before the first engine: the process then uses torch's HIP runtime throughout, as tests/test_gpu_parity.py does

import pixfmt_ref as pr
import yuv_ref as yr
import zly
import zly_model as zm
from oracle_lib import det_fields_equal

pytestmark = pytest.mark.gpu

FMTS = (zly.PIX_RGB, zly.PIX_BGRA, zly.PIX_RGBA)
# each size is a place the fetch can go wrong: the tail loads and the w == 1 letterbox clamp, odd sizes, sizes that are no multiple of a tile,
# a model-sized frame (it must take the general path, not the 12-byte BGR quads) and a common capture size
SIZES = [(1, 1), (2, 1), (1, 2), (3, 5), (100, 62), (418, 330), (416, 416), (640, 480)]
LB = [pytest.param(0, id="stretch"), pytest.param(zly.FLAG_LETTERBOX, id="letterbox")]


def _bgr(w, h, seed):
    return np.ascontiguousarray(zm.synth_frames(1, w, h, seed=seed, rects=w >= 16 and h >= 16)[0])


def _packed(w, h, fmt, seed, x=None):
    """a frame of format fmt with random X bytes (or the given ones) and the BGR frame it stands for"""
    b = _bgr(w, h, seed)
    if x is None:
        x = np.random.default_rng(seed + 7).integers(0, 256, (h, w), dtype=np.uint8)
    f = pr.from_bgr(b, fmt, x=x)
    assert np.array_equal(pr.to_bgr(f, w, h, fmt), b)
    return f, b


def _same_results(a, b):
    return len(a) == len(b) and all(na == nb and det_fields_equal(da, db) for (da, na), (db, nb) in zip(a, b))


def _slab_results(e, n):
    return [(d, int(h["n_kept"])) for h, d in e.read_slabs(n)]


# ---- 1. preprocess, bit-exact ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", LB)
@pytest.mark.parametrize("dtype", [zly.DTYPE_FP32, zly.DTYPE_BF16])
def test_preprocess_packed_equals_preprocess_of_its_bgr(weights_path, dtype, flags):
    e = zly.Engine(weights_path, dtype=dtype, max_batch=1, warmup_runs=0, flags=flags)
    for k, (w, h) in enumerate(SIZES):
        for fmt in FMTS:
            f, b = _packed(w, h, fmt, seed=100 + k)
            got = e.preprocess(f, fmt=fmt)
            want = e.preprocess(b)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (w, h, fmt)
    e.close()


# ---- 2. X is inert -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", LB)
def test_fourth_byte_never_reaches_a_result(weights_path, flags):
    e = zly.Engine(weights_path, dtype=zly.DTYPE_BF16, max_batch=1, max_dets=512, conf_thr=0.05, warmup_runs=0, flags=flags)
    covered = 0
    for k, (w, h) in enumerate([(640, 480), (416, 416), (3, 5), (1, 1)]):
        for fmt in (zly.PIX_BGRA, zly.PIX_RGBA):
            rnd = np.random.default_rng(900 + k).integers(0, 256, (h, w), dtype=np.uint8)
            pre, det = [], []
            for x in (0, 255, rnd):
                f, _ = _packed(w, h, fmt, seed=150 + k, x=x)
                pre.append(e.preprocess(f, fmt=fmt))
                det.append(e.detect(f, fmt=fmt))
            for p, d in zip(pre[1:], det[1:]):
                assert np.array_equal(p.view(np.uint32), pre[0].view(np.uint32)), (w, h, fmt)
                assert d[1] == det[0][1] and det_fields_equal(d[0], det[0][0]), (w, h, fmt)
            covered += det[0][1]
    assert covered > 0
    e.close()


# ---- 3. every front-kernel configuration -----------------------------------------------------------------------------------------
def _front_check(e, n, want_kernel, kernel_index=1):
    """detect_batch on mixed-size frames of mixed packed formats against their BGR conversions, same n: detections and head tensors identical"""
    sizes = [(416, 416), (640, 480), (100, 62), (418, 330)][:n]
    fmts = [FMTS[i % 3] for i in range(n)]
    pairs = [_packed(w, h, f, seed=200 + i) for i, ((w, h), f) in enumerate(zip(sizes, fmts))]
    got = e.detect_batch([p[0] for p in pairs], fmt=fmts)
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


# ---- 4. one batch of every format family -----------------------------------------------------------------------------------------
def _any_frame(fmt, w, h, seed):
    """(frame as the engine takes it, its BGR conversion)"""
    if fmt == zly.PIX_BGR:
        b = _bgr(w, h, seed)
        return b, b
    if fmt in FMTS:
        return _packed(w, h, fmt, seed)
    y = yr.bgr_to_yuv420(_bgr(w, h, seed), fmt)
    return y, yr.yuv420_to_bgr(y, w, h, fmt)


@pytest.mark.parametrize("flags", LB)
def test_mixed_formats_in_one_batch(weights_path, flags):
    e = zly.Engine(weights_path, dtype=zly.DTYPE_BF16, max_batch=6, max_dets=512, conf_thr=0.05, warmup_runs=0, flags=flags)
    fmts = [zly.PIX_BGR, zly.PIX_NV12_BT601, zly.PIX_I420_BT709, zly.PIX_RGB, zly.PIX_BGRA, zly.PIX_RGBA]
    sizes = [(416, 416), (640, 480), (418, 330), (100, 62), (416, 416), (333, 500)]
    pairs = [_any_frame(f, w, h, seed=300 + i) for i, (f, (w, h)) in enumerate(zip(fmts, sizes))]
    got = e.detect_batch([p[0] for p in pairs], fmt=fmts, ws=[s[0] for s in sizes], hs=[s[1] for s in sizes])
    heads = [e.head_tensor(i) for i in range(6)]
    want = e.detect_batch([p[1] for p in pairs])
    assert _same_results(got, want)
    for i in range(6):
        assert np.array_equal(heads[i], e.head_tensor(i))
    assert sum(k for _, k in got) > 0
    e.close()


# ---- 5. views of a pitched capture surface -----------------------------------------------------------------------------------------
def _c_view(fmt, w, h, off, pitch):
    c = zly.FrameView()
    c.fmt, c.w, c.h = fmt, w, h
    c.off[0], c.pitch[0] = off, pitch
    return c


@pytest.mark.parametrize("flags", LB)
@pytest.mark.parametrize("fmt", FMTS)
def test_views_of_a_pitched_surface(weights_path, fmt, flags):
    """regions of one surface with row padding, a pitch that is no multiple of 4 and an odd base offset, through zly_detect_view, zly_submit_view and
    zly_detect_device_view (n views of one device buffer): each equals the _fmt call on the tight frame cut out with numpy; bytes outside the
    regions, and every X byte, never reach a result"""
    bpp = pr.BPP[fmt]
    W, H, off = 480, 300, 3
    pitch = bpp * W + (5 if bpp == 4 else 7)
    assert pitch % 4 and off % 2
    surface, _ = _packed(W, H, fmt, seed=400 + fmt)
    buf, _ = pr.embed(surface, fmt, pitch, off, tail=0, seed=5)
    regions = [(0, 0, W, H), (37, 21, 301, 201), (W - 101, H - 63, 101, 63), (211, 150, 1, 2)]      # the third ends on the buffer's last byte
    last = regions[2]
    assert off + (last[1] + last[3] - 1) * pitch + (last[0] + last[2]) * bpp == buf.size
    whole = _c_view(fmt, W, H, off, pitch)
    assert zly.view_bytes(whole) == buf.size
    views = [zly.view_crop(whole, *r) for r in regions]
    tight = [pr.cut(buf, fmt, pitch, off, *r) for r in regions]
    n = len(regions)
    e = zly.Engine(weights_path, dtype=zly.DTYPE_BF16, max_batch=n, max_dets=512, conf_thr=0.05, warmup_runs=0, flags=flags)
    want1 = [e.detect(t, fmt=fmt) for t in tight]                                  # batches of one, as detect_view / a lone submit_view run
    want_n = e.detect_batch(tight, fmt=[fmt] * n)                                  # the batch of n, as detect_device_view runs
    want_heads = [e.head_tensor(i) for i in range(n)]
    assert sum(k for _, k in want_n) > 0

    def run_all(b):
        out1 = [e.detect_view(b, v) for v in views]
        out2 = []
        for v in views:
            out2.append(e.wait(e.submit_view(b, v)))
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
    # every byte outside a region, and every X byte inside it, takes another value: per region for the single-view calls ...
    for v, r, w1 in zip(views, regions, want1):
        keep = np.zeros(buf.size, dtype=bool)
        x0, y0, w, h = r
        for y in range(h):
            s = off + (y0 + y) * pitch + x0 * bpp
            px = keep[s: s + w * bpp].reshape(w, bpp)
            px[:, :3] = True
        b2 = np.where(keep, buf, buf ^ 0xA5).astype(np.uint8)
        g = e.detect_view(b2, v)
        assert g[1] == w1[1] and det_fields_equal(g[0], w1[0]), r
        g = e.wait(e.submit_view(b2, v))
        assert g[1] == w1[1] and det_fields_equal(g[0], w1[0]), r
    # ... and for the device call everything outside the surface's pixels (row padding, the base offset) and every X byte
    keep = np.zeros(buf.size, dtype=bool)
    for y in range(H):
        s = off + y * pitch
        keep[s: s + W * bpp].reshape(W, bpp)[:, :3] = True
    b3 = np.where(keep, buf, buf ^ 0x5A).astype(np.uint8)
    d3 = torch.from_numpy(b3).cuda()
    torch.cuda.synchronize()
    e.detect_device_view(d3.data_ptr(), b3.nbytes, views)
    assert _same_results(_slab_results(e, n), want_n)
    e.close()


# ---- 6. device path with captured graphs -------------------------------------------------------------------------------------------
def _smallest_throughput_batch(weights_path, flags, limit=64):
    """the smallest batch size whose front launch is the throughput front kernel (preprocess + model.0 + model.1 in one launch), asked of the engine"""
    e = zly.Engine(weights_path, dtype=zly.DTYPE_BF16, max_batch=limit, max_dets=16, use_graph=False, warmup_runs=0, flags=flags)
    try:
        for n in range(1, limit + 1):
            if "stem_model1_kernel" in e.op_kernels(n)[1]:
                return n
    finally:
        e.close()
    raise AssertionError("no batch size up to %d launches stem_model1_kernel" % limit)


@pytest.mark.parametrize("more", [0, 15], ids=["smallest", "tiles-outnumber-workgroups"])
def test_device_path_bgra_graph_replay_alternating(weights_path, more):
    """bench.py's engine flags with captured graphs: BGRA frames resident in HBM give the slabs of their BGR conversions; BGR and BGRA calls alternate on
    one engine so that both replay the captured graph.  At the smallest batch size that launches the throughput front kernel, and at one where its
    persistent workgroups walk more than one tile each"""
    flags = zly.FLAG_NO_HEAD_TENSOR | zly.FLAG_SINGLE_CHAIN
    n = _smallest_throughput_batch(weights_path, flags) + more
    w, h = 416, 416
    e = zly.Engine(weights_path, dtype=zly.DTYPE_BF16, max_batch=n, max_dets=128, use_graph=True, warmup_runs=1, flags=flags)
    assert "stem_model1_kernel" in e.op_kernels(n)[1]
    fmt = zly.PIX_BGRA
    bgr = zm.synth_frames(n, w, h, seed=500, rects=False)
    x = np.random.default_rng(501).integers(0, 256, (n, h, w), dtype=np.uint8)
    bgra = np.stack([pr.from_bgr(b, fmt, x=xx) for b, xx in zip(bgr, x)])
    d_bgra = torch.from_numpy(bgra).cuda()
    d_bgr = torch.from_numpy(np.ascontiguousarray(bgr)).cuda()
    torch.cuda.synchronize()
    prev = None
    replays0 = e.stats()["graph_replays"]
    total = 0
    for rnd in range(3):
        for which, buf in (("bgr", d_bgr), ("bgra", d_bgra)):
            e.detect_device(buf.data_ptr(), n, w, h, fmt=zly.PIX_BGR if which == "bgr" else fmt)
            slabs = e.read_slabs(n)
            if which == "bgr":
                prev = slabs
            else:
                for (hb, db), (hn, dn) in zip(prev, slabs):
                    assert int(hb["n_kept"]) == int(hn["n_kept"]) and int(hb["n_candidates"]) == int(hn["n_candidates"])
                    assert det_fields_equal(db, dn)
                    total += int(hn["n_candidates"])
    assert e.stats()["graph_replays"] - replays0 == 6
    assert total > 0
    e.close()


# ---- 7. pipelined path ---------------------------------------------------------------------------------------------------------------
def test_pipelined_submit_mixed_formats_fp32(weights_path):
    """fp32 engine (exact however the frames are batched): 4 threads submit frames of mixed formats, old and new, and mixed sizes; every ticket equals
    the synchronous BGR detect of the converted frame"""
    e = zly.Engine(weights_path, dtype=zly.DTYPE_FP32, max_batch=8, max_dets=128, conf_thr=0.05, warmup_runs=1)
    sizes = [(416, 416), (640, 480), (100, 62), (418, 330)]
    fmts = [zly.PIX_BGR, zly.PIX_RGB, zly.PIX_NV12_BT601, zly.PIX_BGRA, zly.PIX_I420_BT709, zly.PIX_RGBA, zly.PIX_BGRA]
    reqs = []
    for i in range(14):
        w, h = sizes[i % 4]
        f = fmts[i % 7]
        frame, b = _any_frame(f, w, h, seed=600 + i)
        reqs.append((np.ascontiguousarray(frame), f, w, h, b))
    serial = [e.detect(r[4], cap=128) for r in reqs]
    assert sum(s[1] for s in serial) > 0
    errors, results = [], []
    lock = threading.Lock()

    def worker(tid):
        try:
            for k in range(28):
                j = (tid * 5 + k) % len(reqs)
                frame, f, w, h, _ = reqs[j]
                t = e.submit(frame, fmt=f, w=w, h=h)
                r = e.wait(t, cap=128)
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
    assert len(results) == 112
    for j, (d, n) in results:
        assert n == serial[j][1] and det_fields_equal(d, serial[j][0]), j
    e.close()


def test_pipelined_batch_of_bgra_frames_larger_than_a_staging_slot(weights_path):
    """max_batch model-sized BGRA frames submitted at once are 4/3 of the BGR bytes a default staging slot is sized for: the ring splits them over
    two slots and every ticket still carries its frame's result"""
    n, w, h = 16, 416, 416
    e = zly.Engine(weights_path, dtype=zly.DTYPE_FP32, max_batch=n, max_dets=128, conf_thr=0.05, warmup_runs=0)
    slot = max(8 << 20, int(n * w * h * 3 * 1.25))                                 # the default slot size (no ZLY_STAGE_MB)
    assert "ZLY_STAGE_MB" not in os.environ and n * w * h * 4 > slot
    pairs = [_packed(w, h, zly.PIX_BGRA, seed=650 + i) for i in range(n)]
    want = [e.detect(b, cap=128) for _, b in pairs]
    tickets = [e.submit(f, fmt=zly.PIX_BGRA) for f, _ in pairs]
    got = [e.wait(t, cap=128) for t in tickets]
    assert _same_results(got, want)
    assert sum(k for _, k in got) > 0
    e.close()


# ---- 8. errors -------------------------------------------------------------------------------------------------------------------------
def test_errors_make_no_ticket_and_engine_still_serves(weights_path):
    e = zly.Engine(weights_path, dtype=zly.DTYPE_FP32, max_batch=2, max_dets=128, conf_thr=0.05, warmup_runs=0)
    lib = e.lib
    out = np.zeros(128, dtype=zly.DET_DTYPE)
    out3 = np.zeros((3, 416, 416), np.float32)
    n = C.c_int32(0)
    t = C.c_uint64(12345)
    w, h = 64, 48
    cases = []
    for fmt in FMTS:
        good = np.zeros(w * h * pr.BPP[fmt], np.uint8)
        other = w * h * (3 if pr.BPP[fmt] == 4 else 4)                             # the byte count of the other pixel size
        for nb in (good.nbytes - 1, good.nbytes + 1, other, 0):
            cases.append((fmt, np.zeros(max(nb, good.nbytes), np.uint8), nb, zly.ERR_INVALID_INPUT, good.nbytes))
    for fmt in (5, 15):
        cases.append((fmt, np.zeros(w * h * 4, np.uint8), w * h * 4, zly.ERR_INVALID_ARGUMENT, None))
    for f, buf, nb, code, expected in cases:
        assert lib.zly_detect_fmt(e.h, f, buf.ctypes.data, nb, w, h, out.ctypes.data, 128, C.byref(n)) == code, (f, nb)
        assert lib.zly_submit_fmt(e.h, f, buf.ctypes.data, nb, w, h, C.byref(t)) == code and t.value == 12345
        assert lib.zly_submit_try_fmt(e.h, f, buf.ctypes.data, nb, w, h, C.byref(t)) == code and t.value == 12345
        assert lib.zly_preprocess_fmt(e.h, f, buf.ctypes.data, nb, w, h, out3.ctypes.data) == code
        if code == zly.ERR_INVALID_INPUT:
            assert ("Invalid image data size: expected %d, got %d" % (expected, nb)).encode() in lib.zly_last_error()
        assert lib.zly_detect_device_fmt(e.h, f, 1, None, w, h, None, 0, None) == (code if code == zly.ERR_INVALID_ARGUMENT else zly.ERR_INVALID_INPUT)
    for fmt in FMTS:                                                               # the engine still serves good frames of every format
        f, b = _packed(416, 416, fmt, seed=700 + fmt)
        want = e.detect(b)
        got = e.detect(f, fmt=fmt)
        assert got[1] == want[1] and det_fields_equal(got[0], want[0])
        d2 = e.wait(e.submit(f, fmt=fmt))
        assert d2[1] == want[1] and det_fields_equal(d2[0], want[0])
    e.close()


# ---- 9. the plugin ---------------------------------------------------------------------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _exe(name):
    exe = os.path.join(ROOT, "zero-latency-yolo_amd", "_build", name)
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", ROOT, "host"], check=True, stdout=subprocess.DEVNULL)
    return exe


def _run_plugin(exe, weights_path, tmp_path, sizes, blobs, env):
    fpath, out = tmp_path / "frames.bin", tmp_path / "out.json"
    with open(fpath, "wb") as f:
        f.write(struct.pack("<I", len(blobs)))
        for (w, h), b in zip(sizes, blobs):
            f.write(struct.pack("<HHI", w, h, len(b)))
            f.write(b)
    r = subprocess.run([exe, weights_path, str(fpath), str(out)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ZLY_MAX_BATCH="8", ZLY_FP32="1", **env))     # fp32: exact however the plugin batches
    assert r.returncode == 0, r.stderr
    return json.loads(out.read_text())


def _bits(d):
    return [int(d[c].view(np.uint32)) for c in ("x", "y", "w", "h", "confidence")] + [int(d["class_id"])]


@pytest.mark.parametrize("name,fmt,program", [("rgb", zly.PIX_RGB, "test_hip_engine_yuv"), ("bgra", zly.PIX_BGRA, "test_hip_engine_pix")])
def test_plugin_packed_requests_equal_c_abi(tmp_path, weights_path, name, fmt, program):
    """the plugin with ZLY_INPUT_FORMAT=rgb / bgra: every request's callback carries exactly the detections zly_detect_fmt gives for that frame; a
    request of the wrong size fails alone (no callback, one inference error).  rgb runs the existing program tests/cpp/test_hip_engine_yuv.cpp (an RGB
    frame has a BGR frame's byte count, which is what that program expects callbacks for); bgra needs tests/cpp/test_hip_engine_pix.cpp, which knows
    the format's frame size"""
    sizes = [(416, 416), (640, 480), (100, 62), (416, 416), (418, 330), (3, 5)]
    frames = [_packed(w, h, fmt, seed=800 + i)[0] for i, (w, h) in enumerate(sizes)]
    bad = 3
    blobs = [f.tobytes() for f in frames]
    blobs[bad] = blobs[bad][:-4] if fmt == zly.PIX_RGB else _bgr(416, 416, 899).tobytes()      # a short frame / a BGR-sized frame in a BGRA stream
    j = _run_plugin(_exe(program), weights_path, tmp_path, sizes, blobs, {"ZLY_INPUT_FORMAT": name})
    good = [i for i in range(len(sizes)) if i != bad]
    assert [x["frame_id"] for x in j["results"]] == good
    assert j["status"]["inference_errors"] == "1"
    assert j["status"]["input_format"] == name
    e = zly.Engine(weights_path, dtype=zly.DTYPE_FP32, max_batch=1, max_dets=256, warmup_runs=0)
    total = 0
    for x in j["results"]:
        i = x["frame_id"]
        dets, n = e.detect(frames[i], fmt=fmt, cap=256)
        got = np.array(x["dets"], dtype=np.int64).reshape(-1, 6)
        assert len(got) == len(dets), i
        for k, d in enumerate(dets):
            assert got[k].tolist() == _bits(d), (i, k)
        total += n
    assert total > 0
    e.close()


def test_plugin_crop_of_bgra_requests_at_an_odd_window(tmp_path, weights_path):
    """ZLY_CROP with ZLY_INPUT_FORMAT=bgra at an odd window size (a YUV stream would refuse it): the boxes are zly_detect_view's on the same window,
    mapped to fractions of the whole frame by INTEGRATION.md section 3's map in single fp32 operations"""
    fmt, cw, ch = zly.PIX_BGRA, 301, 201
    sizes = [(640, 480), (417, 333), (301, 201), (200, 300)]                       # the last is smaller than the window on one axis: detected whole
    frames = [_packed(w, h, fmt, seed=850 + i)[0] for i, (w, h) in enumerate(sizes)]
    j = _run_plugin(_exe("test_hip_engine_pix"), weights_path, tmp_path, sizes, [f.tobytes() for f in frames],
                    {"ZLY_INPUT_FORMAT": "bgra", "ZLY_CROP": "%dx%d" % (cw, ch), "ZLY_TEST_CONF_THR": "0.05"})
    assert [x["frame_id"] for x in j["results"]] == list(range(len(sizes)))
    assert j["status"]["crop"] == "%dx%d" % (cw, ch) and j["status"]["inference_errors"] == "0"
    e = zly.Engine(weights_path, dtype=zly.DTYPE_FP32, max_batch=1, max_dets=256, conf_thr=0.05, warmup_runs=0)
    f32 = np.float32
    total = 0
    for x in j["results"]:
        i = x["frame_id"]
        w, h = sizes[i]
        buf = frames[i].reshape(-1)
        got = np.array(x["dets"], dtype=np.int64).reshape(-1, 6)
        if w >= cw and h >= ch:
            x0, y0 = (w - cw) // 2, (h - ch) // 2                                  # odd origins stay odd: no evenness rule for packed formats
            dets, n = e.detect_view(buf, zly.view_crop(zly.view_tight(fmt, w, h), x0, y0, cw, ch), cap=256)
            dets = dets.copy()
            dets["x"] = ((dets["x"] * f32(cw)).astype(f32) + f32(x0)).astype(f32) / f32(w)
            dets["y"] = ((dets["y"] * f32(ch)).astype(f32) + f32(y0)).astype(f32) / f32(h)
            dets["w"] = (dets["w"] * f32(cw)).astype(f32) / f32(w)
            dets["h"] = (dets["h"] * f32(ch)).astype(f32) / f32(h)
        else:
            dets, n = e.detect(frames[i], fmt=fmt, cap=256)
        assert len(got) == len(dets), i
        for k, d in enumerate(dets):
            assert got[k].tolist() == _bits(d), (i, k)
        total += n
    assert total > 0
    e.close()
