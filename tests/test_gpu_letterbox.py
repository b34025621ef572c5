"""The letterbox resize mode (include/zly.h ZLY_FLAG_LETTERBOX) on the GPU, bit-exact throughout against tests/letterbox_ref.py:
the front kernels of a letterbox engine must give, for a request frame, exactly what a stretch engine with the same settings gives for
letterbox_bgr(frame) (a model-sized frame: its resize is the identity), and the boxes must be the head's boxes mapped out of the
letterbox by the stated fp32 operations -- in every front-kernel configuration, on every entry point that takes frames."""
import ctypes as C
import json
import os
import struct
import subprocess
import threading

import numpy as np
import pytest
import torch            # before the first engine: the process then uses torch's HIP runtime throughout, as tests/test_gpu_parity.py does

import letterbox_ref as lb
import yuv_ref as yr
import zly
import zly_model as zm
from oracle_lib import det_fields_equal

pytestmark = pytest.mark.gpu

LBF = zly.FLAG_LETTERBOX
SIZES = [(416, 416), (640, 480), (1280, 720), (1920, 1080), (100, 62), (418, 330), (233, 416), (2, 2), (3, 1001), (4000, 3)]
ALL_FMTS = (zly.PIX_NV12_BT601, zly.PIX_I420_BT601, zly.PIX_NV12_BT709, zly.PIX_I420_BT709)
CONF, IOU = 0.05, 0.45


def _frame(w, h, seed):
    return np.ascontiguousarray(zm.synth_frames(1, w, h, seed=seed, rects=w >= 16 and h >= 16)[0])


def _same_results(a, b):
    return len(a) == len(b) and all(na == nb and det_fields_equal(da, db) for (da, na), (db, nb) in zip(a, b))


@pytest.mark.parametrize("dtype", [zly.DTYPE_FP32, zly.DTYPE_BF16])
def test_preprocess_equals_reference(weights_path, dtype):
    e = zly.Engine(weights_path, dtype=dtype, max_batch=1, warmup_runs=0, flags=LBF)
    for k, (w, h) in enumerate(SIZES):
        f = _frame(w, h, seed=100 + k)
        got = e.preprocess(f)
        want = lb.preprocess_planar(f, 416, 416)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (w, h, int((got != want).sum()))
    e.close()


def test_preprocess_non_square_model(weights_path):
    e = zly.Engine(weights_path, dtype=zly.DTYPE_FP32, model_w=640, model_h=384, max_batch=1, warmup_runs=0, flags=LBF)
    for k, (w, h) in enumerate([(1920, 1080), (384, 640), (640, 384), (100, 62)]):
        f = _frame(w, h, seed=150 + k)
        assert np.array_equal(e.preprocess(f).view(np.uint32), lb.preprocess_planar(f, 640, 384).view(np.uint32)), (w, h)
    e.close()


def _front_check(oracle, make_engine, n, want_kernel, kernel_index=1):
    """detect_batch of mixed-size frames on a letterbox engine: head tensors equal those of a stretch engine with the same settings fed the
    reference's letterboxed frames (same n), detections equal the CPU oracle's post-processing of the un-padded head, and the kernel names
    show the letterbox instantiations"""
    sizes = [(640, 480), (1920, 1080), (100, 62), (233, 416), (416, 416), (418, 330)][:n]
    frames = [_frame(w, h, seed=200 + i) for i, (w, h) in enumerate(sizes)]
    e = make_engine(LBF)
    tw, th = e.model_w, e.model_h
    got = e.detect_batch(frames)
    heads = [e.head_tensor(i) for i in range(n)]
    names = e.op_kernels(n)
    assert want_kernel in names[kernel_index] and "LB" in names[kernel_index], names[kernel_index]
    assert any("head_fused_kernel<LB>" in k for k in names), names
    e.close()
    s = make_engine(0)
    boxed = [lb.letterbox_bgr(f, tw, th) for f in frames]
    s.detect_batch(boxed)
    for i in range(n):
        assert np.array_equal(heads[i], s.head_tensor(i)), (i, sizes[i])
    stretch = s.detect_batch(frames)
    assert not any("LB" in k for k in s.op_kernels(n))
    s.close()
    for i, (w, h) in enumerate(sizes):
        hp, nw, nh = lb.unpad_head(heads[i], w, h, tw, th)
        want = oracle.postprocess(hp, nw, nh, CONF, IOU)
        d, k = got[i]
        assert k == len(want) and det_fields_equal(d, want[:len(d)]), (i, sizes[i], k, len(want))
    assert sum(k for _, k in got) > 0                              # the comparison covered detections
    # a mode that silently does nothing cannot pass: a non-square frame's result differs from the stretch engine's
    assert not _same_results(got[:2], stretch[:2])
    return got


@pytest.mark.parametrize("var", [None, "0", "2"])
def test_front_stem_model1_all_variants(weights_path, oracle, monkeypatch, var):
    if var is not None:
        monkeypatch.setenv("ZLY_STEM1_VAR", var)                   # read at zly_create
    mk = lambda fl: zly.Engine(weights_path, dtype=zly.DTYPE_BF16, max_batch=4, max_dets=512, conf_thr=CONF, warmup_runs=0, flags=fl)
    _front_check(oracle, mk, 4, "stem_model1_kernel")


def test_front_stem_fused_no_stem1(weights_path, oracle, monkeypatch):
    monkeypatch.setenv("ZLY_NO_STEM1", "1")
    mk = lambda fl: zly.Engine(weights_path, dtype=zly.DTYPE_BF16, max_batch=4, max_dets=512, conf_thr=CONF, warmup_runs=0, flags=fl)
    _front_check(oracle, mk, 4, "stem_fused_kernel")


def test_front_no_fusion(weights_path, oracle):
    mk = lambda fl: zly.Engine(weights_path, dtype=zly.DTYPE_BF16, max_batch=4, max_dets=512, conf_thr=CONF, warmup_runs=0, flags=fl | zly.FLAG_NO_FUSION)
    _front_check(oracle, mk, 4, "stem_fused_kernel")


def test_front_yolov8s_stem_fused_two_tiles(tmp_path, oracle):
    spec = zm.build_spec("s")
    p = str(tmp_path / "yolov8s_synth.zlyw")
    zm.write_zlyw(p, spec, zm.synth_weights(spec, seed=9))
    mk = lambda fl: zly.Engine(p, dtype=zly.DTYPE_BF16, max_batch=3, max_dets=512, conf_thr=CONF, warmup_runs=0, flags=fl)
    _front_check(oracle, mk, 3, "stem_fused_kernel")


def test_front_fp32_preprocess_kernel(weights_path, oracle):
    mk = lambda fl: zly.Engine(weights_path, dtype=zly.DTYPE_FP32, max_batch=6, max_dets=512, conf_thr=CONF, warmup_runs=0, flags=fl)
    _front_check(oracle, mk, 6, "preprocess_kernel", kernel_index=0)


def test_decode_without_head_tensor_equals_decode_with_it(weights_path):
    """the production decode site (ZLY_FLAG_NO_HEAD_TENSOR: no head tensor is written) gives the detections of the engine that writes it"""
    sizes = [(640, 480), (1920, 1080), (100, 62), (233, 416)]
    frames = [_frame(w, h, seed=250 + i) for i, (w, h) in enumerate(sizes)]
    a = zly.Engine(weights_path, dtype=zly.DTYPE_BF16, max_batch=4, max_dets=512, conf_thr=CONF, warmup_runs=1, flags=LBF)
    want = a.detect_batch(frames)
    a.close()
    b = zly.Engine(weights_path, dtype=zly.DTYPE_BF16, max_batch=4, max_dets=512, conf_thr=CONF, warmup_runs=1, flags=LBF | zly.FLAG_NO_HEAD_TENSOR)
    got = b.detect_batch(frames)
    b.close()
    assert _same_results(got, want) and sum(k for _, k in got) > 0


def test_model_sized_frames_equal_the_stretch_engine(weights_path):
    """w == model_w and h == model_h: the letterbox map is the identity, and so is the box mapping"""
    frames = [_frame(416, 416, seed=270 + i) for i in range(3)]
    a = zly.Engine(weights_path, dtype=zly.DTYPE_BF16, max_batch=3, max_dets=512, conf_thr=CONF, warmup_runs=1, flags=LBF)
    got = a.detect_batch(frames)
    pre = a.preprocess(frames[0])
    a.close()
    b = zly.Engine(weights_path, dtype=zly.DTYPE_BF16, max_batch=3, max_dets=512, conf_thr=CONF, warmup_runs=1)
    want = b.detect_batch(frames)
    assert np.array_equal(pre, b.preprocess(frames[0]))
    b.close()
    assert _same_results(got, want) and sum(k for _, k in got) > 0


def _yuv(w, h, fmt, seed):
    return yr.bgr_to_yuv420(zm.synth_frames(1, w, h, seed=seed, rects=w >= 16 and h >= 16)[0], fmt)


@pytest.mark.parametrize("dtype", [zly.DTYPE_FP32, zly.DTYPE_BF16])
def test_yuv_frames_equal_their_bgr_conversion(weights_path, dtype):
    e = zly.Engine(weights_path, dtype=dtype, max_batch=5, max_dets=512, conf_thr=CONF, warmup_runs=0, flags=LBF)
    for k, (w, h) in enumerate([(416, 416), (640, 480), (1280, 720), (100, 62), (418, 330), (2, 2)]):
        for fmt in ALL_FMTS:
            y = _yuv(w, h, fmt, seed=300 + k)
            bgr = yr.yuv420_to_bgr(y, w, h, fmt)
            got = e.preprocess(y, fmt=fmt, w=w, h=h)
            assert np.array_equal(got.view(np.uint32), lb.preprocess_planar(bgr, 416, 416).view(np.uint32)), (w, h, fmt)
    # one batch mixes BGR and YUV frames
    fmts = [zly.PIX_BGR, *ALL_FMTS]
    sizes = [(640, 480), (416, 416), (418, 330), (100, 62), (1280, 720)]
    frames, bgr = [], []
    for i, (f, (w, h)) in enumerate(zip(fmts, sizes)):
        if f == zly.PIX_BGR:
            b = _frame(w, h, seed=330 + i)
            frames.append(b); bgr.append(b)
        else:
            y = _yuv(w, h, f, seed=330 + i)
            frames.append(y); bgr.append(yr.yuv420_to_bgr(y, w, h, f))
    got = e.detect_batch(frames, fmt=fmts, ws=[s[0] for s in sizes], hs=[s[1] for s in sizes])
    heads = [e.head_tensor(i) for i in range(5)]
    want = e.detect_batch(bgr)
    assert _same_results(got, want) and sum(k for _, k in got) > 0
    for i in range(5):
        assert np.array_equal(heads[i], e.head_tensor(i))
    e.close()


def test_device_path_batch64_graph_replay(weights_path):
    """the throughput configuration (bf16, batch 64, captured graphs, bench.py's engine flags) in letterbox mode: 1280 x 720 frames resident
    in HBM give the slabs of the same engine's detect_batch for those frames, and every call replays the captured graph"""
    n, w, h = 64, 1280, 720
    e = zly.Engine(weights_path, dtype=zly.DTYPE_BF16, max_batch=n, max_dets=128, conf_thr=0.25, use_graph=True, warmup_runs=1,
                   flags=zly.FLAG_NO_HEAD_TENSOR | zly.FLAG_SINGLE_CHAIN | LBF)
    base = zm.synth_frames(8, w, h, seed=400)
    frames = np.ascontiguousarray(np.stack([base[i % 8] if i < 8 else np.roll(base[i % 8], 16 * (i // 8), axis=1) for i in range(n)]))
    want = e.detect_batch(list(frames), cap=128)
    d = torch.from_numpy(frames).cuda()
    torch.cuda.synchronize()
    st0 = e.stats()
    for _ in range(3):
        e.detect_device(d.data_ptr(), n, w, h)
        slabs = e.read_slabs(n)
        for (hd, dets), (wd, wn) in zip(slabs, want):
            assert int(hd["n_kept"]) == wn and det_fields_equal(dets, wd)
    st1 = e.stats()
    assert st1["graph_replays"] - st0["graph_replays"] == 3 and st1["eager_batches"] == st0["eager_batches"]
    assert sum(k for _, k in want) > 0
    assert "LB" in e.op_kernels(n)[1]
    e.close()


def test_pipelined_submit_mixed_sizes_and_formats_fp32(weights_path):
    """fp32 engine (exact however the frames are batched): 4 threads submit 256 frames of mixed sizes and formats; every ticket equals the
    synchronous detect of its frame"""
    e = zly.Engine(weights_path, dtype=zly.DTYPE_FP32, max_batch=8, max_dets=128, conf_thr=CONF, warmup_runs=1, flags=LBF)
    sizes = [(416, 416), (640, 480), (100, 62), (418, 330), (1280, 720)]
    fmts = [zly.PIX_BGR, zly.PIX_BGR, zly.PIX_NV12_BT601, zly.PIX_I420_BT709]
    reqs = []
    for i in range(10):
        w, h = sizes[i % 5]
        f = fmts[i % 4]
        reqs.append((_frame(w, h, seed=500 + i) if f == zly.PIX_BGR else _yuv(w, h, f, seed=500 + i), f, w, h))
    serial = [e.detect(fr, cap=128, fmt=f, w=w, h=h) for fr, f, w, h in reqs]
    assert sum(k for _, k in serial) > 0
    errors, results = [], []
    lock = threading.Lock()

    def worker(tid):
        try:
            for k in range(64):
                j = (tid * 64 + k) % len(reqs)
                frame, f, w, h = reqs[j]
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
    assert len(results) == 256
    for j, (d, n) in results:
        assert n == serial[j][1] and det_fields_equal(d, serial[j][0]), j
    e.close()


def test_oversized_frames_are_refused_and_engine_still_serves(weights_path):
    e = zly.Engine(weights_path, dtype=zly.DTYPE_FP32, max_batch=2, max_dets=128, conf_thr=CONF, warmup_runs=0, flags=LBF)
    lib = e.lib
    wide = np.zeros((1, 16385, 3), np.uint8)
    tall = np.zeros((16385, 1, 3), np.uint8)
    out = np.zeros(128, dtype=zly.DET_DTYPE)
    n = C.c_int32(0)
    t = C.c_uint64(12345)
    pre = np.zeros((3, 416, 416), np.float32)
    for f in (wide, tall):
        h, w = f.shape[:2]
        assert lib.zly_detect(e.h, f.ctypes.data, f.nbytes, w, h, out.ctypes.data, 128, C.byref(n)) == zly.ERR_INVALID_INPUT
        assert b"letterbox" in lib.zly_last_error()
        assert lib.zly_submit(e.h, f.ctypes.data, f.nbytes, w, h, C.byref(t)) == zly.ERR_INVALID_INPUT and t.value == 12345
        assert lib.zly_submit_try(e.h, f.ctypes.data, f.nbytes, w, h, C.byref(t)) == zly.ERR_INVALID_INPUT and t.value == 12345
        assert lib.zly_preprocess(e.h, f.ctypes.data, f.nbytes, w, h, pre.ctypes.data) == zly.ERR_INVALID_INPUT
    d = torch.zeros(16385 * 3, dtype=torch.uint8, device="cuda")
    assert lib.zly_detect_device(e.h, 1, d.data_ptr(), 16385, 1, None, 0, None) == zly.ERR_INVALID_INPUT
    edge = np.zeros((1, 16384, 3), np.uint8)                       # the limit itself is served
    e.detect(edge)
    good = _frame(640, 480, seed=600)
    want = e.detect(good, cap=128)
    got = e.wait(e.submit(good), cap=128)
    assert got[1] == want[1] and det_fields_equal(got[0], want[0]) and want[1] > 0
    e.close()
    # a stretch engine takes the same frame as before
    s = zly.Engine(weights_path, dtype=zly.DTYPE_FP32, max_batch=1, max_dets=128, warmup_runs=0)
    s.detect(wide)
    s.close()


def test_plugin_letterbox_requests_equal_c_abi(tmp_path, weights_path):
    """the plugin with ZLY_RESIZE=letterbox (the unchanged tests/cpp/test_hip_engine_yuv.cpp, BGR requests): every callback carries exactly
    the detections zly_detect gives on a letterbox engine; the status names the mode; an unknown mode fails initialize()"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "zero-latency-yolo_amd", "_build", "test_hip_engine_yuv")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", root, "host"], check=True, stdout=subprocess.DEVNULL)
    sizes = [(416, 416), (800, 600), (640, 480), (100, 62), (1280, 720), (233, 416)]
    # noise frames beside the rectangle scenes: the plugin runs at the server's confidence threshold (0.5), which the noise frames reach
    frames = [np.ascontiguousarray(zm.synth_frames(1, w, h, seed=5 + i, rects=i == 2)[0]) for i, (w, h) in enumerate(sizes)]
    fpath, out = tmp_path / "frames.bin", tmp_path / "out.json"
    with open(fpath, "wb") as f:
        f.write(struct.pack("<I", len(frames)))
        for (w, h), fr in zip(sizes, frames):
            b = fr.tobytes()
            f.write(struct.pack("<HHI", w, h, len(b)))
            f.write(b)
    env = {k: v for k, v in os.environ.items() if k != "ZLY_INPUT_FORMAT"}
    env.update(ZLY_RESIZE="letterbox", ZLY_MAX_BATCH="8", ZLY_FP32="1")           # fp32: exact however the plugin batches
    r = subprocess.run([exe, weights_path, str(fpath), str(out)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr
    j = json.loads(out.read_text())
    assert j["status"]["resize_mode"] == "letterbox"
    assert sorted(x["frame_id"] for x in j["results"]) == list(range(len(sizes)))
    e = zly.Engine(weights_path, dtype=zly.DTYPE_FP32, max_batch=1, max_dets=256, warmup_runs=0, flags=LBF)
    s = zly.Engine(weights_path, dtype=zly.DTYPE_FP32, max_batch=1, max_dets=256, warmup_runs=0)
    total, differs = 0, False
    for x in j["results"]:
        i = x["frame_id"]
        dets, n = e.detect(frames[i], cap=256)
        got = np.array(x["dets"], dtype=np.int64).reshape(-1, 6)
        assert len(got) == len(dets), i
        total += len(dets)
        for k, d in enumerate(dets):
            bits = [int(d[c].view(np.uint32)) for c in ("x", "y", "w", "h", "confidence")]
            assert list(got[k, :5]) == bits and got[k, 5] == int(d["class_id"]), (i, k)
        sd, sn = s.detect(frames[i], cap=256)
        differs = differs or sn != n or not det_fields_equal(sd, dets)
    assert total > 0 and differs
    e.close()
    s.close()
    bad = subprocess.run([exe, weights_path, str(fpath), str(out)], capture_output=True, text=True, timeout=300, env=dict(env, ZLY_RESIZE="bogus"))
    assert bad.returncode == 4 and "ZLY_RESIZE" in bad.stderr, (bad.returncode, bad.stderr)
