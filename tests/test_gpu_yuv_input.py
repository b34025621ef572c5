"""YUV 4:2:0 request frames (include/zly.h ZLY_PIX_NV12_* / ZLY_PIX_I420_*) on the GPU.  The front kernels convert a YUV frame's pixels
to the B, G, R bytes of tests/yuv_ref.py's integer formula and then take the BGR path, so engine(yuv) must equal, bit for bit,
engine(yuv420_to_bgr(yuv)) on the same engine with the same batch composition -- in every front-kernel configuration."""
import json
import os
import struct
import subprocess
import threading

import numpy as np
import pytest
import torch            # before the first engine: the process then uses torch's HIP runtime throughout, as tests/test_gpu_parity.py does

import yuv_ref as yr
import zly
import zly_model as zm
from oracle_lib import det_fields_equal

pytestmark = pytest.mark.gpu

ALL_FMTS = (zly.PIX_NV12_BT601, zly.PIX_I420_BT601, zly.PIX_NV12_BT709, zly.PIX_I420_BT709)
SIZES = [(416, 416), (640, 480), (1280, 720), (1920, 1080), (100, 62), (418, 330), (2, 2)]


def _yuv(w, h, fmt, seed):
    return yr.bgr_to_yuv420(zm.synth_frames(1, w, h, seed=seed, rects=w >= 16 and h >= 16)[0], fmt)


def _same_results(a, b):
    return len(a) == len(b) and all(na == nb and det_fields_equal(da, db) for (da, na), (db, nb) in zip(a, b))


@pytest.mark.parametrize("dtype", [zly.DTYPE_FP32, zly.DTYPE_BF16])
def test_preprocess_yuv_equals_preprocess_of_its_bgr(weights_path, dtype):
    e = zly.Engine(weights_path, dtype=dtype, max_batch=1, warmup_runs=0)
    for k, (w, h) in enumerate(SIZES):
        for fmt in ALL_FMTS:
            yuv = _yuv(w, h, fmt, seed=100 + k)
            got = e.preprocess(yuv, fmt=fmt, w=w, h=h)
            want = e.preprocess(yr.yuv420_to_bgr(yuv, w, h, fmt))
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (w, h, fmt)
    e.close()


def _front_check(e, n, want_kernel, kernel_index=1):
    """detect_batch on mixed-size YUV frames against their BGR conversions, same n: detections and head tensors identical"""
    sizes = [(416, 416), (640, 480), (100, 62), (418, 330), (1280, 720), (2, 2)][:n]
    fmts = [ALL_FMTS[i % 4] for i in range(n)]
    yuv = [_yuv(w, h, f, seed=200 + i) for i, ((w, h), f) in enumerate(zip(sizes, fmts))]
    bgr = [yr.yuv420_to_bgr(y, w, h, f) for y, (w, h), f in zip(yuv, sizes, fmts)]
    got = e.detect_batch(yuv, fmt=fmts, ws=[s[0] for s in sizes], hs=[s[1] for s in sizes])
    got_heads = [e.head_tensor(i) for i in range(n)]
    want = e.detect_batch(bgr)
    want_heads = [e.head_tensor(i) for i in range(n)]
    assert _same_results(got, want)
    for g, w_ in zip(got_heads, want_heads):
        assert np.array_equal(g, w_)
    assert sum(k for _, k in got) > 0                          # the comparison covered detections
    assert want_kernel in e.op_kernels(n)[kernel_index], e.op_kernels(n)[kernel_index]


@pytest.mark.parametrize("var", [None, "0", "2"])
def test_front_stem_model1_all_variants(weights_path, monkeypatch, var):
    if var is not None:
        monkeypatch.setenv("ZLY_STEM1_VAR", var)               # read at zly_create
    e = zly.Engine(weights_path, dtype=zly.DTYPE_BF16, max_batch=4, max_dets=512, conf_thr=0.05, warmup_runs=0)
    _front_check(e, 4, "stem_model1_kernel")
    e.close()


def test_front_stem_fused_no_stem1(weights_path, monkeypatch):
    monkeypatch.setenv("ZLY_NO_STEM1", "1")
    e = zly.Engine(weights_path, dtype=zly.DTYPE_BF16, max_batch=4, max_dets=512, conf_thr=0.05, warmup_runs=0)
    _front_check(e, 4, "stem_fused_kernel")
    e.close()


def test_front_no_fusion(weights_path):
    e = zly.Engine(weights_path, dtype=zly.DTYPE_BF16, max_batch=4, max_dets=512, conf_thr=0.05, warmup_runs=0, flags=zly.FLAG_NO_FUSION)
    _front_check(e, 4, "stem_fused_kernel")
    e.close()


def test_front_yolov8s_stem_fused_two_tiles(tmp_path):
    spec = zm.build_spec("s")
    p = str(tmp_path / "yolov8s_synth.zlyw")
    zm.write_zlyw(p, spec, zm.synth_weights(spec, seed=9))
    e = zly.Engine(p, dtype=zly.DTYPE_BF16, max_batch=3, max_dets=512, conf_thr=0.05, warmup_runs=0)
    _front_check(e, 3, "stem_fused_kernel")
    e.close()


def test_front_fp32_preprocess_kernel(weights_path):
    e = zly.Engine(weights_path, dtype=zly.DTYPE_FP32, max_batch=4, max_dets=512, conf_thr=0.05, warmup_runs=0)
    _front_check(e, 4, "preprocess_kernel", kernel_index=0)
    e.close()


def test_mixed_formats_in_one_batch(weights_path):
    e = zly.Engine(weights_path, dtype=zly.DTYPE_BF16, max_batch=5, max_dets=512, conf_thr=0.05, warmup_runs=0)
    fmts = [zly.PIX_BGR, *ALL_FMTS]
    sizes = [(640, 480), (416, 416), (418, 330), (100, 62), (416, 416)]
    frames, bgr = [], []
    for i, (f, (w, h)) in enumerate(zip(fmts, sizes)):
        if f == zly.PIX_BGR:
            b = zm.synth_frames(1, w, h, seed=300 + i)[0]
            frames.append(b); bgr.append(b)
        else:
            y = _yuv(w, h, f, seed=300 + i)
            frames.append(y); bgr.append(yr.yuv420_to_bgr(y, w, h, f))
    got = e.detect_batch(frames, fmt=fmts, ws=[s[0] for s in sizes], hs=[s[1] for s in sizes])
    heads = [e.head_tensor(i) for i in range(5)]
    want = e.detect_batch(bgr)
    assert _same_results(got, want)
    for i in range(5):
        assert np.array_equal(heads[i], e.head_tensor(i))
    e.close()


def test_device_path_nv12_batch64_graph_replay_alternating(weights_path):
    """the headline configuration (bf16 YOLOv8n 416 x 416, batch 64, captured graphs, bench.py's engine flags): NV12 frames resident
    in HBM give the slabs of their BGR conversions; BGR and NV12 calls alternate on one engine so that both replay the captured graph"""
    n, w, h = 64, 416, 416
    e = zly.Engine(weights_path, dtype=zly.DTYPE_BF16, max_batch=n, max_dets=128, use_graph=True, warmup_runs=1,
                   flags=zly.FLAG_NO_HEAD_TENSOR | zly.FLAG_SINGLE_CHAIN)
    fmt = zly.PIX_NV12_BT601
    src = zm.synth_frames(n, w, h, seed=400, rects=False)
    nv12 = np.stack([yr.bgr_to_yuv420(f, fmt) for f in src])
    bgr = np.stack([yr.yuv420_to_bgr(y, w, h, fmt) for y in nv12])
    d_nv12 = torch.from_numpy(nv12).cuda()
    d_bgr = torch.from_numpy(bgr).cuda()
    torch.cuda.synchronize()
    prev = None
    replays0 = e.stats()["graph_replays"]
    for rnd in range(3):
        for which, buf in (("bgr", d_bgr), ("nv12", d_nv12)):
            e.detect_device(buf.data_ptr(), n, w, h, fmt=zly.PIX_BGR if which == "bgr" else fmt)
            slabs = e.read_slabs(n)
            if which == "bgr":
                prev = slabs
            else:
                for (hb, db), (hn, dn) in zip(prev, slabs):
                    assert int(hb["n_kept"]) == int(hn["n_kept"]) and int(hb["n_candidates"]) == int(hn["n_candidates"])
                    assert det_fields_equal(db, dn)
    assert e.stats()["graph_replays"] - replays0 == 6
    e.close()


def test_pipelined_submit_mixed_formats_fp32(weights_path):
    """fp32 engine (exact however the frames are batched): 4 threads submit 256 frames of mixed formats and sizes; every ticket equals
    the synchronous BGR detect of the converted frame"""
    e = zly.Engine(weights_path, dtype=zly.DTYPE_FP32, max_batch=8, max_dets=128, conf_thr=0.05, warmup_runs=1)
    sizes = [(416, 416), (640, 480), (100, 62), (418, 330)]
    fmts = [zly.PIX_BGR, *ALL_FMTS]
    reqs = []
    for i in range(10):
        w, h = sizes[i % 4]
        f = fmts[i % 5]
        if f == zly.PIX_BGR:
            b = np.ascontiguousarray(zm.synth_frames(1, w, h, seed=500 + i)[0])
            reqs.append((b, f, w, h, b))
        else:
            y = _yuv(w, h, f, seed=500 + i)
            reqs.append((y, f, w, h, yr.yuv420_to_bgr(y, w, h, f)))
    serial = [e.detect(r[4], cap=128) for r in reqs]
    errors, results = [], []
    lock = threading.Lock()

    def worker(tid):
        try:
            for k in range(64):
                j = (tid * 64 + k) % len(reqs)
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
    assert len(results) == 256
    for j, (d, n) in results:
        assert n == serial[j][1] and det_fields_equal(d, serial[j][0]), j
    e.close()


def test_errors_make_no_ticket_and_engine_still_serves(weights_path):
    e = zly.Engine(weights_path, dtype=zly.DTYPE_FP32, max_batch=2, max_dets=128, conf_thr=0.05, warmup_runs=0)
    lib = e.lib
    import ctypes as C
    odd = np.zeros(417 * 416 * 3 // 2, np.uint8)
    good = _yuv(416, 416, zly.PIX_NV12_BT601, seed=600)
    out = np.zeros(128, dtype=zly.DET_DTYPE)
    n = C.c_int32(0)
    t = C.c_uint64(12345)
    cases = [(zly.PIX_NV12_BT601, odd, odd.nbytes, 417, 416, zly.ERR_INVALID_INPUT),          # odd width
             (zly.PIX_I420_BT601, good, good.nbytes, 416, 415, zly.ERR_INVALID_INPUT),        # odd height
             (zly.PIX_NV12_BT709, good, good.nbytes - 1, 416, 416, zly.ERR_INVALID_INPUT),    # wrong size
             (zly.PIX_NV12_BT601, good, good.nbytes, 1, 1, zly.ERR_INVALID_INPUT),            # too small
             (7, good, good.nbytes, 416, 416, zly.ERR_INVALID_ARGUMENT)]                      # unknown format
    for f, buf, nb, w, h, code in cases:
        assert lib.zly_detect_fmt(e.h, f, buf.ctypes.data, nb, w, h, out.ctypes.data, 128, C.byref(n)) == code
        assert lib.zly_submit_fmt(e.h, f, buf.ctypes.data, nb, w, h, C.byref(t)) == code and t.value == 12345
        assert lib.zly_submit_try_fmt(e.h, f, buf.ctypes.data, nb, w, h, C.byref(t)) == code and t.value == 12345
        out3 = np.zeros((3, 416, 416), np.float32)
        assert lib.zly_preprocess_fmt(e.h, f, buf.ctypes.data, nb, w, h, out3.ctypes.data) == code
        if code == zly.ERR_INVALID_INPUT:
            assert b"Invalid image data size: expected" in lib.zly_last_error()
    assert lib.zly_detect_device_fmt(e.h, 9, 1, None, 416, 416, None, 0, None) == zly.ERR_INVALID_ARGUMENT
    got = e.detect(good, fmt=zly.PIX_NV12_BT601, w=416, h=416)
    want = e.detect(yr.yuv420_to_bgr(good, 416, 416, zly.PIX_NV12_BT601))
    assert got[1] == want[1] and det_fields_equal(got[0], want[0])
    t2 = e.submit(good, fmt=zly.PIX_NV12_BT601, w=416, h=416)
    d2 = e.wait(t2)
    assert d2[1] == want[1] and det_fields_equal(d2[0], want[0])
    e.close()


def test_plugin_nv12_requests_equal_c_abi(tmp_path, weights_path):
    """the plugin with ZLY_INPUT_FORMAT=nv12 (tests/cpp/test_hip_engine_yuv.cpp): every NV12 request's callback carries exactly the detections
    zly_detect_fmt gives for that frame; a BGR-sized request fails alone (no callback, one inference error)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "zero-latency-yolo_amd", "_build", "test_hip_engine_yuv")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", root, "host"], check=True, stdout=subprocess.DEVNULL)
    fmt = zly.PIX_NV12_BT601
    sizes = [(416, 416), (640, 480), (100, 62), (416, 416), (418, 330), (416, 416)]
    frames = [_yuv(w, h, fmt, seed=700 + i) for i, (w, h) in enumerate(sizes)]
    bad = 3
    blobs = [f.tobytes() for f in frames]
    blobs[bad] = zm.synth_frames(1, 416, 416, seed=799)[0].tobytes()          # a BGR-sized request in an NV12 stream
    fpath, out = tmp_path / "frames.bin", tmp_path / "out.json"
    with open(fpath, "wb") as f:
        f.write(struct.pack("<I", len(blobs)))
        for (w, h), b in zip(sizes, blobs):
            f.write(struct.pack("<HHI", w, h, len(b)))
            f.write(b)
    env = dict(os.environ, ZLY_INPUT_FORMAT="nv12", ZLY_MAX_BATCH="8", ZLY_FP32="1")     # fp32: exact however the plugin batches
    r = subprocess.run([exe, weights_path, str(fpath), str(out)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr
    j = json.loads(out.read_text())
    good = [i for i in range(len(sizes)) if i != bad]
    assert [x["frame_id"] for x in j["results"]] == good
    assert j["status"]["inference_errors"] == "1"
    e = zly.Engine(weights_path, dtype=zly.DTYPE_FP32, max_batch=1, max_dets=256, warmup_runs=0)
    for x in j["results"]:
        i = x["frame_id"]
        w, h = sizes[i]
        dets, n = e.detect(frames[i], fmt=fmt, w=w, h=h, cap=256)
        got = np.array(x["dets"], dtype=np.int64).reshape(-1, 6)
        assert len(got) == len(dets), i
        for k, d in enumerate(dets):
            bits = [int(d[c].view(np.uint32)) for c in ("x", "y", "w", "h", "confidence")]
            assert list(got[k, :5]) == bits and got[k, 5] == int(d["class_id"]), (i, k)
    e.close()
