"""Every conv kernel against float64 on the ENGINE'S OWN inputs (run on the MI355X box: pytest -m gpu).  tests/closed_loop_ref.py feeds each
conv's tapped inputs -- exact bf16 / fp32 values -- through a float64 convolution, so the only legitimate difference to the tapped output is
one final rounding plus fp32 accumulation noise: |g - y| <= 2^-8 |y| + C_ACC 2^-24 B per element (2^-24 |y| for fp32 stores).  That tells a
truncating epilogue, a shortcut added after a rounding or a bias lost on a padded channel tile from a correct kernel, which the layer checks
of test_gpu_parity.py (2^-5 of the range, against the oracle's own chain) cannot.  The head tensor is checked against the float64 decode of
the engine's own six logits taps.

Shapes: the smallest that still put every kernel at its edges -- 64 x 64 (maps 32 .. 2 x 2), 96 x 64 (P5 is a 3 x 2 map, smaller than any tile
and than the pool window), 352 x 288 and 224 x 416 (the ragged maps the suite already uses), 416 x 416 where the production selection needs it."""
import numpy as np
import pytest
import torch

import zly
import zly_model as zm
from closed_loop_ref import check_closed_loop, check_head_decode, lds_resident_from_kernels

pytestmark = pytest.mark.gpu

MIN_SWITCHES = dict(ZLY_LDS_MIN_TILES="1", ZLY_STREAM_MIN_GROUPS="1", ZLY_PAIR_MIN_TILES="1", ZLY_WS_MIN_TILES="1")


@pytest.fixture(scope="module")
def model_paths(weights_path, tmp_path_factory):
    spec = zm.build_spec("s")
    p = str(tmp_path_factory.mktemp("closed_loop") / "yolov8s_synth.zlyw")
    zm.write_zlyw(p, spec, zm.synth_weights(spec, seed=9))
    return {"n": weights_path, "s": p}


def _pre(oracle, frames, w, h):
    return np.stack([oracle.preprocess(f, w, h)[1] for f in frames])


def _as_held(x):
    """what the bf16 front kernels hold for a preprocessed frame: bf16(u8 / 255)"""
    return torch.from_numpy(x).to(torch.bfloat16).to(torch.float32).numpy()


def _n_convs(scale):
    return len(zm.build_spec(scale).convs)


@pytest.mark.parametrize("scale,w,h,n", [("n", 64, 64, 3), ("n", 96, 64, 2), ("n", 352, 288, 5), ("n", 224, 416, 4),
                                         ("s", 64, 64, 3), ("s", 96, 64, 2), ("s", 352, 288, 5)])
def test_one_kernel_per_conv(model_paths, oracle, scale, w, h, n):
    """bf16, every conv as its own launch: nothing stays in LDS, every conv of every frame is checked directly; model.0 from the "images" tap"""
    path = model_paths[scale]
    x = _pre(oracle, zm.synth_frames(n, w, h, seed=31, rects=False), w, h)
    e = zly.Engine(path, model_w=w, model_h=h, max_batch=n, warmup_runs=0, flags=zly.FLAG_NO_FUSION | zly.FLAG_DUMP_LOGITS)
    head = e.forward(x)
    assert np.array_equal(e.tap("images", n - 1), _as_held(x[n - 1]))
    assert len(check_closed_loop(e, path, range(n))) == _n_convs(scale)
    for i in range(n):
        check_head_decode(e, head[i], i)
    e.close()


@pytest.mark.parametrize("scale,w,h,n", [("n", 64, 64, 3), ("n", 352, 288, 3), ("s", 64, 64, 3), ("s", 352, 288, 2)])
def test_fp32_engine(model_paths, oracle, scale, w, h, n):
    """the fp32 engine, all taps, with the fp32 form of the bound (2^-24 |y| + C_ACC 2^-24 B)"""
    path = model_paths[scale]
    x = _pre(oracle, zm.synth_frames(n, w, h, seed=32, rects=False), w, h)
    e = zly.Engine(path, model_w=w, model_h=h, dtype=zly.DTYPE_FP32, max_batch=n, warmup_runs=0, flags=zly.FLAG_DUMP_LOGITS)
    head = e.forward(x)
    assert np.array_equal(e.tap("images", 0), x[0])
    assert len(check_closed_loop(e, path, range(n))) == _n_convs(scale)
    for i in range(n):
        check_head_decode(e, head[i], i)
    e.close()


@pytest.mark.parametrize("w,h,n", [(352, 288, 5), (416, 416, 3)])
def test_production_selection(weights_path, oracle, monkeypatch, w, h, n):
    """default flags + the dumps, the throughput kernels forced onto these small batches: after forward(), and again after detect_batch() on
    the same engine -- there the front kernel computes model.1 from its own model.0 map, which it dumps.  What may go through the ambiguity
    allowance is exactly what the kernel table says stays in LDS."""
    for k, v in MIN_SWITCHES.items():
        monkeypatch.setenv(k, v)
    frames = zm.synth_frames(n, w, h, seed=31, rects=False)
    x = _pre(oracle, frames, w, h)
    e = zly.Engine(weights_path, model_w=w, model_h=h, max_batch=n, warmup_runs=0, flags=zly.FLAG_DUMP_LOGITS)
    kn = " | ".join(e.op_kernels(n))
    assert "stem_model1_kernel" in kn and "c2f_kernel<C=16" in kn and "c2f_kernel<C=32" in kn and "conv3x3_ws_pair_kernel" in kn, kn
    assert ("conv3x3_wsk_kernel" in kn) == (n > 4), kn           # batch <= 4: the Detect convs run as merged launches instead
    lds = lds_resident_from_kernels(e, n)
    assert lds == {"model.2.m.0.cv1", "model.4.m.0.cv1", "model.4.m.1.cv1", "model.15.m.0.cv1"}, (lds, kn)
    head = e.forward(x)
    assert len(check_closed_loop(e, weights_path, range(n), lds_resident=lds)) == 63
    for i in range(n):
        check_head_decode(e, head[i], i)
    res = e.detect_batch(list(frames), cap=64)
    assert len(res) == n
    assert len(check_closed_loop(e, weights_path, range(n), lds_resident=lds, first_input=_as_held(x))) == 63
    for i in range(n):
        check_head_decode(e, e.head_tensor(i), i)
    e.close()


@pytest.mark.parametrize("w,h,n", [(352, 288, 5), (416, 416, 3)])
def test_production_selection_with_fused_sppf(weights_path, oracle, monkeypatch, w, h, n):
    """test_production_selection with ZLY_SPPF_FUSED=1: model.9 runs as one sppf_fused_kernel launch (11 x 9 and 13 x 13 maps), whose dump
    writes y and the pooled maps to the concat buffer -- so model.9.cv1 and model.9.cv2 go through the same per-element bound as every
    other conv, after forward() and after detect_batch() (tests/test_gpu_sppf.py drives the kernel alone)."""
    for k, v in MIN_SWITCHES.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("ZLY_SPPF_FUSED", "1")
    frames = zm.synth_frames(n, w, h, seed=31, rects=False)
    x = _pre(oracle, frames, w, h)
    e = zly.Engine(weights_path, model_w=w, model_h=h, max_batch=n, warmup_runs=0, flags=zly.FLAG_DUMP_LOGITS)
    kn = " | ".join(e.op_kernels(n))
    assert "sppf_fused_kernel" in kn and "sppf_pool" not in kn, kn
    lds = lds_resident_from_kernels(e, n)
    head = e.forward(x)
    assert len(check_closed_loop(e, weights_path, range(n), lds_resident=lds)) == 63
    for i in range(n):
        check_head_decode(e, head[i], i)
    assert len(e.detect_batch(list(frames), cap=64)) == n
    assert len(check_closed_loop(e, weights_path, range(n), lds_resident=lds, first_input=_as_held(x))) == 63
    e.close()


@pytest.mark.parametrize("w,h,n", [(416, 416, 1), (96, 64, 1), (352, 288, 4), (416, 416, 4)])
def test_latency_path(weights_path, oracle, w, h, n):
    """batch 1 and batch 4 as they run by default: the Detect convs as two merged launches (conv_igemm_multi_kernel), split-K direct kernels"""
    frames = zm.synth_frames(n, w, h, seed=91, rects=False)
    x = _pre(oracle, frames, w, h)
    e = zly.Engine(weights_path, model_w=w, model_h=h, max_batch=n, warmup_runs=0, flags=zly.FLAG_DUMP_LOGITS)
    assert sum("conv_igemm_multi_kernel" in k for k in e.op_kernels(n)) == 2, e.op_kernels(n)
    lds = lds_resident_from_kernels(e, n)
    head = e.forward(x)
    assert len(check_closed_loop(e, weights_path, range(n), lds_resident=lds)) == 63
    for i in range(n):
        check_head_decode(e, head[i], i)
    e.detect_batch(list(frames), cap=64)
    assert len(check_closed_loop(e, weights_path, range(n), lds_resident=lds, first_input=_as_held(x))) == 63
    e.close()


def test_throughput_path(weights_path, oracle):
    """16 frames at 416 x 416 through zly_detect_device with the flags bench.py uses + the dumps (Detect branches on side streams, per-level
    tails, deferred NMS): the kernels the headline number runs.  The reference is computed for the first and the last frame."""
    n = 16
    frames = zm.synth_frames(n, 416, 416, seed=77, rects=False)
    e = zly.Engine(weights_path, max_batch=n, max_dets=128, warmup_runs=1, flags=zly.FLAG_ASYNC_NMS | zly.FLAG_DUMP_LOGITS)
    lds = lds_resident_from_kernels(e, n)
    assert {"model.2.m.0.cv1", "model.4.m.0.cv1", "model.4.m.1.cv1", "model.15.m.0.cv1"} <= lds, lds
    d = torch.from_numpy(frames).cuda()
    e.detect_device(d.data_ptr(), n, 416, 416)
    e.read_slabs(n)                                               # joins the deferred NMS
    ends = (0, n - 1)
    assert len(check_closed_loop(e, weights_path, ends, lds_resident=lds, first_input=_as_held(_pre(oracle, frames[list(ends)], 416, 416)))) == 63
    for i in ends:
        check_head_decode(e, e.head_tensor(i), i)
    e.close()
