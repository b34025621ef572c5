"""GPU parity of every model shape the loader admits (run on the MI355X box: pytest -m gpu): YOLOv8m and YOLOv8l in bf16 against the
CPU oracles, YOLOv8n with 1 / 17 / 64 classes in both dtypes, and the shapes the engine refuses at zly_create.

What the widths exercise beyond YOLOv8n / -s (tests/test_gpu_parity.py):
  * m (48 / 96 / 192 / 384 / 576, C2f depths 2 and 4): 3x3 convs with cin % 32 == 16 (K = 432 is 13.5 bf16 k-steps), partial 64-channel
    output tiles (48 / 288 / 576 outputs), 1x1 convs over 960 and 1152 inputs, a 48-channel stem on the unfused preprocess + conv path,
    four bottlenecks per C2f;
  * l (64 / 128 / 256 / 512 / 512, depths 3 and 6): six bottlenecks per C2f, the fused 64-channel bottleneck pair chained three times,
    a Detect class branch of 256 channels = exactly HEAD_KMAX bf16 k-steps in the fused tail;
  * n with nc = 1 / 17 (masked rows of a partial class tile, one-class NMS on both of its paths) and 64 (class branch = box branch width).
Refused at load (ZLY_ERR_MODEL_LOAD from zly_create, before any launch): a Detect branch wider than HEAD_KMAX k-steps (m / l in fp32,
x in either dtype) and a class branch whose width max(ch[2], nc) is not a multiple of 16 (65 <= nc <= 79 on n).
Tolerances are test_gpu_parity.py's; the m / l synthetic weights are calibrated like n's (tools/zly_model.py)."""
import numpy as np
import pytest
import torch

import yolov8_ref
import zly
import zly_model as zm
from closed_loop_ref import check_closed_loop, check_head_decode, lds_resident_from_kernels
from oracle_lib import det_fields_equal
from parity_sets import compare_detection_sets
from test_gpu_parity import (BF16_FLIP_BAND, FP32_BOX_TOL, FP32_SCORE_TOL, MIN_COMPARED_FRACTION, _assert_bf16_close,
                             _assert_layer_close, _check_taps, _pre)

pytestmark = pytest.mark.gpu


def _write(tmp_path_factory, scale, nc=80):
    spec = zm.build_spec(scale, nc)
    p = str(tmp_path_factory.mktemp(f"yolov8{scale}_nc{nc}") / "synth.zlyw")
    zm.write_zlyw(p, spec, zm.synth_weights(spec))
    return spec, p


@pytest.fixture(scope="module")
def model_m(tmp_path_factory):
    return _write(tmp_path_factory, "m")


@pytest.fixture(scope="module")
def model_l(tmp_path_factory):
    return _write(tmp_path_factory, "l")


def _kernels(e, n):
    """op name -> kernel it launches at batch n (fused ops are listed under the first conv's name)"""
    return {o["name"].split("+")[0]: k for o, k in zip(e.ops(), e.op_kernels(n))}


def _family_parity(oracle, spec, path, w, h, n, lds_resident):
    """the checks every variant gets: every conv tap of the production engine and of a one-kernel-per-conv engine against the bf16-rounding
    oracle, the head against both oracles, the detections against the fp32 oracle's as sets, detect() == the oracle's post-processing of
    the engine's own head.  Returns the production engine's kernel table at batch n."""
    names = [c.name for c in spec.convs]
    frames = zm.synth_frames(n, w, h, seed=61, rects=False)
    x = _pre(oracle, frames, w, h)
    ref16, ref32 = yolov8_ref.load(path, "bf16"), yolov8_ref.load(path, "fp32")
    want16 = ref16.forward(torch.from_numpy(x)).numpy()
    want32 = ref32.forward(torch.from_numpy(x)).numpy()
    assert want32.shape == (n, 4 + spec.nc, spec.num_anchors(w, h))
    e = zly.Engine(path, model_w=w, model_h=h, max_batch=n, max_dets=512, warmup_runs=0, flags=zly.FLAG_DUMP_LOGITS)
    kern = _kernels(e, n)
    got = e.forward(x)
    _assert_bf16_close(got, want16)
    _assert_bf16_close(got, want32)
    checked = _check_taps(e, ref16, range(n), skip_ok=tuple(lds_resident), names=names)
    assert len(checked) == len(names) - len(lds_resident), sorted(set(names) - set(checked))
    # every conv against float64 on the engine's own tapped inputs, per element, first and last frame (tests/closed_loop_ref.py); what is
    # checked through the ambiguity allowance is what the caller says stays in LDS, and that is what the kernel table says
    assert lds_resident_from_kernels(e, n) == set(lds_resident)
    assert len(check_closed_loop(e, path, (0, n - 1), lds_resident=lds_resident)) == len(names)
    for i in (0, n - 1):
        check_head_decode(e, got[i], i)
    compared = skipped = 0
    for i, f in enumerate(frames):
        dets, k = e.detect(f, cap=512)
        gh = e.head_tensor(0)
        own = oracle.postprocess(gh, w, h)
        assert k == len(own) and det_fields_equal(dets, own[:512]), i
        assert k == 0 or (dets["class_id"][:min(k, 512)] < spec.nc).all()
        _assert_bf16_close(gh[None], want32[i][None])                      # the detect path's front (unfused stem for these widths)
        c, sk, errors = compare_detection_sets(oracle, want32[i], dets, w, h, band=BF16_FLIP_BAND, got_head=gh)
        assert not errors, (i, errors)
        compared += c; skipped += sk
    assert compared >= n and compared >= MIN_COMPARED_FRACTION * (compared + skipped), (compared, skipped)
    e.close()
    # every conv on its own kernel: nothing stays in LDS, every tap is checked
    e = zly.Engine(path, model_w=w, model_h=h, max_batch=n, warmup_runs=0, flags=zly.FLAG_NO_FUSION | zly.FLAG_DUMP_LOGITS)
    got = e.forward(x)
    assert len(_check_taps(e, ref16, range(n), names=names)) == len(names)
    assert len(check_closed_loop(e, path, (0, n - 1))) == len(names)
    for i in (0, n - 1):
        check_head_decode(e, got[i], i)
    _assert_bf16_close(got, want16)
    _assert_bf16_close(got, want32)
    e.close()
    return kern


@pytest.mark.parametrize("w,h", [(320, 320), (352, 288)])
def test_yolov8m_bf16(model_m, oracle, w, h):
    spec, path = model_m
    kern = _family_parity(oracle, spec, path, w, h, 3, lds_resident=())
    # the shapes this variant is about run on the kernels they were checked on here: selection must not change silently
    family = {k: v.split(",")[0] for k, v in kern.items()}
    assert family["preprocess"] == "preprocess_kernel"                                      # 48-channel stem: no fused front kernel
    for name in ("model.0", "model.1") + tuple(f"model.2.m.{i}.cv{j}" for i in range(2) for j in (1, 2)):
        assert family[name] == "conv_igemm_kernel<3x3 generic-K", (name, kern[name])      # cin 8 / 48: K = 72 / 432, a k-step remainder
    for name in [f"model.{b}.m.{i}.cv{j}" for b, nb in ((4, 4), (15, 2), (8, 2), (21, 2)) for i in range(nb) for j in (1, 2)]:
        assert family[name] == "conv_igemm_kernel<3x3", (name, kern[name])                # cin 96 / 288, 96- and 288-channel outputs
    assert family["model.2.cv2"] == "conv1x1_ws_kernel<NK=6"                               # 4 x 48 inputs
    assert family["model.8.cv1"] == family["model.21.cv2"] == family["model.9.cv2"] == "conv_igemm_kernel<1x1"   # 576 outputs, 1152 inputs
    assert family["model.12.cv1"] == "conv_igemm_kernel<1x1 dual-source"                    # 960 inputs, Upsample + Concat fused
    assert kern["detect.tail.P5 (all levels below batch 16)"] == "head_fused_kernel"


def test_yolov8l_bf16(model_l, oracle, monkeypatch):
    spec, path = model_l
    monkeypatch.setenv("ZLY_PAIR_WIDTHS", "64")                   # the fused 64-channel pair is opt-in ...
    monkeypatch.setenv("ZLY_PAIR_MIN_TILES", "1")                 # ... and by default needs more tiles than batch 2 has
    kern = _family_parity(oracle, spec, path, 256, 256, 2, lds_resident=("model.2.m.0.cv1", "model.2.m.1.cv1", "model.2.m.2.cv1"))
    for i in range(3):
        assert kern[f"model.2.m.{i}.cv1"] == "bottleneck_pair_kernel<64>", (i, kern[f"model.2.m.{i}.cv1"])
    assert kern["detect.tail.P5 (all levels below batch 16)"] == "head_fused_kernel"


@pytest.mark.parametrize("scale,dtype,nc", [("m", "fp32", 80), ("l", "fp32", 80), ("x", "bf16", 80), ("x", "fp32", 80),
                                            ("n", "bf16", 72), ("n", "fp32", 72), ("n", "bf16", 79), ("n", "fp32", 65)])
def test_refused_at_load(tmp_path, scale, dtype, nc):
    """zly_create either returns an engine that meets the stated tolerances or refuses the model: a Detect branch beyond the fused tail's
    HEAD_KMAX k-steps (bf16: 256 channels, fp32: 128) and class-branch widths that are not a multiple of 16"""
    spec = zm.build_spec(scale, nc)
    p = str(tmp_path / "refused.zlyw")
    zm.write_zlyw(p, spec, {c.name: (np.zeros((c.cout, c.cin, c.k, c.k), np.float32), np.zeros(c.cout, np.float32)) for c in spec.convs})
    with pytest.raises(zly.ZlyError) as ei:
        zly.Engine(p, model_w=256, model_h=256, dtype=zly.DTYPE_BF16 if dtype == "bf16" else zly.DTYPE_FP32, max_batch=1, warmup_runs=0)
    assert ei.value.code == zly.ERR_MODEL_LOAD
    assert ("k-steps" if scale != "n" else "multiple of 16") in ei.value.message, ei.value.message


# class count -> conf_thr that leaves a usable number of candidates on these frames (nc = 1: <= 128 candidates, the NMS path of few)
NC_CONF = {1: 0.15, 17: 0.3, 64: 0.5}


@pytest.mark.parametrize("nc", [1, 17, 64])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_yolov8n_class_counts(tmp_path, oracle, nc, dtype):
    spec = zm.build_spec("n", nc)
    p = str(tmp_path / f"yolov8n_nc{nc}.zlyw")
    zm.write_zlyw(p, spec, zm.synth_weights(spec))
    frames = zm.synth_frames(3, 416, 416, seed=13, rects=False)
    x = _pre(oracle, frames)
    ref32 = yolov8_ref.load(p, "fp32")
    want32 = ref32.forward(torch.from_numpy(x)).numpy()
    bf16 = dtype == "bf16"
    thr = NC_CONF[nc]
    e = zly.Engine(p, dtype=zly.DTYPE_BF16 if bf16 else zly.DTYPE_FP32, max_batch=3, max_dets=1024, conf_thr=thr, warmup_runs=0,
                   flags=zly.FLAG_DUMP_LOGITS)
    assert e.nc == nc
    got = e.forward(x)
    assert got.shape == want32.shape == (3, 4 + nc, 3549)
    class_taps = [f"model.22.cv3.{l}.{j}" for l in range(3) for j in range(3)]
    if bf16:
        ref16 = yolov8_ref.load(p, "bf16")
        want16 = ref16.forward(torch.from_numpy(x)).numpy()
        _assert_bf16_close(got, want16)
        _assert_bf16_close(got, want32)
        for name in class_taps:
            for i in range(3):
                _assert_layer_close(e.tap(name, i), ref16.taps[name][i].numpy(), f"{name}[{i}]")
    else:
        scale = max(1.0, float(np.abs(want32[:, :4]).max()) / 800.0)
        assert np.abs(got[:, :4] - want32[:, :4]).max() <= 4 * FP32_BOX_TOL * scale
        assert np.abs(got[:, 4:] - want32[:, 4:]).max() <= 2 * FP32_SCORE_TOL
        for name in class_taps:
            for i in range(3):
                g, t = e.tap(name, i), ref32.taps[name][i].numpy()
                assert g.shape == t.shape and np.abs(g - t).max() <= 2e-4 * max(1.0, np.abs(t).max()), (name, i)
    # every conv (the masked rows of a partial class tile among them) against float64 on the engine's own inputs, per element
    assert len(check_closed_loop(e, p, (0, 2), lds_resident=lds_resident_from_kernels(e, 3) if bf16 else ())) == len(spec.convs)
    for i in (0, 2):
        check_head_decode(e, got[i], i)
    total = 0
    for f in frames:
        dets, k = e.detect(f, cap=1024)
        head = e.head_tensor(0)
        assert head.shape == (4 + nc, 3549)
        own = oracle.postprocess(head, 416, 416, thr, 0.45)
        assert k == len(own) and det_fields_equal(dets, own[:1024])
        assert (dets["class_id"][:min(k, 1024)] < nc).all()
        if nc == 1:
            assert 0 <= int((head[4] >= thr).sum()) <= 128
        total += k
    assert total > 0
    e.close()
    if nc == 1:
        # one class, > 1024 candidates per frame: NMS's path for crowded classes on real head tensors
        e = zly.Engine(p, dtype=zly.DTYPE_BF16 if bf16 else zly.DTYPE_FP32, max_batch=1, max_dets=1024, conf_thr=0.05, warmup_runs=0)
        for f in frames:
            dets, k = e.detect(f, cap=1024)
            head = e.head_tensor(0)
            assert int((head[4] >= 0.05).sum()) > 1024
            own = oracle.postprocess(head, 416, 416, 0.05, 0.45)
            assert k == len(own) > 0 and det_fields_equal(dets, own[:1024])
            assert (dets["class_id"][:min(k, 1024)] == 0).all()
        e.close()
