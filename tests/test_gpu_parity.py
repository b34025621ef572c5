"""GPU parity tests (run on the MI355X box: pytest -m gpu).  Every call goes through the C ABI of
libzly.so; the CPU oracle (oracle/) is only the checker.

Tolerances (stated here, used below):
  * preprocess, decode, NMS: BIT-EXACT against oracle/zly_oracle.c (integer / single-rounded fp32 work).
  * fp32 engine head tensor vs fp32 oracle: box rows <= FP32_BOX_TOL px, score rows <= FP32_SCORE_TOL
    (summation-order differences of an exact-fp32 MFMA chain vs MLAS/oneDNN only).
  * bf16 engine head tensor, against the fp32 oracle AND the bf16-rounding oracle: box rows <= 1.5 px, score rows <= 2e-2
    (max over every anchor of every frame), plus rms bounds a few times the measured noise floor of bf16 itself;
    every conv output of the PRODUCTION kernels within 2^-5 of the tensor's range of the bf16-rounding oracle;
    every conv output PER ELEMENT within 2^-8 |y| + C_ACC 2^-24 B of a float64 conv of the engine's own tapped inputs, and the head tensor within
    2^-9 px / 2^-19 of the float64 decode of the engine's own logits (tests/closed_loop_ref.py: bound, derivation, measured constants);
    detection SETS equal to the fp32 oracle's outside the threshold-flip band (tests/parity_sets.py).
  The synthetic weights are calibrated so that these bounds mean something (tools/zly_model.py: noise-stable
  activations, peaked Gaussian DFL): the noise floor of bf16 itself on this model -- bf16-rounding oracle vs fp32
  oracle, both on the CPU -- is box rms 0.05 px / max 0.5 px, score rms 6e-4 / max 9e-3.  The forward pass is PARITY
  UNPINNED against the reference (ONNX Runtime + an ultralytics export are not available offline, oracle/yolov8_ref.py).
"""
import numpy as np
import pytest
import torch

import zly
import zly_model as zm
from closed_loop_ref import check_closed_loop, check_head_decode, lds_resident_from_kernels
from oracle_lib import det_fields_equal
from parity_sets import compare_detection_sets

pytestmark = pytest.mark.gpu

FP32_BOX_TOL = 1e-3      # px
FP32_SCORE_TOL = 1e-4
BF16_BOX_MAX, BF16_SCORE_MAX = 1.5, 2e-2      # px @416 / absolute
BF16_BOX_RMS, BF16_SCORE_RMS = 0.2, 2e-3      # ~4x the noise floor of bf16 itself on this model
BF16_FLIP_BAND = BF16_SCORE_MAX                # confidence tolerance of matched detections (and the flip band where the engine's head is not available)
# Set-level comparison: at least this share of the oracle's detections must be compared EXACTLY (the rest sit in components where a
# threshold decision really differs between the engine's own head tensor and the oracle's; tests/parity_sets.py).  The synthetic head's
# scores are Gaussian-tailed through 0.5 (DESIGN.md section 2 on why a random net cannot be made bimodal), so a band of the full
# tolerance around the thresholds would skip most detections; the actual flips are few.
MIN_COMPARED_FRACTION = 0.7
LAYER_MAX, LAYER_RMS = 2.0 ** -5, 0.03         # conv outputs vs the bf16-rounding oracle: max |d| / max |t|, rms(d) / std(t)
F6 = ["x", "y", "w", "h", "confidence", "class_id"]


@pytest.fixture(scope="module")
def eng32(weights_path):
    e = zly.Engine(weights_path, dtype=zly.DTYPE_FP32, max_batch=4, max_dets=512, warmup_runs=1, flags=zly.FLAG_DUMP_LOGITS)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng16(weights_path):
    e = zly.Engine(weights_path, dtype=zly.DTYPE_BF16, max_batch=8, max_dets=512, warmup_runs=1)
    yield e
    e.close()


def _pre(oracle, frames, tw=416, th=416):
    return np.stack([oracle.preprocess(f, tw, th)[1] for f in frames])


# ---------------------------------------------------------------------------------------------------
# preprocess: bit-exact
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(416, 416), (800, 600), (64, 48), (1920, 1080), (417, 415), (1, 1)])
def test_preprocess_bit_exact(eng16, oracle, w, h):
    rng = np.random.default_rng(w * 10007 + h)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    rc, want = oracle.preprocess(img, 416, 416)
    assert rc == 0
    got = eng16.preprocess(img)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_preprocess_constant_128(eng32):
    got = eng32.preprocess(np.full((416, 416, 3), 128, dtype=np.uint8))
    assert np.all(got == np.float32(128) / np.float32(255.0))


def test_preprocess_wrong_byte_count_is_error_203(eng16):
    img = np.zeros((10, 10, 3), dtype=np.uint8)
    with pytest.raises(zly.ZlyError) as ei:
        eng16.preprocess(img, nbytes=299)
    assert ei.value.code == zly.ERR_INVALID_INPUT and "expected 300" in ei.value.message
    with pytest.raises(zly.ZlyError) as ei:
        eng16.detect(img, nbytes=301)
    assert ei.value.code == zly.ERR_INVALID_INPUT


# ---------------------------------------------------------------------------------------------------
# decode + NMS: bit-exact on caller-supplied head tensors
# ---------------------------------------------------------------------------------------------------
def _rand_head(rng, nc, n, hot=0.02, size=416):
    head = np.zeros((4 + nc, n), dtype=np.float32)
    head[0] = rng.uniform(0, size, n); head[1] = rng.uniform(0, size, n)
    head[2] = rng.uniform(8, size / 2, n); head[3] = rng.uniform(8, size / 2, n)
    head[4:] = rng.uniform(0, 0.45, (nc, n))
    idx = rng.choice(n, max(1, int(hot * n)), replace=False)
    head[4 + rng.integers(0, nc, len(idx)), idx] = rng.uniform(0.5, 1.0, len(idx))
    return head


@pytest.mark.parametrize("nc,n,hot,seed", [(80, 3549, 0.02, 0), (80, 3549, 0.2, 1), (4, 8400, 0.05, 2), (1, 1000, 0.3, 3),
                                           (80, 3549, 0.6, 4), (3, 777, 0.1, 5), (80, 64, 0.5, 6),
                                           # the one-wave NMS path (<= 128 candidates, two per lane) at its edges: 64 / 65 / 128 candidates, one class
                                           # (every box can suppress every later one) and many; 129 falls to the eight-wave path
                                           (1, 64, 1.0, 7), (5, 65, 1.0, 8), (1, 128, 1.0, 9), (80, 128, 1.0, 10), (2, 129, 1.0, 11), (3, 1, 1.0, 12)])
def test_postprocess_bit_exact(eng16, oracle, nc, n, hot, seed):
    head = _rand_head(np.random.default_rng(seed), nc, n, hot)
    want = oracle.postprocess(head, 800, 600)
    got, n_kept, n_cand = eng16.postprocess(head, 800, 600)
    assert n_cand == len(oracle.decode(head, 800, 600))
    assert n_kept == len(want)
    assert det_fields_equal(got, want)


def test_postprocess_many_candidates_in_one_class(eng16, oracle):
    """> 1024 candidates of ONE class: exercises the global-memory NMS path and long greedy chains."""
    rng = np.random.default_rng(9)
    head = _rand_head(rng, 2, 3000, 0.0)
    head[4] = rng.uniform(0.5, 1.0, 3000)
    head[5] = 0
    want = oracle.postprocess(head, 416, 416)
    got, n_kept, n_cand = eng16.postprocess(head, 416, 416)
    assert n_cand == 3000 and n_kept == len(want) and det_fields_equal(got, want)


@pytest.mark.parametrize("n_one,n_other,box", [(129, 0, 40.0), (192, 30, 12.0), (500, 100, 12.0), (600, 60, 60.0), (1000, 24, 20.0), (1020, 4, 6.0),
                                               (1100, 50, 12.0), (1500, 200, 30.0)])
def test_postprocess_crowded_class_blocks(eng16, oracle, n_one, n_other, box):
    """One class holding hundreds of candidates (a crowd): the path that resolves such a class by the whole workgroup in blocks of 64 sorted
    candidates -- in LDS up to 1024 candidates per frame, in global memory beyond -- with small boxes (most are kept: long chains of kept
    boxes across blocks) and large ones (most are suppressed, many by boxes of earlier blocks), next to a few sparse classes."""
    rng = np.random.default_rng(1000 + n_one)
    n = n_one + n_other
    head = np.zeros((4 + 6, n), dtype=np.float32)
    head[0] = rng.uniform(0, 416, n); head[1] = rng.uniform(0, 416, n)
    head[2] = rng.uniform(box / 2, box, n); head[3] = rng.uniform(box / 2, box, n)
    head[4, :n_one] = rng.uniform(0.5, 1.0, n_one)
    head[4, :8] = 0.75                                        # exact confidence ties inside the crowded class (anchor order decides)
    if n_other:
        head[5 + rng.integers(0, 5, n_other), np.arange(n_one, n)] = rng.uniform(0.5, 1.0, n_other)
    perm = rng.permutation(n)
    head = np.ascontiguousarray(head[:, perm])
    want = oracle.postprocess(head, 416, 416)
    got, n_kept, n_cand = eng16.postprocess(head, 416, 416)
    assert n_cand == n and n_kept == len(want) and det_fields_equal(got, want)


@pytest.mark.parametrize("n_one,n_other,box", [(700, 80, 14.0), (1500, 300, 10.0), (2040, 8, 8.0), (2300, 100, 12.0)])
def test_postprocess_crowded_class_8400_anchors(eng16, oracle, n_one, n_other, box):
    """The same on a head tensor of 8400 anchors (640 x 640 models): those get the NMS build that holds 2048 candidates per frame in LDS
    (bitonic sort over 2048 keys, up to 32 blocks per class); 2300 candidates exceed it and take the global-memory path."""
    rng = np.random.default_rng(2000 + n_one)
    N = 8400
    head = np.zeros((4 + 6, N), dtype=np.float32)
    head[0] = rng.uniform(0, 640, N); head[1] = rng.uniform(0, 640, N)
    head[2] = rng.uniform(box / 2, box, N); head[3] = rng.uniform(box / 2, box, N)
    hot = rng.choice(N, n_one + n_other, replace=False)
    head[4, hot[:n_one]] = rng.uniform(0.5, 1.0, n_one)
    head[4, hot[:6]] = 0.625                                  # exact ties
    head[5 + rng.integers(0, 5, n_other), hot[n_one:]] = rng.uniform(0.5, 1.0, n_other)
    want = oracle.postprocess(head, 640, 640)
    got, n_kept, n_cand = eng16.postprocess(head, 640, 640)
    assert n_cand == n_one + n_other and n_kept == len(want) and det_fields_equal(got, want)


def test_postprocess_ties_threshold_and_empty(eng16, oracle):
    head = np.zeros((4 + 4, 8), dtype=np.float32)
    head[0] = [50, 60, 300, 300, 300, 100, 100, 100]; head[1] = 100
    head[2] = 80; head[3] = 80
    half_minus = np.nextafter(np.float32(0.5), np.float32(0))
    head[4] = [0.5, half_minus, 0.8, 0.8, 0.8, 0, 0, 0]      # inclusive threshold; exact ties
    head[5] = [0.0, 0.0, 0.8, 0.0, 0.0, 0, 0, 0]             # first of equal maxima wins
    want = oracle.postprocess(head, 416, 416)
    got, n_kept, _ = eng16.postprocess(head, 416, 416)
    assert n_kept == len(want) and det_fields_equal(got, want)
    empty = np.zeros((4 + 4, 100), dtype=np.float32)
    got, n_kept, n_cand = eng16.postprocess(empty, 416, 416, conf_thr=0.0)
    assert n_kept == 0 and n_cand == 0                        # all-zero scores never pass (class stays -1)


def test_postprocess_cap_overflow_reports_uncapped_count(eng16, oracle):
    head = _rand_head(np.random.default_rng(12), 80, 3549, 0.2)
    want = oracle.postprocess(head, 416, 416)
    got, n_kept, _ = eng16.postprocess(head, 416, 416, cap=16)
    assert n_kept == len(want) > 16 and len(got) == 16 and det_fields_equal(got, want[:16])


# ---------------------------------------------------------------------------------------------------
# forward pass
# ---------------------------------------------------------------------------------------------------
def test_forward_fp32_layers_and_head(eng32, oracle, ref_fp32):
    frames = zm.synth_frames(2, 416, 416, seed=5, rects=False)
    x = _pre(oracle, frames)
    want = ref_fp32.forward(torch.from_numpy(x)).numpy()
    got = eng32.forward(x)
    for name in ("model.0", "model.2.cv2", "model.4.cv2", "model.9.cv2", "model.12.cv2", "model.15.cv2", "model.21.cv2",
                 "model.22.cv2.0.2", "model.22.cv3.2.2"):
        t = ref_fp32.taps[name][1].numpy()
        g = eng32.tap(name, 1)
        assert g.shape == t.shape, name
        assert np.abs(g - t).max() <= 2e-4 * max(1.0, np.abs(t).max()), name
    assert np.abs(got[:, :4] - want[:, :4]).max() <= FP32_BOX_TOL
    assert np.abs(got[:, 4:] - want[:, 4:]).max() <= FP32_SCORE_TOL


def _rms(d):
    return float(np.sqrt(np.mean(np.square(d, dtype=np.float64))))


def _assert_bf16_close(got, want):
    db, ds = got[:, :4] - want[:, :4], got[:, 4:] - want[:, 4:]
    assert _rms(db) <= BF16_BOX_RMS and np.abs(db).max() <= BF16_BOX_MAX, (_rms(db), np.abs(db).max())
    assert _rms(ds) <= BF16_SCORE_RMS and np.abs(ds).max() <= BF16_SCORE_MAX, (_rms(ds), np.abs(ds).max())


def _assert_layer_close(g, t, name):
    """a conv output of the engine against the bf16-rounding oracle's: an indexing / tile-edge bug moves a few elements
    by O(std) = 10-20 % of the range, bf16 rounding flips move them by < 1.6 % (measured floor, CPU)"""
    assert g.shape == t.shape, (name, g.shape, t.shape)
    d = g - t
    assert np.isfinite(g).all(), name
    assert np.abs(d).max() <= LAYER_MAX * np.abs(t).max(), (name, float(np.abs(d).max() / np.abs(t).max()))
    assert _rms(d) <= LAYER_RMS * float(t.std()), (name, _rms(d) / float(t.std()))


def _all_conv_names():
    return [c.name for c in zm.build_spec("n").convs]


def _check_taps(eng, ref, frame_ids, skip_ok=(), names=None):
    """every conv output the engine can expose, for the given frames, against the oracle's taps; returns the names checked
    (names: the model's conv names, default YOLOv8n's)"""
    checked = []
    for name in names if names is not None else _all_conv_names():
        for i in frame_ids:
            try:
                g = eng.tap(name, i)
            except zly.ZlyError as exc:
                assert any(name.endswith(sfx) for sfx in skip_ok), (name, exc.message)
                break
            _assert_layer_close(g, ref.taps[name][i].numpy(), f"{name}[{i}]")
        else:
            checked.append(name)
    return checked


def test_forward_bf16_vs_emulating_oracle(eng16, weights_path, oracle, ref_bf16):
    """bf16 engine vs the oracle that rounds at the same points (weights and every stored activation to bf16, fp32
    accumulate, the six final Detect convs in fp32).  The stem output (identical inputs) must agree to 1 bf16 ulp (2^-7
    relative); EVERY one of the 63 conv outputs to 2^-5 of its range (pins the MFMA indexing of each kernel mode: 3x3
    generic-K, 3x3 fast-K, 3x3 split-K, 1x1, dual-source 1x1, residual, SPPF concat, the fused Detect tail's logits)."""
    frames = zm.synth_frames(2, 416, 416, seed=6, rects=False)
    x = _pre(oracle, frames)
    want = ref_bf16.forward(torch.from_numpy(x)).numpy()
    got = eng16.forward(x)
    _assert_bf16_close(got, want)
    # per-layer taps from an engine that runs every conv as its own kernel (the fused bottleneck keeps m.0.cv1 in LDS)
    e = zly.Engine(weights_path, max_batch=2, warmup_runs=0, flags=zly.FLAG_NO_FUSION | zly.FLAG_DUMP_LOGITS)
    got = e.forward(x)
    t, g = ref_bf16.taps["model.0"][1].numpy(), e.tap("model.0", 1)
    assert np.all(np.abs(g - t) <= 2.0 ** -7 * np.abs(t) + 1e-6)      # same inputs: at most 1 ulp apart
    assert np.mean(g != t) < 0.02                                       # and flips are rare, not systematic
    assert len(_check_taps(e, ref_bf16, (0, 1))) == 63
    _assert_bf16_close(got, want)
    e.close()


@pytest.fixture(scope="module")
def eng16d(weights_path):
    """production kernels + the debug dumps (model.0 from inside the fused stem kernel, the Detect tail's logits)"""
    e = zly.Engine(weights_path, dtype=zly.DTYPE_BF16, max_batch=8, max_dets=512, warmup_runs=1, flags=zly.FLAG_DUMP_LOGITS)
    yield e
    e.close()


def _assert_stem_close(g, t):
    assert g.shape == t.shape
    assert np.all(np.abs(g - t) <= 2.0 ** -7 * np.abs(t) + 1e-6), float(np.abs(g - t).max())      # same inputs: at most 1 bf16 ulp apart
    assert np.mean(g != t) < 0.02                                                                   # and flips are rare, not systematic


@pytest.mark.parametrize("w,h", [(800, 600), (1920, 1080), (417, 415), (64, 48), (1, 1), (416, 416)])
@pytest.mark.parametrize("stem1", [True, False, "persistent"])
def test_fused_stem_kernels_vs_oracle(eng16d, weights_path, oracle, ref_bf16, monkeypatch, w, h, stem1):
    """The PRODUCTION front of the bf16 engine has its own nearest-neighbour resize map, BGR->RGB and u8 -> bf16 scaling:
    stem_model1_kernel (preprocess + model.0 + model.1, the stem map stays in LDS; kernels_stem.hip) and, when that fusion is
    off (ZLY_NO_STEM1 / other widths), stem_fused_kernel (preprocess + model.0).  After detect() on a frame of another size,
    the model.0 tensor must equal conv(preProcess(frame)) of the oracles (reference onnx_engine.cpp:673-693 for the map)
    to 1 bf16 ulp -- a resize index off by one moves whole pixels by O(1) -- and model.1, computed from the LDS map, must
    match the oracle's at layer tolerance."""
    rng = np.random.default_rng(w * 10007 + h)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    rc, pre = oracle.preprocess(img, 416, 416)
    assert rc == 0
    ref_bf16.forward(torch.from_numpy(pre[None]))
    t0, t1 = ref_bf16.taps["model.0"][0].numpy(), ref_bf16.taps["model.1"][0].numpy()
    if stem1 == "persistent":
        # ZLY_STEM1_VAR=2: workgroups walk several tiles (7 workgroups for the 104 tiles of the two-frame batch below: the tile loop crosses the frame
        # boundary and mixes the model-sized frame's quad staging, prefetched a tile ahead, with the other frame's resize map)
        monkeypatch.setenv("ZLY_STEM1_VAR", "2")
        monkeypatch.setenv("ZLY_STEM1_GRID", "7")
        e = zly.Engine(weights_path, max_batch=2, max_dets=64, warmup_runs=0, flags=zly.FLAG_DUMP_LOGITS)
        assert "stem_model1_kernel" in e.op_kernels(1)[1]
    elif stem1:
        e = eng16d
        assert "stem_model1_kernel" in e.op_kernels(1)[1]
    else:
        monkeypatch.setenv("ZLY_NO_STEM1", "1")
        e = zly.Engine(weights_path, max_batch=2, max_dets=64, warmup_runs=0)
        assert "stem_fused_kernel" in e.op_kernels(1)[1]
    e.detect(img, cap=8)
    _assert_stem_close(e.tap("model.0", 0), t0)
    _assert_layer_close(e.tap("model.1", 0), t1, "model.1")
    # and inside a mixed-size batch (per-frame descriptors), as the last frame
    other = zm.synth_frames(1, 416, 416, seed=2, rects=False)[0]
    e.detect_batch([other, img], cap=8)
    _assert_stem_close(e.tap("model.0", 1), t0)
    _assert_layer_close(e.tap("model.1", 1), t1, "model.1")
    if stem1 is not True:
        e.close()


@pytest.mark.parametrize("n,chain", [(16, "lanes"), (64, "lanes"), (64, "single")])
def test_production_kernels_layerwise_vs_oracle(weights_path, oracle, ref_fp32, ref_bf16, n, chain):
    """The kernels the headline number runs, at the batch sizes that select them (conv3x3_lds_kernel S = 1 / 2, resident and
    per-item weights; conv1x1_stream_kernel in every (CT, PT, NK) shape; bottleneck_pair_kernel; stem_fused_kernel; the
    dual-source 1x1 convs; Detect branches on the side streams with per-level tail launches; deferred NMS), checked at
    LAYER level: after one production-path step (zly_detect_device, the flags bench.py uses + the debug dumps) every conv
    output left in HBM -- 59 of 63: the first conv of a fused bottleneck pair stays in LDS -- must match the bf16-rounding
    oracle within 2^-5 of its range for the first, a middle and the last frame of the batch; the head tensor of ALL n
    frames must be within SURVEY 8c's bf16 tolerance of the fp32 oracle, and all n frames' detections must match the
    fp32 oracle's as sets."""
    frames = zm.synth_frames(n, 416, 416, seed=77, rects=False)
    x = torch.from_numpy(_pre(oracle, frames))
    want16 = ref_bf16.forward(x).numpy()
    want32 = ref_fp32.forward(x).numpy()
    # "lanes": one engine, Detect branches on side streams, deferred NMS; "single": ZLY_FLAG_SINGLE_CHAIN, the configuration several
    # engines per GPU run (bench.py --engines 3): per-level tail launches in chain order, NMS in chain order
    flags = (zly.FLAG_ASYNC_NMS if chain == "lanes" else zly.FLAG_SINGLE_CHAIN) | zly.FLAG_DUMP_LOGITS
    e = zly.Engine(weights_path, max_batch=n, max_dets=128, warmup_runs=1, flags=flags)
    d = torch.from_numpy(frames).cuda()
    e.detect_device(d.data_ptr(), n, 416, 416)
    slabs = e.read_slabs(n)
    checked = _check_taps(e, ref_bf16, (0, n // 2 + 1, n - 1), skip_ok=(".m.0.cv1", ".m.1.cv1"))
    assert len(checked) >= 59, checked
    compared = skipped = 0
    for i in range(n):
        gh = e.head_tensor(i)
        _assert_bf16_close(gh[None], want16[i][None])
        _assert_bf16_close(gh[None], want32[i][None])
        c, sk, errors = compare_detection_sets(oracle, want32[i], slabs[i][1], 416, 416, band=BF16_FLIP_BAND, got_head=gh)
        assert not errors, (i, errors)
        compared += c; skipped += sk
    assert compared >= 5 * n and compared >= MIN_COMPARED_FRACTION * (compared + skipped), (compared, skipped)
    e.close()


@pytest.mark.parametrize("w,h,n,env", [(352, 288, 5, {}), (352, 288, 5, {"ZLY_NO_WRES": "1"}), (416, 416, 3, {"ZLY_STREAM_WGS": "8"}),
                                       (224, 416, 4, {"ZLY_LDS_WGS_PER_CU": "1"}), (416, 416, 3, {"ZLY_NO_WS": "1"}),
                                       (416, 416, 3, {"ZLY_C2F64": "1"}), (352, 288, 5, {"ZLY_C2F64": "1"}), (224, 416, 4, {"ZLY_C2F32_NW": "8"}),
                                       (352, 288, 5, {"ZLY_C2F32_NW": "16"}), (416, 416, 3, {"ZLY_WS_ROWT": "1"}), (352, 288, 5, {"ZLY_STREAM_CT2": "1"}), (416, 416, 3, {"ZLY_LDS_S2_PT1": "1"}),
                                       (352, 288, 5, {"ZLY_WS1": "2", "ZLY_WS1_MIN_PX": "1"}), (224, 416, 4, {"ZLY_WS1": "2", "ZLY_WS1_MIN_PX": "1"}),
                                       (416, 416, 3, {"ZLY_WS1": "0"}), (352, 288, 5, {"ZLY_WS1": "2", "ZLY_WS1_MIN_PX": "1", "ZLY_NO_C2F": "1"}),
                                       (416, 416, 3, {"ZLY_WS1_NO_DUAL": "1"}), (352, 288, 5, {"ZLY_WS1": "2", "ZLY_WS1_MIN_PX": "1", "ZLY_WS1_MAX_BYTES": "1"}),
                                       (352, 288, 5, {"ZLY_NO_WS_S2": "1"}), (224, 416, 4, {"ZLY_NO_WS_S2": "1"}), (352, 288, 5, {"ZLY_NO_WS_S2_C32": "1"}),
                                       (352, 288, 5, {"ZLY_WS_MAX_BYTES": "1"}), (416, 416, 3, {"ZLY_STEM1_VAR": "0"}), (352, 288, 5, {"ZLY_STEM1_VAR": "0"}),
                                       (416, 416, 3, {"ZLY_STEM1_VAR": "2"}), (352, 288, 5, {"ZLY_STEM1_VAR": "2", "ZLY_STEM1_GRID": "7"}),
                                       (416, 416, 3, {"ZLY_SPPF_POOL_LDS": "1"}), (352, 288, 5, {"ZLY_SPPF_POOL_LDS": "1"}),
                                       (416, 416, 3, {"ZLY_WS_TPW1_MAXCT": "0"}), (352, 288, 5, {"ZLY_WS_TPW1_MAXCT": "64"}), (416, 416, 3, {"ZLY_NO_WSK": "1"}), (352, 288, 5, {"ZLY_NO_WSK": "1"}), (416, 416, 3, {"ZLY_SPPF_FUSED": "1"}), (224, 416, 4, {"ZLY_SPPF_FUSED": "1"}), (352, 288, 5, {"ZLY_SPPF_FUSED": "1"})])
def test_throughput_kernels_on_ragged_maps(weights_path, oracle, monkeypatch, w, h, n, env):
    """conv3x3_lds_kernel, conv1x1_stream_kernel and bottleneck_pair_kernel forced onto small batches of ragged maps (88x72 ..
    11x9, 104x104 .. 13x13, 56x104 .. 7x13: partial tiles on every edge, 13-row maps, last pixel groups that are not full,
    persistent workgroups that loop over many items), every conv output against the bf16-rounding oracle.  ZLY_C2F64: the opt-in fused
    64-channel C2f kernel (c2f64_kernel: whole blocks, front and back halves, dual-source cv1, partial tiles; its intermediate maps are
    dumped too); ZLY_C2F32_NW: both wave counts of the 32-channel C2f kernel in every mode; ZLY_WS1=2 + ZLY_WS1_MIN_PX=1: the weight-stationary
    1x1 kernel on every single-source pointwise conv with >= 128 input channels (pixel tiles that end mid-column-tile, 4 / 6 / 8 / 12 / 16
    k-steps, one and two channel blocks), ZLY_WS1=0: none of them; ZLY_WS1_MAX_BYTES=1: its fall-back to the direct kernel for tensors
    beyond 32-bit byte offsets; ZLY_NO_WS_S2=1 (ZLY_NO_WS_S2_C32=1): the stride-2 convs with 32 / 64 (32) input channels on the LDS-tiled kernel instead of the weight-stationary one
    (the default runs cover that one: ragged 44x36 -> 22x18 and 28x52 -> 14x26 maps); ZLY_WS_MAX_BYTES=1: the weight-stationary 3x3 kernel's fall-back for tensors
    beyond 32-bit byte offsets; ZLY_STEM1_VAR=0: the front kernel's round-3 staging / tap order (the default, conflict-free one runs in every other case), =2: its persistent form (a workgroup
    walks several tiles, the next tile's input bytes in flight; ZLY_STEM1_GRID=7: 180 tiles on 7 workgroups);
    ZLY_SPPF_FUSED=1: the opt-in fused SPPF kernel (cv1 + three pools + cv2 in one launch; checked tap by tap like the three-launch form: model.9.cv1, model.9.cv2);
    ZLY_SPPF_POOL_LDS=1: SPPF's pools on the six-pass LDS kernel (the default on these 13 x 13 / 11 x 9 / 7 x 13 maps is sppf_pool16_kernel: DPP row windows, one barrier)."""
    import yolov8_ref
    for k, v in dict(ZLY_LDS_MIN_TILES="1", ZLY_STREAM_MIN_GROUPS="1", ZLY_PAIR_MIN_TILES="1", ZLY_WS_MIN_TILES="1", **env).items():
        monkeypatch.setenv(k, v)
    frames = zm.synth_frames(n, w, h, seed=31, rects=False)
    x = _pre(oracle, frames, w, h)
    ref = yolov8_ref.load(weights_path, "bf16")
    want = ref.forward(torch.from_numpy(x)).numpy()
    e = zly.Engine(weights_path, model_w=w, model_h=h, max_batch=n, warmup_runs=0, flags=zly.FLAG_DUMP_LOGITS)
    # the switches must really have selected what the case is about (as process-static variables they were fixed by the first engine
    # of the pytest process and these cases never switched kernels); the engine reads them once, at zly_create
    kn = " | ".join(e.op_kernels(n))
    if "ZLY_NO_WS" in env:
        assert "conv3x3_ws_kernel<TPW" not in kn and "conv3x3_ws_kernel<ROWT" not in kn, kn
    elif "ZLY_WS_ROWT" in env:
        assert "conv3x3_ws_kernel<ROWT" in kn, kn
    elif not env:
        assert "conv3x3_ws_kernel<TPW" in kn and "conv3x3_ws_kernel<ROWT" not in kn, kn
    if "ZLY_WS_TPW1_MAXCT" in env:                  # 64 -> 64 as 4 waves x one tile: never / on every tile size
        assert ("TPW=1,4 channel tiles" in kn) == (env["ZLY_WS_TPW1_MAXCT"] != "0"), kn
    if "ZLY_C2F32_NW" in env:
        nws = [s_.split("NW=")[1].split(",")[0] for s_ in e.op_kernels(n) if s_.startswith("c2f_kernel<C=32")]
        assert nws and all(v == env["ZLY_C2F32_NW"] for v in nws), kn
    if "ZLY_NO_WS_S2" in env:
        assert "conv3x3_ws_kernel<S=2" not in kn, kn
    if env.get("ZLY_WS1") == "0":
        assert "conv1x1_ws_kernel" not in kn, kn
    # the forced fall-backs are planned as the kernels that run: the table names no weight-stationary kernel that would fall back at launch
    if "ZLY_WS_MAX_BYTES" in env:
        assert "conv3x3_ws_kernel<" not in kn, kn
    if "ZLY_WS1_MAX_BYTES" in env:
        assert "conv1x1_ws_kernel" not in kn, kn
    if "ZLY_C2F64" in env:
        assert "c2f_kernel<C=64" in kn, kn
    # the 80 -> 80 class-branch convs: the K-packed five-wave kernel (ragged 13 x 13 tiles of 52 x 52 ... 7 x 13 maps here) unless switched off
    assert ("conv3x3_wsk_kernel" in kn) == ("ZLY_NO_WSK" not in env and n > 4), kn        # batch <= 4: the Detect convs run as merged launches
    # SPPF: cv1 | pool | cv2 launches by default; ZLY_SPPF_FUSED=1: one launch (kernels_sppf.hip: 13 x 13, 7 x 13 and 11 x 9 maps here, split 4 ways by output channels)
    assert ("sppf_fused_kernel" in kn) == ("ZLY_SPPF_FUSED" in env), kn
    assert ("sppf_pool" in kn) == ("ZLY_SPPF_FUSED" not in env), kn
    if "ZLY_SPPF_FUSED" not in env:                 # maps of <= 16 x 16 pixels: the one-barrier kernel (DPP row windows) unless switched back to the six-pass one
        assert ("sppf_pool16_kernel" in kn) == ("ZLY_SPPF_POOL_LDS" not in env) and ("sppf_pool_kernel" in kn) == ("ZLY_SPPF_POOL_LDS" in env), kn
    got = e.forward(x)
    checked = _check_taps(e, ref, range(n), skip_ok=(".m.0.cv1", ".m.1.cv1"))
    assert len(checked) >= 59, checked
    _assert_bf16_close(got, want)
    # ... and every conv against float64 on the engine's own tapped inputs, per element (tests/closed_loop_ref.py), first and last frame
    assert len(check_closed_loop(e, weights_path, (0, n - 1), lds_resident=lds_resident_from_kernels(e, n))) == 63
    for i in (0, n - 1):
        check_head_decode(e, got[i], i)
    # the detect path's front (stem_model1_kernel: ragged tiles of the model.1 map, stem halo beyond the map edges)
    res = e.detect_batch(list(frames), cap=64)
    for i in range(n):
        _assert_stem_close(e.tap("model.0", i), ref.taps["model.0"][i].numpy())
        for name in ("model.1", "model.2.cv2", "model.9.cv2"):
            _assert_layer_close(e.tap(name, i), ref.taps[name][i].numpy(), f"{name}[{i}] after detect")
    assert len(res) == n
    e.close()


@pytest.mark.parametrize("w,h", [(416, 416), (352, 288), (224, 416), (512, 512)])
def test_sppf_pool_kernels_same_bits(weights_path, monkeypatch, w, h):
    """SPPF's three chained 5x5 max pools: the one-barrier kernel of small maps (sppf_pool16_kernel: v_pk_max_i16 in a sortable domain, row windows by
    DPP, column windows of radius 2 / 4 / 6 read directly with clamped rows) against the six-pass fp32 LDS kernel on the same engine otherwise.
    max is a selection: model.9.cv2 -- the conv over [y | p1 | p2 | p3] -- and the detections must come out bit for bit (13 x 13, 11 x 9, 7 x 13 and
    16 x 16 maps: partial DPP rows, non-square maps, the largest map the kernel takes)."""
    frames = zm.synth_frames(3, w, h, seed=77, rects=False)
    outs = []
    for six in (False, True):
        if six: monkeypatch.setenv("ZLY_SPPF_POOL_LDS", "1")
        e = zly.Engine(weights_path, model_w=w, model_h=h, max_batch=3, max_dets=64, warmup_runs=0, flags=zly.FLAG_DUMP_LOGITS)
        assert ("sppf_pool16_kernel" in " ".join(e.op_kernels(3))) == (not six)
        res = e.detect_batch(list(frames), cap=64)
        outs.append(([e.tap("model.9.cv2", i) for i in range(3)], res))
        e.close()
    for i in range(3):
        assert np.array_equal(outs[0][0][i], outs[1][0][i])
        assert outs[0][1][i][1] == outs[1][1][i][1] and det_fields_equal(outs[0][1][i][0], outs[1][1][i][0])


def test_forward_bf16_vs_fp32_oracle(eng16, oracle, ref_fp32):
    frames = np.concatenate([zm.synth_frames(2, 416, 416, seed=7, rects=False), zm.synth_frames(8, 416, 416, seed=1)[6:7]])
    x = _pre(oracle, frames)
    want = ref_fp32.forward(torch.from_numpy(x)).numpy()
    got = eng16.forward(x)
    _assert_bf16_close(got, want)


# ---------------------------------------------------------------------------------------------------
# whole path
# ---------------------------------------------------------------------------------------------------
def _match(got, want, iou_fn, min_iou=0.9):
    used = set()
    for g in got:
        best, bj = 0.0, -1
        for j, w_ in enumerate(want):
            if j in used or w_["class_id"] != g["class_id"]:
                continue
            v = iou_fn([g["x"], g["y"], g["w"], g["h"]], [w_["x"], w_["y"], w_["w"], w_["h"]])
            if v > best:
                best, bj = v, j
        if bj < 0 or best < min_iou:
            return False
        used.add(bj)
    return True


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_detect_equals_oracle_postprocess_of_own_head(eng32, eng16, oracle, dtype):
    """detect() == oracle post-processing applied to the engine's own head tensor, bit for bit:
    pins preprocess -> forward -> decode -> NMS wiring without any NN tolerance."""
    eng = eng32 if dtype == "fp32" else eng16
    frames = list(zm.synth_frames(3, 416, 416, seed=5, rects=False)) + [zm.synth_frames(1, 800, 600, seed=3, rects=False)[0]]
    for f in frames:
        dets, n = eng.detect(f, cap=512)
        want = oracle.postprocess(eng.head_tensor(0), f.shape[1], f.shape[0])
        assert n == len(want) and det_fields_equal(dets, want[:512])
        assert np.all(dets["track_id"] == 0) and (n == 0 or np.all(dets["timestamp"] > 1_600_000_000_000))


def test_detect_fp32_matches_full_cpu_pipeline(eng32, oracle, ref_fp32):
    """Whole path vs whole oracle (oracle preprocess -> fp32 reference forward -> oracle decode/NMS).
    Candidates within 1e-3 of the confidence threshold or pairs within 1e-3 of the IoU threshold may
    legitimately flip, so frames containing such cases are compared as matched sets."""
    frames = zm.synth_frames(3, 416, 416, seed=5, rects=False)
    x = _pre(oracle, frames)
    heads = ref_fp32.forward(torch.from_numpy(x)).numpy()
    for f, head in zip(frames, heads):
        want = oracle.postprocess(head, 416, 416)
        dets, n = eng32.detect(f, cap=512)
        scores = head[4:].max(0)
        near = bool(np.any(np.abs(scores - 0.5) < 1e-3))
        # ... or a same-class pair of candidates whose IoU is within 1e-3 of the NMS threshold (a suppression decision may flip)
        cand = np.nonzero(scores >= 0.5 - 1e-3)[0]
        cls = head[4:, cand].argmax(0)
        for i in range(len(cand)):
            for j in range(i + 1, len(cand)):
                if cls[i] == cls[j] and abs(oracle.iou(list(head[:4, cand[i]]), list(head[:4, cand[j]])) - 0.45) < 1e-3:
                    near = True
        if not near:
            # no threshold decision is within rounding distance: the fp32 engine must produce EXACTLY the oracle's detections (the
            # containment branch below used to be taken whenever the counts differed, so a dropped clear detection would have passed)
            assert n == len(want), (n, len(want))
            assert np.array_equal(dets["class_id"], want["class_id"])
            for k in ("x", "y", "w", "h"):
                assert np.abs(dets[k] - want[k]).max() <= FP32_BOX_TOL / 416 * 2
            assert np.abs(dets["confidence"] - want["confidence"]).max() <= FP32_SCORE_TOL
        else:
            # a flip adds or removes a detection: the smaller set must be contained in the larger one, and they differ by at most 2
            small, large = (dets, want) if n <= len(want) else (want, dets)
            assert abs(n - len(want)) <= 2 and _match(small, large, oracle.iou, 0.5)


def test_detect_bf16_sets_match_fp32_oracle(eng16, oracle, ref_fp32):
    """SURVEY 8c, set level, batch 1 (the latency path): the bf16 engine's FINAL detections against the fp32 oracle's
    (oracle preprocess -> fp32 forward -> oracle decode/NMS), same class + IoU >= 0.9 + confidence within 2e-2, every
    connected group of overlapping candidates compared exactly unless it contains a score within 2e-2 of the
    confidence threshold or an IoU within 2e-2 of the NMS threshold (tests/parity_sets.py).  Includes a stretched
    800x600 request (boxes normalised by the request size)."""
    frames = list(zm.synth_frames(10, 416, 416, seed=5, rects=False)) + [zm.synth_frames(1, 800, 600, seed=3, rects=False)[0],
                                                                            zm.synth_frames(1, 320, 240, seed=23)[0]]
    x = _pre(oracle, frames)
    heads = ref_fp32.forward(torch.from_numpy(x)).numpy()
    compared = skipped = 0
    for f, head in zip(frames, heads):
        dets, n = eng16.detect(f, cap=512)
        assert n == len(dets)
        gh = eng16.head_tensor(0)
        assert np.abs(gh[:4] - head[:4]).max() <= BF16_BOX_MAX and np.abs(gh[4:] - head[4:]).max() <= BF16_SCORE_MAX
        c, sk, errors = compare_detection_sets(oracle, head, dets, f.shape[1], f.shape[0], band=BF16_FLIP_BAND, got_head=gh)
        assert not errors, errors
        compared += c; skipped += sk
    assert compared >= 80 and compared >= MIN_COMPARED_FRACTION * (compared + skipped), (compared, skipped)


def _mixed_frames():
    return [zm.synth_frames(1, 416, 416, seed=21, rects=False)[0], zm.synth_frames(1, 800, 600, seed=22, rects=False)[0],
            zm.synth_frames(1, 320, 240, seed=23)[0], zm.synth_frames(1, 416, 416, seed=24, rects=False)[0]]


def test_batch_equals_single_exactly_fp32(eng32):
    """The fp32 engine uses one kernel configuration for every batch size, so a batch is bit-identical
    to the same frames detected one at a time (the reference only ever runs frames one by one,
    onnx_engine.cpp:348-365), including frames of mixed sizes in one batch."""
    frames = _mixed_frames()
    singles = [eng32.detect(f, cap=512) for f in frames]
    batch = eng32.detect_batch(frames, cap=512)
    for (sd, sn), (bd, bn) in zip(singles, batch):
        assert sn == bn and det_fields_equal(sd, bd)


def test_batch_vs_single_bf16(eng16, oracle):
    """The bf16 engine picks tile shapes / split-K per batch size (fp32 summation order changes, so bf16
    roundings may flip): per frame, batched decode+NMS must be bit-exact on that frame's own head
    tensor, and the batched head tensor must agree with the single-frame one within the bf16 tolerance."""
    frames = _mixed_frames()
    single_heads = []
    for f in frames:
        eng16.detect(f, cap=512)
        single_heads.append(eng16.head_tensor(0))
    batch = eng16.detect_batch(frames, cap=512)
    for i, (f, (bd, bn)) in enumerate(zip(frames, batch)):
        h = eng16.head_tensor(i)
        want = oracle.postprocess(h, f.shape[1], f.shape[0])
        assert bn == len(want) and det_fields_equal(bd, want[:512])
        _assert_bf16_close(h[None], single_heads[i][None])


def test_device_path_slabs_equal_host_path(eng16):
    frames = zm.synth_frames(8, 416, 416, seed=31, rects=False)
    host = eng16.detect_batch(list(frames), cap=512)
    d = torch.from_numpy(frames).cuda()
    torch.cuda.synchronize()
    eng16.detect_device(d.data_ptr(), 8, 416, 416, tag0=100)
    slabs = eng16.read_slabs(8)
    for i, ((hdr, dets), (hd, hn)) in enumerate(zip(slabs, host)):
        assert hdr["n_kept"] == hn and hdr["frame_tag"] == 100 + i and det_fields_equal(dets, hd)


def test_slab_overflow_flag(weights_path):
    e = zly.Engine(weights_path, max_batch=1, max_dets=4, warmup_runs=0)
    f = zm.synth_frames(1, 416, 416, seed=5, rects=False)[0]
    dets, n = e.detect(f, cap=4)
    d = torch.from_numpy(f[None]).cuda()
    e.detect_device(d.data_ptr(), 1, 416, 416)
    hdr, sd = e.read_slabs(1)[0]
    assert n > 4 and len(dets) == 4 and hdr["n_kept"] == n and (hdr["flags"] & zly.SLAB_OVERFLOW)
    e.close()


def test_empty_frame_has_no_detections(eng16):
    f = zm.synth_frames(8, 416, 416, seed=1)[0]          # a rect frame known to score below threshold everywhere
    dets, n = eng16.detect(f)
    assert n == 0 and len(dets) == 0


def test_graph_and_eager_paths_agree(weights_path):
    f = zm.synth_frames(2, 416, 416, seed=41, rects=False)
    a = zly.Engine(weights_path, max_batch=2, max_dets=256, use_graph=True, warmup_runs=1)
    b = zly.Engine(weights_path, max_batch=2, max_dets=256, use_graph=False, warmup_runs=0)
    ra, rb = a.detect_batch(list(f), cap=256), b.detect_batch(list(f), cap=256)
    for (da, na), (db, nb) in zip(ra, rb):
        assert na == nb and det_fields_equal(da, db)
    a.close(); b.close()


def test_full_batch_64_is_batch_invariant(weights_path, oracle):
    """BASELINE config 3 size (batch 64): every frame's slab equals its single-frame result."""
    e = zly.Engine(weights_path, max_batch=64, max_dets=128, warmup_runs=1)
    frames = zm.synth_frames(64, 416, 416, seed=77, rects=False)
    d = torch.from_numpy(frames).cuda()
    e.detect_device(d.data_ptr(), 64, 416, 416)
    slabs = e.read_slabs(64)
    perm = np.random.default_rng(0).permutation(64)
    d2 = torch.from_numpy(frames[perm]).cuda()
    e.detect_device(d2.data_ptr(), 64, 416, 416)
    slabs2 = e.read_slabs(64)
    for i in range(64):
        assert det_fields_equal(slabs2[i][1], slabs[perm[i]][1])      # permutation equivariance
    e.detect_device(d.data_ptr(), 64, 416, 416)
    slabs = e.read_slabs(64)
    for i in (0, 17, 63):                                            # batched decode/NMS indexing, per frame
        want = oracle.postprocess(e.head_tensor(i), 416, 416)
        assert slabs[i][0]["n_kept"] == len(want) and det_fields_equal(slabs[i][1], want[:128])
        bh = e.head_tensor(i)
        e2_d, _ = e.detect(frames[i], cap=128)                       # single-frame run: other tile shapes, same result within bf16 noise
        _assert_bf16_close(bh[None], e.head_tensor(0)[None])
        e.detect_device(d.data_ptr(), 64, 416, 416)
    e.close()


def test_model_file_errors(weights_path, tmp_path):
    with pytest.raises(zly.ZlyError) as ei:
        zly.Engine(str(tmp_path / "missing.zlyw"))
    assert ei.value.code == zly.ERR_MODEL_NOT_FOUND
    bad = tmp_path / "bad.zlyw"
    bad.write_bytes(b"ONNX MODEL PLACEHOLDER")          # what reference start.sh:136-144 writes on export failure
    with pytest.raises(zly.ZlyError) as ei:
        zly.Engine(str(bad))
    assert ei.value.code == zly.ERR_MODEL_LOAD
    # crafted records must not wrap the loader's bounds arithmetic (the file is re-read by the hot-reload watcher)
    import struct
    good = bytearray(open(weights_path, "rb").read())
    rec0 = zm.HDR_SIZE
    cases = {"huge_dims": (rec0 + 48, struct.pack("<II", 0x7fffffff, 0x7fffffff)),          # cin, cout: product wraps size_t
             "w_off_wraps": (rec0 + 48 + 24, struct.pack("<Q", 2 ** 64 - 8)),                # w_off + nw * 4 wraps to a small number
             "b_off_wraps": (rec0 + 48 + 32, struct.pack("<Q", 2 ** 64 - 4)),
             "nc_out_of_range": (8, struct.pack("<I", 100000))}
    for name, (off, patch) in cases.items():
        blob = bytearray(good)
        blob[off:off + len(patch)] = patch
        f = tmp_path / (name + ".zlyw")
        f.write_bytes(bytes(blob))
        with pytest.raises(zly.ZlyError) as ei:
            zly.Engine(str(f))
        assert ei.value.code == zly.ERR_MODEL_LOAD, name


# ---------------------------------------------------------------------------------------------------
# the other BASELINE configurations as parity cases: 640x640 input (config 3) and YOLOv8-s widths (config 4, bf16)
# ---------------------------------------------------------------------------------------------------
def test_640x640_fp32_and_bf16(weights_path, oracle, ref_fp32):
    frames = zm.synth_frames(2, 640, 640, seed=11, rects=False)
    x = _pre(oracle, frames, 640, 640)
    want = ref_fp32.forward(torch.from_numpy(x)).numpy()
    assert want.shape == (2, 84, 8400)
    e = zly.Engine(weights_path, model_w=640, model_h=640, dtype=zly.DTYPE_FP32, max_batch=2, max_dets=512, warmup_runs=0)
    got = e.forward(x)
    assert np.abs(got[:, :4] - want[:, :4]).max() <= 2 * FP32_BOX_TOL and np.abs(got[:, 4:] - want[:, 4:]).max() <= FP32_SCORE_TOL
    e.close()
    e = zly.Engine(weights_path, model_w=640, model_h=640, dtype=zly.DTYPE_BF16, max_batch=2, max_dets=512, warmup_runs=0)
    for f in frames:
        dets, n = e.detect(f, cap=512)
        own = oracle.postprocess(e.head_tensor(0), 640, 640)
        assert n == len(own) and det_fields_equal(dets, own[:512])
    got = e.forward(x)
    _assert_bf16_close(got, want)                                                  # same strides, same pixel tolerance
    compared = skipped = 0
    for f, head in zip(frames, want):
        dets, n = e.detect(f, cap=512)
        c, sk, errors = compare_detection_sets(oracle, head, dets, 640, 640, band=BF16_FLIP_BAND, got_head=e.head_tensor(0))
        assert not errors and c > 0, errors
        compared += c; skipped += sk
    # two 640x640 frames of noise: ~170-280 candidates each in few classes -> large same-class components, where one real flip high in the
    # greedy order leaves everything after it uncomparable; half is what the bf16-rounding oracle itself reaches on these two frames
    assert compared >= 0.5 * (compared + skipped), (compared, skipped)
    e.close()


def test_640x640_batch_32_per_gpu_share(weights_path, oracle):
    """BASELINE configs[3] as one GPU sees it: 640x640, 32 frames per step (batch 256 over 8 GPUs), the production flags
    (fused bottlenecks, streaming 1x1, side streams, deferred NMS).  Size-independent properties: permutation
    equivariance of the slabs, and detect() == the oracle's post-processing of the engine's own head tensor."""
    n = 32
    frames = zm.synth_frames(n, 640, 640, seed=91, rects=False)
    e = zly.Engine(weights_path, model_w=640, model_h=640, max_batch=n, max_dets=128, warmup_runs=1, flags=zly.FLAG_ASYNC_NMS)
    d = torch.from_numpy(frames).cuda()
    e.detect_device(d.data_ptr(), n, 640, 640)
    slabs = e.read_slabs(n)
    perm = np.random.default_rng(1).permutation(n)
    d2 = torch.from_numpy(frames[perm]).cuda()
    e.detect_device(d2.data_ptr(), n, 640, 640)
    slabs2 = e.read_slabs(n)
    for i in range(n):
        assert slabs2[i][0]["n_kept"] == slabs[perm[i]][0]["n_kept"] and det_fields_equal(slabs2[i][1], slabs[perm[i]][1])
    e.detect_device(d.data_ptr(), n, 640, 640)
    slabs = e.read_slabs(n)
    for i in (0, 13, n - 1):
        want = oracle.postprocess(e.head_tensor(i), 640, 640)
        assert slabs[i][0]["n_kept"] == len(want) and det_fields_equal(slabs[i][1], want[:128])
    assert sum(int(s_[0]["n_kept"]) for s_ in slabs) > 0
    e.close()


def test_yolov8s_widths(tmp_path, oracle):
    """YOLOv8-s channel widths (32..512, Detect class branch 128 wide): the plan builder, tile pickers and the
    fused Detect tail are generic in the widths; the 32-channel stem takes the unfused preprocess + conv path."""
    import yolov8_ref
    spec = zm.build_spec("s")
    p = str(tmp_path / "yolov8s_synth.zlyw")
    zm.write_zlyw(p, spec, zm.synth_weights(spec, seed=9))
    ref = yolov8_ref.load(p, "fp32")
    frames = zm.synth_frames(2, 320, 320, seed=12, rects=False)
    x = _pre(oracle, frames, 320, 320)
    want = ref.forward(torch.from_numpy(x)).numpy()
    e = zly.Engine(p, model_w=320, model_h=320, dtype=zly.DTYPE_FP32, max_batch=2, max_dets=512, warmup_runs=0)
    got = e.forward(x)
    scale = max(1.0, float(np.abs(want[:, :4]).max()) / 800.0)
    assert np.abs(got[:, :4] - want[:, :4]).max() <= 4 * FP32_BOX_TOL * scale
    assert np.abs(got[:, 4:] - want[:, 4:]).max() <= 2 * FP32_SCORE_TOL
    e.close()
    e = zly.Engine(p, model_w=320, model_h=320, dtype=zly.DTYPE_BF16, max_batch=2, max_dets=512, conf_thr=0.05, warmup_runs=0,
                   flags=zly.FLAG_DUMP_LOGITS)
    for f in frames:
        dets, n = e.detect(f, cap=512)
        own = oracle.postprocess(e.head_tensor(0), 320, 320, 0.05, 0.45)
        assert n == len(own) and det_fields_equal(dets, own[:512])
    # the bf16 head against both oracles, and every conv output against the bf16-rounding oracle's
    ref16 = yolov8_ref.load(p, "bf16")
    want16 = ref16.forward(torch.from_numpy(x)).numpy()
    got = e.forward(x)
    _assert_bf16_close(got, want16)
    _assert_bf16_close(got, want)
    assert len(_check_taps(e, ref16, (0, 1), skip_ok=(".m.0.cv1", ".m.1.cv1"), names=[c.name for c in spec.convs])) >= 55
    assert len(check_closed_loop(e, p, (0, 1), lds_resident=lds_resident_from_kernels(e, 2))) == len(spec.convs)
    for i in (0, 1):
        check_head_decode(e, got[i], i)
    e.close()


@pytest.mark.parametrize("env", [{}, {"ZLY_WS1": "2", "ZLY_WS1_MIN_PX": "1"}])
def test_yolov8s_640_fp8_weights(tmp_path, oracle, monkeypatch, env):
    """BASELINE configs[4] as one GPU sees it: YOLOv8-s, 640 x 640, fp8 (e4m3) weights (second run: every pointwise conv with >= 128 input
    channels on the weight-stationary 1x1 kernel -- 4 .. 32 k-steps, one channel tile per wave from 768 inputs up, the Upsample + Concat inputs).  The file stores one byte per weight; the
    loader dequantises to values that are exact in bf16, so the engine must match the oracle ON THE SAME DEQUANTISED WEIGHTS at
    the usual bf16 tolerances: every conv output against the bf16-rounding oracle, the head tensor against the fp32 oracle
    (box <= 1.5 px, score <= 2e-2), detect() == the oracle's post-processing of the engine's own head tensor."""
    import yolov8_ref
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    spec = zm.build_spec("s")
    p = str(tmp_path / "yolov8s_synth_fp8.zlyw")
    zm.write_zlyw(p, spec, zm.synth_weights(spec, seed=9), fp8=True)
    ref32, ref16 = yolov8_ref.load(p, "fp32"), yolov8_ref.load(p, "bf16")
    frames = zm.synth_frames(2, 640, 640, seed=11, rects=False)
    x = _pre(oracle, frames, 640, 640)
    want32 = ref32.forward(torch.from_numpy(x)).numpy()
    want16 = ref16.forward(torch.from_numpy(x)).numpy()
    assert want32.shape == (2, 84, 8400)
    e = zly.Engine(p, model_w=640, model_h=640, max_batch=2, max_dets=1024, conf_thr=0.5, warmup_runs=0, flags=zly.FLAG_DUMP_LOGITS)
    assert e.weights_fp8
    got = e.forward(x)
    _assert_bf16_close(got, want16)
    _assert_bf16_close(got, want32)
    assert len(_check_taps(e, ref16, (0, 1), skip_ok=(".m.0.cv1", ".m.1.cv1"))) >= 55
    for i, f in enumerate(frames):
        dets, n = e.detect(f, cap=1024)
        own = oracle.postprocess(e.head_tensor(0), 640, 640, 0.5, 0.45)
        assert n == len(own) and det_fields_equal(dets, own[:1024])
        # the detect path's front for the 32-channel stem (stem_fused_kernel<2>: preprocess + model.0 in one kernel, pair-permuted rows):
        # the head tensor it leads to must be the forward pass of the preprocessed frame within the bf16 tolerance
        _assert_bf16_close(e.head_tensor(0)[None], want32[i][None])
        _assert_layer_close(e.tap("model.0", 0), ref16.taps["model.0"][i].numpy(), f"model.0 of frame {i} (fused stem, 32 channels)")
    e.close()
    # every conv against float64 on the engine's own inputs with the weights as the loader dequantises them, on a 96 x 64 engine beside the 640 one
    # (P5 is a 3 x 2 map; keeps the float64 work small)
    small = _pre(oracle, zm.synth_frames(2, 96, 64, seed=11, rects=False), 96, 64)
    e = zly.Engine(p, model_w=96, model_h=64, max_batch=2, warmup_runs=0, flags=zly.FLAG_DUMP_LOGITS)
    assert e.weights_fp8
    got = e.forward(small)
    assert len(check_closed_loop(e, p, (0, 1), lds_resident=lds_resident_from_kernels(e, 2))) == len(spec.convs)
    for i in (0, 1):
        check_head_decode(e, got[i], i)
    e.close()
    e = zly.Engine(zly.DEFAULT_WEIGHTS, warmup_runs=0)
    assert not e.weights_fp8
    e.close()


def test_production_flags_same_detections(weights_path):
    """ZLY_FLAG_NO_HEAD_TENSOR (what the plugin and bench.py run): the Detect kernel skips the fp32 head tensor, the
    detections are the same bytes; the parity entry points that need the tensor fail loudly."""
    frames = zm.synth_frames(8, 416, 416, seed=41, rects=False)
    a = zly.Engine(weights_path, max_batch=8, max_dets=128, conf_thr=0.25, warmup_runs=0)
    b = zly.Engine(weights_path, max_batch=8, max_dets=128, conf_thr=0.25, warmup_runs=0, flags=zly.FLAG_NO_HEAD_TENSOR)
    ra, rb = a.detect_batch(list(frames), cap=128), b.detect_batch(list(frames), cap=128)
    assert sum(n for _, n in ra) > 0
    for (da, na), (db, nb) in zip(ra, rb):
        assert na == nb and det_fields_equal(da, db)
    with pytest.raises(zly.ZlyError):
        b.head_tensor(0)
    with pytest.raises(zly.ZlyError):
        b.forward(np.zeros((1, 3, 416, 416), np.float32))
    a.close(); b.close()


def test_deferred_nms_same_slabs(weights_path):
    """ZLY_FLAG_ASYNC_NMS: NMS of call k runs on the engine's own stream beside call k+1.  Five calls with different
    batches and slab buffers must give byte-identical slabs to the in-order engine; zly_join / zly_read_slabs /
    zly_sync are the points where a call's slabs are complete."""
    n = 16                                            # deferral applies from batch 16 up
    sets = [zm.synth_frames(n, 416, 416, seed=50 + i, rects=False) for i in range(3)]
    dev = [torch.from_numpy(x).cuda() for x in sets]
    a = zly.Engine(weights_path, max_batch=n, max_dets=64, conf_thr=0.25, warmup_runs=1)
    b = zly.Engine(weights_path, max_batch=n, max_dets=64, conf_thr=0.25, warmup_runs=1, flags=zly.FLAG_ASYNC_NMS)
    sb = a.slab_bytes
    want = []
    for k in range(5):
        a.detect_device(dev[k % 3].data_ptr(), n, 416, 416, tag0=100 * k)
        want.append(a.read_slabs(n))
    stream = torch.cuda.Stream()
    bufs = [torch.zeros(n * sb, dtype=torch.uint8, device="cuda") for _ in range(5)]
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        for k in range(5):
            b.detect_device(dev[k % 3].data_ptr(), n, 416, 416, d_slabs_ptr=bufs[k].data_ptr(), tag0=100 * k, stream=stream.cuda_stream)
        b.join(stream.cuda_stream)
    stream.synchronize()
    total = 0
    for k in range(5):
        got = zly.parse_slabs(bufs[k].cpu().numpy(), n, b.max_dets)
        for i in range(n):
            assert got[i][0]["n_kept"] == want[k][i][0]["n_kept"] and got[i][0]["frame_tag"] == 100 * k + i
            assert det_fields_equal(got[i][1], want[k][i][1])
            total += int(got[i][0]["n_kept"])
    assert total > 0
    # the internal slab buffer + zly_read_slabs (joins by itself), then a synchronous-path call on the same engine
    b.detect_device(dev[1].data_ptr(), n, 416, 416, tag0=7)
    got = b.read_slabs(n)
    assert all(det_fields_equal(got[i][1], want[1][i][1]) for i in range(n))
    b.detect_device(dev[0].data_ptr(), n, 416, 416, tag0=1)                       # deferred ...
    b.detect_device(dev[2].data_ptr(), 4, 416, 416, tag0=9)                       # ... then a small, in-order call on the same engine
    got = b.read_slabs(4)
    a.detect_device(dev[2].data_ptr(), 4, 416, 416, tag0=9)
    ref4 = a.read_slabs(4)
    assert all(det_fields_equal(got[i][1], ref4[i][1]) for i in range(4))
    d1, n1 = b.detect(sets[2][3], cap=64)
    d2, n2 = a.detect(sets[2][3], cap=64)
    assert n1 == n2 and det_fields_equal(d1, d2)
    a.close(); b.close()


@pytest.mark.parametrize("flags,env", [(0, {}), (zly.FLAG_SINGLE_CHAIN, {}), (zly.FLAG_NO_FUSION, {}), (0, {"ZLY_SPPF_FUSED": "1"})],
                         ids=["default", "single_chain", "no_fusion", "sppf_fused"])
def test_launch_introspection_agrees(weights_path, monkeypatch, flags, env):
    """op_kernels(), launches() and profile_ops() describe the same launches (bench.py's roofline table reads all three): an op is covered
    by another op's launch exactly when its kernel name is a parenthesised note, every launch that covers ops covers itself, and the
    per-launch profile books time on exactly the ops that launch"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    e = zly.Engine(weights_path, max_batch=64, warmup_runs=0, flags=flags)
    frames = torch.from_numpy(zm.synth_frames(64, 416, 416, seed=17, rects=False)).cuda()
    torch.cuda.synchronize()
    for n in (1, 4, 5, 16, 64):
        kern, lau = e.op_kernels(n), e.launches(n)
        ms = e.profile_ops(frames.data_ptr(), n, 416, 416, reps=2)
        for i, (k, li) in enumerate(zip(kern, lau)):
            by = li["covered_by"]
            assert (by != i) == k.startswith("("), (n, i, k, by)
            assert lau[by]["covered_by"] == by, (n, i, k, by)
            assert (ms[i] == 0) == (by != i), (n, i, k, float(ms[i]))
    e.close()


def test_latency_path_merged_detect_launches(weights_path, oracle, ref_bf16, monkeypatch):
    """Batch <= 4 (the latency path): the three Detect stem convs run as ONE launch and the six box / class branch convs as another
    (conv_igemm_multi_kernel, blockIdx.z picks the conv).  Every conv output and the detections must be those of the per-conv
    launches (same kernel body, same k order: bit-identical), and every layer must match the bf16-rounding oracle."""
    frames = zm.synth_frames(3, 416, 416, seed=91, rects=False)
    x = _pre(oracle, frames)
    ref_bf16.forward(torch.from_numpy(x))
    e = zly.Engine(weights_path, max_batch=3, max_dets=256, warmup_runs=0, flags=zly.FLAG_DUMP_LOGITS)
    ks = e.op_kernels(1)
    assert sum("conv_igemm_multi_kernel" in k for k in ks) == 2 and sum("merged Detect launch" in k for k in ks) == 7, ks
    res = e.detect_batch(list(frames), cap=256)
    names = [f"model.22.cv{b}.{l}.{j}" for b in (2, 3) for l in range(3) for j in (0, 1, 2)]
    taps = {name: [e.tap(name, i) for i in range(3)] for name in names}
    for name in names:
        for i in range(3):
            _assert_layer_close(taps[name][i], ref_bf16.taps[name][i].numpy(), f"{name}[{i}]")
    e.close()
    monkeypatch.setenv("ZLY_NO_DET_MERGE", "1")
    p = zly.Engine(weights_path, max_batch=3, max_dets=256, warmup_runs=0, flags=zly.FLAG_DUMP_LOGITS)
    assert not any("conv_igemm_multi_kernel" in k for k in p.op_kernels(1))
    res2 = p.detect_batch(list(frames), cap=256)
    for name in names:
        for i in range(3):
            assert np.array_equal(p.tap(name, i), taps[name][i]), (name, i)
    for (d1, n1), (d2, n2) in zip(res, res2):
        assert n1 == n2 and det_fields_equal(d1, d2)
    assert sum(n for _, n in res) > 0
    p.close()


def test_several_single_chain_engines_alternate(weights_path):
    """bench.py's headline configuration: three ZLY_FLAG_SINGLE_CHAIN engines on one GPU, steps alternate between them, each on its
    engine's own stream (the chains overlap), zly_join orders a foreign stream behind a step's NMS before its slabs are consumed.
    Every step's slabs must be the bytes one engine produces for the same frames on its own."""
    n, steps = 16, 9
    sets = [torch.from_numpy(zm.synth_frames(n, 416, 416, seed=80 + i, rects=False)).cuda() for i in range(3)]
    one = zly.Engine(weights_path, max_batch=n, max_dets=64, warmup_runs=1, flags=zly.FLAG_SINGLE_CHAIN)
    want = []
    for k in range(steps):
        one.detect_device(sets[k % 3].data_ptr(), n, 416, 416, tag0=1000 * k)
        want.append(one.read_slabs(n))
    one.close()
    engs = [zly.Engine(weights_path, max_batch=n, max_dets=64, warmup_runs=1, flags=zly.FLAG_SINGLE_CHAIN | zly.FLAG_NO_HEAD_TENSOR) for _ in range(3)]
    sb = engs[0].slab_bytes
    bufs = [torch.zeros(n * sb, dtype=torch.uint8, device="cuda") for _ in range(steps)]
    host = [torch.zeros(n * sb, dtype=torch.uint8).pin_memory() for _ in range(steps)]
    consumer = torch.cuda.Stream()
    torch.cuda.synchronize()
    for k in range(steps):
        e = engs[k % 3]
        e.detect_device(sets[k % 3].data_ptr(), n, 416, 416, d_slabs_ptr=bufs[k].data_ptr(), tag0=1000 * k)     # the engine's own stream
        e.join(consumer.cuda_stream, 0)                                                                         # consumer waits for step k only
        with torch.cuda.stream(consumer):
            host[k].copy_(bufs[k], non_blocking=True)
    consumer.synchronize()
    total = 0
    for k in range(steps):
        got = zly.parse_slabs(host[k].numpy(), n, 64)
        for i in range(n):
            assert int(got[i][0]["frame_tag"]) == 1000 * k + i and int(got[i][0]["n_kept"]) == int(want[k][i][0]["n_kept"])
            assert det_fields_equal(got[i][1], want[k][i][1])
            total += int(got[i][0]["n_kept"])
    assert total > 0
    for e in engs:
        e.close()


def test_streaming_1x1_kernel(weights_path, oracle, monkeypatch):
    """conv1x1_stream_kernel (persistent waves, next pixel group in flight, buffer addressing) against the one-shot 1x1
    kernel: same MFMA order, so bit-identical wherever the one-shot launch does not split K (model.2.cv1 / cv2 with a
    48-channel input / model.4.cv1); ZLY_STREAM_WGS=8 makes every wave loop over many groups, 52x52x3 pixels leave a
    partial last group (hardware range check: reads 0, stores dropped).  Guards the gfx950 store hazard found here: a
    16-byte buffer store with an SGPR soffset followed by a VALU write of its data registers stored garbage in dword 1."""
    frames = zm.synth_frames(3, 416, 416, seed=5, rects=False)
    x = _pre(oracle, frames)
    monkeypatch.setenv("ZLY_NO_STREAM", "1")
    a = zly.Engine(weights_path, max_batch=3, warmup_runs=0, flags=zly.FLAG_NO_FUSION)
    ha = a.forward(x)
    names = ("model.2.cv1", "model.2.cv2", "model.4.cv1")
    ta = {k: [a.tap(k, i) for i in range(3)] for k in names}
    a.close()
    monkeypatch.delenv("ZLY_NO_STREAM")
    monkeypatch.setenv("ZLY_STREAM_MIN_GROUPS", "1")
    for wgs in ("8", "1024"):
        monkeypatch.setenv("ZLY_STREAM_WGS", wgs)
        b = zly.Engine(weights_path, max_batch=3, warmup_runs=0, flags=zly.FLAG_NO_FUSION)
        hb = b.forward(x)
        for k in names:
            for i in range(3):
                assert np.array_equal(b.tap(k, i), ta[k][i]), (wgs, k, i)
        assert np.isfinite(hb).all()
        _assert_bf16_close(hb, ha)
        b.close()


PAIR_TAPS = ("model.2.m.0.cv2", "model.4.m.0.cv2", "model.4.m.1.cv2", "model.15.m.0.cv2")


def _closed_loop_with_dumps(weights_path, w, h, n, x, must_be_resident):
    """an engine under the switches now in the environment, with the debug dumps (the final logits are tappable): every conv of the first and the
    last frame against float64 on the engine's own inputs.  The bottlenecks in `must_be_resident` must really keep their first conv in LDS, so
    that they are checked through their second conv with the ambiguity allowance (tests/closed_loop_ref.py)."""
    e = zly.Engine(weights_path, model_w=w, model_h=h, max_batch=n, warmup_runs=0, flags=zly.FLAG_DUMP_LOGITS)
    lds = lds_resident_from_kernels(e, n)
    assert set(must_be_resident) <= lds, (must_be_resident, lds, e.op_kernels(n))
    head = e.forward(x)
    assert len(check_closed_loop(e, weights_path, (0, n - 1), lds_resident=lds)) == 63
    for i in (0, n - 1):
        check_head_decode(e, head[i], i)
    e.close()


@pytest.mark.parametrize("w,h,n", [(416, 416, 16), (320, 256, 2), (352, 288, 5)])
def test_fused_bottleneck_pairs(weights_path, oracle, monkeypatch, w, h, n):
    """kernels_pair.hip (3x3 -> 3x3 [+ shortcut] with the intermediate map in LDS) against the one-kernel-per-conv path
    and the rounding-emulating oracle.  ZLY_PAIR_MIN_TILES=1 forces the fused kernel onto these small batches; the map
    sizes cover tiles that divide the map (104, 52) and ragged ones (88x72, 44x36, 80x64, 40x32).
    32-channel pairs accumulate in the order of the unfused kernels: bit-identical, all the way to the head tensor, when
    the unfused launch does not split K across waves (batch 16 here; the small batches take the 4-way split-K kernel).
    The 16-channel pair uses one MFMA per tap (the unfused kernel: one per two taps): fp32 sums can differ in the last
    bit before the bf16 rounding, so it is compared at its own output and against the oracle."""
    import yolov8_ref
    monkeypatch.setenv("ZLY_PAIR_MIN_TILES", "1")
    monkeypatch.setenv("ZLY_NO_C2F", "1")                      # this test is about the bottleneck kernel on its own (the C2f kernel contains it)
    frames = zm.synth_frames(n, w, h, seed=31, rects=False)
    x = _pre(oracle, frames, w, h)
    plain = zly.Engine(weights_path, model_w=w, model_h=h, max_batch=n, warmup_runs=0, flags=zly.FLAG_NO_FUSION)
    hp = plain.forward(x)
    tp = {name: [plain.tap(name, i) for i in range(n)] for name in PAIR_TAPS}
    plain.close()

    monkeypatch.setenv("ZLY_PAIR_WIDTHS", "32")
    e = zly.Engine(weights_path, model_w=w, model_h=h, max_batch=n, warmup_runs=0)
    h32 = e.forward(x)
    with pytest.raises(zly.ZlyError):
        e.tap("model.4.m.0.cv1", 0)                           # stays in LDS
    e.tap("model.2.m.0.cv1", 0)                               # this width is not fused in this engine
    for name in PAIR_TAPS[1:2] if n < 16 else PAIR_TAPS:          # small batches: first fused layer only (same input in both engines)
        for i in range(n):
            g = e.tap(name, i)
            if n >= 16:
                assert np.array_equal(g, tp[name][i]), (name, i, float(np.mean(g != tp[name][i])))
            else:
                assert np.abs(g - tp[name][i]).max() <= 2.0 ** -6 * np.abs(g).max() and np.mean(g != tp[name][i]) < 0.05, (name, i)
    if n >= 16:
        assert np.array_equal(h32, hp)
    else:
        _assert_bf16_close(h32, hp)
    e.close()
    _closed_loop_with_dumps(weights_path, w, h, n, x, ("model.4.m.0.cv1",))

    monkeypatch.setenv("ZLY_PAIR_WIDTHS", "16")
    e = zly.Engine(weights_path, model_w=w, model_h=h, max_batch=n, warmup_runs=0)
    h16 = e.forward(x)
    ref = yolov8_ref.load(weights_path, "bf16")
    ref.forward(torch.from_numpy(x))
    for i in range(n):
        g, t = e.tap("model.2.m.0.cv2", i), ref.taps["model.2.m.0.cv2"][i].numpy()
        rng = np.abs(t).max()
        assert np.abs(g - tp["model.2.m.0.cv2"][i]).max() <= 2.0 ** -6 * rng
        assert np.mean(g != tp["model.2.m.0.cv2"][i]) < 0.05
        assert np.abs(g - t).max() <= 2.0 ** -5 * rng
    _assert_bf16_close(h16, hp)
    e.close()
    _closed_loop_with_dumps(weights_path, w, h, n, x, ("model.2.m.0.cv1",))

    # 64-channel pairs (26x26 stage): one shared weight buffer, k order (tap, half) instead of the LDS kernel's (half, tap):
    # same products, other fp32 summation order.  The first such pair sees identical inputs in both engines.
    monkeypatch.setenv("ZLY_PAIR_WIDTHS", "64")
    e = zly.Engine(weights_path, model_w=w, model_h=h, max_batch=n, warmup_runs=0)
    h64 = e.forward(x)
    with pytest.raises(zly.ZlyError):
        e.tap("model.6.m.0.cv1", 0)
    pl = zly.Engine(weights_path, model_w=w, model_h=h, max_batch=n, warmup_runs=0, flags=zly.FLAG_NO_FUSION)
    pl.forward(x)
    for i in range(n):
        g, t = e.tap("model.6.m.0.cv2", i), pl.tap("model.6.m.0.cv2", i)
        assert np.abs(g - t).max() <= 2.0 ** -6 * np.abs(t).max() and np.mean(g != t) < 0.05, (i, np.abs(g - t).max(), np.mean(g != t))
    for name in ("model.6.m.1.cv2", "model.12.m.0.cv2", "model.18.m.0.cv2"):
        g, t = e.tap(name, 0), pl.tap(name, 0)
        assert g.shape == t.shape and np.isfinite(g).all() and _rms(g - t) <= 0.05 * max(_rms(t), 1e-6), name
    _assert_bf16_close(h64, hp)
    e.close(); pl.close()
    _closed_loop_with_dumps(weights_path, w, h, n, x, ("model.6.m.0.cv1",))


C2F_TAPS = ("model.2.cv1", "model.2.m.0.cv2", "model.2.cv2", "model.4.cv1", "model.4.m.0.cv2", "model.4.m.1.cv2", "model.4.cv2",
            "model.15.cv1", "model.15.m.0.cv2", "model.15.cv2")


@pytest.mark.parametrize("w,h,n", [(416, 416, 16), (320, 256, 2), (352, 288, 5), (416, 416, 1)])
def test_fused_c2f_blocks(weights_path, oracle, w, h, n):
    """c2f_kernel (kernels_pair.hip): cv1 -> bottleneck -> cv2 of a C2f block in one launch (model.2, model.15: whole block;
    model.4: front half + back half), every intermediate in LDS, against the one-kernel-per-conv engine and the rounding-
    emulating oracle.  The dumps (ZLY_FLAG_DUMP_LOGITS) expose the LDS-resident intermediates.  32-channel blocks accumulate
    in the order of the unfused kernels: bit-identical taps when the unfused launch does not split K across waves (batch 16);
    the 16-channel block (model.2) uses one MFMA per tap / per 16-channel concat source, so fp32 sums can differ in the last
    bit before the bf16 rounding.  Ragged maps (88x72 .. 40x32) put partial tiles on every edge; model.15.cv1 reads its
    input from two tensors (fused Upsample + Concat)."""
    import yolov8_ref
    frames = zm.synth_frames(n, w, h, seed=33, rects=False)
    x = _pre(oracle, frames, w, h)
    plain = zly.Engine(weights_path, model_w=w, model_h=h, max_batch=n, warmup_runs=0, flags=zly.FLAG_NO_FUSION)
    hp = plain.forward(x)
    tp = {name: [plain.tap(name, i) for i in range(n)] for name in C2F_TAPS}
    plain.close()
    e = zly.Engine(weights_path, model_w=w, model_h=h, max_batch=n, warmup_runs=0, flags=zly.FLAG_DUMP_LOGITS)
    kernels = e.op_kernels(n)
    assert sum("c2f_kernel" in k for k in kernels) == 4, kernels
    hf = e.forward(x)
    with pytest.raises(zly.ZlyError):
        e.tap("model.2.m.0.cv1", 0)                               # stays in LDS even with the dumps
    # ... so the four fused bottlenecks are checked through their second conv, with the ambiguity allowance; every other conv directly
    lds = lds_resident_from_kernels(e, n)
    assert lds == {"model.2.m.0.cv1", "model.4.m.0.cv1", "model.4.m.1.cv1", "model.15.m.0.cv1"}, lds
    assert len(check_closed_loop(e, weights_path, (0, n - 1), lds_resident=lds)) == 63
    for i in (0, n - 1):
        check_head_decode(e, hf[i], i)
    ref = yolov8_ref.load(weights_path, "bf16")
    ref.forward(torch.from_numpy(x))
    tf = {name: [e.tap(name, i) for i in range(n)] for name in C2F_TAPS}           # the fused engine's taps, dumps on
    for name in C2F_TAPS:
        for i in range(n):
            g, t = tf[name][i], tp[name][i]
            _assert_layer_close(g, ref.taps[name][i].numpy(), f"{name}[{i}] vs oracle")
            if n >= 16 and not name.startswith("model.2."):
                assert np.array_equal(g, t), (name, i, float(np.mean(g != t)))
            elif name.startswith("model.2."):          # the first fused block sees identical inputs in both engines: rare last-bit flips only
                assert np.abs(g - t).max() <= 2.0 ** -6 * np.abs(t).max() and np.mean(g != t) < 0.05, (name, i)
            else:                                      # small batches: the unfused engine splits K across waves, flips propagate downstream
                assert np.abs(g - t).max() <= 2.0 ** -5 * np.abs(t).max(), (name, i)
    _assert_bf16_close(hf, hp)
    e.close()
    # without the dumps the LDS-resident intermediates cannot be tapped, the block outputs can, and the results are the same
    e = zly.Engine(weights_path, model_w=w, model_h=h, max_batch=n, warmup_runs=0)
    h2 = e.forward(x)
    assert np.array_equal(h2, hf)
    for name in ("model.2.cv1", "model.15.m.0.cv2", "model.4.m.1.cv2"):
        with pytest.raises(zly.ZlyError):
            e.tap(name, 0)
    for name in ("model.2.cv2", "model.4.cv1", "model.4.m.0.cv2", "model.4.cv2", "model.15.cv2"):
        assert np.array_equal(e.tap(name, n - 1), tf[name][n - 1]), name         # == the block outputs of the engine WITH the dumps (first half of this test)
        _assert_layer_close(e.tap(name, n - 1), ref.taps[name][n - 1].numpy(), name)
    e.close()


def test_four_class_cs16_head(tmp_path, oracle):
    """The reference's CS 1.6 model has 4 classes (constants.h:35-40): head tensor [1, 8, N].  Class branch = one
    16-row MFMA tile with 12 padded rows; decode and NMS must never see the padding."""
    import yolov8_ref
    spec = zm.build_spec("n", 4)
    p = str(tmp_path / "yolov8n_cs16_synth.zlyw")
    zm.write_zlyw(p, spec, zm.synth_weights(spec, seed=10))
    ref = yolov8_ref.load(p, "fp32")
    frames = zm.synth_frames(3, 416, 416, seed=13, rects=False)
    x = _pre(oracle, frames, 416, 416)
    want = ref.forward(torch.from_numpy(x)).numpy()
    assert want.shape == (3, 8, 3549)
    e = zly.Engine(p, dtype=zly.DTYPE_FP32, max_batch=3, max_dets=512, conf_thr=0.5, warmup_runs=0)
    assert e.nc == 4
    got = e.forward(x)
    assert got.shape == want.shape
    scale = max(1.0, float(np.abs(want[:, :4]).max()) / 800.0)
    assert np.abs(got[:, :4] - want[:, :4]).max() <= 4 * FP32_BOX_TOL * scale
    assert np.abs(got[:, 4:] - want[:, 4:]).max() <= 2 * FP32_SCORE_TOL
    e.close()
    e = zly.Engine(p, dtype=zly.DTYPE_BF16, max_batch=3, max_dets=512, conf_thr=0.3, warmup_runs=0)
    got = e.forward(x)
    _assert_bf16_close(got, yolov8_ref.load(p, "bf16").forward(torch.from_numpy(x)).numpy())
    _assert_bf16_close(got, want)
    total = 0
    for f in frames:
        dets, n = e.detect(f, cap=512)
        own = oracle.postprocess(e.head_tensor(0), 416, 416, 0.3, 0.45)
        assert n == len(own) and det_fields_equal(dets, own[:512])
        assert n == 0 or (dets["class_id"][:min(n, 512)] < 4).all()
        total += n
    assert total > 0
    e.close()


def test_one_handle_from_several_host_threads(eng16):
    """The reference calls submitInference from the UDP thread while the monitor thread polls getStatus
    (SURVEY.md section 8b); one zly_engine handle must serialise concurrent callers and give each its own result."""
    import threading
    frames = [zm.synth_frames(1, 416, 416, seed=100 + i, rects=False)[0] for i in range(6)]
    serial = [eng16.detect(f, cap=256) for f in frames]
    errors_before = eng16.stats()["inference_errors"]
    results, errors = {}, []

    def worker(tid):
        try:
            for rep in range(5):
                for i in range(tid, len(frames), 3):
                    results[(tid, rep, i)] = eng16.detect(frames[i], cap=256)
                    eng16.stats()
        except Exception as exc:          # pragma: no cover
            errors.append(exc)

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(3)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors
    for (tid, rep, i), (dets, n) in results.items():
        assert n == serial[i][1] and det_fields_equal(dets, serial[i][0])
    assert eng16.stats()["inference_errors"] == errors_before
