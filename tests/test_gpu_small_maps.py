"""Every kernel on the smallest and thinnest maps a model size allows (run on the MI355X box: pytest -m gpu).  zly_create takes any model size whose
sides are positive multiples of 32; the rest of the suite stops at 64 x 64 / 96 x 64, and runs those without fusion, on the fp32 engine or at batch 1,
where every conv plans to the direct kernel.  tests/small_map_cases.py lists the shapes (a side of 32: one-row, one-column and 1 x 1 maps), the
configurations that send them through the throughput kernels, and the coverage that is expected of them.

Nothing here has a tolerance of its own: per element against float64 on the engine's own tapped inputs with the bound of tests/closed_loop_ref.py
(C_ACC, C_ACC_FP32_ENGINE, DECODE_*_TOL), everything else equality of bytes -- the "images" tap against bf16(u8 / 255) of the oracle's preprocess, the
detections against the oracle's post-processing of the engine's own head tensor, the production-flags engine's slabs against the dump engine's.  The
confidence threshold of every shape comes from the case table (chosen on the CPU from the oracle's head), and every checked frame must have at least
MIN_CANDIDATES anchors above it, so that no comparison of detections is one of empty lists.

test_coverage_is_recorded builds kernel family -> the maps below its smallest tile on which a case reached it, from op_kernels of every engine of this
module, asserts it against MUST_REACH / CANNOT_REACH / MUST_SPAN of the case table and prints it."""
import numpy as np
import pytest
import torch

import small_map_cases as sm
import zly
import zly_model as zm
from batch_sweep_ref import same_slab
from closed_loop_ref import check_closed_loop, check_head_decode, lds_resident_from_kernels
from oracle_lib import det_fields_equal

pytestmark = pytest.mark.gpu

CAP = 128
PROD_FLAGS = zly.FLAG_NO_HEAD_TENSOR | zly.FLAG_ASYNC_NMS
FLAG = {"NO_FUSION": zly.FLAG_NO_FUSION, "DUMP_LOGITS": zly.FLAG_DUMP_LOGITS, "ASYNC_NMS": zly.FLAG_ASYNC_NMS}
RECORD = {}               # case_id -> ({family: maps below its smallest tile}, {family: maps one smallest tile spans in an axis}, launch table)


@pytest.fixture(scope="module")
def model_paths(weights_path, tmp_path_factory):
    spec = zm.build_spec("s")
    p = str(tmp_path_factory.mktemp("small_maps") / "yolov8s_synth.zlyw")
    zm.write_zlyw(p, spec, zm.synth_weights(spec, seed=9))
    return {"n": weights_path, "s": p}


def _as_held(x):
    """what the bf16 front kernels hold for a preprocessed frame: bf16(u8 / 255)"""
    return torch.from_numpy(x).to(torch.bfloat16).to(torch.float32).numpy()


def _engine(monkeypatch, model_paths, case, flags=None, warmup_runs=0):
    """the case's engine (its switches are read once, at create) and what its launch table reaches; flags: instead of the configuration's"""
    (w, h), cfg = case
    scale, dtype, flag_names, env, n, _ = sm.CONFIGS[cfg]
    with monkeypatch.context() as m:
        for k, v in env.items():
            m.setenv(k, v)
        e = zly.Engine(model_paths[scale], model_w=w, model_h=h, conf_thr=sm.CONF_THR[(scale, w, h)], max_batch=n, max_dets=CAP, warmup_runs=warmup_runs,
                       dtype=zly.DTYPE_FP32 if dtype == "fp32" else zly.DTYPE_BF16, flags=sum(FLAG[f] for f in flag_names) if flags is None else flags)
    kern = e.op_kernels(n)
    RECORD[sm.case_id(case) + ("" if flags is None else "-production-flags")] = sm.reached([o["name"] for o in e.ops()], kern, w, h, n) + (kern,)
    return e


def _check_frames(e, oracle, case, path, frames_idx, x_held, lds, results):
    """the closed loop on the engine's taps of the last detect call, the head decode, and the detections against the oracle's post-processing of the
    engine's own head tensor; results[i] = (detections, count) of frame i"""
    (w, h), cfg = case
    scale = sm.CONFIGS[cfg][0]
    thr = sm.CONF_THR[(scale, w, h)]
    assert len(check_closed_loop(e, path, frames_idx, lds_resident=lds, first_input=x_held)) == len(zm.build_spec(scale).convs)
    for i in frames_idx:
        head = e.head_tensor(i)
        check_head_decode(e, head, i)
        assert head.shape[1] == sm.n_anchors(w, h)
        assert sm.candidates(head, thr) >= sm.MIN_CANDIDATES, (i, sm.candidates(head, thr))
        want = oracle.postprocess(head, w, h, conf_thr=thr)
        dets, count = results[i]
        assert len(want) >= 1
        assert count == len(want) and det_fields_equal(dets, want[:CAP]), (i, count, len(want))


@pytest.mark.parametrize("case", [c for c in sm.CASES if sm.CONFIGS[c[1]][5] == "forward+batch"], ids=sm.case_id)
def test_forward_then_detect_batch(model_paths, oracle, monkeypatch, case):
    (w, h), cfg = case
    scale, dtype, _, env, n, _ = sm.CONFIGS[cfg]
    path = model_paths[scale]
    fusion = dtype == "bf16" and "NO_FUSION" not in sm.CONFIGS[cfg][2]
    frames = sm.frames_of(n, w, h)
    x = np.stack([oracle.preprocess(f, w, h)[1] for f in frames])
    held = x if dtype == "fp32" else _as_held(x)
    e = _engine(monkeypatch, model_paths, case)
    kn = " | ".join(e.op_kernels(n))
    if "ZLY_SPPF_FUSED" in env:                                   # taken where the map is 3 x 3 or more, the pool kernels where a side is below 3
        assert ("sppf_fused_kernel" in kn) == (min(sm.maps(w, h)[2]) >= 3), kn
        assert ("sppf_pool" in kn) != ("sppf_fused_kernel" in kn), kn
    if cfg == "h":
        assert "(+ box conv in k-step order" in kn, kn
    if cfg in ("d1", "d4"):
        assert kn.count("conv_igemm_multi_kernel") == 2, kn
    lds = lds_resident_from_kernels(e, n) if fusion else ()
    # 1. zly_forward: every conv from the "images" tap on
    head = e.forward(x)
    for i in range(n):
        assert np.array_equal(e.tap("images", i), held[i])
    assert len(check_closed_loop(e, path, range(n), lds_resident=lds)) == len(zm.build_spec(scale).convs)
    for i in range(n):
        check_head_decode(e, head[i], i)
    # 2. zly_detect_batch on the same engine: the front kernels, the tail's candidates, the NMS
    res = e.detect_batch(list(frames), cap=CAP)
    assert len(res) == n
    _check_frames(e, oracle, case, path, range(n), held, lds, res)
    e.close()


@pytest.mark.parametrize("case", [c for c in sm.CASES if sm.CONFIGS[c[1]][5] == "device"], ids=sm.case_id)
def test_full_batch_of_tiny_frames(model_paths, oracle, monkeypatch, case):
    """64 frames through zly_detect_device with what production selects on its own (no switches): frames 0 and 63 per element, and the slabs of an engine
    with the production flags (no head tensor, deferred NMS, graphs on) must equal the dump engine's at every frame"""
    (w, h), cfg = case
    scale, _, _, _, n, _ = sm.CONFIGS[cfg]
    path = model_paths[scale]
    frames = sm.frames_of(n, w, h)
    d = torch.from_numpy(frames).cuda()
    torch.cuda.synchronize()
    e = _engine(monkeypatch, model_paths, case, warmup_runs=1)
    lds = lds_resident_from_kernels(e, n)
    e.detect_device(d.data_ptr(), n, w, h)
    slabs = e.read_slabs(n)                                       # joins the deferred NMS
    ends = [0, n - 1]
    held = _as_held(np.stack([oracle.preprocess(frames[i], w, h)[1] for i in ends]))
    results = {i: (slabs[i][1], int(slabs[i][0]["n_kept"])) for i in ends}
    _check_frames(e, oracle, case, path, ends, held, lds, results)
    assert [int(hd["frame_tag"]) for hd, _ in slabs] == list(range(n))
    assert min(int(hd["n_candidates"]) for hd, _ in slabs) >= sm.MIN_CANDIDATES
    e.close()
    p = _engine(monkeypatch, model_paths, case, flags=PROD_FLAGS, warmup_runs=1)
    p.detect_device(d.data_ptr(), n, w, h)
    got = p.read_slabs(n)
    p.close()
    bad = [(i, int(got[i][0]["n_kept"]), int(slabs[i][0]["n_kept"])) for i in range(n) if not same_slab(got[i], slabs[i])]
    assert not bad, f"(frame, n_kept production / dump) of {len(bad)} differing slabs: {bad[:16]}"


def test_coverage_is_recorded(model_paths, monkeypatch):
    for case in sm.CASES:                                         # a case this process has not run (a -k selection): its launch table alone
        if sm.case_id(case) not in RECORD:
            _engine(monkeypatch, model_paths, case).close()
    below, spanned = {}, {}
    for cid, (b, s, _) in RECORD.items():
        for fam, ms in b.items():
            below.setdefault(fam, {})[cid] = ms
        for fam, ms in s.items():
            spanned.setdefault(fam, {})[cid] = ms
    fmt = lambda got: "; ".join(f"{cid} ({' '.join(ms)})" for cid, ms in sorted(got.items()))
    print("\nkernel family: case (maps below the family's smallest tile on which the case reaches it)")
    for fam in sm.FAMILIES:
        if fam in sm.CANNOT_REACH:
            print(f"  {fam}: on no map below its smallest tile -- {sm.CANNOT_REACH[fam]}")
            print(f"      on maps that one smallest tile spans in an axis: {fmt(spanned.get(fam, {})) or 'none'}")
        else:
            print(f"  {fam}: {fmt(below.get(fam, {})) or 'NOT REACHED'}")
    print("launches per case (kernel x ops):")
    for cid in sorted(RECORD):
        names = [k for k in RECORD[cid][2] if not k.startswith("(")]
        print(f"  [{cid}] " + "; ".join(f"{k} x {names.count(k)}" for k in dict.fromkeys(names)))
    assert set(sm.MUST_REACH) | set(sm.CANNOT_REACH) == set(sm.FAMILIES) and not set(sm.MUST_REACH) & set(sm.CANNOT_REACH)
    bad = []
    for fam, why in sm.CANNOT_REACH.items():
        if below.get(fam):
            bad.append(f"{fam} is listed as kept off every map below its smallest tile ({why}) but is reached there: {fmt(below[fam])} -- add a shape for it")
    for what, want, got in (("below its smallest tile", sm.MUST_REACH, below), ("spanned by one smallest tile", sm.MUST_SPAN, spanned)):
        for fam, cases in want.items():
            for cid, ms in cases.items():
                have = got.get(fam, {}).get(cid, [])
                if not set(ms) <= set(have):
                    bad.append(f"{fam} must be reached by {cid} on maps {ms} ({what}); it is reached on {have}")
    assert not bad, "\n  ".join(["coverage differs from tests/small_map_cases.py:"] + bad)
