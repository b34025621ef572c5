"""CPU tests of the drop-in boundary: libzly.so loads, exports exactly what include/zly.h declares,
struct layouts match the reference's Detection, and the engine fails loudly without a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import zly

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "zly.h")).read()


def test_library_exports_every_declared_symbol():
    lib = zly.load_library()
    declared = set(re.findall(r"\b(zly_[a-z0-9_]+)\s*\(", _header()))
    declared -= {"zly_slab_bytes(e)"}
    assert declared == set(zly.SYMBOLS), declared ^ set(zly.SYMBOLS)
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.zly_version().startswith(b"zly-hip")


def test_detection_layout_matches_reference_types_h():
    # reference src/common/types.h:16-26: box@0, confidence@16, class_id@20, track_id@24, timestamp@32, sizeof 40
    d = zly.DET_DTYPE
    assert d.itemsize == 40
    assert [d.fields[k][1] for k in ("x", "y", "w", "h", "confidence", "class_id", "track_id", "timestamp")] == [0, 4, 8, 12, 16, 20, 24, 32]
    assert zly.SLAB_HDR_DTYPE.itemsize == 16


def test_detection_layout_against_the_reference_header_itself(tmp_path):
    """tests/golden/reference_abi.json is what the compiler reports for the reference's own src/common/types.h and result.h
    (tests/cpp/abi_reference_probe.cpp, built against them by tests/golden/make_abi_golden.py): sizeof / alignof / offsetof of
    zero_latency::Detection and the zero_latency::ErrorCode values.  A translation unit with include/zly.h static_asserts zly_det and
    the ZLY_* return codes against that record: the compiler checks the header, not a second table of numbers."""
    import json
    import subprocess
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_abi.json")))
    det, state = ref["Detection"], ref["GameState"]["sizeof_member"]
    fields = {"box": "x", "box.x": "x", "box.y": "y", "box.width": "w", "box.height": "h", "confidence": "confidence",
              "class_id": "class_id", "track_id": "track_id", "timestamp": "timestamp"}
    codes = {"OK": "ZLY_OK", "INVALID_ARGUMENT": "ZLY_ERR_INVALID_ARGUMENT", "NOT_INITIALIZED": "ZLY_ERR_NOT_INITIALIZED",
             "INFERENCE_ERROR": "ZLY_ERR_INFERENCE", "MODEL_NOT_FOUND": "ZLY_ERR_MODEL_NOT_FOUND", "MODEL_LOAD_FAILED": "ZLY_ERR_MODEL_LOAD",
             "INVALID_INPUT": "ZLY_ERR_INVALID_INPUT", "SYSTEM_ERROR": "ZLY_ERR_SYSTEM"}
    assert set(det["offsetof"]) == set(fields) and set(ref["ErrorCode"]) == set(codes)
    lines = ["#include <cstddef>", '#include "zly.h"',
             f'static_assert(sizeof(zly_det) == {det["sizeof"]}, "sizeof(Detection)");',
             f'static_assert(alignof(zly_det) == {det["alignof"]}, "alignof(Detection)");',
             f'static_assert(sizeof(((zly_det*)nullptr)->class_id) == {det["sizeof_member"]["class_id"]}, "class_id width");',
             f'static_assert(sizeof(((zly_det*)nullptr)->timestamp) == {det["sizeof_member"]["timestamp"]}, "timestamp width");',
             # GameState: the members the plugin fills (frame_id, timestamp, detections) have the reference's widths
             f'static_assert({state["frame_id"]} == 4 && {state["timestamp"]} == 8 && {state["detections_element"]} == sizeof(zly_det), "GameState");']
    lines += [f'static_assert(offsetof(zly_det, {f}) == {det["offsetof"][k]}, "{k}");' for k, f in fields.items()]
    lines += [f'static_assert({c} == {ref["ErrorCode"][k]}, "ErrorCode::{k}");' for k, c in codes.items()]
    tu = tmp_path / "abi_vs_reference.cpp"
    tu.write_text("\n".join(lines) + "\nint main() { return 0; }\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(tu)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    # the plugin's compat header re-declares the same record (the reference's headers do not compile as a whole): same layout as zly_det
    compat = open(os.path.join(ROOT, "zero-latency-yolo_amd", "host", "hip_inference_engine.cpp")).read()
    assert "static_assert(sizeof(zly_det) == sizeof(Detection)" in compat


def test_error_codes_match_reference_result_h():
    h = _header()
    for name, val in (("ZLY_ERR_NOT_INITIALIZED", 3), ("ZLY_ERR_INFERENCE", 200), ("ZLY_ERR_MODEL_NOT_FOUND", 201),
                      ("ZLY_ERR_MODEL_LOAD", 202), ("ZLY_ERR_INVALID_INPUT", 203), ("ZLY_ERR_SYSTEM", 300)):
        assert re.search(rf"#define\s+{name}\s+{val}\b", h), name


def test_default_config_is_the_reference_config():
    lib = zly.load_library()
    cfg = zly.Config()
    lib.zly_default_config(C.byref(cfg))
    assert (cfg.model_w, cfg.model_h) == (416, 416)                    # configs/server.json:30-31
    assert abs(cfg.conf_thr - 0.5) < 1e-7 and abs(cfg.iou_thr - 0.45) < 1e-7   # configs/server.json:7-8
    assert cfg.warmup_runs == 3                                       # onnx_engine.cpp:919-954


def test_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(zly.ZlyError) as ei:
        zly.Engine()
    assert ei.value.code == zly.ERR_SYSTEM and "no CPU fallback" in ei.value.message


def test_bad_arguments_are_rejected_before_touching_the_device():
    lib = zly.load_library()
    cfg = zly.Config()
    lib.zly_default_config(C.byref(cfg))
    cfg.model_w = 417
    h = C.c_void_p()
    assert lib.zly_create(C.byref(cfg), C.byref(h)) == zly.ERR_INVALID_ARGUMENT
    assert lib.zly_detect(None, None, 0, 0, 0, None, 0, None) == zly.ERR_NOT_INITIALIZED
    assert lib.zly_slab_bytes(None) == 0


def test_parse_slabs():
    cap = 4
    sb = 16 + cap * 40
    raw = np.zeros(2 * sb, dtype=np.uint8)
    hdr = raw[:16].view(zly.SLAB_HDR_DTYPE); hdr["n_kept"] = 2; hdr["frame_tag"] = 7
    raw[sb:sb + 16].view(zly.SLAB_HDR_DTYPE)["n_kept"] = 9            # overflowed slab: only cap stored
    out = zly.parse_slabs(raw, 2, cap)
    assert len(out[0][1]) == 2 and out[0][0]["frame_tag"] == 7 and len(out[1][1]) == cap
