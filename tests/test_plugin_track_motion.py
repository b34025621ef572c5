"""The plugin's ZLY_TRACK_MOTION=1 (host/hip_inference_engine.cpp): every engine enables the tracker's motion model.  CPU-runnable, in the manner
of tests/test_plugin_track.py: tests/cpp/test_plugin_track_motion_stub.cpp compiles the plugin together with a link-time stub of the C ABI that
records every enable (test infrastructure, not a product fallback).  Checked: one zly_track_motion_enable per engine, after that engine's
zly_track_enable, with ZLY_TRACK_BETA / ZLY_TRACK_VMAX or the library's defaults; no call of the motion model while the variable is unset; the
variable refused without ZLY_TRACK=1, and refused when the library lacks the calls.  The last test (gpu) runs the plugin with the variable against
the real library."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "zero-latency-yolo_amd", "_build", "test_plugin_track_motion_stub")


def _run(tmp_path, mode, binary=STUB):
    if not os.path.exists(binary):
        subprocess.run(["make", "-C", ROOT, binary[len(ROOT) + 1:]], check=True, stdout=subprocess.DEVNULL)
    rep_path = tmp_path / "report.txt"
    r = subprocess.run([binary, str(rep_path), mode], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    rep = dict(line.split("=", 1) for line in rep_path.read_text().splitlines())
    log = [rep[f"log[{i}]"] for i in range(sum(k.startswith("log[") for k in rep))]
    return rep, log


def _enables(log):
    return [l for l in log if not l.startswith("submit:")]


def test_motion_is_enabled_once_per_engine_after_tracking_with_the_overrides(tmp_path):
    rep, log = _run(tmp_path, "motion")
    assert rep["init_error"] == "0" and rep["status_tracking"] == "on" and rep["status_motion"] == "on"
    assert _enables(log) == ["enable:0", "motion:0:0.25:0.125", "enable:1", "motion:1:0.25:0.125"]
    assert log[:4] == _enables(log)                                           # all of it before the first frame
    assert rep["callbacks"] == "4" and sum(l.startswith("submit:") for l in log) == 4


def test_without_overrides_the_librarys_defaults_are_passed(tmp_path):
    rep, log = _run(tmp_path, "defaults")
    assert rep["init_error"] == "0" and _enables(log) == ["enable:0", "motion:0:0.5:0.25", "enable:1", "motion:1:0.5:0.25"]


def test_switch_off_calls_nothing_of_the_motion_model(tmp_path):
    rep, log = _run(tmp_path, "plain")
    assert rep["init_error"] == "0" and rep["status_tracking"] == "on" and rep["status_motion"] == "off"
    assert rep["motion_calls"] == "0" and _enables(log) == ["enable:0", "enable:1"] and rep["callbacks"] == "4"


def test_refused_without_zly_track(tmp_path):
    rep, log = _run(tmp_path, "notrack")
    assert rep["init_error"] == "2" and rep["motion_calls"] == "0" and not log          # INVALID_ARGUMENT: ZLY_TRACK_MOTION needs ZLY_TRACK=1


def test_refused_when_the_library_lacks_the_calls(tmp_path):
    rep, log = _run(tmp_path, "motion", STUB + "_nosym")
    assert rep["init_error"] == "300" and not log                                       # SYSTEM_ERROR: the engine library has no zly_track_motion_enable
    rep, log = _run(tmp_path, "plain", STUB + "_nosym")
    assert rep["init_error"] == "0" and _enables(log) == ["enable:0", "enable:1"] and rep["callbacks"] == "4"


@pytest.mark.gpu
def test_plugin_enables_the_model_on_the_real_engine(tmp_path, weights_path):
    """the plugin with ZLY_TRACK=1 ZLY_TRACK_MOTION=1 against libzly.so, where the weakly referenced calls must resolve: three clients send the same
    frame three times each; a box that stands still is predicted where it is, so each client sees its boxes born as ids 1..n and matched to the
    same ids afterwards, exactly as without the model"""
    import json
    import struct

    import numpy as np

    import zly_model as zm
    binary = os.path.join(ROOT, "zero-latency-yolo_amd", "_build", "test_hip_engine")
    if not os.path.exists(binary):
        subprocess.run(["make", "-C", ROOT, "host"], check=True, stdout=subprocess.DEVNULL)
    frame = np.ascontiguousarray(zm.synth_frames(1, 800, 600, seed=5, rects=False)[0])
    fpath, out = tmp_path / "frames.bin", tmp_path / "out.json"
    with open(fpath, "wb") as f:
        f.write(struct.pack("<I", 9))
        for _ in range(9):
            f.write(struct.pack("<HHI", frame.shape[1], frame.shape[0], frame.nbytes))
            f.write(frame.tobytes())
    env = dict(os.environ, ZLY_TRACK="1", ZLY_TRACK_MOTION="1", ZLY_TRACK_STREAMS="4", ZLY_MAX_BATCH="1", ZLY_ENGINES_PER_GPU="2")
    r = subprocess.run([binary, weights_path, str(fpath), str(out)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr
    j = json.loads(out.read_text())
    assert j["init"] == 0 and [x["frame_id"] for x in j["results"]] == list(range(9))
    assert j["status"]["tracking"] == "on" and j["status"]["track_motion"] == "on" and j["status"]["inference_errors"] == "0"
    n = len(j["results"][0]["dets"])
    assert 3 <= n <= 64
    for x in j["results"]:
        assert [d[6] for d in x["dets"]] == list(range(1, n + 1)), x["frame_id"]
    # ... and refused without ZLY_TRACK=1 by the real plugin too
    env = dict(os.environ, ZLY_TRACK_MOTION="1", ZLY_MAX_BATCH="1")
    env.pop("ZLY_TRACK", None)
    r = subprocess.run([binary, weights_path, str(fpath), str(out)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 4 and json.loads(out.read_text())["init"] == 2 and "ZLY_TRACK_MOTION needs ZLY_TRACK=1" in r.stderr
