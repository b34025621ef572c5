"""The plugin's ZLY_TRACK=1 (host/hip_inference_engine.cpp): a client's frames all go to engine client_id % engines, as one stream of that engine.
CPU-runnable: tests/cpp/test_plugin_track_stub.cpp compiles the plugin together with a link-time stub of the C ABI that records (engine, stream) of
every submit and every reset (test infrastructure, not a product fallback).  Checked: engine affinity by client id, stable stream slots,
least-recently-used reuse with a reset before the new client's first frame, initialize() failing when the library lacks the tracking calls, and
no tracking call at all while ZLY_TRACK is unset.  The last test (gpu) runs the plugin with ZLY_TRACK=1 against the real library."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "zero-latency-yolo_amd", "_build", "test_plugin_track_stub")
CLIENTS = [0, 1, 2, 3, 0, 1, 4, 0, 2, 5, 5, 1]


def _run(tmp_path, mode, binary=STUB):
    if not os.path.exists(binary):
        subprocess.run(["make", "-C", ROOT, binary[len(ROOT) + 1:]], check=True, stdout=subprocess.DEVNULL)
    rep_path = tmp_path / "report.txt"
    r = subprocess.run([binary, str(rep_path), mode], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    rep = dict(line.split("=", 1) for line in rep_path.read_text().splitlines())
    log = [rep[f"log[{i}]"] for i in range(sum(k.startswith("log[") for k in rep))]
    seen = [tuple(int(x) for x in rep[f"seen[{i}]"].split(":")) for i in range(sum(k.startswith("seen[") for k in rep))]
    return rep, log, seen


def test_clients_keep_their_engine_and_stream(tmp_path):
    rep, log, seen = _run(tmp_path, "on")
    assert rep["init_error"] == "0" and rep["status_tracking"] == "on"
    # both engines track: ZLY_TRACK_STREAMS slots, 64 track slots, ZLY_TRACK_MAX_LOST, and a slab capacity the tracker accepts (the plugin's default is 256)
    assert log[:2] == ["enable:0:2:64:9:64", "enable:1:2:64:9:64"]
    assert log[2:] == [
        "submit:0:0:1", "submit:1:0:1", "submit:0:1:1", "submit:1:1:1",       # clients 0, 1, 2, 3: engine = client % 2, the next free slot
        "submit:0:0:1", "submit:1:0:1",                                       # clients 0, 1 again: their slots
        "reset:0:1:0", "submit:0:1:1",                                        # client 4: engine 0 is full; client 2's slot was used longest ago: reset, then its first frame
        "submit:0:0:1",                                                       # client 0 keeps slot 0
        "reset:0:1:0", "submit:0:1:1",                                        # client 2 is a new client now: client 4's slot, reset
        "reset:1:1:0", "submit:1:1:1", "submit:1:1:1",                        # client 5 takes client 3's slot on engine 1, and keeps it
        "submit:1:0:1",                                                       # client 1 still has slot 0
    ]
    # every request came back, in submission order, with the track id of its engine and stream; the malformed one failed alone and took no slot
    assert rep["callbacks"] == str(len(CLIENTS)) and rep["status_errors"] == "1" and rep["streams_in_use"] == "4"
    want = [100 * (int(l.split(":")[1]) + 1) + int(l.split(":")[2]) for l in log[2:] if l.startswith("submit")]
    assert seen == list(zip(CLIENTS, want))


def test_switch_off_calls_nothing_of_the_tracker(tmp_path):
    rep, log, seen = _run(tmp_path, "off")
    assert rep["init_error"] == "0" and rep["status_tracking"] == "off" and rep["tracked_calls"] == "0" and rep["streams_in_use"] == "0"
    assert len(log) == len(CLIENTS) and all(l.startswith("submit:") and l.endswith(":-1:0") for l in log)
    assert [int(l.split(":")[1]) for l in log] == [i % 2 for i in range(len(CLIENTS))]          # round robin over the engines, whatever the client
    assert rep["callbacks"] == str(len(CLIENTS)) and [c for c, _ in seen] == CLIENTS and not any(t for _, t in seen)


def test_initialize_fails_without_the_tracking_symbols(tmp_path):
    rep, log, _ = _run(tmp_path, "on", STUB + "_nosym")
    assert rep["init_error"] == "300" and not log                            # SYSTEM_ERROR: the engine library has no zly_submit_view_tracked
    rep, log, _ = _run(tmp_path, "off", STUB + "_nosym")
    assert rep["init_error"] == "0" and rep["callbacks"] == str(len(CLIENTS))


@pytest.mark.gpu
def test_plugin_tracks_on_the_real_engine(tmp_path, weights_path):
    """the plugin with ZLY_TRACK=1 against libzly.so: three clients send the same frame three times each; every client is a stream of its own
    (two of them on one engine), so each sees its boxes born as ids 1..n and matched to the same ids afterwards (IoU 1 with themselves)"""
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
    env = dict(os.environ, ZLY_TRACK="1", ZLY_TRACK_STREAMS="4", ZLY_MAX_BATCH="1", ZLY_ENGINES_PER_GPU="2")
    r = subprocess.run([binary, weights_path, str(fpath), str(out)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr
    j = json.loads(out.read_text())
    assert j["init"] == 0 and [x["frame_id"] for x in j["results"]] == list(range(9))
    assert j["status"]["tracking"] == "on" and j["status"]["track_streams_in_use"] == "3" and j["status"]["inference_errors"] == "0"
    n = len(j["results"][0]["dets"])
    assert 3 <= n <= 64
    for x in j["results"]:                                      # the driver's clients are 1000 + frame % 3
        assert x["client_id"] == 1000 + x["frame_id"] % 3
        assert [d[6] for d in x["dets"]] == list(range(1, n + 1)), x["frame_id"]
        assert [d[:6] for d in x["dets"]] == [d[:6] for d in j["results"][0]["dets"]]
