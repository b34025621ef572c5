"""The plugin's resize modes (host/hip_inference_engine.cpp: ZLY_RESIZE=stretch / letterbox / area / letterbox_area).  CPU-runnable:
tests/cpp/test_plugin_area_stub.cpp compiles the plugin together with a link-time stub of the C ABI whose zly_create records the zly_config it is
handed (test infrastructure, not a product fallback).  Checked: each of the four names gives every engine the expected flags, near misses are
refused by initialize() with a message that names the four modes, and getStatus() reports the mode."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "zero-latency-yolo_amd", "_build", "test_plugin_area_stub")
FLAG_LETTERBOX, FLAG_AREA = 32, 64           # include/zly.h
MODE_BITS = FLAG_LETTERBOX | FLAG_AREA
INVALID_ARGUMENT = 2


def _report(tmp_path):
    if not os.path.exists(STUB):
        subprocess.run(["make", "-C", ROOT, STUB[len(ROOT) + 1:]], check=True, stdout=subprocess.DEVNULL)
    rep_path = tmp_path / "report.txt"
    env = {k: v for k, v in os.environ.items() if not k.startswith("ZLY_")}
    r = subprocess.run([STUB, str(rep_path)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr
    return dict(line.split("=", 1) for line in rep_path.read_text().splitlines())


def test_resize_names_flags_and_status(tmp_path):
    rep = _report(tmp_path)
    want = {"": (0, "stretch"), "stretch": (0, "stretch"), "letterbox": (FLAG_LETTERBOX, "letterbox"), "area": (FLAG_AREA, "area"),
            "letterbox_area": (FLAG_LETTERBOX | FLAG_AREA, "letterbox_area")}
    for name, (bits, status) in want.items():
        code, creates, any_flags, all_flags, reported = rep[f"mode[{name}]"].split(",")
        assert int(code) == 0 and int(creates) >= 1, (name, rep[f"mode[{name}]"])
        assert int(any_flags) & MODE_BITS == bits and int(all_flags) & MODE_BITS == bits, (name, any_flags, all_flags)      # every engine, the same mode
        assert reported == status, (name, reported)


def test_near_misses_are_refused(tmp_path):
    rep = _report(tmp_path)
    for name in ("Area", "letterbox-area", "area_letterbox", "AREA", "area "):
        code, creates, _, _, reported = rep[f"mode[{name}]"].split(",")
        assert int(code) == INVALID_ARGUMENT and int(creates) == 0 and reported == "-", (name, rep[f"mode[{name}]"])
        msg = rep[f"message[{name}]"]
        assert "ZLY_RESIZE" in msg and all(m in msg for m in ("stretch", "letterbox", "area", "letterbox_area")) and name in msg, msg
