"""csrc/frame_rules.h on its own: tests/cpp/test_frame_rules.cpp includes the header and nothing of the engine, walks the case families of
tests/frame_rules_cases.py and checks the invariants that need no recording (the format table, tight view = frame bytes, crops fit their
surface and compose, the tight copy of a crop is a slice of the surface's, every refusal).  It prints one line per failed check."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TARGET = "zero-latency-yolo_amd/_build/test_frame_rules"


def test_frame_rules_standalone():
    path = os.path.join(ROOT, TARGET)
    if not os.path.exists(path):
        subprocess.run(["make", "-C", ROOT, TARGET], check=True, stdout=subprocess.DEVNULL)
    r = subprocess.run([path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert " checks, 0 failed" in r.stdout
