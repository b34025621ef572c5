"""The plugin's ZLY_CROP=WxH (host/hip_inference_engine.cpp): every request is detected in the centred W x H window of its frame and its boxes
are mapped back to fractions of the request frame.  CPU-runnable: tests/cpp/test_plugin_crop_stub.cpp compiles the plugin together with a
link-time stub of the C ABI that records the frame view it is handed and answers one fixed box per frame (test infrastructure, not a product
fallback).  Checked: the window arithmetic, the even rounding for YUV input, the small-request rule, the box map in single fp32 operations."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "zero-latency-yolo_amd", "_build", "test_plugin_crop_stub")
W = H = 416
BOX = np.array([0.25, 0.625, 0.1, 0.3], np.float32)         # what the stub engine detects, as fractions of what it was handed
SIZES = [(1920, 1080), (1918, 1082), (1250, 838), (416, 416), (418, 416), (400, 1080), (1920, 300), (100, 62)]


def _run(tmp_path, fmt):
    if not os.path.exists(STUB):
        subprocess.run(["make", "-C", ROOT, STUB[len(ROOT) + 1:]], check=True, stdout=subprocess.DEVNULL)
    rep_path = tmp_path / "report.txt"
    r = subprocess.run([STUB, str(rep_path), fmt], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return dict(line.split("=", 1) for line in rep_path.read_text().splitlines())


def _bits(x):
    return int(np.float32(x).view(np.uint32))


@pytest.mark.parametrize("fmt", ["bgr", "nv12"])
def test_crop_window_view_and_box_map(tmp_path, fmt):
    rep = _run(tmp_path, fmt)
    yuv = fmt == "nv12"
    for bad in ("416", "416x", "x416", "0x416", "416x-2", "416x416x3", "abc"):
        assert rep[f"bad_crop[{bad}]"] == "2", bad                      # INVALID_ARGUMENT from initialize()
    if yuv:
        assert rep["odd_crop_yuv"] == "2"
    assert rep["status_crop"] == "416x416"
    assert rep["callbacks"] == str(len(SIZES)) and rep["logged"] == str(len(SIZES)) and rep["status_errors"] == "2"
    for i, (fw, fh) in enumerate(SIZES):
        f = [int(x) for x in rep[f"req[{i}]"].split(",")]
        assert f[:2] == [fw, fh] and f[15] == i
        is_view, w, h, pix, off0, off1, pitch0, pitch1, buf_bytes = f[2:11]
        got = f[11:15]
        frame_bytes = fw * fh * 3 // 2 if yuv else fw * fh * 3
        assert pix == (1 if yuv else 0)
        if fw < W or fh < H:
            # smaller than the window on either axis: detected whole, through the plain call; the boxes are the engine's
            assert (is_view, w, h, buf_bytes) == (0, fw, fh, frame_bytes), (fw, fh)
            assert got == [_bits(b) for b in BOX]
            continue
        x0, y0 = (fw - W) // 2, (fh - H) // 2
        if yuv:
            x0, y0 = x0 & ~1, y0 & ~1                                  # rounded down to even
        assert (is_view, w, h, buf_bytes) == (1, W, H, frame_bytes), (fw, fh)
        if yuv:
            assert (pitch0, pitch1) == (fw, fw)
            assert off0 == y0 * fw + x0 and off1 == fw * fh + (y0 // 2) * fw + (x0 // 2) * 2
        else:
            assert pitch0 == 3 * fw and off0 == y0 * 3 * fw + 3 * x0
        # x' = (x*W + x0) / width, w' = w*W / width, and likewise for y: single fp32 operations
        f32 = np.float32
        want = [(BOX[0] * f32(W) + f32(x0)) / f32(fw), (BOX[1] * f32(H) + f32(y0)) / f32(fh), BOX[2] * f32(W) / f32(fw), BOX[3] * f32(H) / f32(fh)]
        assert all(isinstance(v, np.float32) for v in want)
        assert got == [_bits(v) for v in want], (fw, fh)
    # the centre of the window maps to the centre of the frame when the margins are even (1920 x 1080: 752, 332)
    f = [int(x) for x in rep["req[0]"].split(",")]
    assert f[6] == (332 * 1920 + 752) * (1 if yuv else 3)
