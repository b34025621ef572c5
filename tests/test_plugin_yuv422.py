"""The plugin's packed YUV 4:2:2 input (host/hip_inference_engine.cpp: ZLY_INPUT_FORMAT=yuy2 / uyvy / yuy2_709 / uyvy_709).  CPU-runnable:
tests/cpp/test_plugin_yuv422_stub.cpp compiles the plugin together with a link-time stub of the C ABI that records the frame or view it is handed
(test infrastructure, not a product fallback).  Checked: the four names parse and getStatus() reports them, near misses are refused, a request of the
wrong size fails alone, and ZLY_CROP follows the format's x-only evenness rule: W even, any H; x0 rounded down to even, y0 as it is."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "zero-latency-yolo_amd", "_build", "test_plugin_yuv422_stub")
W, H = 416, 415
UYVY_709 = 13
SIZES = [(1920, 1081), (1918, 1081), (1250, 838), (416, 415), (400, 1081), (1920, 301)]
N_BAD = 5


def _report(tmp_path):
    if not os.path.exists(STUB):
        subprocess.run(["make", "-C", ROOT, STUB[len(ROOT) + 1:]], check=True, stdout=subprocess.DEVNULL)
    rep_path = tmp_path / "report.txt"
    r = subprocess.run([STUB, str(rep_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return dict(line.split("=", 1) for line in rep_path.read_text().splitlines())


def test_format_names_sizes_and_crop_rule(tmp_path):
    rep = _report(tmp_path)
    for name in ("yuy2", "uyvy", "yuy2_709", "uyvy_709"):
        assert rep[f"format[{name}]"] == f"0,{name}"
    for name in ("yuyv", "uyvy_601", "YUY2"):
        assert rep[f"format[{name}]"] == "2,-"                        # INVALID_ARGUMENT from initialize()
    assert rep["crop[415x416]"] == "2" and rep["crop[415x415]"] == "2"       # an odd window width is refused ...
    assert rep["crop[416x415]"] == "0" and rep["crop[2x1]"] == "0"           # ... an odd height is not
    assert rep["status_crop"] == "416x415" and rep["status_format"] == "uyvy_709"
    n_good = len(SIZES) + 1
    assert rep["callbacks"] == str(n_good) and rep["logged"] == str(n_good) and rep["status_errors"] == str(N_BAD)
    odd_y0 = 0
    for i, (fw, fh) in enumerate(SIZES):
        is_view, w, h, pix, off0, pitch0, buf_bytes, frame_id = [int(x) for x in rep[f"req[{i}]"].split(",")]
        assert frame_id == i and pix == UYVY_709 and buf_bytes == 2 * fw * fh
        if fw < W or fh < H:
            assert (is_view, w, h) == (0, fw, fh), (fw, fh)             # smaller than the window on either axis: detected whole (odd heights included)
            continue
        x0, y0 = ((fw - W) // 2) & ~1, (fh - H) // 2                   # x0 rounded down to even, y0 not
        odd_y0 += y0 & 1
        assert (is_view, w, h, pitch0) == (1, W, H, 2 * fw), (fw, fh)
        assert off0 == y0 * 2 * fw + 2 * x0, (fw, fh)
    assert odd_y0 >= 2                                                  # the cases do cover odd origins
    assert (SIZES[1][0] - W) // 2 % 2 == 1                              # ... and an x margin that the rounding changes
    # the good request behind the bad ones was served whole
    is_view, w, h, pix, off0, pitch0, buf_bytes, frame_id = [int(x) for x in rep[f"req[{len(SIZES)}]"].split(",")]
    assert (is_view, w, h, pix, buf_bytes, frame_id) == (0, 100, 63, UYVY_709, 100 * 63 * 2, len(SIZES) + N_BAD)
