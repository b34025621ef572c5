"""conv3x3_ws_pair_kernel (run on the MI355X box: pytest -m gpu): a 64-channel bottleneck's two 3x3 convs as one weight-stationary launch must
be BIT-IDENTICAL to the two conv3x3_ws_kernel launches it replaces -- same k-step order, same MFMA, same SiLU, same rounding points.

Every case builds one engine with the kernel on (the default) and one with ZLY_WS_PAIR=0 (the switch is read per engine at create), checks through
op_kernels which of the two each engine runs, and requires np.array_equal, frame by frame, on every pair's cv2 tap, with FLAG_DUMP_LOGITS on every
pair's cv1 tap (the intermediate map, which the kernel then writes out as well), and on the head tensor of forward().  What the shapes are for:
  * 416 x 416, n = 16: 26 x 26 x 16 = 10 816 pixels, exactly the weight-stationary kernel's default pixel gate; the 7 x 13 tiles divide the map; the
    residual pairs (model.6) and the plain ones (model.12, model.18);
  * 352 x 288, n = 5 and 224 x 416, n = 4 (22 x 18 and 14 x 26 maps, ZLY_WS_MIN_TILES=1): partial tiles on every edge, and conv A's region reaches
    outside the frame on all four sides -- those pixels of the intermediate map must be zero, not conv A of padded input;
  * the first of those with ZLY_WS_PAIR_GRID=7: every workgroup walks several tiles (the next-patch DMA, both LDS maps reused across tiles);
  * YOLOv8-s at 320 x 256, n = 3: its 64-channel model.4 pairs on 40 x 32 maps;
  * ZLY_WS_MAX_BYTES=1: the convs fall back to the 64-bit kernels, so no pair kernel may be planned, and the results are the "off" engine's.
The oracle check of the same layers is the existing ragged-map and layer-wise tests', which run with the kernel on by default."""
import numpy as np
import pytest

import zly
import zly_model as zm
from closed_loop_ref import check_closed_loop, lds_resident_from_kernels

pytestmark = pytest.mark.gpu

PAIRS_N = ("model.6.m.0", "model.6.m.1", "model.12.m.0", "model.18.m.0")
SWITCHES = ("ZLY_WS_PAIR", "ZLY_WS_PAIR_GRID", "ZLY_WS_MIN_TILES", "ZLY_WS_MAX_BYTES")


def _engine(monkeypatch, env, path, w, h, n, flags):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return zly.Engine(path, model_w=w, model_h=h, max_batch=n, warmup_runs=0, flags=flags)


def _kernels(e, n):
    return {o["name"].split("+")[0]: k for o, k in zip(e.ops(), e.op_kernels(n))}


def _run(e, x, names):
    head = e.forward(x)
    return head, {nm: [e.tap(nm, i) for i in range(x.shape[0])] for nm in names}


def _on_off(monkeypatch, path, w, h, n, pairs, env, expect_pair=True):
    """engines with the pair kernel on / off under the switches `env`, without and with FLAG_DUMP_LOGITS: kernel names, then bitwise equality"""
    frames = zm.synth_frames(n, w, h, seed=31, rects=False)
    x = None
    for flags in (0, zly.FLAG_DUMP_LOGITS):
        taps = [p + ".cv2" for p in pairs] + ([p + ".cv1" for p in pairs] if flags else [])
        on = _engine(monkeypatch, env, path, w, h, n, flags)
        if x is None:
            x = np.stack([on.preprocess(f) for f in frames])
        kern = _kernels(on, n)
        for p in pairs:
            if expect_pair:
                assert kern[p + ".cv1"].startswith("conv3x3_ws_pair_kernel<"), (p, kern[p + ".cv1"])
                assert kern[p + ".cv2"] == "(fused into the previous launch)", (p, kern[p + ".cv2"])
        if not expect_pair:
            assert not any("ws_pair" in k for k in kern.values()), kern
        got_head, got = _run(on, x, taps)
        if flags:
            # against float64 on the engine's own inputs, per element (tests/closed_loop_ref.py): with the dump flag the pair kernel writes its
            # intermediate map out, so both convs of every pair are checked directly -- none of them through the ambiguity allowance
            lds = lds_resident_from_kernels(on, n)
            assert not lds & {p + ".cv1" for p in pairs}, lds
            assert len(check_closed_loop(on, path or zly.DEFAULT_WEIGHTS, (0, n - 1), lds_resident=lds)) == len(zm.read_zlyw(path or zly.DEFAULT_WEIGHTS)[0]["convs"])
        if expect_pair and not flags:                            # without the dump flag the intermediate map stays in LDS: its tap fails
            with pytest.raises(zly.ZlyError):
                on.tap(pairs[0] + ".cv1", 0)
        on.close()
        off = _engine(monkeypatch, dict(env, ZLY_WS_PAIR="0"), path, w, h, n, flags)
        assert not any("ws_pair" in k for k in _kernels(off, n).values())
        want_head, want = _run(off, x, taps)
        off.close()
        for nm in taps:
            for i in range(n):
                assert got[nm][i].shape == want[nm][i].shape and np.array_equal(got[nm][i], want[nm][i]), (flags, nm, i)
                assert np.isfinite(want[nm][i]).all() and np.abs(want[nm][i]).max() > 0, (flags, nm, i)
        for i in range(n):
            assert np.array_equal(got_head[i], want_head[i]), (flags, i)


def test_default_gate_416_batch16(monkeypatch):
    _on_off(monkeypatch, None, 416, 416, 16, PAIRS_N, {})


@pytest.mark.parametrize("w,h,n", [(352, 288, 5), (224, 416, 4)])
def test_ragged_maps(monkeypatch, w, h, n):
    _on_off(monkeypatch, None, w, h, n, PAIRS_N, {"ZLY_WS_MIN_TILES": "1"})


def test_several_tiles_per_workgroup(monkeypatch):
    _on_off(monkeypatch, None, 352, 288, 5, PAIRS_N, {"ZLY_WS_MIN_TILES": "1", "ZLY_WS_PAIR_GRID": "7"})


def test_yolov8s_model4_pairs(monkeypatch, tmp_path):
    spec = zm.build_spec("s")
    path = str(tmp_path / "yolov8s_synth.zlyw")
    zm.write_zlyw(path, spec, zm.synth_weights(spec))
    _on_off(monkeypatch, path, 320, 256, 3, ("model.4.m.0", "model.4.m.1"), {"ZLY_WS_MIN_TILES": "1"})


def test_falls_back_with_the_convs(monkeypatch):
    _on_off(monkeypatch, None, 416, 416, 16, PAIRS_N, {"ZLY_WS_MAX_BYTES": "1"}, expect_pair=False)
