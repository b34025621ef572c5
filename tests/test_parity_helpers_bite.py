"""CPU proof that the assertion helpers the model-family GPU tests use (tests/test_gpu_parity.py, tests/test_gpu_model_family.py) fail
on the bugs they are there for: the bf16-rounding oracle with one conv mutated stands in for a wrong kernel.
  * YOLOv8m: the remainder k-step of a 48-channel 3x3 conv dropped (K = 9 x 48 = 432 = 13.5 bf16 k-steps; the half step is tap 8,
    channels 32..47) -- what a kernel that rounds K down to whole k-steps would compute;
  * YOLOv8n with 17 classes: the one valid row of the partial class tile (class 16) computed with its neighbour's weights."""
import numpy as np
import pytest
import torch

import yolov8_ref
import zly_model as zm
from test_gpu_parity import _assert_bf16_close, _assert_layer_close, _check_taps


class _OracleAsEngine:
    """the .tap(name, i) interface of zly.Engine over an oracle's taps"""
    def __init__(self, ref):
        self.ref = ref

    def tap(self, name, i):
        return self.ref.taps[name][i].numpy()


def _oracles(spec, mutate, w, h):
    wts = zm.synth_weights(spec)
    meta = dict(nc=spec.nc, reg_max=spec.reg_max, ch=spec.ch, n_c2f=spec.n_c2f, convs=spec.convs)
    bad = {k: (v[0].copy(), v[1].copy()) for k, v in wts.items()}
    mutate(bad)
    x = torch.from_numpy(zm.synth_frames(1, w, h, seed=3, rects=False)[..., ::-1].copy()).permute(0, 3, 1, 2).float() / 255
    good, wrong = yolov8_ref.YoloV8Ref(meta, wts, "bf16"), yolov8_ref.YoloV8Ref(meta, bad, "bf16")
    return good, wrong, good.forward(x).numpy(), wrong.forward(x).numpy()


def test_dropped_remainder_k_step_of_a_48_channel_conv_is_caught():
    spec = zm.build_spec("m")
    name = "model.2.m.0.cv1"
    conv = next(c for c in spec.convs if c.name == name)
    assert (conv.cin, conv.k) == (48, 3) and conv.cin * 9 % 32 == 16

    def drop(wts):
        wts[name][0][:, 32:48, 2, 2] = 0.0                     # k = tap * 48 + c for k in [416, 432): the last, half-filled k-step

    good, wrong, _, _ = _oracles(spec, drop, 128, 96)
    names = [c.name for c in spec.convs]
    assert len(_check_taps(_OracleAsEngine(good), good, (0,), names=names)) == len(names)      # the clean oracle passes its own check
    with pytest.raises(AssertionError, match=name):
        _check_taps(_OracleAsEngine(wrong), good, (0,), names=names)


def test_wrong_row_of_a_partial_class_tile_is_caught():
    spec = zm.build_spec("n", 17)

    def neighbour_row(wts):
        for l in range(3):
            w, b = wts[f"model.22.cv3.{l}.2"]
            w[16], b[16] = w[15], b[15]

    good, wrong, h_good, h_wrong = _oracles(spec, neighbour_row, 160, 128)
    assert h_good.shape == (1, 4 + 17, 20 * 16 + 10 * 8 + 5 * 4)
    _assert_bf16_close(h_good, h_good)
    with pytest.raises(AssertionError):
        _assert_bf16_close(h_wrong, h_good)                     # the head against the oracle's
    for l in range(3):
        name = f"model.22.cv3.{l}.2"
        with pytest.raises(AssertionError, match=name):
            _assert_layer_close(wrong.taps[name][0].numpy(), good.taps[name][0].numpy(), name)   # the class branch's logits tap
    assert np.array_equal(h_wrong[:, :4 + 16], h_good[:, :4 + 16])                             # and nothing but class 16 moved
