"""The closed-loop float64 check (tests/closed_loop_ref.py) must pass a clean engine and bite on a subtly wrong one.  CPU only: the stand-in
engine is oracle/yolov8_ref.py in bf16 mode (weights and every stored activation rounded to bf16, fp32 accumulate), its taps served through
tap().  Clean stand-ins: zero violations at every conv.  Then ONE fault at a time is injected into the stand-in's forward pass at one layer --
everything downstream is computed from the faulty tensor, as in a real engine -- and must be reported at that layer and nowhere else."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import closed_loop_ref as cl
import yolov8_ref
import zly_model as zm


@pytest.fixture(scope="module")
def model_paths(weights_path, tmp_path_factory):
    spec = zm.build_spec("s")
    p = str(tmp_path_factory.mktemp("closed_loop") / "yolov8s_synth.zlyw")
    zm.write_zlyw(p, spec, zm.synth_weights(spec, seed=9))
    return {"n": weights_path, "s": p}


def _images(n, w, h, seed=31):
    f = zm.synth_frames(n, w, h, seed=seed, rects=False)
    return torch.from_numpy(f[..., ::-1].copy()).permute(0, 3, 1, 2).to(torch.float32) / 255.0


# ---------------------------------------------------------------------------------------------------
# clean stand-ins
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale,w,h,n", [("n", 64, 64, 3), ("n", 96, 64, 2), ("s", 64, 64, 3), ("s", 96, 64, 2), ("n", 352, 288, 2)])
@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_clean_stand_in_has_no_violation(model_paths, scale, w, h, n, mode):
    path = model_paths[scale]
    e = cl.StandIn(yolov8_ref.load(path, mode), _images(n, w, h))
    checked, violations, stats = cl.closed_loop(e, path, range(n))
    assert not violations, [str(v) for v in violations]
    assert len(checked) == len(zm.build_spec(scale).convs)
    # the constants stand 16 x above what the CPU reference itself shows on these shapes
    floor = max(v[1] for v in stats.values())
    print(f"yolov8{scale} {w}x{h} {mode}: accumulation floor {floor:.3f} x 2^-24 B, worst |g - y| / bound {max(v[0] for v in stats.values()):.3f}")
    assert 16 * floor <= (cl.C_ACC_FP32_ENGINE if mode == "fp32" else cl.C_ACC)
    for i in range(n):
        db, ds = cl.decode_floor(e, e.head[i], i)
        assert 16 * db <= cl.DECODE_BOX_TOL and 16 * ds <= cl.DECODE_SCORE_TOL, (db, ds)
        cl.check_head_decode(e, e.head[i], i)


def test_bf16_rne_is_the_hardware_rounding():
    rng = np.random.default_rng(0)
    v = np.concatenate([rng.standard_normal(20000) * 10.0 ** rng.integers(-6, 4, 20000), [0.0, 1.0, -1.0, 1.00390625, 1.01171875, 255.5, 2.0 ** -20]])
    v32 = v.astype(np.float32)                                   # exact inputs for the comparison with torch's fp32 -> bf16 RNE
    q, ulp, tie = cl.bf16_rne(v32.astype(np.float64))
    want = torch.from_numpy(v32).to(torch.bfloat16).to(torch.float64).numpy()
    assert np.array_equal(q, want)
    assert np.all(np.abs(q - v32) <= 0.5 * ulp) and np.all(tie <= 0.5 * ulp)
    assert cl.bf16_rne(np.array([1.00390625]))[2][0] == 0.0      # 1 + 2^-8: a tie, rounds to even (1.0)


# ---------------------------------------------------------------------------------------------------
# injected faults
# ---------------------------------------------------------------------------------------------------
def _trunc_bf16(t):
    return (t.contiguous().view(torch.int32) & -65536).view(torch.float32)


class FaultyRef(yolov8_ref.YoloV8Ref):
    """bf16-mode oracle with one fault at one layer; everything downstream sees the faulty tensor"""
    fault, at, flip = None, None, None

    def conv(self, name, x, residual=None, keep_fp32=False):
        if name != self.at or self.fault in (None, "pool", "upsample"):
            return super().conv(name, x, residual, keep_fp32)
        c = self.spec[name]
        w, b = self.w[name]
        pad = c.k // 2
        act = lambda p: p * torch.sigmoid(p) if c.act else p
        y = act(F.conv2d(x, w, b, stride=c.stride, padding=pad))
        if self.fault == "truncate":                             # epilogue truncates to bf16 instead of rounding to nearest even
            y = _trunc_bf16(y + residual if residual is not None else y)
        elif self.fault == "double_round":                       # SiLU output rounded to bf16, then the shortcut added and rounded again
            y = self._q(self._q(y) + residual)
        elif self.fault == "bias":                               # one output channel's bias dropped
            b2 = b.clone(); b2[5] = 0
            y = self._q(act(F.conv2d(x, w, b2, stride=c.stride, padding=pad)) + (residual if residual is not None else 0))
        elif self.fault == "tap00_last_col":                     # tap (0,0) dropped in the last column only
            w2 = w.clone(); w2[:, :, 0, 0] = 0
            y[..., -1] = act(F.conv2d(x, w2, b, stride=c.stride, padding=pad))[..., -1]
            y = self._q(y + (residual if residual is not None else 0))
        elif self.fault == "swap":                               # two output channels swapped
            y = self._q(y + (residual if residual is not None else 0))
            y[:, [3, 4]] = y[:, [4, 3]]
        elif self.fault == "tap21_first_row":                    # eight input channels of tap (2,1) zeroed in the first row only
            w2 = w.clone(); w2[:, 8:16, 2, 1] = 0
            y[:, :, 0] = act(F.conv2d(x, w2, b, stride=c.stride, padding=pad))[:, :, 0]
            y = self._q(y + (residual if residual is not None else 0))
        elif self.fault == "flip_mid":                           # one element of the (LDS-resident) map moved to a neighbouring bf16 value
            y = self._q(y)
            f, ch, yy, xx, value = self.flip
            y[f, ch, yy, xx] = value
        else:
            raise AssertionError(self.fault)
        self.taps[name] = y
        return y

    def sppf(self, x):
        if self.fault != "pool":
            return super().sppf(x)
        y = self.conv("model.9.cv1", x)
        p1 = F.max_pool2d(y, 5, 1, 2)
        p2 = F.max_pool2d(p1, 5, 1, 2)
        p3 = F.max_pool2d(y, 11, 1, 5)                           # third pool with radius 5 instead of 6
        return self.conv("model.9.cv2", torch.cat([y, p1, p2, p3], 1))


def _faulty(path, fault, at, flip=None):
    meta, weights = zm.read_zlyw(path)
    ref = FaultyRef(meta, weights, "bf16")
    ref.fault, ref.at, ref.flip = fault, at, flip
    return ref


LAYER = "model.4.m.0.cv2"


@pytest.mark.parametrize("fault,at", [("truncate", LAYER), ("double_round", LAYER), ("bias", LAYER), ("tap00_last_col", LAYER), ("swap", LAYER),
                                      ("tap21_first_row", LAYER), ("truncate", "model.22.cv3.1.1"), ("bias", "model.22.cv2.2.2"),
                                      ("pool", "model.9.cv2"), ("upsample", "model.12.cv1")])
def test_injected_fault_is_reported_at_its_layer_only(model_paths, monkeypatch, fault, at):
    path = model_paths["n"]
    w, h, n = (352, 288, 1) if fault == "pool" else (160, 128, 2)        # pool: an 11 x 9 map, where radius 5 and 6 differ
    ref = _faulty(path, fault, at)
    with monkeypatch.context() as m:
        if fault == "upsample":                                  # Upsample source index off by one in the last column
            calls = []

            def bad_up(t, scale_factor=2, mode="nearest"):
                u = t.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
                if not calls:                                    # the first Upsample (into model.12.cv1) only
                    u[..., -1] = u[..., -3]
                calls.append(1)
                return u
            m.setattr(yolov8_ref.F, "interpolate", bad_up)
        e = cl.StandIn(ref, _images(n, w, h))
    _, violations, _ = cl.closed_loop(e, path, range(n))
    assert violations, f"{fault} at {at} went unnoticed"
    assert {v.name for v in violations} == {at}, [str(v) for v in violations]
    for v in violations:
        print(v)
    worst = max(violations, key=lambda v: v.count)
    if fault == "tap00_last_col":
        assert all(v.box[2] == (e.tap(at, 0).shape[2] - 1,) * 2 for v in violations), str(worst)       # "last column" at a glance
    if fault == "tap21_first_row":
        assert all(v.box[1] == (0, 0) for v in violations), str(worst)
    if fault == "bias" and at == LAYER:
        assert all(v.box[0] == (5, 5) for v in violations), str(worst)
    if fault == "swap":
        assert all(v.box[0] == (3, 4) for v in violations), str(worst)
    with pytest.raises(AssertionError, match=at.replace(".", r"\.")):
        cl.check_closed_loop(e, path, range(n))


def test_lds_resident_set_must_match_exactly(model_paths):
    path = model_paths["n"]
    mid = "model.4.m.0.cv1"
    x = _images(2, 96, 64)
    e = cl.StandIn(yolov8_ref.load(path, "bf16"), x, hidden=(mid,))
    assert mid in cl.check_closed_loop(e, path, range(2), lds_resident=(mid,))
    with pytest.raises(AssertionError, match="expected LDS-resident"):
        cl.check_closed_loop(e, path, range(2))                                          # a refused tap the caller did not expect
    with pytest.raises(AssertionError, match="expected LDS-resident"):
        cl.check_closed_loop(cl.StandIn(e.ref, x), path, range(2), lds_resident=(mid,))   # a tappable tensor is never loosened
    with pytest.raises(AssertionError, match="only the first conv of a bottleneck"):
        cl.check_closed_loop(cl.StandIn(e.ref, x, hidden=("model.4.cv1",)), path, range(2), lds_resident=("model.4.cv1",))


@pytest.mark.parametrize("scale,w,h", [("n", 64, 64), ("n", 96, 64), ("s", 64, 64), ("s", 96, 64), ("n", 352, 288)])
def test_chained_pairs_are_clean_and_still_bite(model_paths, scale, w, h):
    """every bottleneck's first conv hidden (as bottleneck_pair_kernel / c2f_kernel leave it in LDS): zero violations through the ambiguity
    allowance, and a truncating epilogue at the pair's output still fails"""
    path = model_paths[scale]
    mids = tuple(c.name for c in zm.build_spec(scale).convs if ".m." in c.name and c.name.endswith(".cv1"))
    x = _images(2, w, h)
    e = cl.StandIn(yolov8_ref.load(path, "bf16"), x, hidden=mids)
    checked = cl.check_closed_loop(e, path, range(2), lds_resident=mids)
    assert set(mids) <= set(checked)
    e = cl.StandIn(_faulty(path, "truncate", LAYER), x, hidden=mids)
    _, violations, _ = cl.closed_loop(e, path, range(2), lds_resident=mids)
    assert violations and {v.name for v in violations} == {LAYER} and all(v.allowance for v in violations), [str(v) for v in violations]


def test_ambiguous_mid_may_flip_and_no_other(model_paths):
    """an LDS-resident intermediate one bf16 value off: tolerated where SiLU(p_A) sits at a rounding tie, a failure anywhere else"""
    path = model_paths["n"]
    mid_name, out_name = "model.4.m.0.cv1", LAYER
    x = _images(1, 160, 128)
    clean = cl.StandIn(yolov8_ref.load(path, "bf16"), x)
    half = clean.tap("model.4.cv1", 0)
    xin = half[half.shape[0] // 2:][None]
    mid, amb, ulp, other = cl.mid_of(path, mid_name, xin)
    assert np.array_equal(mid[0], clean.tap(mid_name, 0).astype(np.float64)) or np.mean(mid[0] != clean.tap(mid_name, 0)) < 0.2
    assert 0.01 < amb.mean() < 0.25, amb.mean()
    held = clean.tap(mid_name, 0).astype(np.float64)[None]
    # ambiguous: the largest such element, moved to the value on the other side of its tie
    cand = np.where(amb & (held == mid), np.abs(mid), -1.0)
    ia = np.unravel_index(cand.argmax(), cand.shape)
    e = cl.StandIn(_faulty(path, "flip_mid", mid_name, flip=(*ia, float(other[ia]))), x, hidden=(mid_name,))
    cl.check_closed_loop(e, path, range(1), lds_resident=(mid_name,))
    # not ambiguous: the largest such element, one ulp off
    cand = np.where(~amb & (held == mid), np.abs(mid), -1.0)
    ib = np.unravel_index(cand.argmax(), cand.shape)
    e = cl.StandIn(_faulty(path, "flip_mid", mid_name, flip=(*ib, float(mid[ib] + ulp[ib]))), x, hidden=(mid_name,))
    _, violations, _ = cl.closed_loop(e, path, range(1), lds_resident=(mid_name,))
    assert violations and {v.name for v in violations} == {out_name}, [str(v) for v in violations]
    c0, y0, x0 = violations[0].box
    assert y0[0] >= ib[2] - 1 and y0[1] <= ib[2] + 1 and x0[0] >= ib[3] - 1 and x0[1] <= ib[3] + 1, (ib, str(violations[0]))
