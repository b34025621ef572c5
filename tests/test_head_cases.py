"""tests/head_cases.py without a GPU: the table covers every tie class and boundary it claims (derived from the lane map), the expected
values follow from the biases, the decode tolerances fit the crafted logits, the graded cases' population conditions hold on the CPU
stand-in (oracle/yolov8_ref.py behind closed_loop_ref.StandIn), and the helpers bite: a decode that lets the highest tied class win, one
that compares with >, and an early-out with the margin logit(thr) - 1e-2 each fail the checks the GPU module applies."""
import os

import numpy as np
import pytest
import torch

import closed_loop_ref as cl
import head_cases as hc
import yolov8_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


# ---------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------
def test_lane_map_is_the_kernels():
    src = open(os.path.join(ROOT, "zero-latency-yolo_amd", "csrc", "kernels_head.hip")).read()
    assert "const int ch = c * 16 + kq * 4;" in src and "const int p = lane & 15, kq = lane >> 4;" in src
    for ch in range(80):
        c, kq, r = hc.lane_of(ch)
        assert ch == c * 16 + kq * 4 + r and 0 <= kq < 4 and 0 <= r < 4


def _tie_levels():
    return [lv for f in hc.uniform_table() for lv in f.levels if f.key.startswith("ties_")]


def test_table_covers_every_tie_class():
    pairs = {lv.tied: lv for lv in _tie_levels()}
    want = {(0, 1): {"same_lane_rows"}, (2, 18): {"same_lane_tiles"}, (1, 4): {"lanes_16_apart"}, (1, 8): {"lanes_32_apart"},
            (5, 9): {"quarters_1_and_2"}, (17, 5): {"lanes_16_apart", "high_class_in_low_lane"}, (64, 13): {"high_class_in_low_lane"}}
    for pair, kinds in want.items():
        assert pair in pairs and hc.tie_kinds(*pair) == kinds, (pair, hc.tie_kinds(*pair))
        assert pairs[pair].want_cls == min(pair)
    assert set().union(*[hc.tie_kinds(*p) for p in want]) == set(hc.TIE_KINDS)
    three = [lv for lv in _tie_levels() if len(lv.tied) == 3]
    assert len(three) == 1 and len({hc.lane_of(c)[1] for c in three[0].tied}) >= 2 and len({hc.lane_of(c)[0] for c in three[0].tied}) == 3
    assert any(len(lv.tied) == 80 and lv.want_cls == 0 for lv in _tie_levels())
    for lv in _tie_levels():
        z = lv.cls[list(lv.tied)]
        assert (z == z[0]).all() and (np.delete(lv.cls, list(lv.tied)) < z[0]).all(), lv.name
    # the threshold cases are ties as well, across lanes
    for k in hc.K_VALUES:
        assert len(hc.K_TIED[k]) >= 2
    assert sorted(k for ks in hc.K_FILES for k in ks) == sorted(hc.K_VALUES)


def test_table_covers_the_other_boundaries():
    files = {f.key: f for f in hc.uniform_table()}
    assert {f.nc for f in files.values()} == {80, 1, 3, 17, 64}
    for nc in (1, 3, 17, 64):
        f = files[f"nc{nc}"]
        assert f.conf_thr == 0.04 and all((lv.cls <= -2.5).all() and len(lv.cls) == nc for lv in f.levels)
        assert hc.score_ieee(F32(-3.0)) >= F32(0.04) and hc.score_ieee(F32(0.0)) == F32(0.5)      # a padded row would win if it were looked at
        assert {lv.want_cls for lv in f.levels} == {0, nc - 1}
    sat = files["saturation_dfl"].levels[0]
    assert sat.cls[3] == 20 and sat.cls[40] == 30 and sat.want_cls == 3 and (hc.score_ieee(sat.cls[[3, 40]]) == F32(1.0)).all()
    one, zero = files["conf_one"], files["conf_zero"]
    assert one.conf_thr == 1.0 and [lv.passes for lv in one.levels] == [True, False, True]
    assert hc.score_ieee(F32(20.0)) == F32(1.0) and hc.score_ieee(F32(16.0)) < F32(1.0)
    assert zero.conf_thr == 0.0 and zero.levels[0].passes is False and hc.score_ieee(F32(-120.0)) == 0.0
    tiny = hc.score_ieee(F32([-80.0, -88.0]))
    assert tiny[0] >= np.finfo(np.float32).tiny > tiny[1] > 0                  # a normal and a denormal score
    dfl = {lv.name: lv.box.reshape(4, 16) for f in files.values() for lv in f.levels if lv.name.startswith("dfl_") or lv.name.startswith("saturated")}
    assert (dfl["saturated_3_40"] == 0).all()                                                     # all bins equal: dist 7.5
    assert (dfl["dfl_bin0_zero_area"].argmax(1) == 0).all() and (dfl["dfl_bin15"].argmax(1) == 15).all()
    assert ((dfl["dfl_two_equal_bins"] == 60).sum(1) == 2).all() and dfl["dfl_offset_3e4"].min() > 2.9e4
    assert len({tuple(r) for r in dfl["dfl_mixed_sides"]}) == 4


def test_ladder_brackets_the_prediction():
    for ks in hc.K_FILES:
        for lv, k in zip(hc.ladder_file(ks).levels, ks):
            z0 = hc.lowest_passing_z(hc.thr_of_k(k))
            r = lv.cls[:79]
            assert (np.diff(r) < 0).all() and r[38] > z0 > r[40] and r[39] == z0 and r[0] - z0 >= 3.5 and z0 - r[78] >= 3.5
            assert hc.pick_from_ladder(lv.cls, hc.score_ieee(lv.cls), hc.thr_of_k(k)) == z0
            with pytest.raises(AssertionError):
                hc.pick_from_ladder(lv.cls, np.ones(80, np.float32), hc.thr_of_k(k))             # an edge the ladder does not hold


# ---------------------------------------------------------------------------------------------------
# expected values of the uniform cases; the helpers bite
# ---------------------------------------------------------------------------------------------------
def _passes(f, head, conf):
    """per level: do its anchors pass on this head tensor (uniform: all or none)"""
    _, _, ok = hc.decode_head(head, conf)
    out = []
    for sl in hc.level_slices():
        assert ok[sl].all() or not ok[sl].any()
        out.append(bool(ok[sl][0]))
    return out


@pytest.mark.parametrize("f", hc.uniform_table(), ids=lambda f: f.key)
def test_uniform_expected_outcome(f):
    head = hc.uniform_head(f).astype(np.float32)
    passes = _passes(f, head, f.conf_thr)
    for lv, p in zip(f.levels, passes):
        assert lv.passes is None or lv.passes == p, lv.name
    cls, _, ok = hc.decode_head(head, f.conf_thr)
    hc.check_uniform_outcome(f, passes, cls[ok], int(ok.sum()))
    got = hc.model_outcome(hc.uniform_logits(f), f.conf_thr, bound=hc.skip_logit(f.conf_thr))
    hc.check_uniform_outcome(f, passes, *got)
    if f.key.startswith("ties_") or f.key == "saturation_dfl":
        with pytest.raises(AssertionError):                                    # the highest tied class wins: caught
            hc.check_uniform_outcome(f, passes, *hc.model_outcome(hc.uniform_logits(f), f.conf_thr, tie="highest"))
    # the boxes: all bins equal -> 7.5 bins to every side; bin 0 on four sides -> no area
    for lv, sl, s in zip(f.levels, hc.level_slices(), hc.STRIDES):
        if lv.name == "saturated_3_40":
            assert (head[2, sl] == 15 * s).all() and (head[3, sl] == 15 * s).all()
        if lv.name == "dfl_bin0_zero_area":
            assert (head[2:4, sl] == 0).all()
        if lv.name == "dfl_two_equal_bins":
            assert (head[2:4, sl] == 7 * s).all()


def test_threshold_comparison_bites():
    f = hc.equality_file()
    z = hc.uniform_logits(f)
    for l, lv in enumerate(f.levels):
        s = hc.score_ieee(lv.cls[lv.want_cls])
        for conf, level_passes in ((s, True), (np.nextafter(s, F32(1)), False), (np.nextafter(s, F32(0)), True)):
            passes = [bool(hc.score_ieee(o.cls[o.want_cls]) >= conf) for o in f.levels]
            assert passes[l] == level_passes
            hc.check_uniform_outcome(f, passes, *hc.model_outcome(z, conf))
        with pytest.raises(AssertionError):                                    # > instead of >=: the level is lost at equality
            passes = [bool(hc.score_ieee(o.cls[o.want_cls]) >= s) for o in f.levels]
            hc.check_uniform_outcome(f, passes, *hc.model_outcome(z, s, cmp="gt"))


# known answers: the lowest fp32 logit that scores 1 - k 2^-24 in IEEE fp32 arithmetic (csrc/head_skip.h quotes the first)
LOWEST_PASSING = {2: 15.537, 8: 14.438, 18: 13.691, 34: 13.080, 100: 12.020}


def test_early_out_margin_bites():
    z_of_k = {k: hc.lowest_passing_z(hc.thr_of_k(k)) for k in hc.K_VALUES}
    for k, want in LOWEST_PASSING.items():
        assert abs(float(z_of_k[k]) - want) < 1e-3, (k, float(z_of_k[k]))
    for ks in hc.K_FILES:
        f = hc.k_file(ks, z_of_k)
        z = hc.uniform_logits(f)
        for k in ks:
            thr = hc.thr_of_k(k)
            assert hc.score_ieee(z_of_k[k]) == thr and z_of_k[k] < hc.logit64(thr)
            passes = [bool(hc.score_ieee(lv.cls[lv.want_cls]) >= thr) for lv in f.levels]
            hc.check_uniform_outcome(f, passes, *hc.model_outcome(z, thr))                                        # the engine that writes the head tensor
            hc.check_uniform_outcome(f, passes, *hc.model_outcome(z, thr, bound=hc.skip_logit(thr)))              # production, head_skip.h's bound
            old = hc.model_outcome(z, thr, bound=hc.skip_logit_margin_only(thr))
            if k <= 34:
                assert z_of_k[k] < hc.skip_logit_margin_only(thr)
                with pytest.raises(AssertionError):                            # logit(thr) - 1e-2 drops the level
                    hc.check_uniform_outcome(f, passes, *old)
            else:
                hc.check_uniform_outcome(f, passes, *old)


# ---------------------------------------------------------------------------------------------------
# the decode tolerances on the crafted logits; the graded cases on the stand-in
# ---------------------------------------------------------------------------------------------------
class _HeadStandIn:
    """the oracle's Detect head alone on zero features: for a uniform file the logits are the biases whatever the features are"""

    def __init__(self, ref, n=2):
        dims = hc.level_dims()
        cin = [ref.spec[f"model.22.cv2.{l}.0"].cin for l in range(3)]
        with torch.no_grad():
            self.head = ref.detect([torch.zeros(n, c, mh, mw) for c, (mw, mh) in zip(cin, dims)]).numpy()
        self.ref = ref

    def tap(self, name, frame):
        return self.ref.taps[name][frame].numpy()


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("head_cases")


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
@pytest.mark.parametrize("f", hc.uniform_table() + (hc.equality_file(),), ids=lambda f: f.key)
def test_decode_tolerances_fit_the_uniform_cases(workdir, f, mode):
    path = hc.write_uniform(str(workdir / f"{f.key}.zlyw"), f)
    e = _HeadStandIn(yolov8_ref.load(path, mode))
    want = hc.uniform_head(f)
    for i in range(2):
        db, ds = cl.decode_floor(e, e.head[i], i)
        assert 16 * db <= cl.DECODE_BOX_TOL and 16 * ds <= cl.DECODE_SCORE_TOL, (f.key, db, ds)
        cl.check_head_decode(e, e.head[i], i)
        d = np.abs(e.head[i].astype(np.float64) - want)
        assert d[:4].max() <= cl.DECODE_BOX_TOL and d[4:].max() <= cl.DECODE_SCORE_TOL, (f.key, d[:4].max(), d[4:].max())


@pytest.fixture(scope="module")
def graded(workdir, oracle):
    """{thr: path} chosen on the bf16 stand-in, and the images"""
    paths, _, images = hc.write_graded(workdir, oracle)
    return paths, images


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
@pytest.mark.parametrize("thr", hc.GRADED_THRESHOLDS, ids=lambda t: f"{float(t):.9g}")
def test_graded_populations_on_the_stand_in(graded, thr, mode):
    paths, images = graded
    e = cl.StandIn(yolov8_ref.load(paths[float(thr)], mode), images)
    frames = []
    for i in range(3):
        db, ds = cl.decode_floor(e, e.head[i], i)
        assert 16 * db <= cl.DECODE_BOX_TOL and 16 * ds <= cl.DECODE_SCORE_TOL, (db, ds)
        cl.check_head_decode(e, e.head[i], i)
        frames.append((e.head[i], [e.tap(f"model.22.cv3.{l}.2", i) for l in range(3)]))
    pop = hc.populations(frames, thr)
    print(f"thr {float(thr):.9g} {mode}: {pop}")
    hc.check_populations(pop, thr)
    # with room to spare: the engines' activations differ from the stand-in's by bf16 rounding noise
    assert pop.empty >= 0.3 * pop.tiles and pop.mixed >= 0.3 * pop.tiles and pop.near >= 2 * hc.MIN_NEAR, pop
    if hc.is_high(thr):
        assert pop.window >= 4 * hc.MIN_WINDOW, pop
        # and the earlier margin loses candidates here: the production model with logit(thr) - 1e-2 against the one that skips nothing
        lost = 0
        for _, taps in frames:
            z = [t.reshape(t.shape[0], -1) for t in taps]
            lost += hc.model_outcome(z, thr)[1] - hc.model_outcome(z, thr, bound=hc.skip_logit_margin_only(thr))[1]
            assert hc.model_outcome(z, thr)[1] == hc.model_outcome(z, thr, bound=hc.skip_logit(thr))[1]
        assert lost >= hc.MIN_WINDOW, lost
