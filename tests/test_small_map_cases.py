"""The closed-loop float64 reference alone on the smallest and thinnest maps (tests/small_map_cases.py), with the stand-in engine of
tests/test_closed_loop_ref.py.  CPU only.

Clean stand-ins: every shape of the table in bf16 and fp32 mode at n = 3, zero violations, every conv checked, 16 x the accumulation floor within
C_ACC / C_ACC_FP32_ENGINE and the decode floors within the decode tolerances.  The stand-in is built inside torch.backends.mkldnn.flags(enabled=False):
with oneDNN on, torch's choice for the tiny batched Detect convs at 32 x 32 shows a floor of 6.3 - 6.9 (bf16 mode) and 9.4 - 9.9 (fp32 mode) at n >= 2
-- no violation, but more than the 16 x rule allows -- where the plain CPU conv shows 0.52 and 2.26 (see the comment over C_ACC_CPU_FLOOR).

Bite.  The geometric faults of test_closed_loop_ref.py are blind on these maps, and correctly so: tap (2,1) dropped in the first row, tap (0,0) in the
last column and pool radius 5 for 6 change nothing on a 1 x 1 or 1 x N map.  Three faults that matter on exactly these maps are injected instead, one
at a time, and must be reported at their layer and nowhere else:
  * halo_from_neighbour_frame: the vertical zero padding of one 3 x 3 conv replaced by the adjacent rows of the batch-linear tensor;
  * pool_zero_pad: SPPF's max pools pad with 0 instead of -inf (SiLU outputs go down to -0.278, so even a 1 x 1 map changes);
  * upsample_from_next: the first Upsample reads source pixel (y >> 1, (x >> 1) + 1), clamped in the last column.  On a source of ONE column (32 x 32:
    1 x 1, 32 x 416: 13 x 1) the clamp makes it the identity: there it cannot bite, which test_upsample_fault_cannot_bite_on_one_column states."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import closed_loop_ref as cl
import small_map_cases as sm
import yolov8_ref
import zly_model as zm
from test_closed_loop_ref import LAYER, FaultyRef

MID = "model.8.m.0.cv2"           # the P5-level 3 x 3 conv with a shortcut
OTHER = (32, 416)                 # the one-column counterpart of sm.ONE_ROW


@pytest.fixture(scope="module")
def model_paths(weights_path, tmp_path_factory):
    spec = zm.build_spec("s")
    p = str(tmp_path_factory.mktemp("small_maps") / "yolov8s_synth.zlyw")
    zm.write_zlyw(p, spec, zm.synth_weights(spec, seed=9))
    return {"n": weights_path, "s": p}


def _stand_in(ref, n, w, h, hidden=()):
    with torch.backends.mkldnn.flags(enabled=False):
        return cl.StandIn(ref, sm.images_of(sm.frames_of(n, w, h)), hidden=hidden)


# ---------------------------------------------------------------------------------------------------
# the case table itself
# ---------------------------------------------------------------------------------------------------
def test_table_is_consistent():
    for (w, h), (txt, _) in sm.SHAPES.items():
        assert w % 32 == 0 and h % 32 == 0 and max(w, h) <= 416
        assert txt.split() == [f"{r}x{c}" for r, c in sm.maps(w, h)], (w, h, txt)
    assert sm.maps(*sm.ONE_ROW) == [(4, 52), (2, 26), (1, 13)] and sm.n_anchors(32, 32) == 21
    assert len(set(sm.CASES)) == len(sm.CASES)
    for shape, cfg in sm.CASES:
        assert shape in sm.SHAPES and cfg in sm.CONFIGS
    assert {s for s, _ in sm.CASES} == set(sm.SHAPES)
    ids = {sm.case_id(c): c for c in sm.CASES}
    assert set(sm.MUST_REACH) | set(sm.CANNOT_REACH) == set(sm.FAMILIES) and not set(sm.MUST_REACH) & set(sm.CANNOT_REACH)
    assert set(sm.MUST_SPAN) <= set(sm.CANNOT_REACH)
    for table, test in ((sm.MUST_REACH, sm.below_tile), (sm.MUST_SPAN, lambda fam, r, c, n: sm.spanned_by_tile(fam, r, c) and not sm.below_tile(fam, r, c, n))):
        for fam, cases in table.items():
            assert cases, fam
            for cid, ms in cases.items():
                (w, h), cfg = ids[cid]
                for m in ms:                                      # the maps the table names are what it says they are
                    r, c = (int(v) for v in m.split("x"))
                    assert test(fam, r, c, sm.CONFIGS[cfg][4]), (fam, cid, m)
    # every op of the plan has a map
    for c in zm.build_spec("s").convs:
        assert sm.out_map(c.name, 64, 32) is not None
    assert sm.out_map("model.9.pool", 64, 32) == (1, 2) and sm.out_map("detect.tail.P4", 64, 32) == (2, 4) and sm.out_map("nms", 64, 32) is None


@pytest.mark.parametrize("scale", ["n", "s"])
def test_conf_thr_is_what_the_oracle_head_gives(model_paths, scale):
    """the thresholds of the case table are those choose_conf_thr computes from the oracle's own head, and leave every one of the 64 frames of every
    shape at least MIN_CANDIDATES + 2 anchors 0.03 above them"""
    ref = yolov8_ref.load(model_paths[scale], "bf16")
    for (w, h) in sm.ALL:
        if (scale, w, h) not in sm.CONF_THR:
            continue
        thr = sm.CONF_THR[(scale, w, h)]
        # (the oracle's fp32 sums may differ in the last bits from one CPU to another: one step of 1/64 and 0.005 of the margin are left for that)
        assert abs(thr - sm.choose_conf_thr(ref, w, h)) <= 1.0 / 64, (scale, w, h)
        head = ref.forward(sm.images_of(sm.frames_of(64, w, h))).numpy()
        assert min(sm.candidates(hd, thr + 0.025) for hd in head) >= sm.MIN_CANDIDATES + 2, (scale, w, h)
        assert 0.0 < thr < 1.0
    assert {(s, w, h) for (s, w, h) in sm.CONF_THR if s == scale} >= {(scale, *shape) for shape, cfg in sm.CASES if sm.CONFIGS[cfg][0] == scale}


# ---------------------------------------------------------------------------------------------------
# clean stand-ins
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", sm.ALL)
@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_clean_stand_in_has_no_violation(model_paths, w, h, mode):
    path, n = model_paths["n"], 3
    e = _stand_in(yolov8_ref.load(path, mode), n, w, h)
    checked, violations, stats = cl.closed_loop(e, path, range(n))
    assert not violations, [str(v) for v in violations]
    assert len(checked) == 63
    floor = max(v[1] for v in stats.values())
    print(f"yolov8n {w}x{h} {mode}: accumulation floor {floor:.3f} x 2^-24 B at {max(stats, key=lambda k: stats[k][1])}")
    assert 16 * floor <= (cl.C_ACC_FP32_ENGINE if mode == "fp32" else cl.C_ACC)
    for i in range(n):
        db, ds = cl.decode_floor(e, e.head[i], i)
        assert 16 * db <= cl.DECODE_BOX_TOL and 16 * ds <= cl.DECODE_SCORE_TOL, (db, ds)
        cl.check_head_decode(e, e.head[i], i)


# ---------------------------------------------------------------------------------------------------
# injected faults
# ---------------------------------------------------------------------------------------------------
class SmallMapFaultyRef(FaultyRef):
    """FaultyRef with the faults that matter on one-row, one-column and one-pixel maps"""

    def conv(self, name, x, residual=None, keep_fp32=False):
        if self.fault == "halo_from_neighbour_frame" and name == self.at:
            c = self.spec[name]
            assert c.k == 3
            w, b = self.w[name]
            y = F.conv2d(sm.halo_from_neighbour_frame(x), w, b, stride=c.stride, padding=0)
            y = y * torch.sigmoid(y) if c.act else y
            y = self._q(y + residual if residual is not None else y)
            self.taps[name] = y
            return y
        if self.fault in ("halo_from_neighbour_frame", "pool_zero_pad", "upsample_from_next"):
            return yolov8_ref.YoloV8Ref.conv(self, name, x, residual, keep_fp32)
        return super().conv(name, x, residual, keep_fp32)

    def sppf(self, x):
        if self.fault != "pool_zero_pad":
            return super().sppf(x)
        y = self.conv("model.9.cv1", x)
        pool = lambda t: F.max_pool2d(F.pad(t, (2, 2, 2, 2), value=0.0), 5, 1, 0)
        p1 = pool(y)
        p2 = pool(p1)
        p3 = pool(p2)
        return self.conv("model.9.cv2", torch.cat([y, p1, p2, p3], 1))

    def forward(self, images):
        if self.fault != "upsample_from_next":
            return super().forward(images)
        with sm.first_upsample_replaced(sm.upsample_from_next):
            return super().forward(images)


def _faulty(path, fault, at):
    meta, weights = zm.read_zlyw(path)
    ref = SmallMapFaultyRef(meta, weights, "bf16")
    ref.fault, ref.at = fault, at
    return ref


FAULTS = [("halo_from_neighbour_frame", MID), ("halo_from_neighbour_frame", "model.7"), ("pool_zero_pad", "model.9.cv2"),
          ("upsample_from_next", "model.12.cv1"), ("truncate", MID), ("bias", "model.22.cv2.2.2")]


# every fault on every thin shape and on the one-column counterpart, but upsample_from_next where the source has one column: there the clamp makes
# it the identity (test_upsample_fault_cannot_bite_on_one_column)
FAULT_CASES = [(f, at, w, h) for f, at in FAULTS for w, h in sm.THIN + [OTHER] if not (f == "upsample_from_next" and sm.maps(w, h)[2][1] == 1)]


@pytest.mark.parametrize("fault,at,w,h", FAULT_CASES)
def test_injected_fault_is_reported_at_its_layer_only(model_paths, fault, at, w, h):
    path, n = model_paths["n"], 3
    e = _stand_in(_faulty(path, fault, at), n, w, h)
    _, violations, _ = cl.closed_loop(e, path, range(n))
    assert violations, f"{fault} at {at} went unnoticed at {w} x {h}"
    assert {v.name for v in violations} == {at}, [str(v) for v in violations]
    for v in violations:
        print(v)
    if fault == "halo_from_neighbour_frame" and sm.maps(w, h)[2][0] == 1:
        # a one-row P5: at stride 1 every frame has a neighbour above or below, so every frame is reported; the stride-2 conv from two rows to one reads
        # row -1 only (rows -1, 0, 1 of its input), so every frame but the first
        assert {v.frame for v in violations} == set(range(1 if at == "model.7" else 0, n)), [str(v) for v in violations]
    with pytest.raises(AssertionError, match=at.replace(".", r"\.")):
        cl.check_closed_loop(e, path, range(n))


@pytest.mark.parametrize("w,h", [(32, 32), OTHER])
def test_upsample_fault_cannot_bite_on_one_column(model_paths, w, h):
    """source pixel (x >> 1) + 1 clamped to the last column IS pixel x >> 1 where the source has one column (1 x 1 at 32 x 32, 13 x 1 at 32 x 416): the
    faulty Upsample is the right one, and the check must not report anything"""
    rows, cols = sm.maps(w, h)[2]
    assert cols == 1
    t = torch.randn(3, 8, rows, 1)
    assert torch.equal(sm.upsample_from_next(t), F.interpolate(t, scale_factor=2, mode="nearest"))
    t = torch.randn(3, 8, 1, 2)
    assert not torch.equal(sm.upsample_from_next(t), F.interpolate(t, scale_factor=2, mode="nearest"))
    path, n = model_paths["n"], 3
    e = _stand_in(_faulty(path, "upsample_from_next", "model.12.cv1"), n, w, h)
    _, violations, _ = cl.closed_loop(e, path, range(n))
    assert not violations, [str(v) for v in violations]


@pytest.mark.parametrize("w,h", [(32, 32), (64, 32)])
def test_older_geometric_faults_are_blind_here(model_paths, w, h):
    """written down, not assumed: on a P5 map of 1 x 1 or 1 x 2 the faults of test_closed_loop_ref.py that drop a lower tap in the first row, narrow the
    third pool to radius 5 or (one column) drop a left tap in the last column change nothing -- which is why this file has faults of its own"""
    path, n = model_paths["n"], 3
    meta, weights = zm.read_zlyw(path)
    for fault, at in (("tap21_first_row", MID), ("pool", "model.9.cv2")) + ((("tap00_last_col", MID),) if w == 32 else ()):
        ref = FaultyRef(meta, weights, "bf16")
        ref.fault, ref.at = fault, at
        e = _stand_in(ref, n, w, h)
        assert not cl.closed_loop(e, path, range(n))[1], (fault, w, h)


@pytest.mark.parametrize("scale", ["n", "s"])
@pytest.mark.parametrize("w,h", sm.THIN)
def test_chained_pairs_are_clean_and_still_bite(model_paths, scale, w, h):
    """test_closed_loop_ref.py's test of that name on the thin shapes: every bottleneck's first conv hidden, zero violations through the ambiguity
    allowance, and a truncating epilogue at a pair's output (the P5-level one) still fails"""
    path = model_paths[scale]
    mids = tuple(c.name for c in zm.build_spec(scale).convs if ".m." in c.name and c.name.endswith(".cv1"))
    e = _stand_in(yolov8_ref.load(path, "bf16"), 2, w, h, hidden=mids)
    checked = cl.check_closed_loop(e, path, range(2), lds_resident=mids)
    assert set(mids) <= set(checked)
    for layer in (LAYER, MID):
        e = _stand_in(_faulty(path, "truncate", layer), 2, w, h, hidden=mids)
        _, violations, _ = cl.closed_loop(e, path, range(2), lds_resident=mids)
        assert violations and {v.name for v in violations} == {layer} and all(v.allowance for v in violations), [str(v) for v in violations]
