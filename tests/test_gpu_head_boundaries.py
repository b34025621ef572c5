"""head_fused_kernel at its decision boundaries (run on the MI355X box: pytest -m gpu), on the crafted Detect heads of tests/head_cases.py:
class ties inside a lane and across lanes, saturated scores, class counts that fill no channel tile, conf_thr at a score, one fp32 step
above and below it, 0.0 and 1.0, thresholds of 1 - k 2^-24 whose lowest passing logit lies below logit(thr), DFL extremes, and graded
heads whose tiles are empty, mixed and near the threshold.

For every case, a bf16 and an fp32 engine, frames of different request sizes:
  * the engine that writes the head tensor (with FLAG_DUMP_LOGITS: its six logits taps): the head tensor is decode64 of the biases (uniform
    cases) and of its own taps (all cases); detect equals the CPU oracle's post-processing of that head tensor, n_candidates its decode;
  * the production engine (FLAG_NO_HEAD_TENSOR: the early-out is live) writes the same slab bytes and n_candidates -- from the captured graph
    and from eager launches, as one tail launch and as per-level tails, with the box conv in the tail (ZLY_TAIL_BOX 0 / 1 / 2), in letterbox
    mode, and on YOLOv8-s; op_kernels shows that a variant was really taken.
The thresholds 1 - k 2^-24 need the lowest logit that passes ON THE ENGINE: a ladder file (80 classes = 79 logits around the IEEE
prediction) is run first and the case file is written from what that engine's head tensor shows.

Measured on an MI355X: the module's 55 tests take 10 .. 11 s (some 300 small engines); slowest: the first
test, which also writes the first weight file and loads the library, 0.4 .. 0.5 s; every other test 0.2 .. 0.36 s.
Lowest passing logits found by the ladders, k = 2 / 8 / 18 / 34 / 100 / 1000: fp32 engine 15.5369205 / 14.4383078 / 13.6910934 / 13.0801849 /
12.0204124 / 9.7267780 (the IEEE prediction, every one); bf16 engine the same but for k = 2 and 8, one fp32 step higher.  They lie below
logit(thr) by 0.4055 / 0.1178 / 0.0541 / 0.0290 / 0.0099 / 0.0009.  In the bf16 engine z = -88 scores 0.0 (v_rcp_f32 flushes the denormal
quotient; the fp32 engine's divide gives 6.05e-39) -- either way the anchor's class and the candidate list follow the head tensor.
With the bound logit(thr) - 1e-2 (before csrc/head_skip.h) 18 of the 55 fail, e.g. 0 candidates for 320 at k = 2 and at k = 34, 9 for 81 on
the graded head at 1 - 18 2^-24; with the cross-lane tie taking `oc > cls` 37 fail, with `best > a.conf_thr` 34."""
import os

import numpy as np
import pytest

import closed_loop_ref as cl
import head_cases as hc
import letterbox_ref as lb
import zly
import zly_model as zm
from oracle_lib import det_fields_equal

pytestmark = pytest.mark.gpu

SWITCHES = ("ZLY_TAIL_BOX", "ZLY_TAIL_BOX_MIN_CONF", "ZLY_WS_MIN_TILES", "ZLY_LDS_MIN_TILES", "ZLY_NO_DET_MERGE")
PROD = zly.FLAG_NO_HEAD_TENSOR
IOU = 0.45
DTYPES = [pytest.param(zly.DTYPE_BF16, id="bf16"), pytest.param(zly.DTYPE_FP32, id="fp32")]
NOTE = "(computed in the Detect tail at surviving anchors)"
BOX1 = [f"model.22.cv2.{l}.1" for l in range(3)]
F32 = np.float32


def _engine(monkeypatch, path, dtype, conf, n, flags=0, env=None, use_graph=True, w=hc.MODEL_W, h=hc.MODEL_H, max_dets=512):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    return zly.Engine(path, model_w=w, model_h=h, conf_thr=float(conf), iou_thr=IOU, max_batch=n, max_dets=max_dets, dtype=dtype,
                      warmup_runs=0, use_graph=use_graph, flags=flags)


def _detect(e, frames):
    try:
        return e.detect_batch(frames, cap=e.max_dets)
    except zly.ZlyError as exc:                        # a HIP error may be a GPU fault: nothing more is started on that device
        pytest.exit(f"detect_batch failed: {exc}", returncode=3)


def _slab_bytes(e, n):
    """per frame: the header's bytes, the bytes of the detections behind it, n_kept, n_candidates"""
    raw = np.zeros(n * e.slab_bytes, dtype=np.uint8)
    zly._check(e.lib, e.lib.zly_read_slabs(e.h, n, raw.ctypes.data))
    return [(hdr.tobytes(), dets.tobytes(), int(hdr["n_kept"]), int(hdr["n_candidates"])) for hdr, dets in zly.parse_slabs(raw, n, e.max_dets)]


def _kernels(e, n):
    return {o["name"].split("+")[0]: k for o, k in zip(e.ops(), e.op_kernels(n))}


def _tail_launches(e, n):
    return [k for k in _kernels(e, n).values() if k.startswith("head_fused_kernel")]


def _box_levels(e, n):
    kern = _kernels(e, n)
    return [l for l in range(3) if kern[BOX1[l]] == NOTE]


def _head_engine(monkeypatch, oracle, path, dtype, conf, frames, uniform=None, flags=zly.FLAG_DUMP_LOGITS, env=None, w=hc.MODEL_W, h=hc.MODEL_H,
                 letterbox=False):
    """The engine that writes the head tensor, on `frames`: every assertion that needs no second engine.
    -> (slab bytes per frame, head tensors, class-logit taps per frame or None without the dump flag)"""
    n = len(frames)
    e = _engine(monkeypatch, path, dtype, conf, n, flags=flags | (zly.FLAG_LETTERBOX if letterbox else 0), env=env, w=w, h=h)
    res = _detect(e, frames)
    slabs = _slab_bytes(e, n)
    heads = [e.head_tensor(i) for i in range(n)]
    taps = None
    if flags & zly.FLAG_DUMP_LOGITS:
        taps = [[e.tap(f"model.22.cv3.{l}.2", i) for l in range(3)] for i in range(n)]
        for i in range(n):
            cl.check_head_decode(e, heads[i], i)
    e.close()
    want_head = hc.uniform_head(uniform, w, h) if uniform is not None else None
    for i, fr in enumerate(frames):
        assert np.isfinite(heads[i]).all()
        if want_head is not None:
            d = np.abs(heads[i].astype(np.float64) - want_head)
            assert d[:4].max() <= cl.DECODE_BOX_TOL, (uniform.key, i, float(d[:4].max()), int(d[:4].max(0).argmax()))
            assert d[4:].max() <= cl.DECODE_SCORE_TOL, (uniform.key, i, float(d[4:].max()), int(d[4:].max(0).argmax()))
        fh, fw = fr.shape[:2]
        hp, pw, ph = lb.unpad_head(heads[i], fw, fh, w, h) if letterbox else (heads[i], fw, fh)
        want = oracle.postprocess(hp, pw, ph, float(conf), IOU)
        dets, k = res[i]
        assert k == len(want) and det_fields_equal(dets, want[:len(dets)]), (i, k, len(want))
        n_cand = int(hc.decode_head(heads[i], conf)[2].sum())
        assert len(oracle.decode(hp, pw, ph, float(conf))) == n_cand
        assert slabs[i][2] == k and slabs[i][3] == n_cand, (i, slabs[i][2:], k, n_cand)
    return slabs, heads, taps


def _production_equals(monkeypatch, want, path, dtype, conf, frames, flags=0, env=None, use_graph=True, w=hc.MODEL_W, h=hc.MODEL_H, what=""):
    """a FLAG_NO_HEAD_TENSOR engine, two calls (the second replays the captured graph): the head-tensor engine's slab bytes.  -> the engine, open"""
    n = len(frames)
    e = _engine(monkeypatch, path, dtype, conf, n, flags=PROD | flags, env=env, use_graph=use_graph, w=w, h=h)
    for rep in range(2):
        _detect(e, frames)
        got = _slab_bytes(e, n)
        for i in range(n):
            assert got[i][3] == want[i][3], f"{what} call {rep} frame {i}: {got[i][3]} candidates, the head-tensor engine has {want[i][3]}"
            assert got[i][0] == want[i][0] and got[i][1] == want[i][1], f"{what} call {rep} frame {i}: slab bytes differ (n_kept {got[i][2]} / {want[i][2]})"
    st = e.stats()
    if use_graph:
        assert st["graph_replays"] >= 1, st
    else:
        assert st["graph_replays"] == 0 and st["eager_batches"] >= 2, st
    return e


def _both_productions(monkeypatch, want, path, dtype, conf, frames, what):
    for graph in (True, False):
        _production_equals(monkeypatch, want, path, dtype, conf, frames, use_graph=graph, what=f"{what} {'graph' if graph else 'eager'}").close()


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("head_boundaries")


@pytest.fixture(scope="module")
def uniform_paths(workdir):
    """weight files are written once per module, on first use"""
    cache = {}

    def get(f, scale="n"):
        if (f.key, scale) not in cache:
            cache[(f.key, scale)] = hc.write_uniform(str(workdir / f"{f.key}_{scale}.zlyw"), f, scale)
        return cache[(f.key, scale)]
    return get


# ---------------------------------------------------------------------------------------------------
# uniform cases
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("f", hc.uniform_table(), ids=lambda f: f.key)
def test_uniform(monkeypatch, oracle, uniform_paths, f, dtype):
    path, frames = uniform_paths(f), hc.request_frames(2)
    want, heads, _ = _head_engine(monkeypatch, oracle, path, dtype, f.conf_thr, frames, uniform=f)
    for i, head in enumerate(heads):
        cls, best, ok = hc.decode_head(head, f.conf_thr)
        passes = []
        for lv, sl in zip(f.levels, hc.level_slices()):
            for c in lv.tied[1:]:                                  # a tie is a tie: the tied classes' scores are bit-equal in the head tensor
                assert np.array_equal(head[4 + c, sl], head[4 + lv.tied[0], sl]), (lv.name, c)
            assert (head[4:, sl] == head[4:, sl][:, :1]).all(), lv.name             # uniform: every anchor of the level scores alike
            assert ok[sl].all() or not ok[sl].any(), lv.name
            passes.append(bool(ok[sl][0]))
            assert lv.passes is None or lv.passes == passes[-1], (lv.name, float(best[sl][0]))
        hc.check_uniform_outcome(f, passes, cls[ok], want[i][3])
        print(f"{f.key} frame {i}: levels pass {passes}, best scores {[float(best[sl][0]) for sl in hc.level_slices()]}, n_kept {want[i][2]}")
    _both_productions(monkeypatch, want, path, dtype, f.conf_thr, frames, f.key)


# ---------------------------------------------------------------------------------------------------
# conf_thr at a score, one step above, one step below
# ---------------------------------------------------------------------------------------------------
def _equality(monkeypatch, oracle, path, f, dtype, level, frames, floor=None):
    """s = the engine's own score of the level's tied classes; engines at s, nextafter(s, 1), nextafter(s, 0): all anchors, none, all"""
    head = _head_engine(monkeypatch, oracle, path, dtype, 0.5, frames, uniform=f)[1][0]
    sl, lv = hc.level_slices()[level], f.levels[level]
    s = head[4 + lv.want_cls, sl][0]
    assert (head[4 + lv.want_cls, sl] == s).all() and all(np.array_equal(head[4 + c, sl], head[4 + lv.want_cls, sl]) for c in lv.tied)
    if floor is not None:
        assert s >= floor, (lv.name, float(s), float(floor))
    hw = sl.stop - sl.start
    for conf, count in ((s, hw), (np.nextafter(s, F32(1)), 0), (np.nextafter(s, F32(0)), hw)):
        want, heads, _ = _head_engine(monkeypatch, oracle, path, dtype, conf, frames, uniform=f, flags=0)
        for i in range(len(frames)):
            cls, _, ok = hc.decode_head(heads[i], conf)
            assert int(ok[sl].sum()) == count and (cls[sl][ok[sl]] == lv.want_cls).all(), (lv.name, float(conf), int(ok[sl].sum()), count)
        _both_productions(monkeypatch, want, path, dtype, conf, frames, f"{lv.name} conf {float(conf):.9g}")
    return s


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("level", range(3), ids=[n for n, _, _ in hc.EQUALITY_BIASES])
def test_threshold_at_equality(monkeypatch, oracle, uniform_paths, level, dtype):
    f = hc.equality_file()
    s = _equality(monkeypatch, oracle, uniform_paths(f), f, dtype, level, hc.request_frames(2))
    assert abs(float(s) - float(hc.score_ieee(f.levels[level].cls[f.levels[level].want_cls]))) <= cl.DECODE_SCORE_TOL


_K_LOGITS = {}


def _k_case(monkeypatch, workdir, dtype, k, scale="n"):
    """(file, path, z_of_k) for the file that holds k, on this dtype's arithmetic: the ladder engines run once per dtype"""
    if dtype not in _K_LOGITS:
        z_of_k = {}
        for ks in hc.K_FILES:
            lf = hc.ladder_file(ks)
            path = hc.write_uniform(str(workdir / f"{lf.key}_{dtype}.zlyw"), lf)
            e = _engine(monkeypatch, path, dtype, 0.5, 1)
            _detect(e, hc.request_frames(1))
            head = e.head_tensor(0)
            e.close()
            for lv, sl, kk in zip(lf.levels, hc.level_slices(), ks):
                assert (head[4:, sl] == head[4:, sl][:, :1]).all()
                z_of_k[kk] = hc.pick_from_ladder(lv.cls, head[4:, sl][:, 0], hc.thr_of_k(kk))
        _K_LOGITS[dtype] = z_of_k
        print(f"dtype {dtype}: lowest passing logits {({kk: float(z) for kk, z in z_of_k.items()})}; IEEE prediction "
              f"{({kk: float(hc.lowest_passing_z(hc.thr_of_k(kk))) for kk in z_of_k})}")
    ks = next(ks for ks in hc.K_FILES if k in ks)
    f = hc.k_file(ks, _K_LOGITS[dtype])
    path = str(workdir / f"{f.key}_{dtype}_{scale}.zlyw")
    if not os.path.exists(path):
        hc.write_uniform(path, f, scale)
    return f, path, _K_LOGITS[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", hc.K_VALUES)
def test_threshold_near_one(monkeypatch, oracle, workdir, k, dtype):
    """thr = 1 - k 2^-24 with the class logit at the lowest value that still scores thr on this engine: below logit(thr) by far more than
    1e-2 for small k, so an early-out bound of logit(thr) - 1e-2 ends every tile of the level"""
    f, path, z_of_k = _k_case(monkeypatch, workdir, dtype, k)
    thr = hc.thr_of_k(k)
    level = [lv.name for lv in f.levels].index(f"k{k}")
    gap = hc.logit64(thr) - float(z_of_k[k])
    print(f"k {k}: logit {float(z_of_k[k]):.6f}, below logit(thr) by {gap:.4f}; logit(thr) - 1e-2 = {float(hc.skip_logit_margin_only(thr)):.6f}, bound {float(hc.skip_logit(thr)):.6f}")
    assert gap > 0 and z_of_k[k] >= hc.skip_logit(thr)
    if k <= 34:
        assert z_of_k[k] < hc.skip_logit_margin_only(thr)          # the case bites: the earlier bound would have ended these tiles
    _equality(monkeypatch, oracle, path, f, dtype, level, hc.request_frames(2), floor=thr)


# ---------------------------------------------------------------------------------------------------
# graded cases
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def graded(workdir, oracle):
    paths, frames, _ = hc.write_graded(workdir, oracle)
    return paths, frames


def _graded_reference(monkeypatch, oracle, graded, thr, dtype):
    paths, frames = graded
    want, heads, taps = _head_engine(monkeypatch, oracle, paths[float(thr)], dtype, thr, frames)
    pop = hc.populations(list(zip(heads, taps)), thr)
    print(f"thr {float(thr):.9g} dtype {dtype}: {pop}, candidates {[s[3] for s in want]}, kept {[s[2] for s in want]}")
    hc.check_populations(pop, thr)                                # a case that stopped biting fails
    return paths[float(thr)], frames, want


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("thr", hc.GRADED_THRESHOLDS, ids=lambda t: f"{float(t):.9g}")
def test_graded(monkeypatch, oracle, graded, thr, dtype):
    path, frames, want = _graded_reference(monkeypatch, oracle, graded, thr, dtype)
    _both_productions(monkeypatch, want, path, dtype, thr, frames, f"graded {float(thr):.9g}")


# ---------------------------------------------------------------------------------------------------
# the production engine's other forms
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_one_tail_and_tails_on_lanes(monkeypatch, oracle, workdir, graded, dtype):
    """batch 16 (the Detect branches run on side streams from there): FLAG_SINGLE_CHAIN = one tail launch, else one per level; the graded
    head at the high threshold and the k = 18 file at its threshold, captured graph and eager launches"""
    thr = hc.thr_of_k(18)
    _, kpath, _ = _k_case(monkeypatch, workdir, dtype, 18)
    frames = hc.request_frames(16)
    for path, uniform in ((graded[0][float(thr)], None), (kpath, hc.k_file(hc.K_FILES[0], _K_LOGITS[dtype]))):
        want, _, _ = _head_engine(monkeypatch, oracle, path, dtype, thr, frames, uniform=uniform)
        assert sum(s[3] for s in want) > 0
        for chain, launches in ((zly.FLAG_SINGLE_CHAIN, 1), (0, 3)):
            for graph in (True, False):
                e = _production_equals(monkeypatch, want, path, dtype, thr, frames, flags=chain, use_graph=graph, what=f"chain {chain} graph {graph}")
                assert len(_tail_launches(e, 16)) == launches, _kernels(e, 16)
                e.close()


TAIL_ENV = {"ZLY_WS_MIN_TILES": "1", "ZLY_LDS_MIN_TILES": "1"}


@pytest.mark.parametrize("case", ["graded_0.25", "graded_high", "k18"])
def test_box_conv_in_the_tail(monkeypatch, oracle, workdir, graded, case):
    """352 x 288, batch 5 (maps of 44 x 36, 22 x 18, 11 x 9; bf16): with ZLY_TAIL_BOX 1 (automatic) and 2 (forced) the surviving waves compute
    cv2.L.1 themselves and lanes below the early-out bound are masked; the head-tensor engine with ZLY_TAIL_BOX=0 is the reference"""
    w, h, n, dtype = 352, 288, 5, zly.DTYPE_BF16
    frames = hc.request_frames(n, sizes=((352, 288), (400, 300), (200, 150)))
    if case == "k18":
        thr = hc.thr_of_k(18)
        f, path, _ = _k_case(monkeypatch, workdir, dtype, 18)
    else:
        thr = hc.GRADED_THRESHOLDS[0] if case == "graded_0.25" else hc.thr_of_k(18)
        f, path = None, graded[0][float(thr)]
    want, _, _ = _head_engine(monkeypatch, oracle, path, dtype, thr, frames, uniform=f, env=dict(TAIL_ENV, ZLY_TAIL_BOX="0"), w=w, h=h)
    assert sum(s[3] for s in want) > 0
    for mode in ("0", "1", "2"):
        for graph in (True, False):
            e = _production_equals(monkeypatch, want, path, dtype, thr, frames, env=dict(TAIL_ENV, ZLY_TAIL_BOX=mode), use_graph=graph, w=w, h=h,
                                   what=f"ZLY_TAIL_BOX={mode} graph {graph}")
            lv = _box_levels(e, n)
            assert (lv == []) if mode == "0" else len(lv) >= 1, (mode, _kernels(e, n))
            e.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_letterbox(monkeypatch, oracle, graded, dtype):
    """FLAG_LETTERBOX on non-square frames: the survivors' boxes are mapped out of the letterbox; expected values through unpad_head"""
    thr = hc.thr_of_k(18)
    frames = hc.request_frames(3, seed=91, sizes=((300, 120), (90, 200), (160, 128)))
    want, _, _ = _head_engine(monkeypatch, oracle, graded[0][float(thr)], dtype, thr, frames, letterbox=True)
    assert sum(s[3] for s in want) > 0
    _production_equals(monkeypatch, want, graded[0][float(thr)], dtype, thr, frames, flags=zly.FLAG_LETTERBOX, what="letterbox").close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_yolov8s(monkeypatch, oracle, workdir, dtype):
    """YOLOv8-s: a 128-channel class branch (four k-steps in bf16, eight in fp32) in front of the same decisions"""
    spec = zm.build_spec("s")
    assert {c.name: c for c in spec.convs}["model.22.cv3.0.2"].cin == 128
    f, path, _ = _k_case(monkeypatch, workdir, dtype, 18, scale="s")
    thr, frames = hc.thr_of_k(18), hc.request_frames(2)
    want, _, _ = _head_engine(monkeypatch, oracle, path, dtype, thr, frames, uniform=f)
    hw = [sl.stop - sl.start for sl in hc.level_slices()]
    assert [s[3] for s in want] == [hw[0] + hw[1] + hw[2]] * 2          # 1 - 18 2^-24 is the lowest threshold of the file: every level passes
    _both_productions(monkeypatch, want, path, dtype, thr, frames, "yolov8s")
