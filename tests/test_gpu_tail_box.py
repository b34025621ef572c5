"""The Detect box branch's second conv inside the tail (run on the MI355X box: pytest -m gpu): with ZLY_TAIL_BOX the three dense model.22.cv2.L.1
launches (64 -> 64, 3x3) are gone and head_fused_kernel computes that conv itself, for the 16 anchors of a wave that survives its early-out, in the
k-step order of the dense kernel the planner would have launched -- so everything must be BIT-IDENTICAL to the engine with ZLY_TAIL_BOX=0.

Every case builds one engine with the mode and one without (the switch is read per engine at create), asserts through op_kernels which levels
took it, and requires np.array_equal / equal bytes.  In the forced cases the levels that took it must be EXACTLY those whose dense launch in the
off engine is one of the two kernels whose k-step order the tail carries: a silent fall-back to the dense launch fails the test.  What the shapes are for:
  * 416 x 416, n = 16 forced (ZLY_TAIL_BOX=2: also engines that write the head tensor, every anchor computed): exactly the weight-stationary
    kernel's pixel gate, so P3 and P4 must take the mode; head tensor of forward(), and with FLAG_DUMP_LOGITS the cv2.L.1 / cv2.L.2 taps;
  * 352 x 288, n = 5 and 224 x 416, n = 4 with ZLY_WS_MIN_TILES=1, ZLY_LDS_MIN_TILES=1: maps of 44 x 36, 22 x 18, 11 x 9 and 28 x 52, 14 x 26, 7 x 13 --
    anchors on all four borders, 16-anchor tiles that straddle two or three map rows, last tiles past H * W; all three levels qualify and both
    k-step orders (conv3x3_ws_kernel's and conv3x3_lds_kernel's) occur;
  * YOLOv8-s at 320 x 256, n = 3: c2 = 64 with a 128-channel class branch (another LDS split in the tail);
  * production mode (FLAG_NO_HEAD_TENSOR, automatic): only surviving waves compute, lanes below the threshold are masked; slab headers and
    detections bytewise, one tail launch (FLAG_SINGLE_CHAIN) and per-level tails on the side streams, captured graph and eager launches;
  * the gates, and the launch introspection's three invariants on an engine that has the mode."""
import numpy as np
import pytest
import torch

import zly
import zly_model as zm

pytestmark = pytest.mark.gpu

SWITCHES = ("ZLY_TAIL_BOX", "ZLY_TAIL_BOX_MIN_CONF", "ZLY_WS_MIN_TILES", "ZLY_LDS_MIN_TILES", "ZLY_NO_DET_MERGE")
NOTE = "(computed in the Detect tail at surviving anchors)"
BOX1 = [f"model.22.cv2.{l}.1" for l in range(3)]


def _engine(monkeypatch, env, path, **kw):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return zly.Engine(path, warmup_runs=0, **kw)


def _kernels(e, n):
    return {o["name"].split("+")[0]: k for o, k in zip(e.ops(), e.op_kernels(n))}


def _levels(e, n):
    kern = _kernels(e, n)
    return [l for l in range(3) if kern[BOX1[l]] == NOTE]


def _forced_on_off(monkeypatch, path, w, h, n, env, need_levels, need_orders=()):
    """ZLY_TAIL_BOX=2 against ZLY_TAIL_BOX=0 under the switches `env`, without and with FLAG_DUMP_LOGITS: head tensor and taps of every frame"""
    frames = zm.synth_frames(n, w, h, seed=37, rects=False)
    x = None
    for flags in (0, zly.FLAG_DUMP_LOGITS):
        on = _engine(monkeypatch, dict(env, ZLY_TAIL_BOX="2"), path, model_w=w, model_h=h, max_batch=n, flags=flags)
        if x is None:
            x = np.stack([on.preprocess(f) for f in frames])
        lv = _levels(on, n)
        assert set(need_levels) <= set(lv), (lv, _kernels(on, n))
        taps = [f"model.22.cv2.{l}.{j}" for l in lv for j in (1, 2)] if flags else []
        got_head = on.forward(x)
        got = {nm: [on.tap(nm, i) for i in range(n)] for nm in taps}
        if not flags:                                            # without the dump flag the conv's output exists at no anchor
            with pytest.raises(zly.ZlyError):
                on.tap(BOX1[lv[0]], 0)
        on.close()
        off = _engine(monkeypatch, dict(env, ZLY_TAIL_BOX="0"), path, model_w=w, model_h=h, max_batch=n, flags=flags)
        kern = _kernels(off, n)
        assert _levels(off, n) == [] and not any("box conv" in k for k in kern.values()), kern
        # no silent fall-back to the dense launch: a level takes the mode exactly where the off engine launches one of the two kernels whose
        # k-step order the tail carries (the direct kernel, split-K or not, and the row-tile form stay dense)
        carried = [l for l in range(3) if kern[BOX1[l]].startswith("conv3x3_lds_kernel<") or
                   (kern[BOX1[l]].startswith("conv3x3_ws_kernel<") and "ROWT" not in kern[BOX1[l]])]
        assert lv == carried, (lv, kern)
        for fam in need_orders:                                  # both k-step orders must be under test
            assert any(kern[BOX1[l]].startswith(fam) for l in lv), (fam, kern)
        want_head = off.forward(x)
        want = {nm: [off.tap(nm, i) for i in range(n)] for nm in taps}
        off.close()
        for nm in taps:
            for i in range(n):
                assert got[nm][i].shape == want[nm][i].shape and np.array_equal(got[nm][i], want[nm][i]), (flags, nm, i)
                assert np.isfinite(want[nm][i]).all() and np.abs(want[nm][i]).max() > 0, (flags, nm, i)
        for i in range(n):
            assert np.array_equal(got_head[i], want_head[i]), (flags, i)


def test_forced_416_batch16(monkeypatch):
    _forced_on_off(monkeypatch, None, 416, 416, 16, {}, need_levels=(0, 1))


@pytest.mark.parametrize("w,h,n", [(352, 288, 5), (224, 416, 4)])
def test_ragged_maps(monkeypatch, w, h, n):
    _forced_on_off(monkeypatch, None, w, h, n, {"ZLY_WS_MIN_TILES": "1", "ZLY_LDS_MIN_TILES": "1", "ZLY_NO_DET_MERGE": "1"} if n <= 4 else
                   {"ZLY_WS_MIN_TILES": "1", "ZLY_LDS_MIN_TILES": "1"}, need_levels=(0, 1, 2),
                   need_orders=("conv3x3_ws_kernel<", "conv3x3_lds_kernel<") if n > 4 else ())


def test_both_orders_occur(monkeypatch):
    """over the two ragged cases together both k-step orders are exercised: asserted from the kernel names of the off engines"""
    fams = set()
    for (w, h, n) in ((352, 288, 5), (224, 416, 4)):
        env = {"ZLY_WS_MIN_TILES": "1", "ZLY_LDS_MIN_TILES": "1", "ZLY_TAIL_BOX": "0"}
        if n <= 4:
            env["ZLY_NO_DET_MERGE"] = "1"
        off = _engine(monkeypatch, env, None, model_w=w, model_h=h, max_batch=n)
        kern = _kernels(off, n)
        off.close()
        fams |= {kern[nm].split("<")[0] for nm in BOX1}
    assert {"conv3x3_ws_kernel", "conv3x3_lds_kernel"} <= fams, fams


def test_yolov8s(monkeypatch, tmp_path):
    spec = zm.build_spec("s")
    by_name = {c.name: c for c in spec.convs}
    assert spec.head_c2 == 64 and by_name["model.22.cv3.0.2"].cin == 128          # the tail's 128-channel class GEMM (four k-steps, not three)
    path = str(tmp_path / "yolov8s_synth.zlyw")
    zm.write_zlyw(path, spec, zm.synth_weights(spec))
    _forced_on_off(monkeypatch, path, 320, 256, 3, {"ZLY_WS_MIN_TILES": "1", "ZLY_LDS_MIN_TILES": "1", "ZLY_NO_DET_MERGE": "1"}, need_levels=(0, 1, 2))


def _raw_slabs(e, n):
    raw = np.zeros(n * e.slab_bytes, dtype=np.uint8)
    zly._check(e.lib, e.lib.zly_read_slabs(e.h, n, raw.ctypes.data))
    return raw


def _slab_bytes(e, n):
    """per frame: the header's bytes and the bytes of the n_kept detections behind it"""
    raw = _raw_slabs(e, n)
    out = []
    for i, (hdr, dets) in enumerate(zly.parse_slabs(raw, n, e.max_dets)):
        out.append((hdr.tobytes(), dets.tobytes(), int(hdr["n_kept"]), int(hdr["n_candidates"])))
    return out


@pytest.mark.parametrize("conf", [0.25, 0.5])
@pytest.mark.parametrize("chain", [zly.FLAG_SINGLE_CHAIN, 0], ids=["one_tail", "tails_on_lanes"])
def test_production_mode(monkeypatch, conf, chain):
    n = 16
    dev = torch.from_numpy(zm.synth_frames(n, 416, 416, seed=43, rects=False)).cuda()
    torch.cuda.synchronize()
    flags = zly.FLAG_NO_HEAD_TENSOR | chain
    res = {}
    for name, env, graph in (("on", {}, True), ("on_eager", {}, False), ("off", {"ZLY_TAIL_BOX": "0"}, True)):
        e = _engine(monkeypatch, env, None, max_batch=n, max_dets=64, conf_thr=conf, flags=flags, use_graph=graph)
        lv = _levels(e, n)
        kern = _kernels(e, n)
        if name == "off":
            assert lv == [], kern
        else:
            assert {0, 1} <= set(lv), kern
            tails = {nm: k for nm, k in kern.items() if k.startswith("head_fused_kernel")}
            assert len(tails) == (1 if chain else 3), kern
            for nm, k in tails.items():                              # the launch that stands for a level names the order it carries
                for l in lv:
                    if chain or f"detect.tail.P{3 + l}" in nm:
                        assert f"P{3 + l}:" in k, (nm, k)
        for rep in range(2):                                     # twice: the second call replays the captured graph
            e.detect_device(dev.data_ptr(), n, 416, 416, tag0=5)
            res[(name, rep)] = _slab_bytes(e, n)
        e.close()
    want = res[("off", 0)]
    assert sum(k for _, _, k, _ in want) > 0
    for key, got in res.items():
        for i in range(n):
            assert got[i][3] == want[i][3], (key, i, got[i][3], want[i][3])          # n_candidates
            assert got[i][0] == want[i][0] and got[i][1] == want[i][1], (key, i)


def test_gates(monkeypatch):
    prod = zly.FLAG_NO_HEAD_TENSOR
    e = _engine(monkeypatch, {"ZLY_TAIL_BOX_MIN_CONF": "0.3"}, None, max_batch=16, conf_thr=0.25, flags=prod)
    assert _levels(e, 16) == []                                  # threshold below the floor
    e.close()
    e = _engine(monkeypatch, {"ZLY_TAIL_BOX_MIN_CONF": "0.3"}, None, max_batch=16, conf_thr=0.5, flags=prod)
    assert {0, 1} <= set(_levels(e, 16))
    assert _levels(e, 4) == []                                   # the merged latency-path launch stays
    e.close()
    e = _engine(monkeypatch, {}, None, max_batch=16, conf_thr=0.5)
    assert _levels(e, 16) == []                                  # automatic mode: an engine that writes the head tensor has no early-out
    e.close()
    e = _engine(monkeypatch, {"ZLY_TAIL_BOX": "2"}, None, max_batch=16, flags=zly.FLAG_NO_FUSION)
    assert _levels(e, 16) == []
    e.close()
    e = _engine(monkeypatch, {"ZLY_TAIL_BOX": "2"}, None, max_batch=16, dtype=zly.DTYPE_FP32)
    assert _levels(e, 16) == []
    e.close()
    e = _engine(monkeypatch, {}, None, max_batch=16, conf_thr=0.5, flags=prod)
    frames = torch.from_numpy(zm.synth_frames(16, 416, 416, seed=3, rects=False)).cuda()
    torch.cuda.synchronize()
    e.detect_device(frames.data_ptr(), 16, 416, 416)
    e.read_slabs(16)
    lv = _levels(e, 16)
    assert lv
    with pytest.raises(zly.ZlyError):
        e.tap(BOX1[lv[0]], 0)
    e.close()


def test_launch_introspection(monkeypatch):
    """test_launch_introspection_agrees' three invariants on an engine whose tail covers the box convs"""
    e = _engine(monkeypatch, {}, None, max_batch=64, flags=zly.FLAG_NO_HEAD_TENSOR | zly.FLAG_SINGLE_CHAIN)
    frames = torch.from_numpy(zm.synth_frames(64, 416, 416, seed=17, rects=False)).cuda()
    torch.cuda.synchronize()
    info = e.ops()
    for n in (5, 16, 64):
        kern, lau = e.op_kernels(n), e.launches(n)
        ms = e.profile_ops(frames.data_ptr(), n, 416, 416, reps=2)
        for i, (k, li) in enumerate(zip(kern, lau)):
            by = li["covered_by"]
            assert (by != i) == k.startswith("("), (n, i, k, by)
            assert lau[by]["covered_by"] == by, (n, i, k, by)
            assert (ms[i] == 0) == (by != i), (n, i, k, float(ms[i]))
        if n >= 16:
            covered = [i for i, k in enumerate(kern) if k == NOTE]
            assert len(covered) >= 2, kern
            tail = lau[covered[0]]["covered_by"]
            assert kern[tail].startswith("head_fused_kernel") and all(lau[i]["covered_by"] == tail for i in covered)
            # the covered convs' dense flops are work that is not done: the tail launch books the three tail ops only
            tails = [i for i, o in enumerate(info) if o["name"].startswith("detect.tail")]
            assert abs(lau[tail]["flops_per_frame"] - sum(info[i]["flops"] for i in tails)) < 1.0, (n, lau[tail])
            # its box input is booked: the 64-channel bf16 box half of the stem buffer at every anchor of a covered level
            hw = {"model.22.cv2.0.1": 52 * 52, "model.22.cv2.1.1": 26 * 26, "model.22.cv2.2.1": 13 * 13}
            stem_half = sum(hw[info[i]["name"].split("+")[0]] * 64 * 2 for i in covered)
            plain = sum(info[i]["bytes"] for i in tails)
            assert lau[tail]["bytes_fused_per_frame"] >= stem_half and abs(lau[tail]["bytes_unfused_per_frame"] - plain) < 1.0, (n, lau[tail], stem_half, plain)
    e.close()
