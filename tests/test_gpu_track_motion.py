"""track_motion_kernel behind the C ABI (include/zly.h, "tracking": zly_track_motion_enable, zly_track_read) against the numpy oracle
tests/track_motion_ref.py, bit for bit -- ids, tables and velocities -- in the manner of tests/test_gpu_track.py: crafted slabs
(tests/track_motion_cases.py, tests/track_cases.py) handed to zly_track_slabs, the moving scenes in every composition of calls, and real frames
through the device path with deferred NMS and through the pipelined submit path.  A motion engine with v_max = 0 must give the PLAIN oracle's
bytes on every case and scene of tests/track_cases.py: the new kernel against the old yardstick.  Engines are the suite's smallest (yolov8n at 64 x 64).
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch            # before the first engine: the process then uses torch's HIP runtime throughout, as tests/test_gpu_parity.py does

import track_cases as tc
import track_motion_cases as mc
import track_motion_ref as mr
import track_ref
import zly

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "zly_golden_64.npz"))
CONF, IOU = float(G["conf"]), float(G["iou"])
MAX_STREAMS = 8
HAND = mc.hand_cases()
PLAIN_HAND = tc.hand_cases()
_ENGINES = {}


@pytest.fixture(scope="module")
def engine_for(weights_path):
    """engines by (cap, T, match_iou, max_lost, beta, v_max); beta = None: tracking without the motion model.  Every stream is reset on the way out"""
    def get(cap, T, match_iou, max_lost, beta=0.5, v_max=0.25):
        key = (cap, T, float(np.float32(match_iou)), max_lost, beta, v_max)
        if key not in _ENGINES:
            e = zly.Engine(weights_path, model_w=64, model_h=64, max_batch=64, max_dets=cap, warmup_runs=0, use_graph=False)
            e.track_enable(max_streams=MAX_STREAMS, max_tracks=T, match_iou=match_iou, max_lost=max_lost)
            if beta is not None:
                e.track_motion_enable(beta=beta, v_max=v_max)
            _ENGINES[key] = e
        e = _ENGINES[key]
        e.track_reset(-1, 1)
        return e
    yield get
    for e in _ENGINES.values():
        e.close()
    _ENGINES.clear()


def _track(e, raw, streams):
    """one zly_track_slabs call on a device copy of raw -> the slabs afterwards"""
    d = torch.from_numpy(raw).cuda()
    torch.cuda.synchronize()
    e.track_slabs(streams, d.data_ptr())
    e.sync()
    return d.cpu().numpy()


def _diff(got, want, cap, what):
    if np.array_equal(got, want):
        return None
    i = int(np.flatnonzero((got != want).any(axis=1))[0])
    return f"{what}: slab {i}: ids {tc.slab_ids(got[i], cap).tolist()} want {tc.slab_ids(want[i], cap).tolist()}; bytes differ at {np.flatnonzero(got[i] != want[i])[:8].tolist()}"


def _same_tracks(got, want):
    """zly_track_read against the oracle's read(): every field bit for bit (vx, vy as their uint32 views, like the rest of the record)"""
    assert got.dtype == want.dtype == zly.TRACK_DTYPE
    assert len(got) == len(want), (len(got), len(want))
    for name in zly.TRACK_DTYPE.names:
        a, b = np.ascontiguousarray(got[name]).view(np.uint32), np.ascontiguousarray(want[name]).view(np.uint32)
        assert np.array_equal(a, b), (name, got[name].tolist(), want[name].tolist())


@pytest.mark.parametrize("case", HAND, ids=[c.name for c in HAND])
def test_hand_case(engine_for, case):
    e = engine_for(case.cap, case.T, case.match_iou, case.max_lost, case.beta, case.v_max)
    raw = tc.build_slabs(case.frames, case.cap)
    want = tc.with_ids(raw, [np.array(w, dtype=np.uint32) for w in case.want], case.cap)
    n = len(case.frames)
    # stream 0: one frame per call
    rows = []
    for k in range(n):
        if k in case.reset_before:
            e.track_reset(0, 0)
        rows.append(_track(e, raw[k:k + 1], [0]))
    got = np.concatenate(rows)
    assert np.array_equal(got, want), _diff(got, want, case.cap, case.name)
    # stream 3: the whole sequence in one call (one call per stretch between the case's resets)
    cuts = [0] + list(case.reset_before) + [n]
    rows = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        if a:
            e.track_reset(3, 0)
        rows.append(_track(e, raw[a:b], [3] * (b - a)))
    got = np.concatenate(rows)
    assert np.array_equal(got, want), _diff(got, want, case.cap, case.name + " in one call")
    o = mc.case_trackers(case)[0]
    mc.run_case(case, o)
    for s in (0, 3):
        assert e.track_state(s) == o.state()
        _same_tracks(e.track_read(s), o.read())
    assert e.track_state(1)["frame_no"] == 0 and len(e.track_read(1)) == 0


# ---- v_max = 0: the motion kernel against the plain oracle ------------------------------------------------------------------------
def _same_plain_table(e, s, p):
    """a v_max = 0 motion engine's table against the plain oracle's: boxes, classes, ids, last_seen; velocities are zeros of either sign"""
    assert e.track_state(s) == p.state()
    live = [t for t in range(p.T) if p.live[t]]
    r = e.track_read(s)
    assert r["id"].tolist() == [p.id[t] for t in live] and r["last_seen"].tolist() == [p.last_seen[t] for t in live]
    assert r["class_id"].tolist() == [p.cls[t] for t in live]
    for k, name in enumerate("xywh"):
        assert np.array_equal(r[name].view(np.uint32), np.array([p.box[t][k] for t in live], dtype=np.float32).view(np.uint32))
    assert not np.abs(r["vx"]).any() and not np.abs(r["vy"]).any() and (r["hits"] >= 1).all()


@pytest.mark.parametrize("case", PLAIN_HAND, ids=[c.name for c in PLAIN_HAND])
def test_v_max_0_gives_the_plain_bytes_on_the_plain_hand_cases(engine_for, case):
    e = engine_for(case.cap, case.T, case.match_iou, case.max_lost, 0.5, 0.0)
    if case.first_id:
        e.track_reset(-1, case.first_id)
    raw = tc.build_slabs(case.frames, case.cap, case.n_kept)
    want = tc.with_ids(raw, [np.array(w, dtype=np.uint32) for w in case.want], case.cap)
    got = np.concatenate([_track(e, raw[k:k + 1], [0]) for k in range(len(case.frames))])
    assert np.array_equal(got, want), _diff(got, want, case.cap, case.name)
    got = _track(e, raw, [3] * len(case.frames))
    assert np.array_equal(got, want), _diff(got, want, case.cap, case.name + " in one call")
    o = track_ref.Tracker(case.T, case.cap, case.match_iou, case.max_lost)
    if case.first_id:
        o.reset(case.first_id)
    for k, f in enumerate(case.frames):
        o.step(f, None if case.n_kept is None else case.n_kept[k])
    _same_plain_table(e, 0, o)
    _same_plain_table(e, 3, o)


@pytest.mark.parametrize("sc", tc.SCENES, ids=[s.name for s in tc.SCENES])
def test_v_max_0_gives_the_plain_bytes_on_the_plain_scenes(engine_for, sc):
    frames, ids, trackers = tc.scene(sc)
    e = engine_for(sc.cap, sc.T, sc.match_iou, sc.max_lost, 0.5, 0.0)
    # the scene's streams interleaved, 16 frames per call
    inter = [(s, k) for k in range(sc.n_frames) for s in range(sc.n_streams)]
    for ci in range(0, len(inter), 16):
        call = inter[ci:ci + 16]
        raw = tc.build_slabs([frames[s][k] for s, k in call], sc.cap, tag0=tc.TAG0 + ci)
        want = tc.with_ids(raw, [ids[s][k] for s, k in call], sc.cap)
        got = _track(e, raw, [s for s, _ in call])
        assert np.array_equal(got, want), _diff(got, want, sc.cap, f"{sc.name}, call at {ci}")
    for s in range(sc.n_streams):
        _same_plain_table(e, s, trackers[s])


# ---- the moving scenes in every composition of calls ------------------------------------------------------------------------------
def _compositions(sc):
    """name -> list of calls; a call is a list of (stream, frame index | None for an untracked filler): tests/test_gpu_track.py's compositions"""
    S, Kf = sc.n_streams, sc.n_frames
    rng = np.random.default_rng(sc.seed)
    seq = [s for s in range(S) for _ in range(Kf)]
    rng.shuffle(seq)
    nxt = [0] * S
    inter = []
    for s in seq:
        inter.append((s, nxt[s]))
        nxt[s] += 1
    out = {"one_frame_per_call": [[(s, k)] for k in range(Kf) for s in range(S)],
           "whole_stream_per_call": [[(s, k) for k in range(Kf)] for s in range(S)]}
    for n in (1, 3, 16, 64):
        out[f"interleaved_n{n}"] = [inter[i:i + n] for i in range(0, len(inter), n)]
    mixed = []
    for item in inter:
        if rng.random() < .3:
            mixed.append((-1, None))
        mixed.append(item)
    out["with_untracked_n16"] = [mixed[i:i + 16] for i in range(0, len(mixed), 16)]
    return out


COMPOSITIONS = ["one_frame_per_call", "whole_stream_per_call", "interleaved_n1", "interleaved_n3", "interleaved_n16", "interleaved_n64", "with_untracked_n16"]


@pytest.mark.parametrize("comp", COMPOSITIONS)
@pytest.mark.parametrize("sc", mc.SCENES, ids=[s.name for s in mc.SCENES])
def test_moving_scene_obeys_the_rule(engine_for, sc, comp):
    frames, _, ids, trackers, _ = mc.scene(sc)
    e = engine_for(sc.cap, sc.T, sc.match_iou, sc.max_lost, sc.beta, sc.v_max)
    for ci, call in enumerate(_compositions(sc)[comp]):
        fl = [frames[s][k] if s >= 0 else frames[0][0] for s, k in call]
        raw = tc.build_slabs(fl, sc.cap, tag0=tc.TAG0 + 100 * ci)
        want = tc.with_ids(raw, [ids[s][k] if s >= 0 else None for s, k in call], sc.cap)
        got = _track(e, raw, [s for s, _ in call])
        assert np.array_equal(got, want), _diff(got, want, sc.cap, f"{sc.name} / {comp}, call {ci} = {call}")
    for s in range(sc.n_streams):
        assert e.track_state(s) == trackers[s].state(), (sc.name, comp, s)
        _same_tracks(e.track_read(s), trackers[s].read())
    for s in range(sc.n_streams, MAX_STREAMS):
        assert e.track_state(s) == dict(frame_no=0, next_id=1, n_live=0, evictions=0) and len(e.track_read(s)) == 0


def test_reset_of_one_stream_clears_its_velocities_and_no_others(engine_for):
    sc = mc.SCENES[0]
    frames, _, ids, trackers, _ = mc.scene(sc)
    e = engine_for(sc.cap, sc.T, sc.match_iou, sc.max_lost, sc.beta, sc.v_max)
    half = sc.n_frames // 2
    o = [mr.MotionTracker(sc.T, sc.cap, sc.match_iou, sc.max_lost, sc.beta, sc.v_max) for _ in range(sc.n_streams)]
    for s in range(sc.n_streams):
        raw = tc.build_slabs(frames[s][:half], sc.cap)
        assert np.array_equal(_track(e, raw, [s] * half), tc.with_ids(raw, [o[s].step(f) for f in frames[s][:half]], sc.cap))
    assert all(np.abs(o[s].read()["vx"]).max() > 0 for s in range(sc.n_streams))          # there are velocities to clear, and to keep
    e.track_reset(1, 0)
    o[1].reset(0)
    assert len(e.track_read(1)) == 0 and e.track_state(1) == o[1].state()
    for s in (0, 2, 3):
        _same_tracks(e.track_read(s), o[s].read())
    # the second half: the reset stream starts at rest with its kept next id (stale velocities in its slots would show in the ids and in
    # track_read), the others go on as if nothing had happened
    for s in range(sc.n_streams):
        raw = tc.build_slabs(frames[s][half:], sc.cap)
        got = _track(e, raw, [s] * (sc.n_frames - half))
        want = tc.with_ids(raw, [o[s].step(f) for f in frames[s][half:]], sc.cap)
        assert np.array_equal(got, want), _diff(got, want, sc.cap, f"stream {s} after the reset of stream 1")
        _same_tracks(e.track_read(s), o[s].read())
    for s in (0, 2, 3):
        assert e.track_state(s) == trackers[s].state()
    e.track_reset(-1, 0)
    for s in range(MAX_STREAMS):
        assert len(e.track_read(s)) == 0


def test_engine_without_the_model_reads_zero_velocities_and_gives_plain_ids(engine_for):
    sc = mc.SCENES[0]
    frames, _, ids, _, plain_ids = mc.scene(sc)
    assert any(a.tolist() != b.tolist() for s in range(sc.n_streams) for a, b in zip(ids[s], plain_ids[s]))      # the model matters on this scene
    e = engine_for(sc.cap, sc.T, sc.match_iou, sc.max_lost, None, None)
    for s in range(sc.n_streams):
        raw = tc.build_slabs(frames[s], sc.cap)
        got = _track(e, raw, [s] * sc.n_frames)
        want = tc.with_ids(raw, plain_ids[s], sc.cap)
        assert np.array_equal(got, want), _diff(got, want, sc.cap, f"stream {s}")
        p = track_ref.Tracker(sc.T, sc.cap, sc.match_iou, sc.max_lost)
        for f in frames[s]:
            p.step(f)
        live = [t for t in range(p.T) if p.live[t]]
        r = e.track_read(s)
        assert len(live) >= 1 and r["id"].tolist() == [p.id[t] for t in live] and r["last_seen"].tolist() == [p.last_seen[t] for t in live]
        for k, name in enumerate("xywh"):
            assert np.array_equal(r[name].view(np.uint32), np.array([p.box[t][k] for t in live], dtype=np.float32).view(np.uint32))
        for name in ("vx", "vy", "hits"):
            assert not np.ascontiguousarray(r[name]).view(np.uint32).any(), name


def test_errors_change_nothing(weights_path):
    lib = zly.load_library()
    I, A = zly.ERR_INVALID_ARGUMENT, C.byref
    e = zly.Engine(weights_path, model_w=64, model_h=64, max_batch=8, max_dets=8, warmup_runs=0, use_graph=False)

    def refused(rc):
        assert rc == I and lib.zly_last_error()

    def cfg(**kw):
        c = zly.TrackMotionConfig()
        lib.zly_default_track_motion_config(A(c))
        for k, v in kw.items():
            setattr(c, k, v)
        return c
    d0 = cfg()
    assert d0.beta == 0.5 and d0.v_max == 0.25
    out, n = np.zeros(8, dtype=zly.TRACK_DTYPE), C.c_int32(-7)
    # before zly_track_enable
    refused(lib.zly_track_motion_enable(e.h, A(cfg())))
    refused(lib.zly_track_read(e.h, 0, out.ctypes.data, 8, A(n)))
    e.track_enable(max_streams=2, max_tracks=8, max_lost=2)
    refused(lib.zly_track_motion_enable(e.h, None))
    for bad in (dict(beta=0.0), dict(beta=1.5), dict(beta=float("nan")), dict(v_max=-1.0), dict(v_max=float("inf")), dict(v_max=float("nan"))):
        refused(lib.zly_track_motion_enable(e.h, A(cfg(**bad))))
    # none of the refused calls switched the model on: the accelerating box is lost the way the plain tracker loses it
    case = next(c for c in HAND if c.name == "accelerating_box_keeps_id")
    raw = tc.build_slabs(case.frames, case.cap)
    got = _track(e, raw, [0] * len(case.frames))
    assert np.array_equal(got, tc.with_ids(raw, [np.array(w, dtype=np.uint32) for w in case.plain], case.cap))
    assert lib.zly_track_motion_enable(e.h, A(cfg())) == zly.OK
    # enabling reset the streams as zly_track_reset(e, -1, 0) does: empty tables, next_id kept
    assert e.track_state(0) == dict(frame_no=0, next_id=7, n_live=0, evictions=0) and len(e.track_read(0)) == 0
    refused(lib.zly_track_motion_enable(e.h, A(cfg())))
    refused(lib.zly_track_motion_enable(e.h, A(cfg(beta=0.25))))
    for bad in (-1, 2):
        refused(lib.zly_track_read(e.h, bad, out.ctypes.data, 8, A(n)))
    refused(lib.zly_track_read(e.h, 0, out.ctypes.data, 8, None))
    assert n.value == -7
    # tracking afterwards gives the motion oracle's ids, with the defaults the second enable could not change
    e.track_reset(-1, 1)
    got = _track(e, raw, [1] * len(case.frames))
    assert np.array_equal(got, tc.with_ids(raw, [np.array(w, dtype=np.uint32) for w in case.want], case.cap))
    o = mc.case_trackers(case)[0]
    mc.run_case(case, o)
    _same_tracks(e.track_read(1), o.read())
    # cap below the live count: the first cap slots and the full count
    row = tc.build_slabs([tc.dets(tc.ROW8[:5])], 8)
    _track(e, row, [0])
    full = e.track_read(0)
    assert len(full) == 5 and full["id"].tolist() == [1, 2, 3, 4, 5]
    out[:] = 0
    assert lib.zly_track_read(e.h, 0, out.ctypes.data, 3, A(n)) == zly.OK and n.value == 5
    assert np.array_equal(out[:3].view(np.uint8), full[:3].view(np.uint8)) and not out[3:].view(np.uint8).any()
    assert lib.zly_track_read(e.h, 0, None, 0, A(n)) == zly.OK and n.value == 5
    e.close()


# ---- real frames ---------------------------------------------------------------------------------------------------------------
def _surface():
    """the three golden frames in one buffer, with their tight views"""
    frames = [np.ascontiguousarray(G["frames_64"][0]), np.ascontiguousarray(G["frames_64"][1]), np.ascontiguousarray(G["frame_96x80"])]
    views, off = [], 0
    for f in frames:
        v = zly.view_tight(zly.PIX_BGR, f.shape[1], f.shape[0])
        v.off[0] = off
        views.append(v)
        off += f.nbytes
    return frames, np.concatenate([f.reshape(-1) for f in frames]), views


def _same_detections(a, b):
    return len(a) == len(b) and all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in ("x", "y", "w", "h", "confidence", "class_id"))


def test_device_path_with_deferred_nms_on_real_frames(weights_path):
    cap, n = 64, 16
    _, buf, views = _surface()
    seq = [(3 * i + i // 5) % 3 for i in range(n)]
    e = zly.Engine(weights_path, model_w=64, model_h=64, conf_thr=CONF, iou_thr=IOU, max_batch=n, max_dets=cap, dtype=zly.DTYPE_FP32, warmup_runs=0,
                   flags=zly.FLAG_ASYNC_NMS)
    d_buf = torch.from_numpy(buf).cuda()
    d_ref = torch.zeros(n * e.slab_bytes, dtype=torch.uint8, device="cuda")
    outs = [torch.zeros(n * e.slab_bytes, dtype=torch.uint8, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()
    vs = [views[i] for i in seq]
    e.detect_device_view(d_buf.data_ptr(), buf.nbytes, vs, d_ref.data_ptr(), tag0=0)          # the engine's own untracked detections
    e.sync()
    ref = d_ref.cpu().numpy().reshape(n, e.slab_bytes)
    kept = [int(ref[i, :16].view(zly.SLAB_HDR_DTYPE)["n_kept"][0]) for i in range(n)]
    assert all(3 <= k <= cap for k in kept), kept
    e.track_enable(max_streams=4, max_tracks=64, max_lost=1)
    e.track_motion_enable()
    calls = [[i % 4 for i in range(n)], [(i // 4) % 4 if i % 5 else -1 for i in range(n)], [3 - i % 4 for i in range(n)]]
    for j in range(3):                                   # three detect + track pairs, nothing but enqueues in between
        e.detect_device_view(d_buf.data_ptr(), buf.nbytes, vs, outs[j].data_ptr(), tag0=0)
        e.track_slabs(calls[j], outs[j].data_ptr())
    e.sync()
    trk = {s: mr.MotionTracker(64, cap, max_lost=1) for s in range(4)}
    for j in range(3):
        got = outs[j].cpu().numpy().reshape(n, e.slab_bytes)
        want_ids = [None if s < 0 else trk[s].step(ref[i, 16:].view(zly.DET_DTYPE), kept[i]) for i, s in enumerate(calls[j])]
        want = tc.with_ids(ref, want_ids, cap)
        assert np.array_equal(got, want), _diff(got, want, cap, f"call {j}")
    for s in range(4):
        assert e.track_state(s) == trk[s].state()
        _same_tracks(e.track_read(s), trk[s].read())
    e.close()


def test_pipelined_path_on_real_frames(weights_path):
    cap = 64
    frames, _, _ = _surface()
    kw = dict(model_w=64, model_h=64, conf_thr=CONF, iou_thr=IOU, max_batch=8, max_dets=cap, dtype=zly.DTYPE_FP32, warmup_runs=0)
    plain = zly.Engine(weights_path, **kw)
    serial = [plain.detect(f, cap=cap) for f in frames]
    plain.close()
    assert all(3 <= n <= cap for _, n in serial)
    e = zly.Engine(weights_path, **kw)
    e.track_enable(max_streams=3, max_tracks=64)
    e.track_motion_enable()
    tight = [zly.view_tight(zly.PIX_BGR, f.shape[1], f.shape[0]) for f in frames]
    plan = []
    for k in range(5):                                   # 3 streams x 5 frames interleaved, an untracked submit after every third
        for s in range(3):
            plan.append((s, (s + k // 2) % 3))
            if len(plan) % 4 == 3:
                plan.append((-1, k % 3))
    trk = {s: mr.MotionTracker(64, cap) for s in range(3)}
    pending, results = [], []

    def drain(keep):
        while len(pending) > keep:
            s, fi, t = pending.pop(0)
            results.append((s, fi, e.wait(t, cap=cap)))

    for s, fi in plan:                                   # one thread; at most four tickets outstanding
        f = frames[fi]
        pending.append((s, fi, e.submit_view_tracked(f.reshape(-1), tight[fi], s)))
        drain(4)
    drain(0)
    assert len(results) == len(plan)
    for s, fi, (dets, n) in results:
        sd, sn = serial[fi]
        assert n == sn and _same_detections(dets, sd)
        if s < 0:
            assert not dets["track_id"].any()
        else:
            assert dets["track_id"].tolist() == trk[s].step(sd, sn).tolist(), (s, fi)
    for s in range(3):
        assert e.track_state(s) == trk[s].state()
        _same_tracks(e.track_read(s), trk[s].read())
    e.close()
