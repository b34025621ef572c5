"""track_kernel behind the C ABI (include/zly.h, "tracking") against the numpy oracle tests/track_ref.py, bit for bit.

The crafted cases (tests/track_cases.py) run no forward pass: slabs are built in numpy, put in a torch device buffer, handed to
zly_track_slabs with d_slabs set, and read back -- every byte other than the track_id fields must come back unchanged.  THE RULE is held
by running the same random scenes through different compositions of calls; the last tests drive real frames through the device path, the
device path with deferred NMS, and the pipelined submit path.  Engines are the suite's smallest (yolov8n at 64 x 64).
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch            # before the first engine: the process then uses torch's HIP runtime throughout, as tests/test_gpu_parity.py does

import track_cases as tc
import track_ref
import zly

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "zly_golden_64.npz"))
CONF, IOU = float(G["conf"]), float(G["iou"])       # the golden fixtures' thresholds: the CPU oracle finds 19, 27 and 29 detections in the three frames
MAX_STREAMS = 8
HAND = tc.hand_cases()
_ENGINES = {}


@pytest.fixture(scope="module")
def engine_for(weights_path):
    """engines by (cap, T, match_iou, max_lost): tracking is configured once per engine, so every configuration of the cases has its own"""
    def get(cap, T, match_iou, max_lost):
        key = (cap, T, float(np.float32(match_iou)), max_lost)
        if key not in _ENGINES:
            e = zly.Engine(weights_path, model_w=64, model_h=64, max_batch=64, max_dets=cap, warmup_runs=0, use_graph=False)
            e.track_enable(max_streams=MAX_STREAMS, max_tracks=T, match_iou=match_iou, max_lost=max_lost)
            _ENGINES[key] = e
        e = _ENGINES[key]
        e.track_reset(-1, 1)
        return e
    yield get
    for e in _ENGINES.values():
        e.close()
    _ENGINES.clear()


def _same_detections(a, b):
    """bit-exact comparison of everything but track_id and the wall-clock timestamp"""
    return len(a) == len(b) and all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in ("x", "y", "w", "h", "confidence", "class_id"))


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


@pytest.mark.parametrize("case", HAND, ids=[c.name for c in HAND])
def test_hand_case(engine_for, case):
    e = engine_for(case.cap, case.T, case.match_iou, case.max_lost)
    if case.first_id:
        e.track_reset(-1, case.first_id)
    raw = tc.build_slabs(case.frames, case.cap, case.n_kept)
    want = tc.with_ids(raw, [np.array(w, dtype=np.uint32) for w in case.want], case.cap)
    # stream 0: one frame per call; stream 3: the whole sequence in one call
    got = np.concatenate([_track(e, raw[k:k + 1], [0]) for k in range(len(case.frames))])
    assert np.array_equal(got, want), _diff(got, want, case.cap, case.name)
    got = _track(e, raw, [3] * len(case.frames))
    assert np.array_equal(got, want), _diff(got, want, case.cap, case.name + " in one call")
    o = track_ref.Tracker(case.T, case.cap, case.match_iou, case.max_lost)
    if case.first_id:
        o.reset(case.first_id)
    for k, f in enumerate(case.frames):
        o.step(f, None if case.n_kept is None else case.n_kept[k])
    assert e.track_state(0) == o.state() and e.track_state(3) == o.state()
    assert e.track_state(1)["frame_no"] == 0


def _compositions(sc):
    """name -> list of calls; a call is a list of (stream, frame index | None for an untracked filler)"""
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
@pytest.mark.parametrize("sc", tc.SCENES, ids=[s.name for s in tc.SCENES])
def test_scene_obeys_the_rule(engine_for, sc, comp):
    frames, ids, trackers = tc.scene(sc)
    e = engine_for(sc.cap, sc.T, sc.match_iou, sc.max_lost)
    for ci, call in enumerate(_compositions(sc)[comp]):
        fl = [frames[s][k] if s >= 0 else frames[0][0] for s, k in call]
        raw = tc.build_slabs(fl, sc.cap, tag0=tc.TAG0 + 100 * ci)
        want = tc.with_ids(raw, [ids[s][k] if s >= 0 else None for s, k in call], sc.cap)
        got = _track(e, raw, [s for s, _ in call])
        assert np.array_equal(got, want), _diff(got, want, sc.cap, f"{sc.name} / {comp}, call {ci} = {call}")
    for s in range(sc.n_streams):
        assert e.track_state(s) == trackers[s].state(), (sc.name, comp, s)
    for s in range(sc.n_streams, MAX_STREAMS):
        assert e.track_state(s) == dict(frame_no=0, next_id=1, n_live=0, evictions=0)


def test_more_than_64_frames_of_one_stream_in_one_call(weights_path):
    """the kernel takes a stream's frame indices in chunks of 64: 96 frames of one stream in a call of 100, behind one frame of another stream"""
    sc = tc.SCENES[0]
    frames = [f for fs in tc.scene(sc)[0] for f in fs]
    assert len(frames) == 96
    e = zly.Engine(weights_path, model_w=64, model_h=64, max_batch=100, max_dets=sc.cap, warmup_runs=0, use_graph=False)
    e.track_enable(max_streams=3, max_tracks=sc.T, match_iou=sc.match_iou, max_lost=sc.max_lost)
    fl = [frames[5]] + frames[:40] + [frames[0]] * 3 + frames[40:]
    streams = [1] + [2] * 40 + [-1] * 3 + [2] * 56
    trk = {s: track_ref.Tracker(sc.T, sc.cap, sc.match_iou, sc.max_lost) for s in (1, 2)}
    raw = tc.build_slabs(fl, sc.cap)
    want = tc.with_ids(raw, track_ref.run_streams(trk, fl, streams), sc.cap)
    got = _track(e, raw, streams)
    assert np.array_equal(got, want), _diff(got, want, sc.cap, "96 frames")
    assert e.track_state(2) == trk[2].state() and e.track_state(1) == trk[1].state() and e.track_state(2)["frame_no"] == 96
    e.close()


def test_reset_of_one_stream_leaves_the_others_alone(engine_for):
    sc = tc.SCENES[1]                                   # the scene with evictions
    frames, ids, trackers = tc.scene(sc)
    e = engine_for(sc.cap, sc.T, sc.match_iou, sc.max_lost)
    for s in range(sc.n_streams):
        raw = tc.build_slabs(frames[s], sc.cap)
        assert np.array_equal(_track(e, raw, [s] * sc.n_frames), tc.with_ids(raw, ids[s], sc.cap))
    assert sum(trackers[s].state()["evictions"] for s in range(sc.n_streams)) >= 10
    e.track_reset(1, 0)
    keep = trackers[1].state()["next_id"]
    assert e.track_state(1) == dict(frame_no=0, next_id=keep, n_live=0, evictions=0)
    for s in (0, 2, 3):
        assert e.track_state(s) == trackers[s].state()
    # the others' tables too: a repeat of a stream's last frame matches every box to its id
    for s in (0, 2, 3):
        last = frames[s][-1]
        o = track_ref.Tracker(sc.T, sc.cap, sc.match_iou, sc.max_lost)
        for f in frames[s]:
            o.step(f)
        want_ids = o.step(last)
        raw = tc.build_slabs([last], sc.cap)
        got = _track(e, raw, [s])
        assert np.array_equal(got, tc.with_ids(raw, [want_ids], sc.cap)), s
    # the reset stream starts over with its kept next id
    raw = tc.build_slabs(frames[1][:3], sc.cap)
    o = track_ref.Tracker(sc.T, sc.cap, sc.match_iou, sc.max_lost, first_id=keep)
    assert np.array_equal(_track(e, raw, [1, 1, 1]), tc.with_ids(raw, [o.step(f) for f in frames[1][:3]], sc.cap))
    e.track_reset(-1, 0)
    for s in range(MAX_STREAMS):
        st = e.track_state(s)
        assert (st["frame_no"], st["n_live"], st["evictions"]) == (0, 0, 0)
    assert e.track_state(1)["next_id"] == o.state()["next_id"]
    e.track_reset(2, 77)
    assert e.track_state(2)["next_id"] == 77 and e.track_state(3)["next_id"] == trackers[3].state()["next_id"]


def test_errors_enqueue_nothing(weights_path):
    lib = zly.load_library()
    I, A = zly.ERR_INVALID_ARGUMENT, C.byref
    e = zly.Engine(weights_path, model_w=64, model_h=64, max_batch=4, max_dets=8, warmup_runs=0, use_graph=False)
    raw = tc.build_slabs([tc.dets([tc.ROW8[0]])] * 4, 8)
    d = torch.from_numpy(raw).cuda()
    torch.cuda.synchronize()
    st, t, s4 = zly.TrackState(), C.c_uint64(0xABCD), (C.c_int32 * 4)(0, 0, 0, 0)
    frame = np.ascontiguousarray(G["frames_64"][0])
    view = zly.view_tight(zly.PIX_BGR, 64, 64)

    def refused(rc):
        assert rc == I and lib.zly_last_error()

    # every tracked call before zly_track_enable
    refused(lib.zly_track_slabs(e.h, 1, s4, d.data_ptr(), None))
    refused(lib.zly_track_reset(e.h, 0, 0))
    refused(lib.zly_track_state_at(e.h, 0, A(st)))
    refused(lib.zly_submit_view_tracked(e.h, frame.ctypes.data, frame.nbytes, A(view), 0, A(t)))
    refused(lib.zly_submit_try_view_tracked(e.h, frame.ctypes.data, frame.nbytes, A(view), -1, A(t)))
    assert t.value == 0xABCD
    # configurations
    def cfg(**kw):
        c = zly.TrackConfig()
        lib.zly_default_track_config(A(c))
        for k, v in kw.items():
            setattr(c, k, v)
        return c
    d0 = cfg()
    assert (d0.max_streams, d0.max_tracks, d0.max_lost) == (64, 64, 6) and d0.match_iou == np.float32(0.3)
    refused(lib.zly_track_enable(e.h, None))
    for bad in (dict(max_streams=0), dict(max_tracks=7), dict(max_tracks=65), dict(match_iou=-0.01), dict(match_iou=1.0), dict(match_iou=float("nan")),
                dict(max_lost=-1)):
        refused(lib.zly_track_enable(e.h, A(cfg(**bad))))
    big = zly.Engine(weights_path, model_w=64, model_h=64, max_batch=1, max_dets=65, warmup_runs=0, use_graph=False)
    refused(lib.zly_track_enable(big.h, A(cfg())))
    big.close()
    good = cfg(max_streams=2, max_tracks=8)
    assert lib.zly_track_enable(e.h, A(good)) == zly.OK
    refused(lib.zly_track_enable(e.h, A(good)))
    # streams and batch sizes
    for bad in (-2, 2):
        refused(lib.zly_track_slabs(e.h, 4, (C.c_int32 * 4)(0, bad, 0, 0), d.data_ptr(), None))
        refused(lib.zly_track_reset(e.h, bad, 0))
        refused(lib.zly_submit_view_tracked(e.h, frame.ctypes.data, frame.nbytes, A(view), bad, A(t)))
        refused(lib.zly_submit_try_view_tracked(e.h, frame.ctypes.data, frame.nbytes, A(view), bad, A(t)))
    for bad in (-1, 2):
        refused(lib.zly_track_state_at(e.h, bad, A(st)))
    refused(lib.zly_track_state_at(e.h, 0, None))
    refused(lib.zly_track_slabs(e.h, 0, s4, d.data_ptr(), None))
    refused(lib.zly_track_slabs(e.h, 5, s4, d.data_ptr(), None))
    refused(lib.zly_track_slabs(e.h, 4, None, d.data_ptr(), None))
    assert t.value == 0xABCD
    # nothing was enqueued: the tables and the slabs are as they were; a call of nothing but -1 changes nothing either
    e.track_slabs([-1, -1, -1, -1], d.data_ptr())
    e.sync()
    assert np.array_equal(d.cpu().numpy(), raw)
    for s in range(2):
        assert e.track_state(s) == dict(frame_no=0, next_id=1, n_live=0, evictions=0)
    e.track_slabs([1, -1, 1, 0], d.data_ptr())
    e.sync()
    got = d.cpu().numpy()
    assert [tc.slab_ids(got[i], 8).tolist() for i in range(4)] == [[1], [0], [1], [1]] and np.array_equal(got[1], raw[1])
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


def _oracle_ids(raw_untracked, streams, cap, trackers):
    """the oracle on the untracked slabs, frames taken in index order"""
    out = []
    for i, s in enumerate(streams):
        if s < 0:
            out.append(None)
            continue
        hdr = raw_untracked[i, :16].view(zly.SLAB_HDR_DTYPE)[0]
        out.append(trackers[s].step(raw_untracked[i, 16:].view(zly.DET_DTYPE), int(hdr["n_kept"])))
    return out


def test_device_path_on_real_frames(weights_path):
    cap = 64
    _, buf, views = _surface()
    seq = [0, 0, 1, 0, 2, 2, 1, 1, 0, 2]
    e = zly.Engine(weights_path, model_w=64, model_h=64, conf_thr=CONF, iou_thr=IOU, max_batch=16, max_dets=cap, dtype=zly.DTYPE_FP32, warmup_runs=0)
    d_buf = torch.from_numpy(buf).cuda()
    d_ref = torch.zeros(len(seq) * e.slab_bytes, dtype=torch.uint8, device="cuda")
    d_out = torch.zeros(len(seq) * e.slab_bytes, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    e.detect_device_view(d_buf.data_ptr(), buf.nbytes, [views[i] for i in seq], d_ref.data_ptr(), tag0=7)
    e.sync()
    ref = d_ref.cpu().numpy().reshape(len(seq), e.slab_bytes)
    kept = [int(ref[i, :16].view(zly.SLAB_HDR_DTYPE)["n_kept"][0]) for i in range(len(seq))]
    assert all(3 <= k <= cap for k in kept), kept
    e.track_enable(max_streams=4, max_tracks=64)
    # the whole sequence as stream 2 in one call, with an untracked frame in it
    streams = [2] * len(seq)
    streams[3] = -1
    e.detect_device_view(d_buf.data_ptr(), buf.nbytes, [views[i] for i in seq], d_out.data_ptr(), tag0=7)
    e.track_slabs(streams, d_out.data_ptr())
    e.sync()
    got = d_out.cpu().numpy().reshape(len(seq), e.slab_bytes)
    trk = {2: track_ref.Tracker(64, cap)}
    want = tc.with_ids(ref, _oracle_ids(ref, streams, cap, trk), cap)
    assert np.array_equal(got, want), _diff(got, want, cap, "one call")
    assert e.track_state(2) == trk[2].state()
    # the engine's own slab buffer, one frame per call, read through zly_read_slabs
    o = track_ref.Tracker(64, cap)
    for i in seq:
        e.detect_device_view(d_buf.data_ptr(), buf.nbytes, [views[i]], tag0=7 + seq.index(i))
        e.track_slabs([1])
        hdr, dets = e.read_slabs(1)[0]
        r = ref[seq.index(i)]
        want_ids = o.step(r[16:].view(zly.DET_DTYPE), int(hdr["n_kept"]))
        assert int(hdr["n_kept"]) == kept[seq.index(i)] and dets["track_id"].tolist() == want_ids.tolist()
        assert _same_detections(dets, r[16:].view(zly.DET_DTYPE)[:len(dets)])
    e.close()


def test_device_path_with_deferred_nms_and_no_host_sync(weights_path):
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
    e.detect_device_view(d_buf.data_ptr(), buf.nbytes, vs, d_ref.data_ptr(), tag0=0)
    e.sync()
    ref = d_ref.cpu().numpy().reshape(n, e.slab_bytes)
    e.track_enable(max_streams=4, max_tracks=64, max_lost=1)
    calls = [[i % 4 for i in range(n)], [(i // 4) % 4 if i % 5 else -1 for i in range(n)], [3 - i % 4 for i in range(n)]]
    for j in range(3):                                   # three detect + track pairs, nothing but enqueues in between
        e.detect_device_view(d_buf.data_ptr(), buf.nbytes, vs, outs[j].data_ptr(), tag0=0)
        e.track_slabs(calls[j], outs[j].data_ptr())
    e.sync()
    trk = {s: track_ref.Tracker(64, cap, max_lost=1) for s in range(4)}
    for j in range(3):
        got = outs[j].cpu().numpy().reshape(n, e.slab_bytes)
        want = tc.with_ids(ref, _oracle_ids(ref, calls[j], cap, trk), cap)
        assert np.array_equal(got, want), _diff(got, want, cap, f"call {j}")
    for s in range(4):
        assert e.track_state(s) == trk[s].state()
    e.close()


def test_pipelined_path_tracks_in_ticket_order(weights_path):
    cap = 64
    frames, _, _ = _surface()
    kw = dict(model_w=64, model_h=64, conf_thr=CONF, iou_thr=IOU, max_batch=8, max_dets=cap, dtype=zly.DTYPE_FP32, warmup_runs=0)
    plain = zly.Engine(weights_path, **kw)
    serial = [plain.detect(f, cap=cap) for f in frames]
    plain.close()
    assert all(3 <= n <= cap for _, n in serial)
    e = zly.Engine(weights_path, **kw)
    e.track_enable(max_streams=3, max_tracks=64)
    tight = [zly.view_tight(zly.PIX_BGR, f.shape[1], f.shape[0]) for f in frames]
    # 3 streams x 5 frames interleaved, an untracked submit after every third; stream s sees frames (s + k) % 3 with a repeat
    plan = []
    for k in range(5):
        for s in range(3):
            plan.append((s, (s + k // 2) % 3))
            if len(plan) % 4 == 3:
                plan.append((-1, k % 3))
    trk = {s: track_ref.Tracker(64, cap) for s in range(3)}
    pending, results = [], []

    def drain(keep):
        while len(pending) > keep:
            s, fi, t = pending.pop(0)
            results.append((s, fi, e.wait(t, cap=cap)))

    for s, fi in plan:                                   # one thread; at most four tickets outstanding, fewer than the ring has slots
        f = frames[fi]
        t = e.submit_view_tracked(f.reshape(-1), tight[fi], s) if (s >= 0 or len(pending) % 2) else e.submit_view(f.reshape(-1), tight[fi])
        pending.append((s, fi, t))
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
    e.close()
