"""Camera motion on the GPU (include/zly.h "Camera motion"; csrc/kernels_camera.hip), byte for byte against tests/camera_ref.py: after every call the
WHOLE record of every stream -- header, SAD table and every byte the rule does not write -- must equal the oracle applied to the frames the stream was
given.  The records are the engine's own (zly_camera_enable zeroes them); the test keeps a mirror of each from the zeroes on and PRIMES the streams
with two unrelated frames, so that every table entry the engine's radius reaches is non-zero before the frames under test (_prime): a kernel that
wrote a table on a FIRST frame would be seen.  (Entries at and beyond (2R + 1)^2 are never written by an engine, whose radius is fixed: they must
stay zero.)

1. The kernels: the shapes of the issue, five formats tight and through pitched views in a poisoned buffer, sequences of three to five frames, several
   streams in one call and split over calls, in any batch position, reset between frames.  72 x 40 at C = 8 is 9 x 5 cells, which the rule itself
   refuses for R = 3 and 4 (gh < 2R + 1), and 200 x 120 at C = 64 is 4 x 2 cells, refused for every R: those are asserted as refusals, and
   72 x 72 (gw = gh = 2R + 1 at R = 4) and 200 x 136 take their place.
2. Resident surfaces with update -> camera -> update and nothing but enqueues in between.
3. Step A on track tables; the pan scene through zly_track_slabs; one zoom composition.
4. Every refusal, each followed by a good call that gives what a twin engine gives."""
import ctypes as C

import numpy as np
import pytest
import torch            # before the first engine: the process then uses torch's HIP runtime throughout, as tests/test_gpu_parity.py does

import camera_cases as cs
import camera_ref as cam
import change_ref
import chip_cases as cc
import test_camera_ref as tcr
import track_cases as tc
import zly
import zoom_ref

pytestmark = pytest.mark.gpu

POISON = cc.POISON
ARG, INPUT = zly.ERR_INVALID_ARGUMENT, zly.ERR_INVALID_INPUT
BGR, BGRA, NV12, I420, YUY2 = zly.PIX_BGR, zly.PIX_BGRA, zly.PIX_NV12_BT601, zly.PIX_I420_BT709, zly.PIX_YUY2_BT601
assert (BGR, BGRA, NV12, I420, YUY2) == cs.FORMATS
F = np.float32


def _engine(weights_path, cfg, max_streams=8, enable=True, surfaces=0, surface_bytes=0, track=False, motion=False, max_dets=8, max_batch=16):
    """the suite's smallest engine (yolov8n at 64 x 64): no test here runs a forward pass"""
    e = zly.Engine(weights_path, model_w=64, model_h=64, max_batch=max_batch, max_dets=max_dets, warmup_runs=0, use_graph=False)
    if enable:
        e.camera_enable(max_streams, cell=cfg.cell, radius=cfg.radius, max_residual_q4=cfg.max_residual_q4)
        assert e.camera_layout() == cam.layout()
    if surfaces:
        e.surfaces_enable(surfaces, surface_bytes)
    if track:
        e.track_enable(max_streams=8, max_tracks=max_dets)
    if motion:
        e.track_motion_enable()
    return e


def _pack(items):
    """[(buffer, view tuple)] -> (one host buffer with every item at a multiple of 256 behind 3 poisoned bytes, the views in it)"""
    parts, views, o = [], [], 0
    for buf, view in items:
        lead = 3
        size = -(-(lead + buf.size) // 256) * 256
        p = np.full(size, POISON, dtype=np.uint8)
        p[lead:lead + buf.size] = buf
        parts.append(p)
        views.append(cc.to_c(cc.shifted(view, o + lead)))
        o += size
    return np.concatenate(parts), views


class Mirror:
    """the oracle's streams and the bytes their records must hold"""

    def __init__(self, cfg, n=8):
        self.cfg = cfg
        self.streams = [cam.Stream() for _ in range(n)]
        self.recs = [np.zeros(cam.REC_BYTES, dtype=np.uint8) for _ in range(n)]
        self.flags = set()

    def frame(self, s, bgr):
        h = self.streams[s].frame(bgr, self.cfg, self.recs[s])
        self.flags.add(int(h["flags"]))
        return h

    def reset(self, s):
        for i in (range(len(self.streams)) if s < 0 else [s]):
            self.streams[i].reset(self.recs[i])

    def check(self, e, streams, what=""):
        for s in streams:
            got = e.camera_read(s)
            if not np.array_equal(got, self.recs[s]):
                bad = np.flatnonzero(got != self.recs[s])
                raise AssertionError(f"{what}: stream {s}: {len(bad)} bytes differ, first at {bad[:6].tolist()}; header {got[:96].view(cam.HDR_DTYPE)[0]} "
                                     f"want {self.recs[s][:96].view(cam.HDR_DTYPE)[0]}")


def _call(e, mirror, items, streams, what="", stream=0):
    """one zly_camera_device_view call: items = [(buffer, view tuple, BGR image)]; every stream's whole record against the oracle"""
    host, views = _pack([(b, v) for b, v, _ in items])
    d = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    e.camera_device_view(d.data_ptr(), host.nbytes, views, streams, stream=stream)
    for s, (_, _, bgr) in zip(streams, items):
        mirror.frame(s, bgr)
    mirror.check(e, streams, what)


def _prime(e, m, streams, w, h, seed=90):
    """two unrelated random BGR frames of a geometry at least as large as the test's largest: afterwards every table entry within the radius is
    non-zero -- asserted here on the mirror"""
    rng = np.random.default_rng(seed)
    side = 2 * m.cfg.radius + 1
    w, h = max(w, side * m.cfg.cell), max(h, side * m.cfg.cell)
    for k in range(2):
        bgr = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        _call(e, m, [(bgr.reshape(-1), cc.tight_view(BGR, w, h), bgr)] * len(streams), streams, ("prime", k))
    for s in streams:
        assert m.recs[s][cam.HDR_BYTES:cam.HDR_BYTES + 8 * side * side].view(np.uint64).all() and not m.recs[s][cam.HDR_BYTES + 8 * side * side:].any()


def _items(fmt, bgr, pitched):
    f, img = cs.as_format(fmt, bgr)
    h, w = bgr.shape[:2]
    return (cc.pitched(f, fmt, w, h) if pitched else (f, cc.tight_view(fmt, w, h))) + (img,)


def _code(f, *a, **k):
    with pytest.raises(zly.ZlyError) as ei:
        f(*a, **k)
    return ei.value.code


# ---- 1. the kernels -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 2, 3, 4])
def test_small_grids_at_every_radius(weights_path, R):
    """72 x 40 at C = 8 (9 x 5 cells: gh = 2R + 1 at R = 2; refused at R = 3, 4) and 72 x 72 (gw = gh = 2R + 1 at R = 4: a window of one cell),
    pans of four frames with a shift of R cells (CLIPPED), tight on stream 0 and pitched on stream 1"""
    cfg = cam.Config(cell=8, radius=R, max_residual_q4=4080)
    e, m = _engine(weights_path, cfg), Mirror(cfg)
    _prime(e, m, [0, 1], 72, 72)
    for (w, h) in ((72, 40), (72, 72)):
        frames = cs.pan(w, h, [(8 * R, 0), (-3, 2), (5, -8 * R)], 1, seed=10 * R + h)
        if not cam.grid_ok(w, h, cfg):
            assert R > 2 and h == 40
            host, views = _pack([_items(BGR, frames[0], False)[:2]])
            d = torch.from_numpy(host).cuda()
            torch.cuda.synchronize()
            assert _code(e.camera_device_view, d.data_ptr(), host.nbytes, views, [0]) == INPUT
            m.check(e, [0, 1], "refused")
            continue
        for k, bgr in enumerate(frames):
            _call(e, m, [_items(BGR, bgr, False), _items(BGR, bgr, True)], [0, 1], (R, w, h, k))
    assert m.flags >= {0, cam.FIRST, cam.CLIPPED}, m.flags
    e.close()


@pytest.mark.parametrize("C", cam.CELLS)
def test_five_formats_tight_and_pitched_at_every_cell(weights_path, C):
    """201 x 121 (rounded up to what the format allows; neither a multiple of any C) at R = 1; at C = 64 that is 4 x 2 cells and refused, and 201 x 137
    takes its place.  Per format a pan of four frames, tight on stream 0, pitched with odd plane origins on stream 1, both in one call"""
    cfg = cam.Config(cell=C, radius=1, max_residual_q4=4080)
    e, m = _engine(weights_path, cfg), Mirror(cfg)
    _prime(e, m, [0, 1], 202, 138)
    for fmt in cs.FORMATS:
        w, h = cc.legal(fmt, 201, 137 if C == 64 else 121)
        for k, bgr in enumerate(cs.pan(w, h, [(C // 4, 0), (2, -3), (-C, C // 4)], 2, seed=fmt + C)):
            _call(e, m, [_items(fmt, bgr, False), _items(fmt, bgr, True)], [0, 1], (fmt, C, k))
    if C == 64:
        host, views = _pack([_items(BGR, cs.gray(200, 120, 9), False)[:2]])
        d = torch.from_numpy(host).cuda()
        torch.cuda.synchronize()
        assert _code(e.camera_device_view, d.data_ptr(), host.nbytes, views, [0]) == INPUT
        m.check(e, [0, 1], "refused")
    assert m.flags >= {0, cam.FIRST}, m.flags
    e.close()


def test_1080p_at_cell_16(weights_path):
    """1920 x 1080 BGRA at C = 16, R = 4: 120 x 68 = 8160 cells, the last row half a cell high; three frames"""
    cfg = cam.Config(cell=16, radius=4, max_residual_q4=4080)
    e, m = _engine(weights_path, cfg), Mirror(cfg)
    for k, bgr in enumerate(cs.pan(1920, 1080, [(37, -12), (-64, 16)], 4, seed=77)):
        _call(e, m, [_items(BGRA, bgr, False)], [2], ("1080p", k))
    h = m.recs[2][:96].view(cam.HDR_DTYPE)[0]
    assert (int(h["dx"]), int(h["dy"]), int(h["gw"]), int(h["gh"])) == (-4, 1, 120, 68)
    e.close()


def test_sads_above_two_to_the_32(weights_path):
    """6144 x 4096 I420 at C = 64, all white then all black: every SAD is 64 * 64 * 255 * 88 * 56, above 2^32, and they are all equal.  The oracle's
    grids are made of one cell's sum, computed by the oracle on a 64 x 64 frame of the same bytes"""
    W, H = 6144, 4096
    cfg = cam.Config(cell=64, radius=4, max_residual_q4=4080)
    e = _engine(weights_path, cfg)
    s, rec = cam.Stream(), np.zeros(cam.REC_BYTES, np.uint8)
    for k, y in enumerate((255, 0)):
        tile = np.concatenate([np.full(64 * 64, y, np.uint8), np.full(2 * 32 * 32, 128, np.uint8)])
        cell = int(change_ref.sums(np.ascontiguousarray(cs.chip_ref.bgr_of(I420, tile, 64, 64)), 64)[0][0, 0])
        assert cell == 64 * 64 * y
        frame = torch.cat([torch.full((W * H,), y, dtype=torch.uint8, device="cuda"), torch.full((W * H // 2,), 128, dtype=torch.uint8, device="cuda")])
        torch.cuda.synchronize()
        e.camera_device_view(frame.data_ptr(), frame.numel(), [zly.view_tight(I420, W, H)], [0])
        s.frame_sums(np.full((64, 96), cell, np.uint32), W, H, cfg, rec)
        assert np.array_equal(e.camera_read(0), rec), k
    tab = rec[cam.HDR_BYTES:cam.HDR_BYTES + 8 * 81].view(np.uint64)
    assert int(tab[0]) == 64 * 64 * 255 * 88 * 56 > 1 << 32 and (tab == tab[0]).all()
    e.close()


def test_streams_in_one_call_split_over_calls_in_any_batch_position_and_reset(weights_path):
    """four streams of four formats and sizes over five steps: engine A takes each step in one call, engine B in two calls with the streams in
    another order and on a caller's stream.  Both must hold the oracle's records.  Between steps 2 and 3 stream 1 is reset, after step 3 all are"""
    cfg = cam.Config(cell=8, radius=2, max_residual_q4=48)
    a, b, ma, mb = _engine(weights_path, cfg), _engine(weights_path, cfg), Mirror(cfg), Mirror(cfg)
    shapes = ((BGR, 101, 77), (NV12, 128, 64), (YUY2, 66, 41), (BGRA, 43, 47))
    _prime(a, ma, [0, 1, 2, 3], 128, 77)
    _prime(b, mb, [3, 2, 1, 0], 128, 77)
    pans = [cs.pan(w, h, [(8, 0), (-5, 3), (2, 2), (40, 1)], 1 + i % 2, seed=40 + i) for i, (fmt, w, h) in enumerate(shapes)]
    caller = torch.cuda.Stream()
    for k in range(5):
        items = [_items(fmt, pans[i][k], i % 2 == 1) for i, (fmt, w, h) in enumerate(shapes)]
        _call(a, ma, items, [0, 1, 2, 3], ("A", k))
        _call(b, mb, [items[3], items[1]], [3, 1], ("B1", k), stream=caller.cuda_stream)
        _call(b, mb, [items[2], items[0]], [2, 0], ("B2", k))
        if k in (2, 3):
            for e, m in ((a, ma), (b, mb)):
                e.camera_reset(1 if k == 2 else -1)
                m.reset(1 if k == 2 else -1)
                m.check(e, [0, 1, 2, 3], ("reset", k))
    for s in range(4):
        assert np.array_equal(ma.recs[s], mb.recs[s])
    assert ma.flags >= {0, cam.FIRST} and any(f & cam.LOST for f in ma.flags), ma.flags
    a.close()
    b.close()


# ---- 2. resident surfaces -------------------------------------------------------------------------------------------------------------------
def test_update_camera_update_with_nothing_but_enqueues(weights_path):
    """update k on the engine's stream, zly_camera_surfaces k on a caller's stream, update k + 1, ... over six pictures of a pan.  Step k gives picture
    k to stream k (its second frame) and to stream k + 1 (its first), so that after the loop stream k's record is the shift from picture k - 1 to
    picture k for every k: a patch kernel that overtook a sums kernel would have handed it the next picture"""
    cfg = cam.Config(cell=16, radius=2, max_residual_q4=4080)
    W, H, steps = 320, 200, 6
    e, m = _engine(weights_path, cfg, surfaces=1, surface_bytes=W * H * 4), Mirror(cfg)
    frames = [cs.as_format(BGRA, f) for f in cs.pan(W, H, [(16, 0), (3, 7), (-20, -9), (0, 32), (5, 5)], 2, seed=60)]
    whole = zly.view_tight(BGRA, W, H)
    callers = [torch.cuda.Stream(), torch.cuda.Stream()]
    e.surface_define(0, BGRA, W, H)
    for k in range(steps):
        e.surface_update([(0, 0, 0, frames[k][0], whole)])
        e.camera_surfaces([0, 0], [k, k + 1], stream=callers[k % 2].cuda_stream)
        m.frame(k, frames[k][1])
        m.frame(k + 1, frames[k][1])
    for c in callers:
        c.synchronize()
    m.check(e, list(range(steps + 1)), "surfaces")
    assert [int(m.recs[k][:96].view(cam.HDR_DTYPE)[0]["dx"]) for k in range(1, 6)] == [1, 0, -1, 0, 0]
    e.close()


# ---- 3. step A ------------------------------------------------------------------------------------------------------------------------------
def _track(e, frames, streams, cap=8):
    """one zly_track_slabs call on crafted slabs -> the slabs' ids"""
    d = torch.from_numpy(tc.build_slabs(frames, cap)).cuda()
    torch.cuda.synchronize()
    e.track_slabs(streams, d.data_ptr())
    e.sync()
    got = d.cpu().numpy()
    return [tc.slab_ids(got[i], cap).tolist() for i in range(len(frames))]


@pytest.mark.parametrize("motion", [False, True], ids=["plain", "motion"])
def test_apply_moves_the_live_tracks_and_nothing_else(weights_path, motion):
    """streams 0 and 1 hold tracks (five and two live slots; with the motion model, velocities and hits from two matched frames) and a pending shift
    from two frames; stream 2 has tracks and no camera frame (no geometry: skipped whole).  zly_track_read before and after: x and y as bit patterns
    against the oracle, every other field -- and zly_track_state_at -- unchanged; the records' three fields, and no other byte"""
    cfg = cam.Config(cell=8, radius=3, max_residual_q4=4080)
    e, m = _engine(weights_path, cfg, track=True, motion=motion), Mirror(cfg)
    boxes = [(0.2, 0.3, 0.1, 0.1), (0.5, 0.5, 0.2, 0.1), (0.7, 0.2, 0.1, 0.2), (0.3, 0.8, 0.1, 0.1), (0.85, 0.85, 0.1, 0.1)]
    for k in range(2):                                                     # the second frame's boxes move a little: matched, with a velocity
        moved = [(x + 0.01 * k, y - 0.005 * k, w, h) for x, y, w, h in boxes]
        assert _track(e, [tc.dets(moved), tc.dets(moved[:2]), tc.dets(moved[2:])], [0, 1, 2]) == [[1, 2, 3, 4, 5], [1, 2], [1, 2, 3]]
    for k, (f0, f1) in enumerate(zip(cs.pan(200, 120, [(13, -6), (5, 2)], 1, seed=70), cs.pan(96, 64, [(-8, 8), (-3, 0)], 1, seed=71))):
        _call(e, m, [_items(BGR, f0, False), _items(NV12, f1, True)], [0, 1], ("frames", k))
    before = {s: (e.track_read(s).copy(), e.track_state(s)) for s in (0, 1, 2)}
    assert all(m.streams[s].pend != [0, 0] for s in (0, 1))
    e.camera_apply_tracks([1, 2, 0])
    for s in (0, 1, 2):
        got, want = e.track_read(s), before[s][0].copy()
        sh = m.streams[s].shift() if s < 2 else None
        if sh is not None:
            want["x"], want["y"] = (want["x"] + sh[0]).astype(F), (want["y"] + sh[1]).astype(F)
            assert sh[0] != 0 and sh[1] != 0
        assert got.tobytes() == want.tobytes() and e.track_state(s) == before[s][1], (s, got, want)
        if motion and s < 2:
            assert (got["hits"] == 2).all() and (got["vx"] != 0).all()
        x, y = np.zeros(0, F), np.zeros(0, F)
        m.streams[s].apply(x, y, [], m.recs[s])
    m.check(e, [0, 1, 2], "after the apply")
    assert [int(m.recs[s][:96].view(cam.HDR_DTYPE)[0]["n_applied"]) for s in (0, 1, 2)] == [1, 1, 0]
    moved = e.track_read(0).copy()
    e.camera_apply_tracks([0])                                             # nothing pending: the tracks stay, n_applied advances
    assert e.track_read(0).tobytes() == moved.tobytes()
    m.streams[0].apply(np.zeros(0, F), np.zeros(0, F), [], m.recs[0])
    m.check(e, [0, 1, 2], "a second apply")
    e.close()


@pytest.mark.parametrize("apply", [True, False], ids=["with_apply", "without"])
def test_ids_under_a_pan_through_track_slabs(weights_path, apply):
    """tests/test_camera_ref.py's pan scene, frame by frame: zly_camera_device_view, zly_camera_apply_tracks (or not), zly_track_slabs on crafted
    slabs, on a caller's stream and with nothing but enqueues between them.  The ids equal the CPU composition: they persist with the apply, and
    every box gets a fresh id every frame without it"""
    frames, dets = tcr.pan_scene()
    want = tcr.pan_ids(frames, dets, apply)
    assert want == ([[1, 2, 3]] * 7 if apply else [[3 * k + 1, 3 * k + 2, 3 * k + 3] for k in range(7)])
    e = _engine(weights_path, tcr.PAN_CFG, track=True)
    caller = torch.cuda.Stream()
    host, views = _pack([(f.reshape(-1), cc.tight_view(BGR, tcr.PAN_W, tcr.PAN_H)) for f in frames])
    d = torch.from_numpy(host).cuda()
    slabs = torch.from_numpy(tc.build_slabs(dets, 8)).cuda()
    torch.cuda.synchronize()
    for k in range(len(frames)):
        e.camera_device_view(d.data_ptr(), host.nbytes, [views[k]], [5], stream=caller.cuda_stream)
        if apply:
            e.camera_apply_tracks([5], stream=caller.cuda_stream)
        e.track_slabs([5], slabs.data_ptr() + k * tc.slab_bytes(8), stream=caller.cuda_stream)
    caller.synchronize()
    got = slabs.cpu().numpy()
    assert [tc.slab_ids(got[k], 8).tolist() for k in range(len(frames))] == want
    hdr = e.camera_read(5)[:96].view(cam.HDR_DTYPE)[0]
    assert (int(hdr["sx_q4"]), int(hdr["sy_q4"]), int(hdr["n_applied"])) == (16 * tcr.PAN[0], 16 * tcr.PAN[1], 7 if apply else 0)
    e.close()


def test_a_zoom_plan_after_camera_and_apply(weights_path):
    """camera -> apply -> the plan kernel: the plan's track regions equal tests/zoom_ref.py on the stream's table shifted by the oracle"""
    cfg = cam.Config(cell=8, radius=4, max_residual_q4=4080)
    zcfg = zoom_ref.Config(regions=3, region_w=96, region_h=64, max_age=2, class_id=-1)
    e = _engine(weights_path, cfg, track=True)
    e.zoom_enable(regions=zcfg.regions, region_w=zcfg.region_w, region_h=zcfg.region_h, max_age=zcfg.max_age, class_id=zcfg.class_id)
    W, H = 640, 360
    assert _track(e, [tc.dets([(0.2, 0.3, 0.05, 0.05), (0.6, 0.7, 0.04, 0.08)])], [3]) == [[1, 2]]
    s, rec = cam.Stream(), np.zeros(cam.REC_BYTES, np.uint8)
    frames = cs.pan(W, H, [(27, -14)], 1, seed=80)
    host, views = _pack([(f.reshape(-1), cc.tight_view(BGR, W, H)) for f in frames])
    d = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    table = zoom_ref.Table(frame_no=e.track_state(3)["frame_no"])
    for r in e.track_read(3):
        table.add(r["x"], r["y"], r["w"], r["h"], cls=int(r["class_id"]), id=int(r["id"]), last_seen=int(r["last_seen"]))
    unshifted = zoom_ref.plan(table, zcfg, W, H)
    for k in range(2):
        e.camera_device_view(d.data_ptr(), host.nbytes, [views[k]], [3])
        s.frame(frames[k], cfg, rec)
    e.camera_apply_tracks([3])
    nx, ny = s.shift()
    table.box = [(F(x + nx), F(y + ny), w, h) for x, y, w, h in table.box]
    got, want = e.zoom_plan([(W, H)], [3])[0], zoom_ref.plan(table, zcfg, W, H)
    assert got.tobytes() == want.tobytes() and (want["slot"] >= 0).sum() == 2, (got, want)
    assert want.tobytes() != unshifted.tobytes()                          # the shift moved the regions
    e.close()


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_is_followed_by_a_good_call_that_gives_what_a_twin_gives(weights_path):
    cfg = cam.Config(cell=8, radius=2, max_residual_q4=100)
    plain = _engine(weights_path, cfg, enable=False)
    frames = cs.pan(64, 48, [(8, 0), (0, -8), (3, 3), (-8, 8)], 1, seed=1)
    f = frames[0].reshape(-1)
    d = torch.from_numpy(np.concatenate([f, np.zeros(64, np.uint8)])).cuda()
    torch.cuda.synchronize()
    v = zly.view_tight(BGR, 64, 48)
    # an engine without the feature
    assert _code(plain.camera_device_view, d.data_ptr(), f.size, [v], [0]) == ARG and _code(plain.camera_surfaces, [0], [0]) == ARG
    assert _code(plain.camera_read, 0) == ARG and _code(plain.camera_layout) == ARG and _code(plain.camera_reset, 0) == ARG
    assert _code(plain.camera_apply_tracks, [0]) == ARG
    for bad in (dict(cell=0), dict(cell=24), dict(cell=128), dict(radius=0), dict(radius=9), dict(max_residual_q4=-1), dict(max_residual_q4=4081), dict(max_streams=0)):
        assert _code(plain.camera_enable, **bad) == ARG, bad
    assert plain.lib.zly_camera_enable(plain.h, None, 4) == ARG
    c = zly.CameraConfig()
    plain.lib.zly_default_camera_config(c)
    assert (c.cell, c.radius, c.max_residual_q4) == (16, 4, 64)
    e, twin = plain, _engine(weights_path, cfg, max_streams=4, track=True)
    e.camera_enable(4, cell=8, radius=2, max_residual_q4=100)
    assert _code(e.camera_enable, 4) == ARG                                                          # twice
    assert _code(e.camera_apply_tracks, [0]) == ARG                                                  # no track tables
    e.track_enable(max_streams=3, max_tracks=8)                                                      # fewer streams than the camera has
    twin_m, m, step = Mirror(cfg, 4), Mirror(cfg, 4), [0]

    def good(what):
        """a good call on both engines: the next frame of the pan on streams 0 and 1, then an apply on stream 1"""
        bgr = frames[step[0] % len(frames)]
        step[0] += 1
        for eng, mir in ((e, m), (twin, twin_m)):
            _call(eng, mir, [_items(BGR, bgr, False)] * 2, [0, 1], what)
            eng.camera_apply_tracks([1])
            mir.streams[1].apply(np.zeros(0, F), np.zeros(0, F), [], mir.recs[1])
            mir.check(eng, [0, 1, 2, 3], what)
        for s in range(4):
            assert np.array_equal(e.camera_read(s), twin.camera_read(s)), (what, s)

    good("the first")
    call = lambda vs, ss, nbytes=f.size: e.camera_device_view(d.data_ptr(), nbytes, vs, ss)          # noqa: E731
    bad_fmt, odd, short, wide, many, thin, flat = (zly.view_tight(BGR, 64, 48) for _ in range(7))
    bad_fmt.fmt = 5
    odd.fmt, odd.w = NV12, 63
    short.pitch[0] = 3 * 64 - 1
    wide.w, wide.h = 16385, 40
    wide.pitch[0] = 3 * 16385
    many.w, many.h = 1024, 520                                                                       # 128 x 65 cells of 8
    many.pitch[0] = 3 * 1024
    thin.w, thin.pitch[0] = 32, 3 * 32                                                               # 4 x 6 cells: gw < 2R + 1
    flat.h = 32                                                                                      # 8 x 4 cells: gh < 2R + 1
    refusals = [
        ("n = 0", lambda: call([], []), ARG),
        ("n above max_batch", lambda: call([v] * 17, list(range(17))), ARG),
        ("null views", lambda: zly._check(e.lib, e.lib.zly_camera_device_view(e.h, 1, d.data_ptr(), f.size, None, (C.c_int32 * 1)(0), None)), ARG),
        ("null streams", lambda: zly._check(e.lib, e.lib.zly_camera_device_view(e.h, 1, d.data_ptr(), f.size, (zly.FrameView * 1)(v), None, None)), ARG),
        ("a stream twice", lambda: call([v, v], [1, 1]), ARG),
        ("a stream beyond the table", lambda: call([v, v], [0, 4]), ARG),
        ("a negative stream", lambda: call([v, v], [0, -1]), ARG),
        ("an unknown format", lambda: call([v, bad_fmt], [0, 1]), ARG),
        ("an odd NV12 width", lambda: call([v, odd], [0, 1]), INPUT),
        ("a pitch below the row", lambda: call([v, short], [0, 1]), INPUT),
        ("a view beyond the buffer", lambda: call([v, v], [0, 1], f.size - 1), INPUT),
        ("W above ZLY_AREA_MAX_DIM", lambda: call([v, wide], [0, 1], 1 << 22), INPUT),
        ("too many cells", lambda: call([v, many], [0, 1], 1 << 22), INPUT),
        ("gw below 2R + 1", lambda: call([v, thin], [0, 1]), INPUT),
        ("gh below 2R + 1", lambda: call([v, flat], [0, 1]), INPUT),
        ("read: a stream out of range", lambda: e.camera_read(4), ARG),
        ("read: a small buffer", lambda: zly._check(e.lib, e.lib.zly_camera_read(e.h, 0, np.zeros(95, np.uint8).ctypes.data, 95)), ARG),
        ("read: a null buffer", lambda: zly._check(e.lib, e.lib.zly_camera_read(e.h, 0, None, 4096)), ARG),
        ("reset: a stream out of range", lambda: e.camera_reset(4), ARG),
        ("surfaces: no store", lambda: e.camera_surfaces([0], [0]), ARG),
        ("apply: n = 0", lambda: e.camera_apply_tracks([]), ARG),
        ("apply: n above the streams", lambda: e.camera_apply_tracks([0, 1, 2, 0, 1]), ARG),
        ("apply: null streams", lambda: zly._check(e.lib, e.lib.zly_camera_apply_tracks(e.h, 1, None, None)), ARG),
        ("apply: a stream twice", lambda: e.camera_apply_tracks([1, 1]), ARG),
        ("apply: a stream beyond the track tables", lambda: e.camera_apply_tracks([0, 3]), ARG),
        ("apply: a stream beyond the camera's", lambda: e.camera_apply_tracks([4]), ARG),
        ("apply: a negative stream", lambda: e.camera_apply_tracks([-1]), ARG),
    ]
    for what, fn, code in refusals:
        assert _code(fn) == code, what
        m.check(e, [0, 1, 2, 3], what)                                                               # no record changed ...
        good(what)                                                                                   # ... and no state
    e.surfaces_enable(2, 64 * 48 * 3)
    assert _code(e.camera_surfaces, [0], [0]) == ARG and _code(e.camera_surfaces, [2], [0]) == ARG   # undefined, out of range
    e.surface_define(0, BGR, 64, 48)
    assert _code(e.camera_surfaces, [0], [0]) == INPUT                                               # defined, no keyframe
    m.check(e, [0, 1, 2, 3], "the store's refusals")
    good("after the store's refusals")
    e.surface_update([(0, 0, 0, frames[1].reshape(-1), v)])
    e.camera_surfaces([0, 0], [0, 2])
    m.frame(0, frames[1])
    m.frame(2, frames[1])
    m.check(e, [0, 1, 2, 3], "the accepted surfaces call")
    e.close()
    twin.close()
