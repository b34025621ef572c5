"""Zoom regions on the GPU (include/zly.h "Zoom regions"; csrc/kernels_zoom.hip).

1. The plan kernel's records against the numpy oracle (tests/zoom_ref.py) on track tables that hand-made slab sequences built through zly_track_slabs.
2. THE RULE: the zoom call's merged, tracked slabs equal, byte for byte, those of a twin engine driven through the explicit sequence of existing calls
   (the oracle's plan from zly_track_read, zly_view_crop, zly_detect_device_view, zly_merge_slabs, zly_track_slabs) -- on stretch, letterbox and area
   engines, with and without ZLY_FLAG_ASYNC_NMS, on five pixel formats, and on resident surfaces with nothing but enqueues between the steps.
3. Refusals enqueue nothing; an engine that never enables zoom is unchanged.
A 416 x 416 engine, max_batch 16, K = 3 regions of 208 x 208 on surfaces of at most 640 x 480: the smallest shapes at which clamps, coverage and
three-plane offsets all occur; THE RULE once more at K = 1 and K = 15 with tables of 16 slots and a class filter.  (The plan kernel on tables no
tracker reaches from a reset, at every K: tests/test_gpu_track_tables.py.)"""
import os

import numpy as np
import pytest
import torch            # before the first engine: the process then uses torch's HIP runtime throughout, as tests/test_gpu_parity.py does

import yuv422_ref
import yuv_ref
import zly
import zoom_ref
from track_motion_ref import MotionTracker
from track_ref import Tracker
import zoom_cases as zc
from zoom_cases import CFG0, hand_cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "zly_golden_64.npz"))
CONF, IOU = float(G["conf"]), float(G["iou"])
CAP, POISON = 64, 0xCD
BGR, BGRA, NV12, I420, YUY2 = zly.PIX_BGR, zly.PIX_BGRA, zly.PIX_NV12_BT601, zly.PIX_I420_BT709, zly.PIX_YUY2_BT601
MODES = {"stretch": 0, "letterbox": zly.FLAG_LETTERBOX, "area": zly.FLAG_AREA}


def _engine(weights_path, flags=0, track=True, motion=False, zoom=True, max_batch=16, surfaces=0, cfg=CFG0, max_tracks=64):
    """max_dets = min(CAP, max_tracks): a tracking engine stores at most as many detections as its tables have slots"""
    e = zly.Engine(weights_path, dtype=zly.DTYPE_BF16, max_batch=max_batch, max_dets=min(CAP, max_tracks), conf_thr=CONF, iou_thr=IOU, warmup_runs=0, flags=flags)
    if track:
        e.track_enable(max_streams=8, max_tracks=max_tracks)
    if motion:
        e.track_motion_enable()
    if zoom:
        e.zoom_enable(regions=cfg.regions, region_w=cfg.region_w, region_h=cfg.region_h, max_age=cfg.max_age, class_id=cfg.class_id)
    if surfaces:
        e.surfaces_enable(surfaces, 640 * 480 * 4)
    return e


# ---- 1. plan bytes ---------------------------------------------------------------------------------------------------------------
def _slabs(frames, sb):
    """frames: lists of (x, y, w, h, cls) -> one slab each, as NMS would have stored them"""
    raw = np.zeros((len(frames), sb), dtype=np.uint8)
    for i, boxes in enumerate(frames):
        hdr = raw[i, :16].view(zly.SLAB_HDR_DTYPE)
        hdr["n_kept"], hdr["n_candidates"] = len(boxes), len(boxes)
        d = raw[i, 16:].view(zly.DET_DTYPE)
        for k, (x, y, w, h, c) in enumerate(boxes):
            d[k]["x"], d[k]["y"], d[k]["w"], d[k]["h"], d[k]["class_id"], d[k]["confidence"] = x, y, w, h, c, 0.9
    return raw


def _sequence_of(t):
    """a slab sequence that builds a table with a hand case's geometry: every live slot is born in the frame it was last seen in (its slot index and
    id are then the tracker's choice, not the case's: the oracle runs on the tracker's table)"""
    frames = []
    for f in range(1, t.frame_no + 1):
        frames.append([tuple(t.box[s]) + (t.cls[s],) for s in range(t.T) if t.live[s] and t.last_seen[s] == f])
    return frames


def _scenarios():
    out = []
    for name, t, cfg, W, H, _ in hand_cases():
        if cfg == CFG0 and 0 < t.frame_no < 100 and not any(np.isnan(v) or v != 0 for v in t.vx + t.vy):
            out.append((name, _sequence_of(t), [(W, H)], False))
    # the hand case 'product-rounded-first' (dropped above: it has a velocity), through the slab sequence that gives a motion engine its velocity: on
    # the plain engine vx = 0 and the region follows the stored box; on the motion engine a fused prediction would put x0 at 512 instead of 510
    box = (0.5, zc.FUSED_SIZE, zc.FUSED_SIZE, 0)
    out.append(("product-rounded-first", [[(zc.FUSED_X1,) + box], [], [], [(zc.FUSED_X2,) + box], [], []], [(zc.FUSED_W, 480)], False))
    rng = np.random.default_rng(77)
    for k in range(6):                                      # seeded: targets that drift, drop out and come back; with and without the motion model
        n_t, steps = int(rng.integers(3, 40)), int(rng.integers(2, 7))
        pos, vel = rng.uniform(0, 1, (n_t, 2)), rng.uniform(-0.03, 0.03, (n_t, 2))
        size, cls = rng.uniform(0.01, 0.4, (n_t, 2)) * rng.choice([1, 0.25], (n_t, 1)), rng.integers(0, 3, n_t)
        frames = []
        for f in range(steps):
            seen = rng.random(n_t) < 0.8
            frames.append([(pos[i, 0] + f * vel[i, 0], pos[i, 1] + f * vel[i, 1], size[i, 0], size[i, 1], int(cls[i])) for i in range(n_t) if seen[i]])
        sizes = [(640, 480), (641, 479), (int(rng.integers(2, 641)), int(rng.integers(2, 481))), (101, 77)]
        out.append((f"seeded{k}", frames, sizes, bool(k % 2)))
    return out


def test_plan_records_equal_the_oracle(weights_path):
    engines = {False: _engine(weights_path), True: _engine(weights_path, motion=True)}
    sb = engines[False].slab_bytes
    n_zoomed = n_covered = 0
    for name, frames, sizes, motion in _scenarios():
        for with_motion in ((False, True) if not motion else (True,)):
            e = engines[with_motion]
            e.track_reset(-1, 1)
            trk = MotionTracker(64, CAP) if with_motion else Tracker(64, CAP)
            raw = _slabs(frames, sb)
            d = torch.from_numpy(raw.reshape(-1)).cuda()
            torch.cuda.synchronize()
            for f in range(len(frames)):                    # one frame per call: stream 3, on an engine that has made no detect call
                e.track_slabs([3], d.data_ptr() + f * sb)
                trk.step(raw[f, 16:].view(zly.DET_DTYPE), len(frames[f]))
            assert e.track_state(3) == trk.state(), name
            table = zoom_ref.table_of(trk)
            want = []
            for W, H in sizes:
                w, covered = zoom_ref.plan(table, CFG0, W, H, with_covered=True)
                want.append(w)
                n_zoomed += int((w["slot"] >= 0).sum())
                n_covered += len(covered)
            # all sizes in one call, the stream repeated; an untouched stream (no tracks: fallbacks) rides along
            got = e.zoom_plan(list(sizes) + [(640, 480)], [3] * len(sizes) + [5])
            for i, w in enumerate(want):
                assert got[i].tobytes() == w.tobytes(), (name, with_motion, sizes[i], got[i], w)
            if name == "product-rounded-first" and with_motion:             # the table is the hand case's, and the kernel did not fuse the prediction
                tr = e.track_read(3)
                assert len(tr) == 1 and tr[0]["vx"] == zc.FUSED_VX and tr[0]["x"] == zc.FUSED_X2
                assert int(got[0][0]["x0"]) == zc.FUSED_X0 != zc.FUSED_X0_IF_FUSED
            assert got[len(sizes)].tobytes() == zoom_ref.plan(zoom_ref.Table(), CFG0, 640, 480).tobytes()
            # ... and the same frames in another order give the same records
            again = e.zoom_plan([(640, 480)] + list(sizes)[::-1], [5] + [3] * len(sizes))
            assert again[1:].tobytes() == got[:len(sizes)][::-1].tobytes() and again[0].tobytes() == got[len(sizes)].tobytes(), name
    assert n_zoomed >= 40 and n_covered >= 5, (n_zoomed, n_covered)
    for e in engines.values():
        e.close()


# ---- 2. the rule -----------------------------------------------------------------------------------------------------------------
def _picture(w, h, dx, dy, variant=0):
    """a w x h BGR picture tiled from the golden frames, shifted by (dx, dy)"""
    f = G["frames_64"]
    cell = np.zeros((144, 160, 3), dtype=np.uint8)
    cell[:64, :64], cell[:64, 64:128], cell[64:144, :96] = f[variant % 2], f[(variant + 1) % 2], G["frame_96x80"]
    cell[64:128, 96:160], cell[:64, 128:160] = f[variant % 2], f[(variant + 1) % 2][:, :32]
    big = np.tile(cell, ((h + 2 * 144) // 144 + 1, (w + 2 * 160) // 160 + 1, 1))
    return np.ascontiguousarray(big[dy % 144:dy % 144 + h, dx % 160:dx % 160 + w])


def _as_format(fmt, bgr):
    if fmt == BGR:
        return np.ascontiguousarray(bgr).reshape(-1)
    if fmt == BGRA:
        return np.ascontiguousarray(np.concatenate([bgr, np.full(bgr.shape[:2] + (1,), 255, np.uint8)], axis=2)).reshape(-1)
    if fmt in (NV12, I420):
        return yuv_ref.bgr_to_yuv420(bgr, fmt)
    return yuv422_ref.from_bgr(bgr, fmt)


def _pack(surfaces):
    """surfaces: (fmt, w, h, tight bytes, pitch of plane 0 or None) -> (host buffer, one FrameView per surface), the surfaces one behind the other"""
    parts, views, off = [], [], 256
    for fmt, w, h, px, pitch in surfaces:
        v = zly.view_tight(fmt, w, h)
        if pitch is None:
            data = px
        else:                                               # single-plane formats only: rows `pitch` bytes apart
            rb = int(v.pitch[0])
            data = np.full(h * pitch, 0x5A, dtype=np.uint8)
            data.reshape(h, pitch)[:, :rb] = px.reshape(h, rb)
            v.pitch[0] = pitch
        for p in range(3):
            v.off[p] += off
        parts.append((off, data))
        views.append(v)
        off = (off + data.size + 255) // 256 * 256 + 64
    host = np.full(off, 0xA5, dtype=np.uint8)
    for o, data in parts:
        host[o:o + data.size] = data
    return host, views


def _table_from_engine(e, stream):
    """the stream's table as the plan reads it, from zly_track_read: the live slots in slot order (consecutive indices keep the order)"""
    t = zoom_ref.Table(frame_no=e.track_state(stream)["frame_no"])
    for r in e.track_read(stream):
        t.add(r["x"], r["y"], r["w"], r["h"], cls=int(r["class_id"]), id=int(r["id"]), last_seen=int(r["last_seen"]), vx=r["vx"], vy=r["vy"])
    return t


class Twin:
    """the explicit sequence of existing calls on an engine of its own"""

    def __init__(self, e, cfg=CFG0):
        self.e, self.cfg, self.covered = e, cfg, 0

    def frame(self, d_ptr, nbytes, views, streams, d_out_ptr, tag0, sync=False):
        tiles, call_views, plans = [], [], []
        for i, (v, s) in enumerate(zip(views, streams)):
            plan, covered = zoom_ref.plan(_table_from_engine(self.e, s), self.cfg, v.w, v.h, with_covered=True)
            self.covered += len(covered)
            plans.append(plan)
            call_views.append(v)
            tiles.append(zly.tile(0, 0, v.w, v.h, v.w, v.h, group=i))
            for r in plan:
                call_views.append(zly.view_crop(v, int(r["x0"]), int(r["y0"]), int(r["w"]), int(r["h"])))
                tiles.append(zly.tile(int(r["x0"]), int(r["y0"]), int(r["w"]), int(r["h"]), v.w, v.h, group=i))
        self.e.detect_device_view(d_ptr, nbytes, call_views)
        self.e.merge_slabs(tiles, len(views), d_out_ptr=d_out_ptr, tag0=tag0)
        self.e.track_slabs(list(streams), d_out_ptr)
        if sync:
            self.e.sync()
        return plans


def _same_plan(got, want):
    """the records but for the slot index, which zly_track_read does not tell"""
    return all(np.array_equal(got[k], want[k]) for k in ("x0", "y0", "w", "h", "track_id")) and np.array_equal(got["slot"] < 0, want["slot"] < 0)


def _run_rule(e1, e2, steps, what, min_kept=1, cfg=CFG0):
    """steps: lists of (fmt, w, h, tight bytes, pitch), one surface per stream.  e1 takes the zoom call (its zoom config: cfg), e2 the explicit sequence"""
    twin = Twin(e2, cfg)
    sb = e1.slab_bytes
    zoomed_steps = 0
    for k, surfaces in enumerate(steps):
        n = len(surfaces)
        streams = list(range(1, n + 1))
        host, views = _pack(surfaces)
        d_host = torch.from_numpy(host).cuda()
        d1 = torch.full((n * sb + 64,), POISON, dtype=torch.uint8, device="cuda")
        d2 = torch.full((n * sb + 64,), POISON, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        e1.detect_device_zoom(d_host.data_ptr(), host.nbytes, views, streams, d_out_ptr=d1.data_ptr(), tag0=100 * k)
        plans = twin.frame(d_host.data_ptr(), host.nbytes, views, streams, d2.data_ptr(), 100 * k)
        e1.sync()
        e2.sync()
        got, want = d1.cpu().numpy(), d2.cpu().numpy()
        assert np.array_equal(got, want), (what, k, np.flatnonzero(got != want)[:8])
        assert (got[n * sb:] == POISON).all()
        kept = [int(got[i * sb:i * sb + 16].view(zly.SLAB_HDR_DTYPE)["n_kept"][0]) for i in range(n)]
        assert min(kept) >= min_kept, (what, k, kept)
        plan1 = e1.zoom_read_plan(n)
        for i, s in enumerate(streams):
            assert _same_plan(plan1[i], plans[i]), (what, k, i, plan1[i], plans[i])
            assert e1.track_state(s) == e2.track_state(s) and e1.track_read(s).tobytes() == e2.track_read(s).tobytes(), (what, k, s)
        if k >= 1:
            assert all((p["slot"] >= 0).any() for p in plans), (what, k, plans)       # from the second step on every frame zooms into a track
            zoomed_steps += 1
    return twin, zoomed_steps


SIZES = ((640, 480), (589, 431), (418, 240))


@pytest.mark.parametrize("flags", [0, zly.FLAG_ASYNC_NMS], ids=["in_stream_order", "deferred_nms"])
@pytest.mark.parametrize("mode", list(MODES))
def test_the_rule_on_three_streams_over_six_steps(weights_path, mode, flags):
    e1, e2 = _engine(weights_path, MODES[mode] | flags), _engine(weights_path, MODES[mode] | flags, zoom=False)
    # with the flag a fourth stream rides along: 4 x (1 + K) = 16 views, the batch size from which the engine defers its NMS
    sizes = SIZES + (((334, 250),) if flags else ())
    steps = [[(BGR, w, h, _as_format(BGR, _picture(w, h, 7 * k + 31 * i, 5 * k + 17 * i, i)), None) for i, (w, h) in enumerate(sizes)] for k in range(6)]
    twin, zoomed_steps = _run_rule(e1, e2, steps, (mode, flags))
    assert zoomed_steps == 5 and twin.covered >= 1, (zoomed_steps, twin.covered)          # the run skipped at least one slot as covered
    e1.close()
    e2.close()


def test_the_rule_on_five_formats(weights_path):
    """the plane offsets the kernel computes: a pitched BGRA surface, NV12 and I420 in one call, YUY2 and tight BGR in another; two steps each, so that
    the second one's regions come from tracks"""
    e1, e2 = _engine(weights_path), _engine(weights_path, zoom=False)
    for group in (((BGRA, 418, 240, 4 * 418 + 72), (NV12, 640, 480, None), (I420, 590, 432, None)), ((YUY2, 418, 241, None), (BGR, 333, 251, None))):
        steps = [[(fmt, w, h, _as_format(fmt, _picture(w, h, 9 * k + 13 * i, 3 * k + 29 * i, i)), pitch) for i, (fmt, w, h, pitch) in enumerate(group)] for k in range(2)]
        e1.track_reset(-1, 1)
        e2.track_reset(-1, 1)
        _, zoomed_steps = _run_rule(e1, e2, steps, [g[0] for g in group])
        assert zoomed_steps == 1
    e1.close()
    e2.close()


def _dominant_class(e, cfg, steps):
    """the golden frames' dominant class on this engine: the class most of the live tracks have -- among those a region can hold -- after the explicit
    sequence has run over the steps WITHOUT a class filter.  The stream is reset afterwards"""
    twin = Twin(e, zoom_ref.Config(regions=cfg.regions, region_w=cfg.region_w, region_h=cfg.region_h, max_age=cfg.max_age, class_id=-1))
    for surfaces in steps:
        host, views = _pack(surfaces)
        d_host = torch.from_numpy(host).cuda()
        d_out = torch.zeros(e.slab_bytes, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        twin.frame(d_host.data_ptr(), host.nbytes, views, [1], d_out.data_ptr(), 0, sync=True)
    classes = [int(r["class_id"]) for r in e.track_read(1) if r["w"] * views[0].w <= cfg.region_w and r["h"] * views[0].h <= cfg.region_h]
    e.track_reset(-1, 1)
    hist = np.bincount(classes)
    print("K", cfg.regions, "live tracks that fit a region, per class:", {int(c): int(n) for c, n in enumerate(hist) if n})
    return int(hist.argmax())


@pytest.mark.parametrize("regions", [1, 15])
def test_the_rule_at_one_and_fifteen_regions(weights_path, regions):
    """the host side of the plan kernel's index arithmetic at the ends of K: the uploaded descriptor, view-record and merge tables with every region at
    its fallback origin, and at K = 15 sixteen views from one frame in a batch of 16 and the merge of 16 tiles.  Tables of 16 slots (so 16 stored
    detections), a class filter; one stream, 640 x 480 BGR and (three planes) I420, three steps each.
    Regions of the model's size, the default.  With 16 slots, 15 regions and a class filter the table is easily lost between two steps: slabs are
    stored in class order and cut at 16, so the regions' own detections of lower classes push the filtered class out and evict its tracks.  Measured
    on an MI355X over four region sizes and five picture sequences: THE RULE held in all 40 runs; the zoom condition below held at K = 1 in all of them,
    at K = 15 and 208 x 208 in none for both formats, at 416 x 416 for these pictures with 11 and 17 slots skipped as covered.  Either case takes
    less than 0.65 s (K = 1: 0.14 s)"""
    pictures = [_picture(640, 480, 7 * k + 3, 5 * k + 2, 1) for k in range(3)]
    kw = dict(max_batch=16 if regions == 15 else 1 + regions, max_tracks=16)
    e2 = _engine(weights_path, zoom=False, **kw)
    cfg = zoom_ref.Config(regions=regions, region_w=e2.model_w, region_h=e2.model_h, max_age=CFG0.max_age, class_id=-1)
    cfg.class_id = _dominant_class(e2, cfg, [[(BGR, 640, 480, _as_format(BGR, bgr), None)] for bgr in pictures])
    e1 = _engine(weights_path, cfg=cfg, **kw)
    assert e1.max_dets == 16 and e1.zoom_regions == regions and cfg.class_id >= 0
    for fmt in (BGR, I420):
        steps = [[(fmt, 640, 480, _as_format(fmt, bgr), None)] for bgr in pictures]
        e1.track_reset(-1, 1)
        e2.track_reset(-1, 1)
        twin, zoomed_steps = _run_rule(e1, e2, steps, (regions, fmt), cfg=cfg)
        assert zoomed_steps == 2
        assert regions == 1 or twin.covered >= 1            # fifteen overlapping regions: the greedy choice skipped covered slots
    e1.close()
    e2.close()


def test_resident_surfaces_with_nothing_but_enqueues(weights_path):
    """update k, zoom k on two callers' streams in turn, update k + 1, ...: every step a whole new picture.  The patch kernel of update k + 1 must wait
    for the zoom call's reads (ev_read behind the call's LAST kernel, its tracker) and the zoom call for the patch (ev_patch): the twin synchronises
    after every call.  That chain -- tracker k, ev_read, patch k + 1, ev_patch, zoom k + 1 -- already puts the plan kernel behind the tracker before
    it, so this test does NOT exercise the plan kernel's own wait on Track::ev; the deferred-NMS runs of the rule test do (their tracker runs on the
    engine's NMS stream, the next plan on the call's)."""
    e1, e2 = _engine(weights_path, surfaces=4), _engine(weights_path, surfaces=4)
    shapes = ((BGRA, 640, 480), (NV12, 418, 240), (BGR, 333, 251))
    n, steps, sb = len(shapes), 4, e1.slab_bytes
    films = [[_as_format(fmt, _picture(w, h, 11 * k + 40 * i, 6 * k + 23 * i, i + k)) for k in range(steps)] for i, (fmt, w, h) in enumerate(shapes)]
    callers = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [torch.full((steps * n * sb,), POISON, dtype=torch.uint8, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    for e in (e1, e2):
        for i, (fmt, w, h) in enumerate(shapes):
            e.surface_define(i, fmt, w, h)
    plans = []
    for which, e in enumerate((e1, e2)):
        for k in range(steps):
            e.surface_update([(i, 0, 0, films[i][k], zly.view_tight(fmt, w, h)) for i, (fmt, w, h) in enumerate(shapes)])
            if which:
                e.sync()
            e.detect_surfaces_zoom(list(range(n)), [1, 2, 3], d_out_ptr=outs[which].data_ptr() + k * n * sb, tag0=10 * k, stream=callers[k % 2].cuda_stream)
            if which:
                callers[k % 2].synchronize()
                e.sync()
                plans.append(e.zoom_read_plan(n))
        for c in callers:
            c.synchronize()
        e.sync()
    got, want = outs[0].cpu().numpy(), outs[1].cpu().numpy()
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    assert all((p["slot"] >= 0).any() for plan in plans[1:] for p in plan)            # the later steps zoomed into tracks: the plan depended on the step before
    assert e1.zoom_read_plan(n).tobytes() == plans[-1].tobytes()
    for s in (1, 2, 3):
        assert e1.track_read(s).tobytes() == e2.track_read(s).tobytes()
    e1.close()
    e2.close()


# ---- 3. refusals, unchanged engines ---------------------------------------------------------------------------------------------
def _code(f, *a, **k):
    with pytest.raises(zly.ZlyError) as ei:
        f(*a, **k)
    return ei.value.code


def test_refusals_enqueue_nothing(weights_path):
    e = _engine(weights_path, surfaces=2)
    ARG = zly.ERR_INVALID_ARGUMENT
    sb = e.slab_bytes
    pics = [(BGR, w, h, _as_format(BGR, _picture(w, h, 0, 0, i)), None) for i, (w, h) in enumerate(SIZES)]
    host, views = _pack(pics)
    d_host = torch.from_numpy(host).cuda()
    d_out = torch.full((16 * sb,), POISON, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    e.detect_device_zoom(d_host.data_ptr(), host.nbytes, views, [1, 2, 3], d_out_ptr=d_out.data_ptr())       # a good call first: tables and a plan to disturb
    e.sync()
    before = (d_out.cpu().numpy(), [e.track_read(s).tobytes() for s in range(8)], [e.track_state(s) for s in range(8)], e.zoom_read_plan(3).tobytes(),
              [(h, d.tobytes()) for h, d in e.read_slabs(12)])
    d_out.fill_(POISON)
    torch.cuda.synchronize()
    call = lambda vs, ss, **kw: e.detect_device_zoom(d_host.data_ptr(), host.nbytes, vs, ss, d_out_ptr=d_out.data_ptr(), **kw)
    assert _code(call, views, [1, 2, 1]) == ARG                                      # a stream twice
    assert _code(call, views, [1, -1, 3]) == ARG                                     # an untracked frame
    assert _code(call, views, [1, 2, 8]) == ARG                                      # beyond max_streams
    assert _code(call, views + views[:2], [1, 2, 3, 4, 5]) == ARG                    # 5 x 4 views > max_batch
    narrow = zly.view_tight(BGR, 1, 64)
    assert _code(call, [views[0], narrow], [1, 2]) == ARG                            # W < 2
    unknown = zly.view_tight(BGR, 64, 64)
    unknown.fmt = 9
    assert _code(call, [views[0], unknown], [1, 2]) == ARG                           # an unknown format
    assert _code(call, views, [1, 2, 3], thr=1.5) == ARG                             # the merge's config
    assert _code(e.detect_device_zoom, d_host.data_ptr(), int(views[2].off[0]) + 16, views, [1, 2, 3], d_out_ptr=d_out.data_ptr()) == zly.ERR_INVALID_INPUT
    assert _code(e.detect_surfaces_zoom, [2], [1], d_out_ptr=d_out.data_ptr()) == ARG                          # a slot the store does not have
    e.surface_define(0, BGR, 64, 64)
    assert _code(e.detect_surfaces_zoom, [0], [1], d_out_ptr=d_out.data_ptr()) == zly.ERR_INVALID_INPUT        # defined, no keyframe
    assert _code(e.zoom_plan, [(1, 64)], [1]) == ARG and _code(e.zoom_plan, [(64, 64)], [8]) == ARG
    assert _code(e.zoom_read_plan, 2) == ARG                                         # the last call had three frames
    assert _code(e.zoom_enable) == ARG                                               # twice
    e.sync()
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == POISON).all()
    after = ([e.track_read(s).tobytes() for s in range(8)], [e.track_state(s) for s in range(8)], e.zoom_read_plan(3).tobytes(),
             [(h, d.tobytes()) for h, d in e.read_slabs(12)])
    assert after == before[1:]
    e.close()
    # enabling: out-of-range configs, engines without tables, too many regions for the batch or the merge
    plain = _engine(weights_path, track=False, zoom=False, max_batch=4)
    assert _code(plain.zoom_enable) == ARG and "zly_track_enable" in zly.load_library().zly_last_error().decode()
    assert _code(plain.detect_device_zoom, d_host.data_ptr(), host.nbytes, views[:1], [1]) == ARG             # an engine without zoom (and without tracking)
    plain.track_enable(max_streams=2, max_tracks=64)
    assert _code(plain.detect_device_zoom, d_host.data_ptr(), host.nbytes, views[:1], [1]) == ARG             # tracking, no zoom
    assert _code(plain.zoom_plan, [(64, 64)], [1]) == ARG and _code(plain.zoom_read_plan, 1) == ARG
    for bad in (dict(regions=0), dict(regions=16), dict(region_w=207), dict(region_h=0), dict(region_w=16386), dict(max_age=-1), dict(class_id=-2),
                dict(regions=4)):                                                    # 1 + 4 > max_batch
        assert _code(plain.zoom_enable, **bad) == ARG, bad
    assert plain.lib.zly_zoom_enable(plain.h, None) == ARG
    plain.zoom_enable(regions=3)                                                     # the defaults: regions of the model's size
    assert _code(plain.zoom_read_plan, 1) == ARG                                     # no zoom call yet
    plain.close()


def test_an_engine_that_never_zooms_is_unchanged(weights_path):
    """the plain calls give the same bytes on an engine that enabled zoom (and zoomed) as on one that never did, and the two engines' launch tables
    are equal.  That shows zooming alters neither; that a non-zooming engine's tables and kernels are the PARENT's is not something a test of one build
    can show -- it follows from the diff (run_path, resolve_launches and every existing kernel are untouched; tools/isa_diff.py --allow-added against
    the parent lists zoom_plan_kernel alone) and from the existing suites, which pin the launch kinds and pass unchanged."""
    plain, zooming = _engine(weights_path, track=False, zoom=False), _engine(weights_path)
    pics = [(BGR, w, h, _as_format(BGR, _picture(w, h, 3, 4, i)), None) for i, (w, h) in enumerate(SIZES)]
    host, views = _pack(pics)
    d_host = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    got = []
    for e in (plain, zooming):
        rounds = []
        for r in range(2):
            if e is zooming:                                # a zoom call in front: it leaves kernel-written descriptors behind
                e.detect_device_zoom(d_host.data_ptr(), host.nbytes, views, [1, 2, 3])
            e.detect_device_view(d_host.data_ptr(), host.nbytes, views, tag0=3)
            rounds.append([(h.copy(), d.tobytes()) for h, d in e.read_slabs(3)])
        got.append(rounds)
    assert got[0] == got[1] and all(int(h["n_kept"]) >= 1 for h, _ in got[0][0])
    for n in (1, 4, 12, 16):
        assert plain.launches(n) == zooming.launches(n)
    plain.close()
    zooming.close()
