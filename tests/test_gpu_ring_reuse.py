"""The upload rings (csrc/upload_ring.h) across the wrap: a call's table -- the tracker's grouping, the tile table, the frame records of the zoom
plan, the chips and the change map -- reaches its kernel through a ring of eight entries, and the feature tests mostly make fewer calls per engine
than that.  Here every case makes 19 consecutive calls on one engine, two laps and three, with a table that differs from the previous call's every
time, and compares every call's result with the feature's host reference.  Where the calls only enqueue (tracking, merge, chips) all 19 are
enqueued, each on buffers of its own, before the first result is read: an entry rewritten before its kernel had read it would show in an earlier
call's output.  No case runs the network: slabs are crafted, frames are small, max_batch = 4, max_dets = 16.
"""
import numpy as np
import pytest
import torch            # before the first engine: the process then uses torch's HIP runtime throughout, as tests/test_gpu_parity.py does

import change_cases as cs
import change_ref as chr_
import chip_cases as cc
import chip_ref as cr
import merge_cases as mc
import merge_ref
import test_gpu_change as tch
import track_cases as tc
import track_ref
import zly
import zoom_ref

pytestmark = pytest.mark.gpu

CALLS, CAP, B = 19, 16, 4
BGR = zly.PIX_BGR
assert CALLS == 2 * 8 + 3


def _engine(weights_path):
    return zly.Engine(weights_path, model_w=64, model_h=64, max_batch=B, max_dets=CAP, warmup_runs=0, use_graph=False)


def _boxes(rng, n, lo=0.05, hi=0.3):
    """n boxes inside the unit square, in sixteenths of it at the centre: (x, y, w, h)"""
    return [(float(rng.integers(3, 14)) / 16, float(rng.integers(3, 14)) / 16, float(rng.uniform(lo, hi)), float(rng.uniform(lo, hi))) for _ in range(n)]


# ---- tracking ---------------------------------------------------------------------------------------------------------------------------------
def _drift(rng, n_frames, n_obj):
    """n_frames frames of n_obj drifting boxes of two classes, each seen in about four frames of five"""
    pos, vel = rng.uniform(0.2, 0.8, (n_obj, 2)), rng.uniform(-0.01, 0.01, (n_obj, 2))
    size, cls = rng.uniform(0.08, 0.2, (n_obj, 2)), rng.integers(0, 2, n_obj)
    frames = []
    for f in range(n_frames):
        seen = [i for i in range(n_obj) if rng.random() < 0.8]
        frames.append(tc.dets([(pos[i, 0] + f * vel[i, 0], pos[i, 1] + f * vel[i, 1], size[i, 0], size[i, 1]) for i in seen], [int(cls[i]) for i in seen]))
    return frames


# the groupings of a call's four slabs: -1 entries, one stream twice, two streams interleaved, a third stream; consecutive calls never share one
GROUPINGS = [[0, 1, 0, 1], [-1, 0, 0, 1], [1, 1, -1, 0], [0, -1, 1, -1], [2, 0, 1, 2], [1, 0, 1, 0], [-1, -1, 2, -1]]


def test_tracking_groupings_over_two_laps(weights_path):
    e = _engine(weights_path)
    e.track_enable(max_streams=3, max_tracks=CAP, match_iou=0.3, max_lost=2)
    rng = np.random.default_rng(191)
    films = {s: _drift(rng, 2 * CALLS, 6) for s in range(3)}
    nxt = {s: 0 for s in range(3)}
    trk = {s: track_ref.Tracker(CAP, CAP, 0.3, 2) for s in range(3)}
    filler = tc.dets(_boxes(rng, 3))
    calls = []
    for k in range(CALLS):
        streams = GROUPINGS[k % len(GROUPINGS)]
        assert k == 0 or streams != GROUPINGS[(k - 1) % len(GROUPINGS)]
        fl = []
        for s in streams:
            fl.append(filler if s < 0 else films[s][nxt[s]])
            nxt[max(s, 0)] += s >= 0
        raw = tc.build_slabs(fl, CAP, tag0=tc.TAG0 + 16 * k)
        want = tc.with_ids(raw, track_ref.run_streams(trk, fl, streams), CAP)
        calls.append((streams, torch.from_numpy(raw).cuda(), want))
    torch.cuda.synchronize()
    for streams, d, _ in calls:                                     # nothing but enqueues
        e.track_slabs(streams, d.data_ptr())
    e.sync()
    for k, (streams, d, want) in enumerate(calls):
        got = d.cpu().numpy()
        if not np.array_equal(got, want):
            i = int(np.flatnonzero((got != want).any(axis=1))[0])
            pytest.fail(f"call {k} = {streams}: slab {i}: ids {tc.slab_ids(got[i], CAP).tolist()} want {tc.slab_ids(want[i], CAP).tolist()}")
    for s, o in trk.items():
        assert e.track_state(s) == o.state(), s
        live = [t for t in range(o.T) if o.live[t]]
        want = np.zeros(len(live), dtype=zly.TRACK_DTYPE)                # vx, vy, hits: 0 without the motion model
        for j, t in enumerate(live):
            want[j]["x"], want[j]["y"], want[j]["w"], want[j]["h"] = o.box[t]
            want[j]["class_id"], want[j]["id"], want[j]["last_seen"] = o.cls[t], o.id[t], o.last_seen[t]
        assert len(live) >= 3 and e.track_read(s).tobytes() == want.tobytes(), (s, e.track_read(s), want)
    assert sum(o.counts["matches"] for o in trk.values()) >= 100 and sum(o.counts["births"] for o in trk.values()) >= 18
    e.close()


# ---- merge ------------------------------------------------------------------------------------------------------------------------------------
def test_merge_tile_tables_over_two_laps(weights_path):
    """four source slabs, the same in every call; the tile table -- who belongs to which of two groups, who sits out, and every tile's x0, y0 --
    changes from call to call, and the survivors with it: boxes that coincide under one pair of offsets lie apart under the next"""
    e = _engine(weights_path)
    rng = np.random.default_rng(192)
    frames = []
    for i in range(B):
        f = tc.dets(_boxes(rng, 12), [int(c) for c in rng.integers(0, 2, 12)])
        f["confidence"] = np.sort(rng.uniform(0.3, 0.95, 12).astype(np.float32))[::-1]
        frames.append(f)
    raw = tc.build_slabs(frames, CAP, tag0=mc.TAG0)
    d_src = torch.from_numpy(raw).cuda()
    sb, calls, prev = mc.slab_bytes(CAP), [], None
    for k in range(CALLS):
        tiles = []
        for i in range(B):
            g = -1 if (i + k) % 5 == 4 else (i + k // 2) % 2
            tiles.append((g, 8 * ((3 * k + 5 * i) % 17), 8 * ((5 * k + 2 * i) % 17), 128, 128, 256, 256))
        assert tiles != prev and {t[0] for t in tiles} >= {0, 1}
        prev = tiles
        before = mc.poison(2, CAP, 64)
        want = merge_ref.merge_slabs(raw, tiles, 2, CAP, merge_ref.IOS, 0.5, mc.TAG0 + 8 * k, before[:2 * sb].reshape(2, sb))
        calls.append((tiles, torch.from_numpy(before).cuda(), want))
    torch.cuda.synchronize()
    for k, (tiles, d_out, _) in enumerate(calls):                  # nothing but enqueues
        e.merge_slabs([zly.Tile(*t) for t in tiles], 2, merge_ref.IOS, 0.5, d_src.data_ptr(), d_out.data_ptr(), mc.TAG0 + 8 * k)
    e.sync()
    kept = set()
    for k, (tiles, d_out, want) in enumerate(calls):
        got = d_out.cpu().numpy()
        assert np.array_equal(got[:2 * sb].reshape(2, sb), want), f"call {k}: tiles {tiles}: headers {got[:16].view(zly.SLAB_HDR_DTYPE)} want {want[0, :16].view(zly.SLAB_HDR_DTYPE)}"
        assert (got[2 * sb:] == mc.POISON).all(), f"call {k}: bytes behind the last slab were written"
        kept.add(tuple(int(want[g, :16].view(zly.SLAB_HDR_DTYPE)["n_kept"][0]) for g in range(2)))
    assert len(kept) >= 5, kept                                    # the tables really give different results
    assert np.array_equal(d_src.cpu().numpy(), raw), "the sources were modified"
    e.close()


# ---- chips ------------------------------------------------------------------------------------------------------------------------------------
def test_chip_views_over_two_laps(weights_path):
    """two crops of one 96 x 80 BGR surface per call, origin and size changing every call; the boxes are fractions of the crop, so every chip does"""
    cfg = cr.Config(chip_w=16, chip_h=16, max_chips=4, class_id=-1, scale=1.0, layout=cr.BGR8)
    e = _engine(weights_path)
    e.chips_enable(chip_w=cfg.chip_w, chip_h=cfg.chip_h, max_chips=cfg.max_chips, class_id=cfg.class_id, scale=cfg.scale, layout=cfg.layout)
    W, H = 96, 80
    flat, surf = cc.frame(BGR, W, H, seed=193)
    d_base = torch.from_numpy(flat).cuda()
    dets = [(0.5, 0.5, 0.5, 0.5, 0.9, 0, 7), (0.25, 0.25, 0.25, 0.25, 0.8, 1, 8), (0.75, 0.625, 0.25, 0.5, 0.7, 0, 9)]
    slabs = np.stack([cr.make_slab(dets, cap=CAP, frame_tag=50, fill=0xEE), cr.make_slab(dets[::-1], cap=CAP, frame_tag=51, fill=0xEE)])
    d_slabs = torch.from_numpy(slabs).cuda()
    sb = cr.layout(cfg)[0]
    calls, prev = [], None
    for k in range(CALLS):
        crops = [((7 * k) % 40, (5 * k) % 30, 24 + (3 * k) % 32, 20 + (7 * k) % 30), ((11 * k + 3) % 50, (3 * k + 1) % 40, 16 + (5 * k) % 30, 40 - k)]
        assert crops != prev and all(x0 + w <= W and y0 + h <= H for x0, y0, w, h in crops)
        prev = crops
        views = [cc.to_c((BGR, w, h, [(y0 * W + x0) * 3, 0, 0], [W * 3, 0, 0])) for x0, y0, w, h in crops]
        before = np.full((2, sb), cc.POISON, dtype=np.uint8)
        want = cr.chip_slabs(slabs, [np.ascontiguousarray(surf[y0:y0 + h, x0:x0 + w]) for x0, y0, w, h in crops], cfg, before, cap=CAP)
        calls.append((views, torch.from_numpy(before).cuda(), want))
    torch.cuda.synchronize()
    for views, d_chips, _ in calls:                                 # nothing but enqueues
        e.chips_device_view(d_base.data_ptr(), flat.nbytes, views, d_slabs_ptr=d_slabs.data_ptr(), d_chips_ptr=d_chips.data_ptr())
    e.sync()
    torch.cuda.synchronize()
    for k, (_, d_chips, want) in enumerate(calls):
        got = d_chips.cpu().numpy()
        assert np.array_equal(got, want), f"call {k}: {np.count_nonzero(got != want)} bytes differ, first at (frame, byte) {np.argwhere(got != want)[:4].tolist()}"
        assert int(want[0, :16].view(cr.HDR_DTYPE)[0]["n_chips"]) == 3
    e.close()


# ---- change map -------------------------------------------------------------------------------------------------------------------------------
def test_change_views_and_a_reset_over_two_laps(weights_path):
    """stream 0 sees a film of one geometry (real differences), stream 1 a frame of another size every call (a first frame each time, whose grid leaves
    the larger grids' cells behind it alone); their order in the call alternates.  The reset before call 10 takes a ring entry of its own mid-lap.
    Every stream's whole record is read and compared after every call"""
    cfg = chr_.Config(cell=16, threshold_q4=8, max_active_permille=600, max_peaks=3, window_w=32, window_h=32)
    e = _engine(weights_path)
    e.change_enable(2, cell=cfg.cell, threshold_q4=cfg.threshold_q4, max_active_permille=cfg.max_active_permille, max_peaks=cfg.max_peaks,
                    window_w=cfg.window_w, window_h=cfg.window_h)
    assert e.change_layout() == chr_.layout(cfg)
    m = tch.Mirror(cfg, 2)
    film = cs.film(BGR, 96, 64, ["new"] + ["blocks", "flat", "same", "blocks"] * 5, seed=194)
    for k in range(CALLS):
        if k == 10:
            e.change_reset(0)
            m.streams[0].reset()
        w, h = 33 + (17 * k) % 90, 21 + (11 * k) % 70
        other = cc.frame(BGR, w, h, seed=300 + k)
        items = [(film[k][0], cc.tight_view(BGR, 96, 64), film[k][1]), (other[0], cc.tight_view(BGR, w, h), other[1])]
        tch._call(e, m, items[::-1] if k % 2 else items, [1, 0] if k % 2 else [0, 1], f"call {k}")
    flags = lambda s: int(m.recs[s][:32].view(chr_.HDR_DTYPE)[0]["flags"])          # noqa: E731
    assert m.flags >= {0, chr_.FIRST} and m.peaks >= 6 and flags(1) == chr_.FIRST, (m.flags, m.peaks)
    assert int(m.recs[0][:32].view(chr_.HDR_DTYPE)[0]["step"]) == CALLS - 10     # the reset took: stream 0 counts from call 10
    e.close()


# ---- zoom plan --------------------------------------------------------------------------------------------------------------------------------
def test_zoom_plans_over_two_laps(weights_path):
    """Tracked slabs seed streams 0 and 1; then 19 zly_zoom_plan calls of one to four frames whose sizes and streams change every call (stream 2 has
    no tracks: fallbacks).  zly_zoom_plan returns its own records; zly_zoom_read_plan belongs to the frame calls, which run the network, and must go
    on refusing here: the plan calls' ring entries are none of its business"""
    cfg = zoom_ref.Config(regions=3, region_w=48, region_h=32, max_age=2, class_id=-1)
    e = _engine(weights_path)
    e.track_enable(max_streams=3, max_tracks=CAP, match_iou=0.3, max_lost=2)
    e.zoom_enable(regions=cfg.regions, region_w=cfg.region_w, region_h=cfg.region_h, max_age=cfg.max_age, class_id=cfg.class_id)
    rng = np.random.default_rng(195)
    trk = {s: track_ref.Tracker(CAP, CAP, 0.3, 2) for s in range(3)}
    for f in range(3):
        fl = [tc.dets(_boxes(np.random.default_rng(500 + s), 6, 0.03, 0.12), [0, 1, 0, 2, 1, 0]) for s in (0, 1)]      # the same boxes every frame: matches
        d = torch.from_numpy(tc.build_slabs(fl, CAP)).cuda()
        torch.cuda.synchronize()
        e.track_slabs([0, 1], d.data_ptr())
        e.sync()
        track_ref.run_streams(trk, fl, [0, 1])
    tables = {s: zoom_ref.table_of(trk[s]) for s in range(3)}
    n_zoomed, prev = 0, None
    for k in range(CALLS):
        n = 1 + k % B
        sizes = [(int(rng.integers(40, 641)), int(rng.integers(30, 481))) for _ in range(n)]
        streams = [(k + i) % 3 for i in range(n)]
        assert (sizes, streams) != prev
        prev = (sizes, streams)
        got = e.zoom_plan(sizes, streams)
        for i, ((W, H), s) in enumerate(zip(sizes, streams)):
            want = zoom_ref.plan(tables[s], cfg, W, H)
            assert got[i].tobytes() == want.tobytes(), (k, i, (W, H), s, got[i], want)
            n_zoomed += int((want["slot"] >= 0).sum())
    assert n_zoomed >= 30, n_zoomed
    out = np.zeros((1, cfg.regions), dtype=zly.ZOOM_REGION_DTYPE)
    assert e.lib.zly_zoom_read_plan(e.h, 1, out.ctypes.data) == zly.ERR_INVALID_ARGUMENT
    e.close()
