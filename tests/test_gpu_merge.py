"""merge_kernel behind the C ABI (include/zly.h, "Tiles") against the numpy oracle tests/merge_ref.py, byte for byte.

The crafted cases (tests/merge_cases.py) run no forward pass: source slabs are built in numpy, put in a torch device buffer and handed to
zly_merge_slabs with d_slabs and d_out set.  The output buffer is poisoned first: the records at or beyond the stored count and the bytes behind
the last slab must come back untouched, and so must the sources.  The last tests close the loop on real frames: a surface made of the golden
frames, tiled with overlap, through zly_detect_device_view -> zly_merge_slabs (with and without deferred NMS), zly_detect_tiled and the tracker.
Engines are the suite's smallest (yolov8n at 64 x 64, warmup_runs = 0).
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch            # before the first engine: the process then uses torch's HIP runtime throughout, as tests/test_gpu_parity.py does

import merge_cases as mc
import merge_ref
import track_cases as tc
import track_ref
import view_ref
import yuv_ref
import zly

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "zly_golden_64.npz"))
CONF, IOU_THR = float(G["conf"]), float(G["iou"])
HAND = mc.hand_cases()
EXTRA = 64                          # poisoned bytes behind the last output slab
_ENGINES = {}


@pytest.fixture(scope="module")
def engine_for(weights_path):
    """engines by slab capacity; none of them ever runs a forward pass"""
    def get(cap):
        if cap not in _ENGINES:
            _ENGINES[cap] = zly.Engine(weights_path, model_w=64, model_h=64, max_batch=64, max_dets=cap, warmup_runs=0, use_graph=False)
        return _ENGINES[cap]
    yield get
    for e in _ENGINES.values():
        e.close()
    _ENGINES.clear()


def _ctiles(tiles):
    return [zly.Tile(*t) for t in tiles]


def _merge(e, raw, tiles, n_groups, metric, thr, tag0=mc.TAG0, out=None):
    """one zly_merge_slabs call on device copies -> (the output buffer afterwards, flat; the sources afterwards)"""
    d_src = torch.from_numpy(np.array(raw, dtype=np.uint8)).cuda()
    d_out = torch.from_numpy(mc.poison(n_groups, e.max_dets, EXTRA) if out is None else out).cuda()
    torch.cuda.synchronize()
    e.merge_slabs(_ctiles(tiles), n_groups, metric, float(thr), d_src.data_ptr(), d_out.data_ptr(), tag0)
    e.sync()
    return d_out.cpu().numpy(), d_src.cpu().numpy()


def _check(got_flat, want, what):
    """want: u8 [n_groups][slab_bytes] on a poisoned buffer; got_flat: the whole output buffer, EXTRA bytes behind the slabs"""
    n, sb = want.shape
    got = got_flat[:n * sb].reshape(n, sb)
    if not np.array_equal(got, want):
        g = int(np.flatnonzero((got != want).any(axis=1))[0])
        hg, hw = got[g, :16].view(zly.SLAB_HDR_DTYPE)[0], want[g, :16].view(zly.SLAB_HDR_DTYPE)[0]
        pytest.fail(f"{what}: group {g}: header {hg} want {hw}; bytes differ at {np.flatnonzero(got[g] != want[g])[:8].tolist()}")
    assert (got_flat[n * sb:] == mc.POISON).all(), f"{what}: bytes behind the last slab were written"


@pytest.mark.parametrize("case", HAND, ids=[c.name for c in HAND])
def test_hand_case(engine_for, case):
    e = engine_for(case.cap)
    raw = mc.case_raw(case)
    got, src = _merge(e, raw, case.tiles, case.n_groups, case.metric, case.thr)
    _check(got, mc.hand_expected(case), case.name)
    assert np.array_equal(src, raw), "the sources were modified"


@pytest.mark.parametrize("sc,target", mc.SCENE_PARAMS, ids=mc.SCENE_IDS)
def test_scene(engine_for, sc, target):
    tiles, raw, want = mc.scene(sc, target)
    e = engine_for(sc.cap)
    got, src = _merge(e, raw, tiles, 1, sc.metric, sc.thr)
    _check(got, want, f"{sc.name} M={target}")
    assert np.array_equal(src, raw), "the sources were modified"


def test_default_config_is_ios_at_one_half(engine_for):
    sc = mc.SCENES[2]
    tiles, raw, want = mc.scene(sc, None)
    assert (sc.metric, sc.thr) == (merge_ref.IOS, 0.5)
    e = engine_for(sc.cap)
    d_src, d_out = torch.from_numpy(np.array(raw, dtype=np.uint8)).cuda(), torch.from_numpy(mc.poison(1, sc.cap, EXTRA)).cuda()
    torch.cuda.synchronize()
    e.merge_slabs(_ctiles(tiles), 1, d_slabs_ptr=d_src.data_ptr(), d_out_ptr=d_out.data_ptr(), tag0=mc.TAG0)
    e.sync()
    _check(d_out.cpu().numpy(), want, "defaults")


def test_groups_in_one_call_or_split_over_calls_give_the_same_bytes(engine_for):
    """three scenes of one capacity as three interleaved groups of one call, with two slabs that take no part; then one group per call"""
    picks = [(mc.SCENES[2], None), (mc.SCENES[3], 257), (mc.SCENES[3], 129)]
    cap = 64
    e = engine_for(cap)
    parts = [mc.scene(sc, t) for sc, t in picks]
    assert len({(sc.metric, float(sc.thr)) for sc, _ in picks}) == 1
    metric, thr = picks[0][0].metric, picks[0][0].thr
    slots = []                                                         # (group, index in the group's scene), round robin over the groups
    for k in range(max(len(p[0]) for p in parts)):
        for g, p in enumerate(parts):
            if k < len(p[0]):
                slots.append((g, k))
    slots.insert(3, (-1, 0))
    slots.append((-1, 1))
    raw = np.stack([parts[max(g, 0)][1][k] for g, k in slots])
    tiles = [(g,) + tuple(parts[max(g, 0)][0][k][1:]) for g, k in slots]
    want = np.concatenate([p[2] for p in parts]).copy()
    for g in range(3):
        want[g, :16].view(zly.SLAB_HDR_DTYPE)["frame_tag"] = mc.TAG0 + g
    got, src = _merge(e, raw, tiles, 3, metric, thr)
    _check(got, want, "three groups in one call")
    assert np.array_equal(src, raw)
    # one group per call, into the same buffer: the other groups' slabs take no part
    out = mc.poison(3, cap, EXTRA)
    sb = mc.slab_bytes(cap)
    for g in range(3):
        alone = [((0,) + t[1:]) if t[0] == g else ((-1,) + t[1:]) for t in tiles]
        one, _ = _merge(e, raw, alone, 1, metric, thr, tag0=mc.TAG0 + g)
        _check(one, want[g:g + 1], f"group {g} alone")
        out[g * sb:(g + 1) * sb] = one[:sb]
    assert np.array_equal(out, got)
    # the tiles of a group in two calls of half the tiles each do NOT merge across the calls: the rule is per call, and says so
    half = [t if i < len(tiles) // 2 else ((-1,) + t[1:]) for i, t in enumerate(tiles)]
    part, _ = _merge(e, raw, half, 3, metric, thr)
    before = np.full((3, sb), mc.POISON, dtype=np.uint8)
    _check(part, merge_ref.merge_slabs(raw, half, 3, cap, metric, thr, mc.TAG0, before), "half of the tiles")


def test_engine_owned_buffers_and_read_merged(engine_for):
    """d_out = NULL: the engine-owned merge buffer, read with zly_read_merged; a smaller result later leaves the earlier records beyond its count"""
    sc = mc.SCENES[2]
    tiles, raw, want = mc.scene(sc, None)
    e = engine_for(sc.cap)
    d_src = torch.from_numpy(np.array(raw, dtype=np.uint8)).cuda()
    torch.cuda.synchronize()
    e.merge_slabs(_ctiles(tiles), 1, sc.metric, float(sc.thr), d_src.data_ptr(), 0, mc.TAG0)
    (hdr, dets), = e.read_merged(1)
    whdr = want[0, :16].view(zly.SLAB_HDR_DTYPE)[0]
    k = min(int(whdr["n_kept"]), sc.cap)
    assert hdr == whdr and np.array_equal(dets.view(np.uint8), want[0, 16:16 + 40 * k])
    raw2 = np.zeros(e.slab_bytes * 2, dtype=np.uint8)
    assert e.lib.zly_read_merged(e.h, 2, raw2.ctypes.data) == zly.OK
    first = raw2[:e.slab_bytes].copy()
    small = mc.scene(mc.SCENES[0], 2)                                  # cap 8: another engine; here only its two boxes, rebuilt at this capacity
    src2 = tc.build_slabs([small[1][0, 16:].view(zly.DET_DTYPE)[:2]], sc.cap, tag0=mc.TAG0)
    d2 = torch.from_numpy(src2).cuda()
    torch.cuda.synchronize()
    e.merge_slabs(_ctiles(small[0][:1]), 1, sc.metric, float(sc.thr), d2.data_ptr(), 0, 5)
    raw3 = np.zeros(e.slab_bytes, dtype=np.uint8)
    assert e.lib.zly_read_merged(e.h, 1, raw3.ctypes.data) == zly.OK
    assert np.array_equal(raw3, merge_ref.merge_slabs(src2, small[0][:1], 1, sc.cap, sc.metric, sc.thr, 5, first[None])[0])


def test_errors_leave_the_output_untouched(weights_path, engine_for):
    lib = zly.load_library()
    I, R = zly.ERR_INVALID_ARGUMENT, C.byref
    e = zly.Engine(weights_path, model_w=64, model_h=64, max_batch=4, max_dets=8, warmup_runs=0, use_graph=False)
    case = HAND[0]
    raw = np.concatenate([mc.case_raw(case), mc.case_raw(case)])
    d_src, d_out = torch.from_numpy(raw).cuda(), torch.from_numpy(mc.poison(4, 8, EXTRA)).cuda()
    torch.cuda.synchronize()
    cfg = zly.merge_config()
    A, B = mc.A, mc.B

    def refused(tiles, n_groups=1, c=cfg, n=None, eng=e):
        n = len(tiles) if n is None else n
        ct = (zly.Tile * max(len(tiles), 1))(*_ctiles(tiles)) if tiles is not None else None
        rc = lib.zly_merge_slabs(eng.h, n, ct, n_groups, R(c) if c is not None else None, d_src.data_ptr(), d_out.data_ptr(), 0, None)
        assert rc == I and lib.zly_last_error(), (tiles, n_groups, n)

    assert lib.zly_read_merged(e.h, 1, raw.ctypes.data) == I          # nothing merged yet
    refused([A, B], n=0)
    refused([A, B, A, B, A], n=5)                                      # above max_batch
    refused([A, B], n_groups=0)
    refused([A, B], n_groups=3)
    refused(None, n=2)
    refused([A, mc.grp(B, -2)])
    refused([A, mc.grp(B, 1)])
    refused([A, mc.grp(B, 2)], n_groups=2)
    for bad in ((0, 129, 0, 128, 256, 256, 256), (0, 0, 1, 128, 256, 256, 256), (0, -1, 0, 128, 256, 256, 256), (0, 0, -1, 128, 256, 256, 256),
                (0, 0, 0, 0, 256, 256, 256), (0, 0, 0, 128, 0, 256, 256), (0, 0, 0, 128, -5, 256, 256), (0, 0, 0, 1, 1, 1 << 24, 256), (0, 0, 0, 1, 1, 256, 1 << 24),
                (0, 0, 0, 1, 1, 0, 256), (0, 0x7fffffff, 0, 0x7fffffff, 256, 256, 256)):
        refused([A, bad])
    refused([A, (0, 64, 0, 128, 256, 512, 256)])                       # the tiles of a group disagree on W
    refused([A, (0, 64, 0, 128, 256, 256, 512)])
    refused([A, B], c=None)
    for metric, thr in ((2, .5), (-1, .5), (0, -0.01), (1, 1.0), (1, float("nan")), (0, float("inf"))):
        refused([A, B], c=zly.MergeConfig(metric, thr))
    big = engine_for(1024)                                             # 5 tiles x 1024 > ZLY_MERGE_MAX_CANDIDATES; 4 + one left out is fine
    refused([A] * 5, eng=big)
    assert lib.zly_merge_slabs(None, 2, (zly.Tile * 2)(*_ctiles([A, B])), 1, R(cfg), d_src.data_ptr(), d_out.data_ptr(), 0, None) == zly.ERR_NOT_INITIALIZED
    for bad_n in (0, 5):
        assert lib.zly_read_merged(e.h, bad_n, raw.ctypes.data) == I
    e.sync()
    big.sync()
    assert (d_out.cpu().numpy() == mc.POISON).all() and np.array_equal(d_src.cpu().numpy(), raw)
    # the same arguments, valid: the call works, and a group of different surfaces in DIFFERENT groups is fine
    got, _ = _merge(e, raw, [A, B, mc.grp((0, 0, 0, 64, 64, 64, 64), 1), mc.grp(B, -1)], 2, merge_ref.IOU, .5)
    hdr = got[:16].view(zly.SLAB_HDR_DTYPE)[0]
    assert (int(hdr["n_kept"]), int(hdr["n_candidates"])) == (1, 2)
    e.close()


# ---- real frames ---------------------------------------------------------------------------------------------------------------
SW, SH, TILE, OVERLAP = 128, 96, 40, 16           # 5 x 4 = 20 tiles: above the batch size from which a flagged engine defers its NMS


def _image(variant=0):
    """a 128 x 96 BGR picture made of the golden frames: the two 64 x 64 ones side by side, a strip of the 96 x 80 one below"""
    f = G["frames_64"]
    img = np.zeros((SH, SW, 3), dtype=np.uint8)
    img[:64, :64], img[:64, 64:] = f[variant % 2], f[(variant + 1) % 2]
    img[64:, :96] = G["frame_96x80"][8 * variant:8 * variant + 32]
    img[64:, 96:] = f[0][:32, 16:48]
    return img


def _surfaces(variant=0):
    """(name, buffer, surface view) for the tight BGR surface and a pitched NV12 one"""
    img = _image(variant)
    out = [("bgr", img.reshape(-1).copy(), zly.view_tight(zly.PIX_BGR, SW, SH))]
    buf, v = view_ref.embed(yuv_ref.bgr_to_yuv420(img, zly.PIX_NV12_BT601), zly.PIX_NV12_BT601, SW, SH, [160, 192], 0, 0, 0x55, w=SW, h=SH)
    out.append(("nv12_pitched", buf, view_ref.to_c(v)))
    return out


def _fields_equal(a, b):
    return len(a) == len(b) and all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in ("x", "y", "w", "h", "confidence", "class_id", "track_id"))


@pytest.mark.parametrize("flags", [0, zly.FLAG_ASYNC_NMS], ids=["in_stream_order", "deferred_nms"])
def test_closed_loop_on_real_frames(weights_path, flags):
    cap = 64
    tiles = zly.tile_grid(SW, SH, TILE, TILE, OVERLAP, OVERLAP, even=True)
    ttup = [(t.group, t.x0, t.y0, t.w, t.h, t.W, t.H) for t in tiles]
    n = len(tiles)
    assert n == 20 and ttup == merge_ref.tile_grid(SW, SH, TILE, TILE, OVERLAP, OVERLAP, True)
    e = zly.Engine(weights_path, model_w=64, model_h=64, conf_thr=CONF, iou_thr=IOU_THR, max_batch=32, max_dets=cap, dtype=zly.DTYPE_FP32, warmup_runs=0, flags=flags)
    sb = e.slab_bytes
    for name, buf, surf in _surfaces():
        views = [zly.view_crop(surf, t.x0, t.y0, t.w, t.h) for t in tiles]
        d_buf = torch.from_numpy(buf).cuda()
        d_slabs = torch.zeros(n * sb, dtype=torch.uint8, device="cuda")
        d_out = torch.from_numpy(mc.poison(1, cap, EXTRA)).cuda()
        torch.cuda.synchronize()
        # nothing but enqueues between the detect and the merge
        e.detect_device_view(d_buf.data_ptr(), buf.nbytes, views, d_slabs.data_ptr(), tag0=100)
        e.merge_slabs(tiles, 1, d_slabs_ptr=d_slabs.data_ptr(), d_out_ptr=d_out.data_ptr(), tag0=9)
        e.sync()
        raw = d_slabs.cpu().numpy().reshape(n, sb)
        kept = [int(raw[i, :16].view(zly.SLAB_HDR_DTYPE)["n_kept"][0]) for i in range(n)]
        assert sum(kept) >= 40 and max(kept) <= cap, (name, kept)
        want = merge_ref.merge_slabs(raw, ttup, 1, cap, merge_ref.IOS, 0.5, 9, np.full((1, sb), mc.POISON, dtype=np.uint8))
        _check(d_out.cpu().numpy(), want, f"{name}, flags {flags}")
        whdr = want[0, :16].view(zly.SLAB_HDR_DTYPE)[0]
        assert 0 < int(whdr["n_kept"]) < int(whdr["n_candidates"]) == sum(kept), (name, whdr)
        # the engine's own buffers: sources in its slab buffer, the result in its merge buffer
        e.detect_device_view(d_buf.data_ptr(), buf.nbytes, views, tag0=100)
        e.merge_slabs(tiles, 1, tag0=9)
        (hdr, dets), = e.read_merged(1)
        stored = want[0, 16:].view(zly.DET_DTYPE)[:min(int(whdr["n_kept"]), cap)]
        assert hdr == whdr and _fields_equal(dets, stored), name
        for i, (h, d) in enumerate(e.read_slabs(n)):                  # the engine's source slabs are what the explicit buffer held
            assert h == raw[i, :16].view(zly.SLAB_HDR_DTYPE)[0] and np.array_equal(d.view(np.uint8), raw[i, 16:16 + 40 * kept[i]]), (name, i)
        # the synchronous host entry on the host copy of the surface
        tdets, tn = e.detect_tiled(buf, surf, tiles, cap=cap)
        assert tn == int(whdr["n_kept"]) and _fields_equal(tdets, stored) and (tdets["timestamp"] > 0).all(), name
        few, fn = e.detect_tiled(buf, surf, tiles, cap=3)
        assert fn == tn and _fields_equal(few, stored[:3])
    # refusals of the host entry: nothing comes back
    name, buf, surf = _surfaces()[0]
    lib, out, cnt = e.lib, np.zeros(cap, dtype=zly.DET_DTYPE), C.c_int32(-7)
    cfg = zly.merge_config()
    call = lambda b, nb, s, ts, c=cfg: lib.zly_detect_tiled(e.h, b, nb, C.byref(s), len(ts), (zly.Tile * len(ts))(*ts), C.byref(c) if c is not None else None,
                                                            out.ctypes.data, cap, C.byref(cnt))
    assert call(buf.ctypes.data, buf.nbytes - 1, surf, tiles) == zly.ERR_INVALID_INPUT
    assert call(buf.ctypes.data, buf.nbytes, surf, [zly.tile(0, 0, 40, 40, SW, SH, group=1)]) == zly.ERR_INVALID_ARGUMENT
    assert call(buf.ctypes.data, buf.nbytes, surf, [zly.tile(0, 0, 40, 40, SW + 2, SH)]) == zly.ERR_INVALID_ARGUMENT
    assert call(buf.ctypes.data, buf.nbytes, surf, [zly.tile(100, 0, 40, 40, SW, SH)]) == zly.ERR_INVALID_ARGUMENT
    assert call(buf.ctypes.data, buf.nbytes, surf, tiles, None) == zly.ERR_INVALID_ARGUMENT
    bad = zly.view_tight(zly.PIX_BGR, SW, SH)
    bad.fmt = 9
    assert call(buf.ctypes.data, buf.nbytes, bad, tiles) == zly.ERR_INVALID_ARGUMENT
    assert cnt.value == -7 and not out["confidence"].any()
    e.close()


@pytest.mark.parametrize("flags", [0, zly.FLAG_ASYNC_NMS], ids=["in_stream_order", "deferred_nms"])
def test_tracking_the_merged_slabs_of_three_frames(weights_path, flags):
    """detect -> merge -> track, three surfaces in a row with nothing but enqueues in between: the ids are track_ref's on the merged lists"""
    cap = 64
    tiles = zly.tile_grid(SW, SH, TILE, TILE, OVERLAP, OVERLAP)
    ttup = [(t.group, t.x0, t.y0, t.w, t.h, t.W, t.H) for t in tiles]
    n = len(tiles)
    e = zly.Engine(weights_path, model_w=64, model_h=64, conf_thr=CONF, iou_thr=IOU_THR, max_batch=32, max_dets=cap, dtype=zly.DTYPE_FP32, warmup_runs=0, flags=flags)
    e.track_enable(max_streams=2, max_tracks=64)
    sb = e.slab_bytes
    surf = zly.view_tight(zly.PIX_BGR, SW, SH)
    views = [zly.view_crop(surf, t.x0, t.y0, t.w, t.h) for t in tiles]
    bufs = [torch.from_numpy(_image(v).reshape(-1).copy()).cuda() for v in (0, 0, 1)]
    d_slabs = [torch.zeros(n * sb, dtype=torch.uint8, device="cuda") for _ in range(3)]
    d_out = torch.from_numpy(mc.poison(3, cap, EXTRA)).cuda()
    torch.cuda.synchronize()
    for k in range(3):
        e.detect_device_view(bufs[k].data_ptr(), SW * SH * 3, views, d_slabs[k].data_ptr(), tag0=0)
        e.merge_slabs(tiles, 1, d_slabs_ptr=d_slabs[k].data_ptr(), d_out_ptr=d_out.data_ptr() + k * sb, tag0=k)
        e.track_slabs([1], d_out.data_ptr() + k * sb)
    e.sync()
    trk = track_ref.Tracker(64, cap)
    want = np.full((3, sb), mc.POISON, dtype=np.uint8)
    for k in range(3):
        raw = d_slabs[k].cpu().numpy().reshape(n, sb)
        want[k:k + 1] = merge_ref.merge_slabs(raw, ttup, 1, cap, merge_ref.IOS, 0.5, k, want[k:k + 1])
        hdr = want[k, :16].view(zly.SLAB_HDR_DTYPE)[0]
        ids = trk.step(want[k, 16:].view(zly.DET_DTYPE), int(hdr["n_kept"]))
        assert len(ids) >= 5
        want[k:k + 1] = tc.with_ids(want[k:k + 1], [ids], cap)
    _check(d_out.cpu().numpy(), want, f"three tracked frames, flags {flags}")
    assert e.track_state(1) == trk.state() and trk.counts["matches"] >= 5
    e.close()


def test_an_engine_that_never_merges_computes_what_one_that_merged_does(weights_path):
    frames = [np.ascontiguousarray(G["frames_64"][0]), np.ascontiguousarray(G["frames_64"][1])]
    buf = np.concatenate([f.reshape(-1) for f in frames])
    views = []
    for i, f in enumerate(frames):
        v = zly.view_tight(zly.PIX_BGR, 64, 64)
        v.off[0] = i * f.nbytes
        views.append(v)
    kw = dict(model_w=64, model_h=64, conf_thr=CONF, iou_thr=IOU_THR, max_batch=4, max_dets=64, dtype=zly.DTYPE_FP32, warmup_runs=0)
    d_buf = torch.from_numpy(buf).cuda()
    torch.cuda.synchronize()
    plain, merging = zly.Engine(weights_path, **kw), zly.Engine(weights_path, **kw)
    tiles = [zly.tile(0, 0, 64, 64, 128, 64), zly.tile(64, 0, 64, 64, 128, 64)]
    got = []
    for eng, merges in ((plain, False), (merging, True)):
        rounds = []
        for _ in range(2):
            eng.detect_device_view(d_buf.data_ptr(), buf.nbytes, views, tag0=3)
            rounds.append([(h.copy(), d.copy()) for h, d in eng.read_slabs(2)])
            if merges:
                eng.merge_slabs(tiles, 1)
                (hdr, _), = eng.read_merged(1)
                assert int(hdr["n_candidates"]) == sum(int(h["n_kept"]) for h, _ in rounds[-1])
        got.append(rounds)
    for r in range(2):
        for i in range(2):
            (h0, d0), (h1, d1) = got[0][r][i], got[1][r][i]
            assert h0 == h1 and np.array_equal(d0.view(np.uint8), d1.view(np.uint8)) and int(h0["n_kept"]) >= 3
    plain.close()
    merging.close()
