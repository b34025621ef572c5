"""zoom_plan_kernel (csrc/kernels_zoom.hip) and the two tracking kernels (csrc/kernels_track.hip) on track tables WRITTEN BYTE FOR BYTE by the test, not
grown from a reset: every K in 1..15, fewer than 64 slots, class filters, max_age 0, frame_no around 2^32, NaN and out-of-range predictions, up to 64
frames in one plan launch, all twelve pixel formats with plane offsets above 2^32, sparse tables with holes.  The launches go through
tests/cpp/track_probe.hip, which links the kernels_zoom.o and kernels_track.o of libzly.so itself; results are compared as bytes with the existing
oracles (tests/zoom_ref.py, tests/track_ref.py, tests/track_motion_ref.py), the hand-written expectations of tests/zoom_cases.py and zly.view_crop.
No engine, no weights.

Measured on an MI355X: the module's 26 cases take 1.6 s together (sum of the calls; the process start and imports come on top): slowest
test_seeded_tables_equal_the_oracle 1.05 s (600 launches and 600 oracle plans), test_hand_cases 0.21 s (the first launch of the process),
test_the_wrap_runs_cover_the_tracker 0.14 s (it computes the six oracle runs the wrap tests share), test_many_frames_patch_every_table[40x15] 0.04 s;
every other case 0.01 s or less.
Four one-line mutations of a scratch copy of the plan kernel, each run once: `lane < T` -> `lane < 64` fails test_fewer_slots_than_lanes (4 of 4);
`lane < chosen` -> `lane <= chosen` fails the hand cases, the seeded tables, all four T and both many-frame launches; `b = i * (1 + K) + 1 + lane` ->
`i * K + 1 + lane` and `planes > 2` -> `planes > 1` each fail both many-frame launches.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import track_cases as tc
import track_motion_cases as tmc
import zly
import zoom_cases as zc
import zoom_ref
from track_motion_ref import MotionTracker
from track_ref import Tracker

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE_TARGET = "zero-latency-yolo_amd/_build/libtrack_probe.so"
FILL, GUARD = 0xA7, 256
U32 = 0xFFFFFFFF
F32 = np.float32

# the records of csrc/zly_internal.h and csrc/zoom_device.h; the probe fixture asserts them against the compiler's sizeof / offsetof
_S = 64
TS_DTYPE = np.dtype([("frame_no", "<u4"), ("next_id", "<u4"), ("evictions", "<u4"), ("pad_", "<u4"), ("live", "<u4", _S), ("x", "<f4", _S), ("y", "<f4", _S),
                     ("w", "<f4", _S), ("h", "<f4", _S), ("cls", "<i4", _S), ("id", "<u4", _S), ("last_seen", "<u4", _S)])
TM_DTYPE = np.dtype([("vx", "<f4", _S), ("vy", "<f4", _S), ("hits", "<u4", _S)])
ZF_DTYPE = np.dtype([("off", "<u8", 3), ("pitch", "<i4", 3), ("W", "<i4"), ("H", "<i4"), ("stream", "<i4"), ("fmt", "<i4"), ("planes", "<i4"),
                     ("xstep", "u1", 3), ("xsh", "u1", 3), ("ysh", "u1", 3), ("pad_", "u1", 7)])
DESC_DTYPE = np.dtype([("src_off", "<u8"), ("w", "<i4"), ("h", "<i4")])
VREC_DTYPE = np.dtype([("off1", "<u8"), ("off2", "<u8"), ("pitch0", "<i4"), ("pitch1", "<i4"), ("pitch2", "<i4"), ("pad_", "<i4")])
REGION_DTYPE = zoom_ref.REGION_DTYPE
DESC_FMT_SHIFT = 56
TS_SLOT_FIELDS = ("live", "x", "y", "w", "h", "cls", "id", "last_seen")

FORMATS = (zly.PIX_BGR, zly.PIX_NV12_BT601, zly.PIX_I420_BT601, zly.PIX_NV12_BT709, zly.PIX_I420_BT709, zly.PIX_YUY2_BT601, zly.PIX_UYVY_BT601,
           zly.PIX_YUY2_BT709, zly.PIX_UYVY_BT709, zly.PIX_RGB, zly.PIX_BGRA, zly.PIX_RGBA)
YUV420 = (zly.PIX_NV12_BT601, zly.PIX_I420_BT601, zly.PIX_NV12_BT709, zly.PIX_I420_BT709)
YUV422 = (zly.PIX_YUY2_BT601, zly.PIX_UYVY_BT601, zly.PIX_YUY2_BT709, zly.PIX_UYVY_BT709)


@pytest.fixture(scope="module")
def probe():
    """ctypes handle on the probe; built on demand (after `make` it is there: the target is part of `all`).  The layout check comes first: a record
    that changed fails here instead of shifting fields under every test below"""
    path = os.path.join(ROOT, PROBE_TARGET)
    if not os.path.exists(path):
        subprocess.run(["make", "-C", ROOT, PROBE_TARGET], check=True, stdout=subprocess.DEVNULL)
    lib = C.CDLL(path)
    vp, i = C.c_void_p, C.c_int
    lib.track_probe_layout.argtypes, lib.track_probe_layout.restype = [vp], i
    lib.track_probe_zoom.argtypes = [vp, i, vp, vp, vp, i, i, i, i, i, i, i, vp, vp, vp, vp, vp, vp, i, i]
    lib.track_probe_zoom.restype = i
    lib.track_probe_track.argtypes = [vp, i, vp, vp, i, vp, i, i, i, C.c_float, C.c_uint32, C.c_float, C.c_float, i, i]
    lib.track_probe_track.restype = i
    out = np.full(64, -1, dtype=np.int32)
    n = lib.track_probe_layout(out.ctypes.data)
    of = lambda dt, *names: [dt.fields[k][1] for k in names]
    want = ([TS_DTYPE.itemsize] + of(TS_DTYPE, "frame_no", "next_id", "evictions", *TS_SLOT_FIELDS)
            + [TM_DTYPE.itemsize] + of(TM_DTYPE, "vx", "vy", "hits")
            + [ZF_DTYPE.itemsize] + of(ZF_DTYPE, "off", "pitch", "W", "H", "stream", "fmt", "planes", "xstep", "xsh", "ysh")
            + [REGION_DTYPE.itemsize] + of(REGION_DTYPE, "slot", "track_id")
            + [DESC_DTYPE.itemsize] + of(DESC_DTYPE, "src_off", "w", "h")
            + [VREC_DTYPE.itemsize] + of(VREC_DTYPE, "off1", "off2")
            + [7, _S, 15])
    assert n == len(want) and out[:n].tolist() == want, (out[:n].tolist(), want)
    assert C.sizeof(zly.FrameView) == 56 and REGION_DTYPE == zly.ZOOM_REGION_DTYPE
    return lib


# ---------------------------------------------------------------------------------------------------
# tables as bytes
# ---------------------------------------------------------------------------------------------------
def table_records(t: zoom_ref.Table, next_id=1, evictions=0, hits=None):
    """a zoom_ref.Table (up to 64 slots; the rest stay zero) -> (TrackStream record, TrackMotion record)"""
    ts, tm = np.zeros((), dtype=TS_DTYPE), np.zeros((), dtype=TM_DTYPE)
    ts["frame_no"], ts["next_id"], ts["evictions"] = t.frame_no & U32, next_id, evictions
    for s in range(t.T):
        ts["live"][s] = 1 if t.live[s] else 0
        ts["x"][s], ts["y"][s], ts["w"][s], ts["h"][s] = t.box[s]
        ts["cls"][s], ts["id"][s], ts["last_seen"][s] = t.cls[s], t.id[s], t.last_seen[s]
        tm["vx"][s], tm["vy"][s] = t.vx[s], t.vy[s]
        tm["hits"][s] = 0 if hits is None else hits[s]
    return ts, tm


def tracker_records(trk):
    """the state of a Tracker / MotionTracker -> (TrackStream record, TrackMotion record), slots >= trk.T zero"""
    return table_records(zoom_ref.table_of(trk), trk.next_id, trk.evictions, getattr(trk, "hits", None))


def load_tracker(trk, ts, tm=None):
    """mirrors slots [0, trk.T) and the header of a TrackStream record (and of a TrackMotion record) into an oracle tracker"""
    trk.frame_no, trk.next_id, trk.evictions = int(ts["frame_no"]), int(ts["next_id"]), int(ts["evictions"])
    for s in range(trk.T):
        trk.live[s] = bool(ts["live"][s])
        trk.box[s] = (F32(ts["x"][s]), F32(ts["y"][s]), F32(ts["w"][s]), F32(ts["h"][s]))
        trk.cls[s], trk.id[s], trk.last_seen[s] = int(ts["cls"][s]), int(ts["id"][s]), int(ts["last_seen"][s])
        if tm is not None:
            trk.vx[s], trk.vy[s], trk.hits[s] = F32(tm["vx"][s]), F32(tm["vy"][s]), int(tm["hits"][s])
    return trk


def _stack(records, dtype):
    out = np.zeros(len(records), dtype=dtype)
    for i, r in enumerate(records):
        out[i] = r
    return out


def _guarded(payload: np.ndarray) -> np.ndarray:
    """payload bytes + GUARD bytes (the host side of the guard is never uploaded; 0x11 so that a guard that did not come back shows)"""
    b = np.frombuffer(payload.tobytes(), dtype=np.uint8)
    return np.concatenate([b, np.full(GUARD, 0x11, dtype=np.uint8)])


def _guard_ok(buf: np.ndarray, nbytes: int) -> bool:
    return len(buf) == nbytes + GUARD and bool((buf[nbytes:] == FILL).all())


def _hip_error(what, rc):
    # a HIP error may be a GPU fault: nothing more is started on that device
    pytest.exit(f"{what}: HIP error {rc}", returncode=3)


# ---------------------------------------------------------------------------------------------------
# the zoom plan kernel
# ---------------------------------------------------------------------------------------------------
def zoom_launch(probe, states, motion, views, streams, cfg, T, desc=None, tab=None):
    """one launch.  states: TS_DTYPE array; motion: TM_DTYPE array or None; views: FrameView list; desc / tab: u8 / i4 arrays (copied) or None
    -> dict(rc, plan REGION_DTYPE [n][K], desc u8, tab i4, frames ZF_DTYPE [n]); the guards and the untouched tables are asserted here"""
    n, K = len(views), cfg.regions
    states = np.ascontiguousarray(states, dtype=TS_DTYPE).reshape(-1)
    cv = (zly.FrameView * n)(*views)
    cs = np.ascontiguousarray(streams, dtype=np.int32)
    plan_bytes = n * K * REGION_DTYPE.itemsize
    plan = np.full(plan_bytes + GUARD, 0x11, dtype=np.uint8)
    st_out = np.full(states.nbytes + GUARD, 0x11, dtype=np.uint8)
    fr_out = np.full(n * ZF_DTYPE.itemsize + GUARD, 0x11, dtype=np.uint8)
    mo = mo_out = None
    if motion is not None:
        mo = np.ascontiguousarray(motion, dtype=TM_DTYPE).reshape(-1)
        assert len(mo) == len(states)
        mo_out = np.full(mo.nbytes + GUARD, 0x11, dtype=np.uint8)
    d_io = None if desc is None else _guarded(np.ascontiguousarray(desc, dtype=np.uint8))
    t_io = None if tab is None else _guarded(np.ascontiguousarray(tab, dtype=np.int32))
    ptr = lambda a: None if a is None else a.ctypes.data
    rc = probe.track_probe_zoom(ptr(states), len(states), ptr(mo), C.cast(cv, C.c_void_p), ptr(cs), n, K, T, cfg.region_w, cfg.region_h, cfg.max_age, cfg.class_id,
                                ptr(d_io), ptr(t_io), ptr(plan), ptr(st_out), ptr(mo_out), ptr(fr_out), FILL, GUARD)
    if rc > 0:
        _hip_error("track_probe_zoom", rc)
    if rc != 0:
        return dict(rc=rc)
    assert _guard_ok(plan, plan_bytes), "the guard behind the plan was written"
    assert _guard_ok(st_out, states.nbytes) and st_out[:states.nbytes].tobytes() == states.tobytes(), "the plan kernel changed a track table"
    assert _guard_ok(fr_out, n * ZF_DTYPE.itemsize), "the guard behind the frame records was written"
    if mo is not None:
        assert _guard_ok(mo_out, mo.nbytes) and mo_out[:mo.nbytes].tobytes() == mo.tobytes(), "the plan kernel changed the motion state"
    out = dict(rc=0, plan=plan[:plan_bytes].view(REGION_DTYPE).reshape(n, K), frames=fr_out[:n * ZF_DTYPE.itemsize].view(ZF_DTYPE))
    if d_io is not None:
        assert _guard_ok(d_io, len(d_io) - GUARD), "the guard behind the descriptor block was written"
        out["desc"] = d_io[:-GUARD]
    if t_io is not None:
        assert _guard_ok(t_io, len(t_io) - GUARD), "the guard behind the merge table was written"
        out["tab"] = t_io[:-GUARD].view(np.int32)
    return out


def _plan_of_table(probe, t, cfg, W, H, T=64, with_motion=True):
    ts, tm = table_records(t)
    r = zoom_launch(probe, ts, tm if with_motion else None, [zly.view_tight(zly.PIX_BGR, W, H)], [0], cfg, T)
    assert r["rc"] == 0, (r, cfg, W, H)
    return r["plan"][0]


def test_hand_cases(probe):
    """(a) all 21 hand cases with their own config, surface and table, velocities in a TrackMotion: the hand-written regions and the oracle's"""
    cases = zc.hand_cases()
    assert len(cases) == 21
    configs = set()
    for name, t, cfg, W, H, expected in cases:
        got = _plan_of_table(probe, t, cfg, W, H)
        rw, rh, _, _ = zoom_ref.size(cfg, W, H)
        want = [(x0, y0, rw, rh, slot, t.id[slot] if slot >= 0 else 0) for x0, y0, slot in expected]
        assert [tuple(int(v) for v in r) for r in got] == want, (name, got, want)
        assert got.tobytes() == zoom_ref.plan(t, cfg, W, H).tobytes(), name
        configs.add((cfg.region_w, cfg.class_id))
    assert len(configs) >= 3                               # the cases the engine test cannot reach for their config are among them
    # the case that tells a rounded product from an fma, as a table
    fused = next(c for c in cases if c[0] == "product-rounded-first")
    assert int(_plan_of_table(probe, *fused[1:5])[0]["x0"]) == zc.FUSED_X0 != zc.FUSED_X0_IF_FUSED


N_SEEDED = 600


def test_seeded_tables_equal_the_oracle(probe):
    """(b) the first 600 tables of random_case(default_rng(2024)), one launch per table; the conditions below are on the oracle's output alone"""
    rng = np.random.default_rng(2024)
    per_k = np.zeros(16, dtype=int)
    n_follow = n_covered = n_full15 = n_k1_fallback = n_class = n_age0 = n_clipped = 0
    for i in range(N_SEEDED):
        t, cfg, W, H = zc.random_case(rng)
        want, covered = zoom_ref.plan(t, cfg, W, H, with_covered=True)
        got = _plan_of_table(probe, t, cfg, W, H)
        assert got.tobytes() == want.tobytes(), (i, cfg, W, H, t.frame_no, got, want)
        rw, rh, _, _ = zoom_ref.size(cfg, W, H)
        per_k[cfg.regions] += 1
        n_follow += int((want["slot"] >= 0).sum())
        n_covered += len(covered)
        n_full15 += cfg.regions == 15 and bool((want["slot"] >= 0).all())
        n_k1_fallback += cfg.regions == 1 and int(want["slot"][0]) < 0
        n_class += cfg.class_id != -1
        n_age0 += cfg.max_age == 0
        n_clipped += rw < cfg.region_w or rh < cfg.region_h
    print("seeded tables:", dict(per_k=per_k[1:].tolist(), follow=n_follow, covered=n_covered, full15=n_full15, k1_fallback=n_k1_fallback,
                                 class_filter=n_class, max_age_0=n_age0, clipped=n_clipped))
    assert (per_k[1:] >= 1).all(), per_k
    assert n_follow >= 2000 and n_covered >= 500, (n_follow, n_covered)
    assert n_full15 >= 1 and n_k1_fallback >= 1, (n_full15, n_k1_fallback)
    assert n_class >= 100 and n_age0 >= 100 and n_clipped >= 100, (n_class, n_age0, n_clipped)


def _table_with_decoys(T):
    """64 slots on a 640 x 480 surface, F = 9: slots < T of age 1 and 0.1 x 0.1, slots >= T of age 0 and 0.01 x 0.01 -- first in the order if they counted"""
    t = zoom_ref.Table(frame_no=9)
    for s in range(64):
        if s < T:
            t.add(0.08 + 0.84 * ((s * 7) % 32) / 32, 0.1 + 0.8 * ((s * 5) % 16) / 16, 0.1, 0.1, cls=s % 3, id=500 + s, last_seen=8, vx=0.002 * (s % 5 - 2))
        else:
            t.add(0.05 + 0.9 * ((s * 11) % 64) / 64, 0.05 + 0.9 * ((s * 3) % 64) / 64, 0.01, 0.01, cls=s % 3, id=900 + s, last_seen=9)
    return t


@pytest.mark.parametrize("T", [1, 2, 31, 63])
def test_fewer_slots_than_lanes(probe, T):
    """(c) a launch with T < 64 plans from the first T slots only"""
    t = _table_with_decoys(T)
    first = zoom_ref.Table(frame_no=t.frame_no, live=t.live[:T], box=t.box[:T], cls=t.cls[:T], id=t.id[:T], last_seen=t.last_seen[:T], vx=t.vx[:T], vy=t.vy[:T])
    for cfg in (zc.CFG0, zoom_ref.Config(regions=15, region_w=64, region_h=48, max_age=1, class_id=-1)):
        want, all64 = zoom_ref.plan(first, cfg, 640, 480), zoom_ref.plan(t, cfg, 640, 480)
        assert want.tobytes() != all64.tobytes()            # the slots beyond T would change the plan: the test can fail
        assert (want["slot"] >= 0).any()
        got = _plan_of_table(probe, t, cfg, 640, 480, T=T)
        assert got.tobytes() == want.tobytes(), (T, cfg, got, want)
    assert _plan_of_table(probe, t, zc.CFG0, 640, 480, T=64).tobytes() == zoom_ref.plan(t, zc.CFG0, 640, 480).tobytes()


def _planes(fmt):
    v = zly.view_tight(fmt, 4, 4)
    return sum(1 for p in range(3) if v.pitch[p] > 0)


def _frame_views(n):
    """n surfaces, each of its own size, over all twelve formats: pitched, every plane at an offset above 2^32"""
    fixed = [(2, 2), (641, 479), (3, 2), (101, 77), (1203, 481), (209, 161), (208, 160), (2, 1199), (1999, 3)]
    views, seen = [], set()
    for i in range(n):
        fmt = FORMATS[i % len(FORMATS)]
        W, H = fixed[i // 2] if i % 2 == 0 and i // 2 < len(fixed) else (5 + (i * 197) % 1990, 5 + (i * 89) % 1190)
        if fmt in YUV420:
            W, H = max(W & ~1, 2), max(H & ~1, 2)
        elif fmt in YUV422:
            W = max(W & ~1, 2)
        while (W, H) in seen:
            H += 2
        seen.add((W, H))
        v = zly.view_tight(fmt, W, H)
        for p in range(_planes(fmt)):
            v.pitch[p] += 2 * ((i + p) % 9)
            v.off[p] = ((3 + 4 * p + i % 5) << 32) + 4096 * i + 2 * p + 1
        views.append(v)
    return views


def _stream_tables():
    """six streams: seeded tables with frame_no before and after the wrap, and one empty stream (index 2)"""
    rng = np.random.default_rng(31)
    tables = [zc.random_case(rng)[0] for _ in range(6)]
    tables[2] = zoom_ref.Table(frame_no=0xFFFFFFFF)
    for _ in range(64):
        tables[2].add(0, 0, 0, 0, live=False, id=0)
    return tables


@pytest.mark.parametrize("n,cfg", [(40, zoom_ref.Config(regions=15, region_w=208, region_h=160, max_age=3, class_id=-1)),
                                   (64, zoom_ref.Config(regions=1, region_w=416, region_h=416, max_age=2, class_id=1))], ids=["40x15", "64x1"])
def test_many_frames_patch_every_table(probe, n, cfg):
    """(d) one launch of n frames: the plan, and exactly the bytes of the descriptor block and the merge table that depend on an origin"""
    K = cfg.regions
    views, tables = _frame_views(n), _stream_tables()
    streams = [(5 * i + i // 6) % 6 for i in range(n)]
    assert set(streams) == set(range(6)) and len(streams) > len(set(streams)) and 2 in streams
    assert {v.fmt for v in views} == set(FORMATS) and (2, 2) in {(v.w, v.h) for v in views} and any(v.w & 1 and v.h & 1 for v in views)
    assert all(int(v.off[p]) > 1 << 32 for v in views for p in range(_planes(v.fmt)))
    recs = [table_records(t) for t in tables]
    states, motion = _stack([r[0] for r in recs], TS_DTYPE), _stack([r[1] for r in recs], TM_DTYPE)
    want = np.array([zoom_ref.plan(tables[s], cfg, v.w, v.h) for v, s in zip(views, streams)], dtype=REGION_DTYPE)
    assert (want["slot"] >= 0).sum() >= n // 2 and (want["slot"] < 0).any()

    nb = n * (1 + K)
    rng = np.random.default_rng(n)
    desc0 = rng.integers(1, 256, nb * (DESC_DTYPE.itemsize + VREC_DTYPE.itemsize), dtype=np.uint8)          # no zero byte: a field written with 0 shows
    tab0 = rng.integers(1, 1 << 30, n + 1 + nb * 7).astype(np.int32)
    r = zoom_launch(probe, states, motion, views, streams, cfg, 64, desc=desc0, tab=tab0)
    assert r["rc"] == 0
    assert r["plan"].tobytes() == want.tobytes(), [(i, r["plan"][i], want[i]) for i in range(n) if r["plan"][i].tobytes() != want[i].tobytes()][:2]
    for i, (v, s) in enumerate(zip(views, streams)):        # the record the engine makes: zoom_frame_of
        f = r["frames"][i]
        assert (int(f["W"]), int(f["H"]), int(f["stream"]), int(f["fmt"]), int(f["planes"])) == (v.w, v.h, s, v.fmt, _planes(v.fmt))

    desc_want, tab_want = desc0.copy(), tab0.copy()
    d = desc_want[:nb * DESC_DTYPE.itemsize].view(DESC_DTYPE)
    vr = desc_want[nb * DESC_DTYPE.itemsize:].view(VREC_DTYPE)
    for i, v in enumerate(views):
        for j in range(K):
            b, reg = i * (1 + K) + 1 + j, want[i][j]
            crop = zly.view_crop(v, int(reg["x0"]), int(reg["y0"]), int(reg["w"]), int(reg["h"]))
            d[b]["src_off"] = int(crop.off[0]) | (v.fmt << DESC_FMT_SHIFT)
            if _planes(v.fmt) > 1:
                vr[b]["off1"] = int(crop.off[1])
            if _planes(v.fmt) > 2:
                vr[b]["off2"] = int(crop.off[2])
            tab_want[n + 1 + 7 * b + 1], tab_want[n + 1 + 7 * b + 2] = int(reg["x0"]), int(reg["y0"])
    diff = np.flatnonzero(r["desc"] != desc_want)
    assert diff.size == 0, f"descriptor block: {diff.size} bytes differ, first at {diff[:4]} (descriptors end at {nb * 16}, 16 + 32 bytes per item, {1 + K} items per frame)"
    diff = np.flatnonzero(r["tab"] != tab_want)
    assert diff.size == 0, f"merge table: {diff.size} ints differ, first at {diff[:4]} (members begin at {n + 1}, 7 ints each)"
    assert (r["desc"] != desc0).sum() > 0 and (r["tab"] != tab0).sum() >= n        # and the launch did patch

    plain = zoom_launch(probe, states, motion, views, streams, cfg, 64)
    assert plain["rc"] == 0 and plain["plan"].tobytes() == want.tobytes()           # null desc and tab: the same plan
    # without velocities: a null pointer and a TrackMotion of zeros give the same bytes, the oracle's for vx = vy = 0
    still = []
    for t in tables:
        still.append(zoom_ref.Table(frame_no=t.frame_no, live=t.live, box=t.box, cls=t.cls, id=t.id, last_seen=t.last_seen, vx=[F32(0)] * t.T, vy=[F32(0)] * t.T))
    want0 = np.array([zoom_ref.plan(still[s], cfg, v.w, v.h) for v, s in zip(views, streams)], dtype=REGION_DTYPE)
    null = zoom_launch(probe, states, None, views, streams, cfg, 64, desc=desc0, tab=tab0)
    zero = zoom_launch(probe, states, np.zeros(len(states), dtype=TM_DTYPE), views, streams, cfg, 64, desc=desc0, tab=tab0)
    assert null["rc"] == 0 and zero["rc"] == 0
    assert null["plan"].tobytes() == zero["plan"].tobytes() == want0.tobytes() and want0.tobytes() != want.tobytes()
    assert null["desc"].tobytes() == zero["desc"].tobytes() and null["tab"].tobytes() == zero["tab"].tobytes()


def test_probe_refuses_what_the_kernels_must_not_see(probe):
    ts, _ = table_records(zc.hand_cases()[1][1])
    v = [zly.view_tight(zly.PIX_BGR, 640, 480)]
    cfg = lambda **k: zoom_ref.Config(**{**dict(regions=3, region_w=208, region_h=208, max_age=2, class_id=-1), **k})
    assert zoom_launch(probe, ts, None, v, [0], cfg(), 64)["rc"] == 0
    assert zoom_launch(probe, ts, None, v, [0], cfg(regions=0), 64)["rc"] == -1
    assert zoom_launch(probe, ts, None, v, [0], cfg(regions=16), 64)["rc"] == -1
    assert zoom_launch(probe, ts, None, v, [0], cfg(region_w=207), 64)["rc"] == -1
    assert zoom_launch(probe, ts, None, v, [0], cfg(), 0)["rc"] == -1
    assert zoom_launch(probe, ts, None, v, [0], cfg(), 65)["rc"] == -1
    assert zoom_launch(probe, ts, None, v, [1], cfg(), 64)["rc"] == -1               # a stream outside the array
    assert zoom_launch(probe, ts, None, v, [-1], cfg(), 64)["rc"] == -1
    bad = zly.view_tight(zly.PIX_BGR, 640, 480)
    bad.fmt = 9
    assert zoom_launch(probe, ts, None, [bad], [0], cfg(), 64)["rc"] == -1
    assert probe.track_probe_zoom(None, 1, None, None, None, 1, 3, 64, 208, 208, 2, -1, None, None, None, None, None, None, FILL, GUARD) == -1
    st = _guarded(np.zeros(1, dtype=TS_DTYPE))
    slabs = _guarded(tc.build_slabs([tc.dets([(.5, .5, .2, .2)])], 8))
    run = lambda grp, cap=8, T=8, n_slabs=1: probe.track_probe_track(st.ctypes.data, 1, None, np.array(grp, dtype=np.int32).ctypes.data, len(grp), slabs.ctypes.data,
                                                                      n_slabs, cap, T, 0.3, 2, 0.5, 0.25, FILL, GUARD)
    assert run([1, 0, 1, 0, 0], cap=65, T=64) == -1                                  # cap > 64
    assert run([1, 0, 1, 0, 0], cap=8, T=4) == -1                                    # cap > T
    assert run([1, 0, 1, 0, 0], T=65) == -1
    assert run([1, 0, 1, 1, 0]) == -1                                                # a stream outside the array
    assert run([1, 0, 1, 0, 1]) == -1                                                # a slab outside the buffer
    assert run([2, 0, 1, 2, 0, 0, 0, 0]) == -1                                       # more segments than streams
    assert probe.track_probe_track(None, 1, None, None, 5, None, 1, 8, 8, 0.3, 2, 0.5, 0.25, FILL, GUARD) == -1


# ---------------------------------------------------------------------------------------------------
# the tracking kernels
# ---------------------------------------------------------------------------------------------------
def track_launch(probe, states, motion, grp, slabs, cap, T, match_iou, max_lost, beta=0.5, v_max=0.25):
    """one launch, in place: states (TS_DTYPE array), motion (TM_DTYPE array or None) and slabs (u8 [n][slab_bytes]) are overwritten with the result"""
    st = _guarded(states)
    mo = None if motion is None else _guarded(motion)
    sl = _guarded(slabs)
    g = np.ascontiguousarray(grp, dtype=np.int32)
    rc = probe.track_probe_track(st.ctypes.data, len(states), None if mo is None else mo.ctypes.data, g.ctypes.data, len(g), sl.ctypes.data, len(slabs), cap, T,
                                 float(match_iou), int(max_lost), float(beta), float(v_max), FILL, GUARD)
    if rc > 0:
        _hip_error("track_probe_track", rc)
    assert rc == 0, rc
    assert _guard_ok(st, states.nbytes) and _guard_ok(sl, slabs.nbytes) and (mo is None or _guard_ok(mo, motion.nbytes)), "a guard was written"
    states[...] = st[:states.nbytes].view(TS_DTYPE).reshape(states.shape)
    slabs[...] = sl[:slabs.nbytes].reshape(slabs.shape)
    if motion is not None:
        motion[...] = mo[:motion.nbytes].view(TM_DTYPE).reshape(motion.shape)


def _grp(stream_frames):
    """stream_frames: [(stream index, [slab indices])] in the order of the streams' first occurrence -> the call's table (csrc/zly_internal.h)"""
    S = len(stream_frames)
    offs, frames = [0], []
    for _, fs in stream_frames:
        frames += list(fs)
        offs.append(len(frames))
    return [S] + offs + [s for s, _ in stream_frames] + frames


def _expected_records(trk, ts0, tm0):
    """what the kernels must leave of a stream whose table began as (ts0, tm0) and whose oracle is trk: the oracle's state in slots < T and the
    header; in slots >= T the bytes they had, but live = 0 (the kernels store `lane < T && live`, and every other field as they loaded it)"""
    ts, tm = tracker_records(trk)
    ts["pad_"] = ts0["pad_"]
    for k in TS_SLOT_FIELDS:
        ts[k][trk.T:] = 0 if k == "live" else ts0[k][trk.T:]
    for k in ("vx", "vy", "hits"):
        tm[k][trk.T:] = tm0[k][trk.T:]
    return ts, tm


WRAP_START = 0xFFFFFFFD            # frame_no = 2^32 - 3: the third frame is frame 0
WRAP_FRAMES = 10
WRAP_PLAIN = ("walks_T8_lost2", "crowd_T8_lost6", "full_T64_cap64")
WRAP_MOTION = ("moving_T8_5", "moving_T64_60", "moving_T8_5_vmax_small")


def _wrap_start(T, first_frame, max_lost, salt):
    """a table before the wrap: slots 1, 3, 4 hold the first frame's first detections, last seen 1, 2 and max_lost frames ago (a match, a
    re-acquisition, a match at the last moment); slot 6 a box that nothing matches, one frame from expiry; next_id close to its own wrap.
    With T = 64 slots 8..62 are live too, seen 1..4 frames ago: the first births evict"""
    ts, tm = np.zeros((), dtype=TS_DTYPE), np.zeros((), dtype=TM_DTYPE)
    ts["frame_no"], ts["next_id"], ts["evictions"] = WRAP_START, 0xFFFFFFFA, 5 + salt
    ages = (1, 2, max(max_lost, 1))
    for k, slot in enumerate((1, 3, 4)):
        if k < len(first_frame):
            d = first_frame[k]
            ts["live"][slot], ts["cls"][slot], ts["id"][slot] = 1, d["class_id"], 7000 + slot
            ts["x"][slot], ts["y"][slot], ts["w"][slot], ts["h"][slot] = d["x"], d["y"], d["w"], d["h"]
            ts["last_seen"][slot] = (WRAP_START - ages[k]) & U32
            tm["hits"][slot] = 1 + k
    ts["live"][6], ts["cls"][6], ts["id"][6], ts["last_seen"][6] = 1, 77, 7006, (WRAP_START - max_lost) & U32
    ts["x"][6], ts["y"][6], ts["w"][6], ts["h"][6] = 0.02, 0.02, 0.01, 0.01
    tm["hits"][6] = 3
    if T == 64:
        for slot in range(8, 63):
            ts["live"][slot], ts["cls"][slot], ts["id"][slot], ts["last_seen"][slot] = 1, 90 + slot % 2, 8000 + slot, (WRAP_START - 1 - (slot * 7) % 4) & U32
            ts["x"][slot], ts["y"][slot], ts["w"][slot], ts["h"][slot] = 0.01 * slot, 0.97, 0.005, 0.005
            tm["hits"][slot] = 2
    return ts, tm


def _wrap_runs():
    """[(scene, motion?, frames[stream][k], start records per stream, oracle trackers after the frames, ids[stream][k])], computed once"""
    if not _WRAP_CACHE:
        for names, scenes, with_motion in ((WRAP_PLAIN, tc.SCENES, False), (WRAP_MOTION, tmc.SCENES, True)):
            for name in names:
                sc = next(s for s in scenes if s.name == name)
                all_frames = tc.scene_frames(sc) if not with_motion else tmc.scene_frames(sc)[0]
                n_streams = min(2, sc.n_streams)
                frames = [all_frames[s][:WRAP_FRAMES] for s in range(n_streams)]
                starts, trks, ids = [], [], []
                for s in range(n_streams):
                    ts, tm = _wrap_start(sc.T, frames[s][0], sc.max_lost, s)
                    trk = (MotionTracker(sc.T, sc.cap, sc.match_iou, sc.max_lost, sc.beta, sc.v_max) if with_motion else Tracker(sc.T, sc.cap, sc.match_iou, sc.max_lost))
                    load_tracker(trk, ts, tm if with_motion else None)
                    starts.append((ts, tm))
                    ids.append([trk.step(f) for f in frames[s]])
                    trks.append(trk)
                _WRAP_CACHE.append((sc, with_motion, frames, starts, trks, ids))
    return _WRAP_CACHE


_WRAP_CACHE = []


def test_the_wrap_runs_cover_the_tracker():
    """(e) the oracle's counts over the six runs: matches, expiries, evictions and re-acquisitions all occur, before and behind frame 0"""
    runs = _wrap_runs()
    assert WRAP_FRAMES >= 8
    tot = dict(matches=0, births=0, expiries=0, evictions=0, reacquisitions=0)
    for sc, _, frames, _, trks, _ in runs:
        assert len(frames[0]) == WRAP_FRAMES
        for t in trks:
            assert t.frame_no == WRAP_FRAMES - 3                                       # the wrap fell inside the run
            for k in tot:
                tot[k] += t.counts[k]
    print("wrap runs:", tot)
    assert all(v >= 1 for v in tot.values()), tot
    for with_motion in (False, True):                      # and each kernel sees each of them
        sub = {k: sum(t.counts[k] for _, m, _, _, trks, _ in runs if m == with_motion for t in trks) for k in tot}
        assert all(v >= 1 for v in sub.values()), (with_motion, sub)
    assert any(int(i) == 1 for _, _, _, _, _, ids in runs for per in ids for f in per for i in f)      # next_id wrapped too: 0xFFFFFFFF, then 1


@pytest.mark.parametrize("per_frame", [False, True], ids=["one_launch", "launch_per_frame"])
@pytest.mark.parametrize("run", range(6), ids=list(WRAP_PLAIN + WRAP_MOTION))
def test_tracking_across_the_wrap(probe, run, per_frame):
    """(e) from a written table at frame_no = 2^32 - 3 over ten frames, two streams: ids in the slabs, the whole tables, next_id, the motion state"""
    sc, with_motion, frames, starts, trks, ids = _wrap_runs()[run]
    S, n = len(frames), WRAP_FRAMES
    where = [2, 0][:S]                                      # the streams' indices in the state array; index 1 belongs to nobody
    states = np.zeros(3, dtype=TS_DTYPE)
    motion = np.zeros(3, dtype=TM_DTYPE)
    states["frame_no"][1], states["live"][1], motion["hits"][1] = 123, 1, 9
    for s in range(S):
        states[where[s]], motion[where[s]] = starts[s]
    states0, motion0 = states.copy(), motion.copy()
    order = [(k, s) for k in range(n) for s in range(S)]    # slab k * S + s: frame k of stream s
    raw = tc.build_slabs([frames[s][k] for k, s in order], sc.cap)
    slabs = raw.copy()
    kw = dict(beta=sc.beta, v_max=sc.v_max) if with_motion else {}
    mo = motion if with_motion else None
    if per_frame:
        for k, s in order:
            track_launch(probe, states, mo, _grp([(where[s], [k * S + s])]), slabs, sc.cap, sc.T, sc.match_iou, sc.max_lost, **kw)
    else:
        track_launch(probe, states, mo, _grp([(where[s], [k * S + s for k in range(n)]) for s in range(S)]), slabs, sc.cap, sc.T, sc.match_iou, sc.max_lost, **kw)
    want = tc.with_ids(raw, [ids[s][k] for k, s in order], sc.cap)
    for i, (k, s) in enumerate(order):
        assert np.array_equal(slabs[i], want[i]), (sc.name, "frame", k, "stream", s, tc.slab_ids(slabs[i], sc.cap), ids[s][k])
    for s in range(S):
        ts, tm = _expected_records(trks[s], *starts[s])
        got = states[where[s]]
        assert (int(got["frame_no"]), int(got["next_id"]), int(got["evictions"])) == (n - 3, trks[s].next_id, trks[s].evictions), (sc.name, s)
        for k in TS_SLOT_FIELDS:
            assert got[k].tobytes() == ts[k].tobytes(), (sc.name, s, k, got[k], ts[k])
        assert got.tobytes() == ts.tobytes()
        if with_motion:
            assert motion[where[s]].tobytes() == tm.tobytes(), (sc.name, s, motion[where[s]], tm)
    assert states[1].tobytes() == states0[1].tobytes() and motion[1].tobytes() == motion0[1].tobytes()      # nobody's table
    if not with_motion:
        assert motion.tobytes() == motion0.tobytes()


def _sparse_start(T):
    """holes and a last_seen that does not follow the slot order, F = 40; slots >= T hold live-looking non-zero bytes"""
    ts, tm = np.zeros((), dtype=TS_DTYPE), np.zeros((), dtype=TM_DTYPE)
    ts["frame_no"], ts["next_id"], ts["evictions"], ts["pad_"] = 40, 300, 2, 0x5EED
    free = {0, 2, 5} if T == 8 else {1, 4, 9, 17, 30, 32}
    for s in range(64):
        ts["x"][s], ts["y"][s], ts["w"][s], ts["h"][s] = (s % 8 + 0.5) / 8, (s // 8 + 0.5) / 8, 0.0625, 0.0625
        ts["cls"][s], ts["id"][s], ts["last_seen"][s] = 0, 100 + s, 40 - (s * 5) % 4          # ages 0..3 in the pattern 0 3 2 1 by slot
        ts["live"][s] = 0 if s in free else 1
        tm["vx"][s], tm["vy"][s], tm["hits"][s] = 0.001 * (s % 3), -0.001 * (s % 2), 2 + s % 3
        if s >= T:
            ts["live"][s], ts["last_seen"][s], ts["cls"][s] = 0xFFFFFFFF if s % 2 else 1, 0, 1      # the oldest of all, and of the births' class
    return ts, tm, sorted(free)


@pytest.mark.parametrize("with_motion", [False, True], ids=["plain", "motion"])
@pytest.mark.parametrize("T", [8, 33])
def test_sparse_tables_and_fewer_slots(probe, T, with_motion):
    """(f) births fill the holes in ascending order, then evict by (last_seen, slot); nothing at or beyond slot T is matched or born into.  What the
    kernels leave there: live = 0, every other field as it was (csrc/zly_internal.h, TrackStream)"""
    ts0, tm0, free = _sparse_start(T)
    cap, max_lost = T, 6
    # frame 1: boxes of class 1 that sit exactly on slots >= T (a match if those counted) and, for T = 8, on nothing else; more of them than holes
    n_new = len(free) + 3
    beyond = [s for s in range(T, 64)][:n_new]
    f1 = tc.dets([(float(ts0["x"][s]), float(ts0["y"][s]), 0.0625, 0.0625) for s in beyond], [1] * n_new)
    # frame 2: the same boxes again (they match their new slots) and the boxes of two old slots that survived (matches of class 0)
    evictable = sorted((s for s in range(T) if s not in free), key=lambda s: (int(ts0["last_seen"][s]), s))
    victims, kept = evictable[:3], evictable[3:5]
    f2 = tc.dets([(float(ts0["x"][s]), float(ts0["y"][s]), 0.0625, 0.0625) for s in beyond + kept], [1] * n_new + [0] * len(kept))
    frames = [f1, f2]
    trk = MotionTracker(T, cap, 0.3, max_lost) if with_motion else Tracker(T, cap, 0.3, max_lost)
    load_tracker(trk, ts0, tm0 if with_motion else None)
    ids = [trk.step(f) for f in frames]
    # the rule, by hand: ids 300.. go to the holes in ascending order, then to the victims in (last_seen, slot) order; frame 2 matches them all
    assert ids[0].tolist() == list(range(300, 300 + n_new)) and ids[1].tolist() == ids[0].tolist() + [100 + s for s in kept]
    assert [trk.id[s] for s in free + victims] == ids[0].tolist() and trk.evictions == 2 + 3 and trk.counts["matches"] == n_new + 2

    states, motion = _stack([ts0], TS_DTYPE), _stack([tm0], TM_DTYPE)
    raw = tc.build_slabs(frames, cap)
    slabs = raw.copy()
    track_launch(probe, states, motion if with_motion else None, _grp([(0, [0, 1])]), slabs, cap, T, 0.3, max_lost)
    assert np.array_equal(slabs, tc.with_ids(raw, ids, cap)), [tc.slab_ids(s, cap) for s in slabs]
    ts, tm = _expected_records(trk, ts0, tm0)
    got = states[0]
    for k in TS_SLOT_FIELDS:
        assert got[k][:T].tobytes() == ts[k][:T].tobytes(), (k, got[k][:T], ts[k][:T])
        if k != "live":
            assert got[k][T:].tobytes() == ts0[k][T:].tobytes(), k                    # beyond T: as it was ...
    assert not got["live"][T:].any()                                                   # ... but for live, which the kernels store as 0
    assert got.tobytes() == ts.tobytes() and int(got["pad_"]) == 0x5EED
    assert motion[0].tobytes() == (tm if with_motion else tm0).tobytes()
