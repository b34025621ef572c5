"""The cases of tests/golden/call_refusals_parent.json and how one case is put to a libzly.so: what the device entries and the read-backs of
include/zly.h answer when they REFUSE a call -- on engines that lack the resident store, the feature the entry belongs to, or both (which refusal
comes first), and on a fully equipped engine for an out-of-range n, a null argument and a bad stream index -- and how far a successful call of each
device entry moves the engine's counters.

The golden file records what the library answered BEFORE the entries' shared scaffolding in csrc/engine.cpp was joined (one frame table, one detect
tail, one store source, one read-back); tests/test_gpu_call_refusals.py replays it through the library of the tree.  It was written once, against a
library built from the commit before that change:

    ZLY_LIB=<that commit's libzly.so> python3 tests/call_refusal_cases.py --record [--out FILE]

and is not regenerated from the code under test: a refusal that is meant to change shows as a diff of the file.

A case is (set-up, entry, variant); its recording is [return code, zly_last_error text ("" if the call succeeded), the deltas of STAT_FIELDS].
Layout of the file: {"refusals": {set-up: [[entry, variant, rc, text, deltas], ...]}, "success": [[entry, deltas], ...]}.

Sizes: a 64 x 64 model, max_batch 4, max_dets 16, no warm-up, no graphs; frames and surfaces of 37 x 29 BGR.  Cases that
tests/test_gpu_surface.py::test_an_engine_without_a_store_refuses_every_call pins (the store's own entries on an engine with nothing enabled) are
left out."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zero-latency-yolo_amd"))
import zly  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "call_refusals_parent.json")
W, H, FMT = 37, 29, zly.PIX_BGR
FB = W * H * 3
MODEL, MAX_BATCH, MAX_DETS, MAX_STREAMS = 64, 4, 16, 4
N = 2                                     # frames of a call whose n is in range
BAD_STREAM, BAD_SLOT = 9, 99
STAT_FIELDS = ("inference_count", "inference_errors", "batches", "graph_replays", "eager_batches")

# what an engine of each set-up has enabled
SETUPS = {"bare": (), "store": ("store",), "track": ("track",), "features": ("track", "zoom", "chips", "change"),
          "full": ("store", "track", "zoom", "chips", "change")}
# what an entry needs before its arguments are looked at; "merged" and "zoomed" (a merge / a zoom call made) hold on no engine while the refusals run
NEEDS = {"detect_device_fmt": (), "detect_device_view": (), "detect_device_zoom": ("zoom",),
         "detect_surfaces": ("store",), "change_surfaces": ("store", "change"), "chips_surfaces": ("store", "chips"),
         "detect_surfaces_zoom": ("store", "zoom"), "detect_delta": ("store",),
         "read_slabs": (), "read_merged": ("merged",), "read_chips": ("chips",), "zoom_read_plan": ("zoom", "zoomed"), "change_read": ("change",),
         "surface_read": ("store",), "track_read": ("track",), "track_state_at": ("track",), "zoom_plan": ("zoom",)}
# the bad arguments put to a fully equipped engine.  n0 / n_big: n = 0 / max_batch + 1 (an entry without an n: a capacity of 0 -- track_read: -1 --
# / slot 99); n_over: n x (1 + regions) beyond max_batch; null: one null argument; bad_stream: stream index 9 of 4
VARIANTS = {"detect_device_fmt": ("n0", "n_big", "null"), "detect_device_view": ("n0", "n_big", "null"),
            "detect_device_zoom": ("n0", "n_big", "n_over", "null", "bad_stream"),
            "detect_surfaces": ("n0", "n_big", "null"), "change_surfaces": ("n0", "n_big", "null", "bad_stream"), "chips_surfaces": ("n0", "n_big", "null"),
            "detect_surfaces_zoom": ("n0", "n_big", "n_over", "null", "bad_stream"), "detect_delta": ("n0", "n_big", "null"),
            "read_slabs": ("n0", "n_big", "null"), "read_merged": ("n0", "n_big", "null"), "read_chips": ("n0", "n_big", "null"),
            "zoom_read_plan": ("n0", "n_big", "null"), "change_read": ("n0", "null", "bad_stream"), "surface_read": ("n0", "n_big", "null"),
            "track_read": ("n0", "null", "bad_stream"), "track_state_at": ("null", "bad_stream"), "zoom_plan": ("n0", "n_big", "null", "bad_stream")}
SUCCESS = ("plain", "view", "surfaces", "zoom", "tiled", "delta")


def cases(setup):
    """[(entry, variant)] of a set-up, in the order they are made: every entry the set-up cannot serve with good arguments, then -- on the full
    engine -- every entry with each of its bad arguments"""
    have = SETUPS[setup]
    out = []
    for entry, needs in NEEDS.items():
        missing = [x for x in needs if x not in have]
        if not missing or (setup == "bare" and needs == ("store",)):
            continue
        out.append((entry, "good"))
    if setup == "full":
        out += [(entry, v) for entry, vs in VARIANTS.items() for v in vs]
    return out


def frames():
    return np.random.default_rng(20240611).integers(0, 256, (N, H, W, 3), dtype=np.uint8)


class Ctx:
    """an engine of a set-up, the two frames in device memory and as resident surfaces 0 and 1 (slot 2: defined, no keyframe)"""

    def __init__(self, weights, setup):
        import torch            # the process uses torch's HIP runtime throughout, as the other GPU tests do
        self.torch = torch
        self.setup, have = setup, SETUPS[setup]
        self.host = frames()
        self.d = torch.from_numpy(self.host.reshape(-1).copy()).cuda()
        torch.cuda.synchronize()
        self.dptr, self.nbytes = self.d.data_ptr(), N * FB
        self.views = (zly.FrameView * (MAX_BATCH + 1))()
        for i in range(MAX_BATCH + 1):
            v = zly.view_tight(FMT, W, H)
            v.off[0] = (i % N) * FB
            self.views[i] = v
        e = self.e = zly.Engine(weights, model_w=MODEL, model_h=MODEL, dtype=zly.DTYPE_BF16, max_batch=MAX_BATCH, max_dets=MAX_DETS, conf_thr=0.05,
                                warmup_runs=0, use_graph=False)
        if "store" in have:
            e.surfaces_enable(3, FB)
            for s in range(3):
                e.surface_define(s, FMT, W, H)
            e.surface_update([(s, 0, 0, self.host[s].reshape(-1), zly.view_tight(FMT, W, H)) for s in range(N)])
        if "track" in have:
            e.track_enable(max_streams=MAX_STREAMS, max_tracks=MAX_DETS)
        if "zoom" in have:
            e.zoom_enable(regions=1)
        if "chips" in have:
            e.chips_enable()
        if "change" in have:
            e.change_enable(MAX_STREAMS, cell=8)
        e.sync()
        self.out = np.zeros(1 << 16, dtype=np.uint8)          # more than any read-back of these sizes
        self.n_out = (C.c_int32 * (MAX_BATCH + 1))()
        self.mc = zly.merge_config()

    def close(self):
        self.e.close()

    def stats(self):
        st = self.e.stats()
        return [int(st[k]) for k in STAT_FIELDS]


def call(ctx, entry, variant):
    """the raw C call of a case -> its return code"""
    lib, h = ctx.e.lib, ctx.e.h
    n = {"n0": 0, "n_big": MAX_BATCH + 1, "n_over": 3}.get(variant, N)
    null, bad = variant == "null", variant == "bad_stream"
    i32 = lambda xs: (C.c_int32 * len(xs))(*xs)
    surfaces, streams = i32([0, 1, 0, 1, 0]), i32([0, BAD_STREAM if bad else 1, 2, 3, 0])
    stream = BAD_STREAM if bad else 0
    cap = 0 if variant == "n0" else ctx.out.nbytes
    out = None if null else ctx.out.ctypes.data
    mc = C.byref(ctx.mc)
    if entry == "detect_device_fmt":
        return lib.zly_detect_device_fmt(h, FMT, n, None if null else ctx.dptr, W, H, None, 0, None)
    if entry == "detect_device_view":
        return lib.zly_detect_device_view(h, n, ctx.dptr, ctx.nbytes, None if null else ctx.views, None, 0, None)
    if entry == "detect_device_zoom":
        return lib.zly_detect_device_zoom(h, n, ctx.dptr, ctx.nbytes, ctx.views, None if null else streams, mc, None, 0, None)
    if entry == "detect_surfaces":
        return lib.zly_detect_surfaces(h, n, None if null else surfaces, None, None, 0, None)
    if entry == "change_surfaces":
        return lib.zly_change_surfaces(h, n, surfaces, None if null else streams, None)
    if entry == "chips_surfaces":
        return lib.zly_chips_surfaces(h, n, None if null else surfaces, None, zly.CHIPS_SRC_SLABS, None, None)
    if entry == "detect_surfaces_zoom":
        return lib.zly_detect_surfaces_zoom(h, n, surfaces, None if null else streams, mc, None, 0, None)
    if entry == "detect_delta":
        return lib.zly_detect_delta(h, 0, None, None, None, None, n, surfaces, out, MAX_DETS, ctx.n_out)
    if entry == "read_slabs":
        return lib.zly_read_slabs(h, n, out)
    if entry == "read_merged":
        return lib.zly_read_merged(h, n, out)
    if entry == "read_chips":
        return lib.zly_read_chips(h, n, out)
    if entry == "zoom_read_plan":
        return lib.zly_zoom_read_plan(h, n, out)
    if entry == "change_read":
        return lib.zly_change_read(h, stream, out, cap)
    if entry == "surface_read":
        return lib.zly_surface_read(h, BAD_SLOT if variant == "n_big" else 0, out, cap)
    if entry == "track_read":
        return lib.zly_track_read(h, stream, ctx.out.ctypes.data, -1 if variant == "n0" else 64, None if null else ctx.n_out)
    if entry == "track_state_at":
        return lib.zly_track_state_at(h, stream, None if null else C.cast(ctx.out.ctypes.data, C.POINTER(zly.TrackState)))
    if entry == "zoom_plan":
        sizes = i32([W] * (MAX_BATCH + 1)), i32([H] * (MAX_BATCH + 1))
        return lib.zly_zoom_plan(h, n, sizes[0], sizes[1], None if null else streams, ctx.out.ctypes.data)
    raise KeyError(entry)


def run_refusals(ctx):
    """every case of the context's set-up -> [[entry, variant, rc, text, deltas]]"""
    got = []
    for entry, variant in cases(ctx.setup):
        before = ctx.stats()
        rc = call(ctx, entry, variant)
        text = ctx.e.lib.zly_last_error().decode() if rc != zly.OK else ""
        got.append([entry, variant, rc, text, [a - b for a, b in zip(ctx.stats(), before)]])
    return got


def good_call(ctx):
    """one call the set-up serves, and everything it left to be read, as bytes: through the store and the zoom regions where the engine has both,
    else on the frame views"""
    e = ctx.e
    if "store" in SETUPS[ctx.setup] and "zoom" in SETUPS[ctx.setup]:
        e.detect_surfaces_zoom([0, 1], [0, 1])
        raws = [np.zeros(2 * N * e.slab_bytes, dtype=np.uint8), np.zeros(N * e.slab_bytes, dtype=np.uint8)]
        zly._check(e.lib, e.lib.zly_read_slabs(e.h, 2 * N, raws[0].ctypes.data))
        zly._check(e.lib, e.lib.zly_read_merged(e.h, N, raws[1].ctypes.data))
        return [r.tobytes() for r in raws] + [e.zoom_read_plan(N).tobytes()] + [e.track_read(s).tobytes() for s in range(N)]
    e.detect_device_view(ctx.dptr, ctx.nbytes, [ctx.views[i] for i in range(N)])
    raw = np.zeros(N * e.slab_bytes, dtype=np.uint8)
    zly._check(e.lib, e.lib.zly_read_slabs(e.h, N, raw.ctypes.data))
    return [raw.tobytes()]


def run_success(ctx):
    """one successful call of each device entry on a full engine -> [[entry, deltas]]"""
    e = ctx.e
    views = [ctx.views[i] for i in range(N)]
    surface = zly.view_tight(FMT, W, H)
    tiles = [zly.tile(0, 0, 20, H, W, H), zly.tile(17, 0, 20, H, W, H)]
    calls = {"plain": lambda: e.detect_device(ctx.dptr, N, W, H), "view": lambda: e.detect_device_view(ctx.dptr, ctx.nbytes, views),
             "surfaces": lambda: e.detect_surfaces([0, 1]), "zoom": lambda: e.detect_device_zoom(ctx.dptr, ctx.nbytes, views, [0, 1]),
             "tiled": lambda: e.detect_tiled(ctx.host[0].reshape(-1), surface, tiles), "delta": lambda: e.detect_delta([], [0, 1])}
    got = []
    for name in SUCCESS:
        before = ctx.stats()
        calls[name]()
        e.sync()
        got.append([name, [a - b for a, b in zip(ctx.stats(), before)]])
    return got


def load():
    with open(GOLDEN) as f:
        return json.load(f)


def record(weights, path):
    golden = {"refusals": {}, "success": None}
    for setup in SETUPS:
        ctx = Ctx(weights, setup)
        golden["refusals"][setup] = run_refusals(ctx)
        kept = [int(np.frombuffer(b, dtype=np.int32)[0]) for b in good_call(ctx)[:1]]
        print(f"{setup}: {len(golden['refusals'][setup])} cases, {sum(r[2] != 0 for r in golden['refusals'][setup])} refused; n_kept of slab 0 after them: {kept}")
        ctx.close()
    ctx = Ctx(weights, "full")
    golden["success"] = run_success(ctx)
    ctx.close()
    print("success:", golden["success"])
    rows = lambda xs: "[\n" + ",\n".join(json.dumps(x) for x in xs) + "\n]"                    # one case per line
    with open(path, "w") as f:
        f.write('{"refusals": {\n' + ",\n".join(f'"{s}": {rows(r)}' for s, r in golden["refusals"].items()) + '\n},\n"success": ' + rows(golden["success"]) + "\n}\n")


if __name__ == "__main__":
    assert sys.argv[1:2] == ["--record"], __doc__
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else GOLDEN
    print("recording from", os.environ.get("ZLY_LIB") or zly.LIB_PATH)
    record(os.path.join(ROOT, "zero-latency-yolo_amd", "_build", "yolov8n_synth.zlyw"), out)
