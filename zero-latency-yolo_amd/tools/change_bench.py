#!/usr/bin/env python3
"""change_bench.py -- what the change map costs per frame (include/zly.h "Change map"), alone and inside a zoom call, against doing without it.

On ONE engine (bf16 YOLOv8n 416 x 416, max_dets 64, no head tensor, one chain of launches) with 1920 x 1080 BGRA RESIDENT surfaces, cells of 32, for
1 and for 8 surfaces per call, K = 3 regions of 416 x 416, it times, in ms per frame:

    a_change    zly_change_surfaces alone: the two kernels and the two copies of the call's frame records
    b_detect    zly_detect_surfaces alone                                                    (what an engine without any option costs)
    c_zoom_off  zly_detect_surfaces_zoom with zly_zoom_use_change(e, 0)                      (zoom as it was)
    c_zoom_on   zly_detect_surfaces_zoom with zly_zoom_use_change(e, 1)                      (c_zoom_on - c_zoom_off: what the option costs a zoom call)
    d_grid      the full zly_tile_grid of 416 x 416 tiles, overlap 64 (18 tiles per surface), merged and tracked, as tools/zoom_bench.py's arm d

Every stream has TWO resident surfaces whose pictures differ by two patches of 48 x 48 pixels, and every arm alternates between them from step to
step: the change map sees a change in every frame, chooses peaks and -- in arm c_zoom_on -- fills fallback regions, as it would on a capture with a
static camera.  The surfaces' updates are not part of a step.  a_change is also given as a multiple of the time to read the frames' bytes once at the
copy bandwidth of profiles/r01_copy_bandwidth.txt (7.0 TB/s of traffic).  All arms run in one process, alternating window by window; every arm is
warmed up first; a window is steps of one arm bracketed by a synchronise and lasts at least --window seconds (host clock); --repeats windows per arm
show the spread.

--arms NAMES times the named arms alone (a kernel trace of a_change is taken that way).  --parent times b_detect and c_zoom_off alone and needs
nothing of the change map: with --package DIR (a package directory of another commit's build: its zly.py and _build/) it is how the two are measured
on the parent commit, in a process of its own.

    python zero-latency-yolo_amd/tools/change_bench.py [--window 1.0] [--repeats 5] [--warmup 30] [--parent] [--arms a,b] [--package DIR] [--out profiles/FILE.txt]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch        # noqa: F401  (the process uses torch's HIP runtime throughout, as the tests do)

HERE = os.path.dirname(os.path.abspath(__file__))

SW, SH, TILE, OVERLAP, K, CELL = 1920, 1080, 416, 64, 3, 32
COPY_TBPS = 7.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=1.0, help="least seconds per timed window")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--parent", action="store_true")
    ap.add_argument("--arms", default="", help="comma-separated arm names: time these alone (a kernel trace of a_change, say)")
    ap.add_argument("--package", default="", help="import zly (and load its _build/) from this package directory instead of this tool's own")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    pkg = os.path.abspath(a.package) if a.package else os.path.dirname(HERE)
    sys.path.insert(0, os.path.join(pkg, "tools"))
    sys.path.insert(0, pkg)
    import zly
    import zly_model as zm

    B, cap, S = 64, 64, 8
    eng = zly.Engine(dtype=zly.DTYPE_BF16, model_w=TILE, model_h=TILE, max_batch=B, max_dets=cap, use_graph=True, warmup_runs=1,
                     flags=zly.FLAG_NO_HEAD_TENSOR | zly.FLAG_SINGLE_CHAIN)
    eng.track_enable(max_streams=S, max_tracks=64)
    eng.zoom_enable(regions=K, region_w=TILE, region_h=TILE)
    eng.surfaces_enable(2 * S, SW * SH * 4)
    if not a.parent:
        eng.change_enable(S, cell=CELL, window_w=TILE, window_h=TILE)
    lib, h = eng.lib, eng.h
    whole = zly.view_tight(zly.PIX_BGRA, SW, SH)
    pictures = zm.synth_frames(S, SW, SH, seed=21, rects=True)
    for s in range(S):
        for alt in (0, 1):                                   # slot s and slot S + s: the stream's two pictures
            pic = pictures[s].copy()
            for j, (px, py) in enumerate(((200 + 600 * alt, 150 + 300 * alt), (1500 - 500 * alt, 800 - 100 * alt))):
                pic[py:py + 48, px:px + 48] = 255 - pic[py:py + 48, px:px + 48] if j else 255
            eng.surface_define(s + S * alt, zly.PIX_BGRA, SW, SH)
            bgra = np.ascontiguousarray(np.concatenate([pic, np.full((SH, SW, 1), 255, np.uint8)], axis=2)).reshape(-1)
            eng.surface_update([(s + S * alt, 0, 0, bgra, whole)])
    eng.sync()
    grid = zly.tile_grid(SW, SH, TILE, TILE, OVERLAP, OVERLAP)
    per_call = B // len(grid)
    cfg = zly.merge_config()
    d_out = torch.zeros(S * eng.slab_bytes, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    tick = [0]

    def ids(n, alt=0):
        return (C.c_int32 * n)(*range(S * alt, S * alt + n))

    def a_change(n, slots, streams):
        zly._check(lib, lib.zly_change_surfaces(h, n, slots, streams, None))

    def b_detect(n, slots, streams):
        zly._check(lib, lib.zly_detect_surfaces(h, n, slots, None, None, 0, None))

    def c_zoom(n, slots, streams):
        zly._check(lib, lib.zly_detect_surfaces_zoom(h, n, slots, streams, C.byref(cfg), d_out.data_ptr(), 0, None))

    def grid_args(n, alt):
        calls = []
        for first in range(0, n, per_call):
            group = list(range(first, min(n, first + per_call)))
            surf = [s + S * alt for s in group for _ in grid]
            rois = [zly.Roi(t.x0, t.y0, t.w, t.h) for _ in group for t in grid]
            tiles = [zly.tile(t.x0, t.y0, t.w, t.h, SW, SH, group=g) for g in range(len(group)) for t in grid]
            calls.append((len(group), (C.c_int32 * len(surf))(*surf), (zly.Roi * len(surf))(*rois), (zly.Tile * len(surf))(*tiles), (C.c_int32 * len(group))(*group)))
        return calls

    def d_grid(calls):
        for n_surf, c_surf, c_rois, c_tiles, c_streams in calls:
            nv = len(c_surf)
            zly._check(lib, lib.zly_detect_surfaces(h, nv, c_surf, c_rois, None, 0, None))
            zly._check(lib, lib.zly_merge_slabs(h, nv, c_tiles, n_surf, C.byref(cfg), None, d_out.data_ptr(), 0, None))
            zly._check(lib, lib.zly_track_slabs(h, n_surf, c_streams, d_out.data_ptr(), None))

    lines = [f"change_bench: bf16 YOLOv8n {TILE} x {TILE}, max_dets {cap}, one engine (single chain), resident {SW} x {SH} BGRA surfaces, two pictures per stream in turn; "
             f"cells of {CELL}, K = {K} regions of {TILE} x {TILE}; grid: {len(grid)} tiles; windows of >= {a.window} s, {a.repeats} per arm, alternating"
             + (" [parent arms only]" if a.parent else ""),
             f"{'arm':<11}{'surfaces':>9}{'ms/frame (median)':>19}{'min':>9}{'max':>9}   windows (ms/frame)"]
    for n in (1, S):
        slots, streams, gcalls = (ids(n, 0), ids(n, 1)), ids(n), (grid_args(n, 0), grid_args(n, 1))

        def alternating(fn):
            def step():
                tick[0] ^= 1
                fn(n, slots[tick[0]], streams)
            return step

        def zoom_with(on):
            inner = alternating(c_zoom)

            def step():
                inner()
            step.before = lambda: None if a.parent else eng.zoom_use_change(on)
            return step

        def grid_step():
            tick[0] ^= 1
            d_grid(gcalls[tick[0]])

        arms = {"b_detect": alternating(b_detect), "c_zoom_off": zoom_with(False)}
        if not a.parent:
            arms.update({"a_change": alternating(a_change), "c_zoom_on": zoom_with(True), "d_grid": grid_step})
        if a.arms:
            arms = {k: v for k, v in arms.items() if k in a.arms.split(",")}
        eng.track_reset(-1, 1)
        steps_of = {}
        for k, step in arms.items():                         # warm-up, then a short timed run that sizes the arm's windows
            getattr(step, "before", lambda: None)()
            for _ in range(a.warmup):
                step()
            eng.sync()
            t0 = time.perf_counter()
            for _ in range(20):
                step()
            eng.sync()
            steps_of[k] = max(20, int(a.window / ((time.perf_counter() - t0) / 20) * 1.15) + 1)
        per = {k: [] for k in arms}
        names = list(arms)
        filled = 0
        for r in range(a.repeats):
            for k in names[r % len(names):] + names[:r % len(names)]:
                step = arms[k]
                getattr(step, "before", lambda: None)()
                eng.sync()
                t0 = time.perf_counter()
                for _ in range(steps_of[k]):
                    step()
                eng.sync()                                   # ONE synchronise ends the window: the enqueue-only arms run ahead of the device inside it
                per[k].append((time.perf_counter() - t0) / (steps_of[k] * n) * 1e3)
                if k == "c_zoom_on":
                    filled = int((eng.zoom_read_plan(n)["slot"] == -2).sum())
        for k in sorted(names):
            v = per[k]
            lines.append(f"{k:<11}{n:>9}{float(np.median(v)):>19.4f}{min(v):>9.4f}{max(v):>9.4f}   " + " ".join(f"{x:.4f}" for x in v))
        if "a_change" in per:
            bound = SW * SH * 4 / (COPY_TBPS * 1e12) * 1e3
            med = float(np.median(per["a_change"]))
            hdr, peaks, _ = zly.parse_change_record(eng.change_read(0), 3)
            lines.append(f"  ({n} surfaces: a_change is {med / bound:.1f} x the {bound:.5f} ms that reading a frame's {SW * SH * 4} bytes once takes at {COPY_TBPS} TB/s; "
                         f"stream 0's last frame: {int(hdr['n_active'])} of {int(hdr['n_cells'])} cells active, {len(peaks)} peaks, flags {int(hdr['flags'])}; "
                         f"the last c_zoom_on call filled {filled} of {n * K} regions)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    eng.close()


if __name__ == "__main__":
    main()
