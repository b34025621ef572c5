#!/usr/bin/env python3
"""zoom_bench.py -- what zooming into a stream's tracked targets costs per frame (include/zly.h "Zoom regions"), against the ways to do without it.

On ONE engine (bf16 YOLOv8n 416 x 416, max_dets 64, no head tensor, one chain of launches) with 1920 x 1080 BGRA RESIDENT surfaces, for 1 and for 8
streams per call, K = 3 regions of 416 x 416, it times four arms, in ms per frame:

    a_whole   zly_detect_surfaces on the whole surfaces + zly_track_slabs                                   (no zoom at all: the floor)
    b_zoom    zly_detect_surfaces_zoom: the plan on the GPU, 1 + K views per frame, merge, track            (the feature)
    c_host    the same work driven from the host with the existing calls: zly_track_read per stream (it synchronises with the previous frame's
              tracker), the regions as rois of zly_detect_surfaces, zly_merge_slabs, zly_track_slabs         (the yardstick of the device-side plan)
    d_grid    the full zly_tile_grid of 416 x 416 tiles, overlap 64 as tools/tile_bench.py (18 tiles per surface; calls of at most max_batch views),
              merged and tracked                                                                             (the yardstick of the feature)

Arm c's plan ARITHMETIC is not timed: a host implementation in C costs about a microsecond, a Python one would cost more than the frame, so the arm
reuses the regions the GPU planned for the same (static) pictures and is charged only for zly_track_read and the calls -- which favours arm c.
The surfaces hold static pictures: their updates cost every arm the same and are not part of a step.  All arms run in one process, alternating
window by window; every arm is warmed up first; a window is steps of one arm bracketed by a synchronise and lasts at least --window seconds (host
clock); --repeats windows per arm show the spread.  Writes one text file.

    python zero-latency-yolo_amd/tools/zoom_bench.py [--window 1.0] [--repeats 5] [--warmup 30] [--out profiles/FILE.txt]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch        # noqa: F401  (the process uses torch's HIP runtime throughout, as the tests do)

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import zly            # noqa: E402
import zly_model as zm  # noqa: E402

SW, SH, TILE, OVERLAP, K = 1920, 1080, 416, 64, 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=1.0, help="least seconds per timed window")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    B, cap, S = 64, 64, 8
    eng = zly.Engine(dtype=zly.DTYPE_BF16, model_w=TILE, model_h=TILE, max_batch=B, max_dets=cap, use_graph=True, warmup_runs=1,
                     flags=zly.FLAG_NO_HEAD_TENSOR | zly.FLAG_SINGLE_CHAIN)
    eng.track_enable(max_streams=S, max_tracks=64)
    eng.zoom_enable(regions=K, region_w=TILE, region_h=TILE)
    eng.surfaces_enable(S, SW * SH * 4)
    lib, h = eng.lib, eng.h
    whole = zly.view_tight(zly.PIX_BGRA, SW, SH)
    pictures = zm.synth_frames(S, SW, SH, seed=21, rects=True)
    for s in range(S):
        eng.surface_define(s, zly.PIX_BGRA, SW, SH)
        bgra = np.ascontiguousarray(np.concatenate([pictures[s], np.full((SH, SW, 1), 255, np.uint8)], axis=2)).reshape(-1)
        eng.surface_update([(s, 0, 0, bgra, whole)])
    eng.sync()
    grid = zly.tile_grid(SW, SH, TILE, TILE, OVERLAP, OVERLAP)
    per_call = B // len(grid)                                # whole surfaces' grids per call
    cfg = zly.merge_config()
    d_out = torch.zeros(S * eng.slab_bytes, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    trk = np.zeros(64, dtype=zly.TRACK_DTYPE)
    n_trk = C.c_int32(0)

    def ids(n):
        return (C.c_int32 * n)(*range(n))

    def a_whole(n, c_ids):
        zly._check(lib, lib.zly_detect_surfaces(h, n, c_ids, None, None, 0, None))
        zly._check(lib, lib.zly_track_slabs(h, n, c_ids, None, None))

    def b_zoom(n, c_ids):
        zly._check(lib, lib.zly_detect_surfaces_zoom(h, n, c_ids, c_ids, C.byref(cfg), d_out.data_ptr(), 0, None))

    def tiled(n_surf, c_surf, c_rois, c_tiles, c_streams):
        nv = len(c_surf)
        zly._check(lib, lib.zly_detect_surfaces(h, nv, c_surf, c_rois, None, 0, None))
        zly._check(lib, lib.zly_merge_slabs(h, nv, c_tiles, n_surf, C.byref(cfg), None, d_out.data_ptr(), 0, None))
        zly._check(lib, lib.zly_track_slabs(h, n_surf, c_streams, d_out.data_ptr(), None))

    def host_args(n, plan):
        """the call arguments of arm c for n streams whose regions are plan[n][K]"""
        surf, rois, tiles = [], [], []
        for i in range(n):
            surf.append(i); rois.append(zly.Roi(0, 0, SW, SH)); tiles.append(zly.tile(0, 0, SW, SH, SW, SH, group=i))
            for r in plan[i]:
                surf.append(i); rois.append(zly.Roi(int(r["x0"]), int(r["y0"]), int(r["w"]), int(r["h"])))
                tiles.append(zly.tile(int(r["x0"]), int(r["y0"]), int(r["w"]), int(r["h"]), SW, SH, group=i))
        nv = len(surf)
        return (C.c_int32 * nv)(*surf), (zly.Roi * nv)(*rois), (zly.Tile * nv)(*tiles), ids(n)

    def c_host(n, args):
        for s in range(n):                                   # what the host needs to plan: every stream's table, behind the previous frame's tracker
            zly._check(lib, lib.zly_track_read(h, s, trk.ctypes.data, 64, C.byref(n_trk)))
        tiled(n, *args)

    def grid_args(n):
        calls = []
        for first in range(0, n, per_call):
            group = list(range(first, min(n, first + per_call)))
            surf = [s for s in group for _ in grid]
            rois = [zly.Roi(t.x0, t.y0, t.w, t.h) for _ in group for t in grid]
            tiles = [zly.tile(t.x0, t.y0, t.w, t.h, SW, SH, group=g) for g in range(len(group)) for t in grid]
            calls.append((len(group), (C.c_int32 * len(surf))(*surf), (zly.Roi * len(surf))(*rois), (zly.Tile * len(surf))(*tiles), (C.c_int32 * len(group))(*group)))
        return calls

    def d_grid(calls):
        for call in calls:
            tiled(*call)

    lines = [f"zoom_bench: bf16 YOLOv8n {TILE} x {TILE}, max_dets {cap}, one engine (single chain), resident {SW} x {SH} BGRA surfaces; K = {K} regions of "
             f"{TILE} x {TILE}; grid: {len(grid)} tiles of {TILE}, overlap {OVERLAP}; windows of >= {a.window} s, {a.repeats} per arm, alternating",
             f"{'arm':<10}{'streams':>8}{'views/frame':>12}{'ms/frame (median)':>19}{'min':>9}{'max':>9}   windows (ms/frame)"]
    for n in (1, S):
        c_ids = ids(n)
        eng.track_reset(-1, 1)
        for _ in range(3):                                   # tracks to zoom into, and the regions arm c reuses
            b_zoom(n, c_ids)
        plan = eng.zoom_read_plan(n)
        zoomed = int((plan["slot"] >= 0).sum())
        hargs, gcalls = host_args(n, plan), grid_args(n)
        arms = {"a_whole": (lambda: a_whole(n, c_ids), 1), "b_zoom": (lambda: b_zoom(n, c_ids), 1 + K),
                "c_host": (lambda: c_host(n, hargs), 1 + K), "d_grid": (lambda: d_grid(gcalls), len(grid))}
        steps_of = {}
        for k, (step, _) in arms.items():                    # warm-up, then a short timed run that sizes the arm's windows
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
        shortest = float('inf')
        for r in range(a.repeats):
            for k in names[r % len(names):] + names[:r % len(names)]:
                step = arms[k][0]
                eng.sync()
                t0 = time.perf_counter()
                for _ in range(steps_of[k]):
                    step()
                eng.sync()                                   # ONE synchronise ends the window: the enqueue-only arms run ahead of the device inside it
                dt = time.perf_counter() - t0
                shortest = min(shortest, dt)
                per[k].append(dt / (steps_of[k] * n) * 1e3)
        for k in names:
            v = per[k]
            lines.append(f"{k:<10}{n:>8}{arms[k][1]:>12}{float(np.median(v)):>19.4f}{min(v):>9.4f}{max(v):>9.4f}   " + " ".join(f"{x:.4f}" for x in v))
        lines.append(f"  ({n} streams: {zoomed} of {n * K} regions follow a track, the others are fallbacks; the shortest window took {shortest:.2f} s)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    eng.close()


if __name__ == "__main__":
    main()
