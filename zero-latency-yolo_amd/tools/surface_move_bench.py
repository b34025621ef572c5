#!/usr/bin/env python3
"""surface_move_bench.py -- what a move inside a resident surface (include/zly.h "Resident surfaces", MOVES) costs against what a feeder had to do
without it: send the moved region's destination rectangle through zly_surface_update, i.e. through pinned staging and PCIe again.

One engine, a store of 8 slots of 1920 x 1080 BGRA (8.3 MB each), 1 and 8 surfaces per call (the same move, or the same rectangle, on every one).
Two scenarios, each as a move and as the update of its destination rectangle:

    scroll   the 1280 x 720 region at (320, 220) moves up by 40 rows: it overlaps itself, so one phase of two launches -- gathered into the
             bounce buffer, scattered back (3.7 MB read and written twice per surface)
    clear    the 640 x 480 region at (100, 100) moves to (1000, 500), clear of itself: one launch, store -> store (1.2 MB per surface)

A timed call is the entry point followed by zly_sync: host time until the store holds the result.  Median ms per call over alternating timed
blocks, after a warm-up (both legs of a scenario leave the store's contents irrelevant to their cost).

    python zero-latency-yolo_amd/tools/surface_move_bench.py [--steps 200] [--warmup 20] [--blocks 10] [--counts 1,8] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch          # noqa: F401  (before the first engine: the process then uses torch's HIP runtime throughout)

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import zly            # noqa: E402
import zly_model as zm  # noqa: E402

W, H, SLOTS = 1920, 1080, 8
SCENARIOS = {"scroll": (320, 220, 320, 180, 1280, 720), "clear": (100, 100, 1000, 500, 640, 480)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200, help="timed calls per leg")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--counts", default="1,8", help="surfaces per call")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    e = zly.Engine(dtype=zly.DTYPE_BF16, max_batch=1, max_dets=128, warmup_runs=0)
    e.surfaces_enable(SLOTS, W * H * 4)
    e.surface_moves_enable(0)
    bgr = zm.synth_frames(1, W, H, seed=13, rects=True)[0]
    frame = np.ascontiguousarray(np.concatenate([bgr, np.full((H, W, 1), 255, np.uint8)], axis=2).reshape(-1))
    whole = zly.view_tight(zly.PIX_BGRA, W, H)
    for s in range(SLOTS):
        e.surface_define(s, zly.PIX_BGRA, W, H)
    e.surface_update([(s, 0, 0, frame, whole) for s in range(SLOTS)])
    e.sync()
    lines = []
    for n in [int(x) for x in a.counts.split(",")]:
        for name, (sx, sy, dx, dy, w, h) in SCENARIOS.items():
            moves = [(s, sx, sy, dx, dy, w, h) for s in range(n)]
            rects = [(s, dx, dy, frame, zly.view_crop(whole, dx, dy, w, h)) for s in range(n)]
            legs = {"move": lambda: e.surface_move(moves), "update": lambda: e.surface_update(rects)}
            for f in legs.values():
                for _ in range(a.warmup):
                    f()
                    e.sync()
            per = {k: [] for k in legs}
            order = list(legs)
            for b in range(a.blocks):
                cnt = a.steps // a.blocks + (1 if b < a.steps % a.blocks else 0)
                for k in (order if b % 2 == 0 else order[::-1]):
                    e.sync()
                    t0 = time.perf_counter()
                    for _ in range(cnt):
                        legs[k]()
                        e.sync()
                    per[k].append((time.perf_counter() - t0) / cnt * 1e3)
            res = {"tool": "surface_move_bench", "scenario": name, "surfaces_per_call": n, "move": [sx, sy, dx, dy, w, h], "bytes_per_surface": w * h * 4,
                   "steps_per_leg": a.steps, "blocks": a.blocks}
            for k in legs:
                res[f"{k}_ms_per_call"] = round(float(np.median(per[k])), 4)
                res[f"{k}_blocks"] = [round(x, 4) for x in per[k]]
            res["update_over_move"] = round(res["update_ms_per_call"] / res["move_ms_per_call"], 2)
            line = json.dumps(res)
            print(line, flush=True)
            lines.append(line)
    e.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
