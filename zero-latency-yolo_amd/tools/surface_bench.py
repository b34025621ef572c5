#!/usr/bin/env python3
"""surface_bench.py -- what resident surfaces (include/zly.h "Resident surfaces") cost and save on the synchronous host-memory path.

One engine per batch size (bf16 YOLOv8n 416 x 416, bench.py's flags), 1920 x 1080 frames in host memory as BGRA (8.3 MB) and as NV12 (3.1 MB),
batch 1 and batch 8 (one stream per frame of the batch).  Median ms per call over alternating timed blocks of four legs:

    a  whole     zly_detect_batch_view with the whole frames: the baseline, every byte copied to staging and uploaded
    b  one_rect  zly_detect_delta with ONE rectangle of 1/16 of the area per stream (480 x 270)
    c  32_rects  zly_detect_delta with 32 rectangles per stream that sum to 1/16 of the area (90 x 44 and 90 x 46)
    d  keyframe  zly_detect_delta with a rectangle that covers the whole surface, every call: the cost of going through the store -- the same
                 bytes staged and uploaded as in (a), plus one pass over them in HBM by the patch kernel

--legs a runs on a library without the feature too (the parent commit's, through ZLY_LIB and its own zly.py): the two (a) figures bound the
run-to-run spread against which b - d are read.

    python zero-latency-yolo_amd/tools/surface_bench.py [--steps 200] [--warmup 20] [--blocks 10] [--legs abcd] [--batches 1,8] [--out FILE]
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

W, H = 1920, 1080


def _frames(shape, B):
    base = zm.synth_frames(min(B, 4), W, H, seed=13, rects=True)
    if shape == "bgra1080":
        one = [np.concatenate([b, np.full((H, W, 1), 255, np.uint8)], axis=2).reshape(-1) for b in base]
        fmt = zly.PIX_BGRA
    else:
        # luma from the picture's green channel, flat chroma: the bytes' values do not change what the copies cost
        one = [np.concatenate([b[:, :, 1].reshape(-1), np.full(W * H // 2, 128, np.uint8)]) for b in base]
        fmt = zly.PIX_NV12_BT601
    return [np.ascontiguousarray(one[i % len(one)]) for i in range(B)], fmt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200, help="timed calls per leg")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--legs", default="abcd")
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--shapes", default="bgra1080,nv12_1080")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lines = []
    names = {"a": "whole", "b": "one_rect", "c": "32_rects", "d": "keyframe"}
    for B in [int(x) for x in a.batches.split(",")]:
        e = zly.Engine(dtype=zly.DTYPE_BF16, max_batch=B, max_dets=128, use_graph=True, warmup_runs=1, flags=zly.FLAG_NO_HEAD_TENSOR | zly.FLAG_SINGLE_CHAIN)
        if a.legs != "a":
            e.surfaces_enable(B, W * H * 4)
        for shape in a.shapes.split(","):
            frames, fmt = _frames(shape, B)
            whole = zly.view_tight(fmt, W, H)
            streams = list(range(B))
            one = [(s, 720, 404, frames[s], zly.view_crop(whole, 720, 404, 480, 270)) for s in streams]
            # 90 x 44 and 90 x 46 alternately (NV12 needs even sizes): 32 * 90 * 45 pixels in all
            many = [(s, 60 + 230 * (k % 8), 40 + 260 * (k // 8), frames[s], zly.view_crop(whole, 60 + 230 * (k % 8), 40 + 260 * (k // 8), 90, 44 + 2 * (k % 2)))
                    for s in streams for k in range(32)]
            key = [(s, 0, 0, frames[s], whole) for s in streams]
            legs = {"a": lambda: e.detect_batch_view(frames, [whole] * B)}
            if a.legs != "a":
                for s in streams:
                    e.surface_define(s, fmt, W, H)
                e.surface_update(key)
                legs.update({"b": lambda: e.detect_delta(one, streams), "c": lambda: e.detect_delta(many, streams), "d": lambda: e.detect_delta(key, streams)})
            legs = {k: f for k, f in legs.items() if k in a.legs}
            for f in legs.values():
                for _ in range(a.warmup):
                    f()
            per = {k: [] for k in legs}
            order = list(legs)
            for b in range(a.blocks):
                n = a.steps // a.blocks + (1 if b < a.steps % a.blocks else 0)
                for k in (order if b % 2 == 0 else order[::-1]):
                    e.sync()
                    t0 = time.perf_counter()
                    for _ in range(n):
                        legs[k]()
                    per[k].append((time.perf_counter() - t0) / n * 1e3)      # every leg is synchronous
            res = {"tool": "surface_bench", "batch": B, "shape": shape, "frame": [W, H], "frame_bytes": int(frames[0].nbytes), "steps_per_leg": a.steps, "blocks": a.blocks}
            for k in legs:
                res[f"{k}_{names[k]}_ms_per_call"] = round(float(np.median(per[k])), 4)
                res[f"{k}_{names[k]}_blocks"] = [round(x, 4) for x in per[k]]
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
