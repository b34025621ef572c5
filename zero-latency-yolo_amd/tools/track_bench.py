#!/usr/bin/env python3
"""track_bench.py -- what tracking costs on the device path (include/zly.h "tracking": zly_track_slabs behind zly_detect_device).

On ONE engine at the headline configuration (bf16 YOLOv8n 416 x 416, max_dets 64, no head tensor, one chain of launches) it times, with bench.py's
block structure (warm-up, then consecutive timed blocks bracketed by a synchronize; the median block counts):

    b64            zly_detect_device on 64 frames                                     (the untracked step)
    b64_streams64  the same + zly_track_slabs, every frame a stream of its own         (64 workgroups of one wave, one frame each)
    b64_stream1    the same + zly_track_slabs, all 64 frames ONE stream                (one wave walks 64 frames: the serial worst case)
    b1             zly_detect_device on 1 frame
    b1_tracked     the same + zly_track_slabs

The legs of one batch size alternate block by block, so that clock ramps and neighbours on the box hit all alike.  Every tracked step walks the
streams' tables on (frames repeat from step to step, so the steady state is all matches: no births, no evictions).  Writes one text file.

    python zero-latency-yolo_amd/tools/track_bench.py [--steps 300] [--warmup 40] [--blocks 10] [--legs b64,b64_stream1] [--out profiles/FILE.txt]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import zly            # noqa: E402
import zly_model as zm  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300, help="timed steps per leg")
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--legs", default="", help="comma-separated subset of the legs (a profiler run of one tracked leg: its track_kernel times are that leg's)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    B, S = 64, a.size
    frames = np.ascontiguousarray(zm.synth_frames(B, S, S, seed=11, rects=True)).reshape(-1)
    d_frames = torch.from_numpy(frames).cuda()
    torch.cuda.synchronize()
    eng = zly.Engine(dtype=zly.DTYPE_BF16, model_w=S, model_h=S, max_batch=B, max_dets=64, use_graph=True, warmup_runs=1,
                     flags=zly.FLAG_NO_HEAD_TENSOR | zly.FLAG_SINGLE_CHAIN)
    eng.track_enable(max_streams=B, max_tracks=64)
    lib, h = eng.lib, eng.h
    each = (C.c_int32 * B)(*range(B))
    one = (C.c_int32 * B)(*([0] * B))

    def detect(n):
        zly._check(lib, lib.zly_detect_device(h, n, d_frames.data_ptr(), S, S, None, 0, None))

    def tracked(n, streams):
        detect(n)
        zly._check(lib, lib.zly_track_slabs(h, n, streams, None, None))

    groups = [
        {"b64": lambda: detect(B), "b64_streams64": lambda: tracked(B, each), "b64_stream1": lambda: tracked(B, one)},
        {"b1": lambda: detect(1), "b1_tracked": lambda: tracked(1, one)},
    ]
    if a.legs:
        groups = [{k: v for k, v in g.items() if k in a.legs.split(",")} for g in groups]
        groups = [g for g in groups if g]
    detect(B)
    kept = [int(hd["n_kept"]) for hd, _ in eng.read_slabs(B)]
    lines = [f"track_bench: bf16 YOLOv8n {S} x {S}, max_dets 64, one engine (single chain), device path; {a.steps} steps per leg in {a.blocks} blocks, median block",
             f"detections per frame of the 64 synthetic frames: min {min(kept)}, median {int(np.median(kept))}, max {max(kept)} (stored: at most 64)",
             f"{'leg':<16}{'frames':>7}{'ms/step':>10}{'frames/s':>12}{'over untracked':>16}   blocks (ms/step)"]
    for legs in groups:
        eng.track_reset(-1, 1)
        for step in legs.values():
            for _ in range(a.warmup):
                step()
        eng.sync()
        per = {k: [] for k in legs}
        names = list(legs)
        for b in range(a.blocks):
            n = a.steps // a.blocks + (1 if b < a.steps % a.blocks else 0)
            for k in names[b % len(names):] + names[:b % len(names)]:
                eng.sync()
                t0 = time.perf_counter()
                for _ in range(n):
                    legs[k]()
                eng.sync()
                per[k].append((time.perf_counter() - t0) / n * 1e3)
        base = float(np.median(per[names[0]]))
        for k in names:
            nf = B if k.startswith("b64") else 1
            ms = float(np.median(per[k]))
            lines.append(f"{k:<16}{nf:>7}{ms:>10.4f}{nf / ms * 1e3:>12.0f}{(ms - base) * 1e3:>+13.1f} us   " + " ".join(f"{x:.4f}" for x in per[k]))
    st = [eng.track_state(s) for s in (0, B - 1)]
    lines.append(f"stream 0 afterwards: {st[0]}; stream {B - 1}: {st[1]}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    eng.close()


if __name__ == "__main__":
    main()
