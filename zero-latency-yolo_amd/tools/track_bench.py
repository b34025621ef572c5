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

--motion adds a second engine of the same configuration with the motion model on (zly_track_motion_enable) and, beside every tracked leg, the
same leg on that engine (NAME_motion: track_motion_kernel in place of track_kernel), alternating with the others in the same blocks: the cost of
the motion launch read beside the plain one, in one session.

    python zero-latency-yolo_amd/tools/track_bench.py [--steps 300] [--warmup 40] [--blocks 10] [--legs b64,b64_stream1] [--motion] [--out profiles/FILE.txt]
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
    ap.add_argument("--motion", action="store_true", help="also time every tracked leg on a second engine with the motion model on (legs NAME_motion)")
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
    eng_m = None
    if a.motion:
        eng_m = zly.Engine(dtype=zly.DTYPE_BF16, model_w=S, model_h=S, max_batch=B, max_dets=64, use_graph=True, warmup_runs=1,
                           flags=zly.FLAG_NO_HEAD_TENSOR | zly.FLAG_SINGLE_CHAIN)
        eng_m.track_enable(max_streams=B, max_tracks=64)
        eng_m.track_motion_enable()
    each = (C.c_int32 * B)(*range(B))
    one = (C.c_int32 * B)(*([0] * B))

    def detect(n):
        zly._check(lib, lib.zly_detect_device(h, n, d_frames.data_ptr(), S, S, None, 0, None))

    def tracked(n, streams, hh=None):
        hh = hh or h
        zly._check(lib, lib.zly_detect_device(hh, n, d_frames.data_ptr(), S, S, None, 0, None))
        zly._check(lib, lib.zly_track_slabs(hh, n, streams, None, None))

    groups = [
        {"b64": lambda: detect(B), "b64_streams64": lambda: tracked(B, each), "b64_stream1": lambda: tracked(B, one)},
        {"b1": lambda: detect(1), "b1_tracked": lambda: tracked(1, one)},
    ]
    if eng_m is not None:
        hm = eng_m.h
        groups[0].update({"b64_streams64_motion": lambda: tracked(B, each, hm), "b64_stream1_motion": lambda: tracked(B, one, hm)})
        groups[1].update({"b1_tracked_motion": lambda: tracked(1, one, hm)})
    if a.legs:
        groups = [{k: v for k, v in g.items() if k in a.legs.split(",")} for g in groups]
        groups = [g for g in groups if g]
    detect(B)
    kept = [int(hd["n_kept"]) for hd, _ in eng.read_slabs(B)]
    lines = [f"track_bench: bf16 YOLOv8n {S} x {S}, max_dets 64, one engine (single chain), device path; {a.steps} steps per leg in {a.blocks} blocks, median block",
             f"detections per frame of the 64 synthetic frames: min {min(kept)}, median {int(np.median(kept))}, max {max(kept)} (stored: at most 64)",
             f"{'leg':<22}{'frames':>7}{'ms/step':>10}{'frames/s':>12}{'over untracked':>16}   blocks (ms/step)"]
    for legs in groups:
        eng.track_reset(-1, 1)
        if eng_m is not None:
            eng_m.track_reset(-1, 1)
        for step in legs.values():
            for _ in range(a.warmup):
                step()
        eng.sync()
        if eng_m is not None:
            eng_m.sync()
        per = {k: [] for k in legs}
        names = list(legs)
        for b in range(a.blocks):
            n = a.steps // a.blocks + (1 if b < a.steps % a.blocks else 0)
            for k in names[b % len(names):] + names[:b % len(names)]:
                sync = eng_m.sync if k.endswith("_motion") else eng.sync
                sync()
                t0 = time.perf_counter()
                for _ in range(n):
                    legs[k]()
                sync()
                per[k].append((time.perf_counter() - t0) / n * 1e3)
        base = float(np.median(per[names[0]]))
        for k in names:
            nf = B if k.startswith("b64") else 1
            ms = float(np.median(per[k]))
            lines.append(f"{k:<22}{nf:>7}{ms:>10.4f}{nf / ms * 1e3:>12.0f}{(ms - base) * 1e3:>+13.1f} us   " + " ".join(f"{x:.4f}" for x in per[k]))
    st = [eng.track_state(s) for s in (0, B - 1)]
    lines.append(f"stream 0 afterwards: {st[0]}; stream {B - 1}: {st[1]}")
    if eng_m is not None:
        st = [eng_m.track_state(s) for s in (0, B - 1)]
        lines.append(f"motion engine, stream 0 afterwards: {st[0]}; stream {B - 1}: {st[1]}")
        eng_m.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    eng.close()


if __name__ == "__main__":
    main()
