#!/usr/bin/env python3
"""camera_bench.py -- what the camera motion estimate costs per frame (include/zly.h "Camera motion"), beside a change call in the same sitting.

On ONE engine (bf16 YOLOv8n 416 x 416, max_dets 64, no head tensor, one chain of launches) with 1920 x 1080 BGRA RESIDENT surfaces, camera cells of
16 and a radius of 4, for 1 and for 8 surfaces per call, it times, in ms per frame:

    a_camera        zly_camera_surfaces alone: the sums kernel, the search, the pick and the copy of the call's frame records
    b_camera_apply  zly_camera_surfaces, then zly_camera_apply_tracks on the same streams
    c_change        zly_change_surfaces alone, at the change map's defaults (cells of 32), as tools/change_bench.py's arm a_change

Every stream has TWO resident surfaces, cut from one picture 24 pixels apart, and every arm alternates between them from step to step: the search
sees a pan of one and a half cells in every frame.  The surfaces' updates are not part of a step.  a_camera is also given as a multiple of the time
to read the frames' bytes once at the copy bandwidth of profiles/r01_copy_bandwidth.txt (7.0 TB/s of traffic).  All arms run in one process,
alternating window by window; every arm is warmed up first; a window is steps of one arm bracketed by a synchronise and lasts at least --window
seconds (host clock); --repeats windows per arm show the spread.  --arms NAMES times the named arms alone (a kernel trace is taken that way).

    python zero-latency-yolo_amd/tools/camera_bench.py [--window 1.0] [--repeats 5] [--warmup 30] [--arms a,b] [--out profiles/FILE.txt]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch        # noqa: F401  (the process uses torch's HIP runtime throughout, as the tests do)

HERE = os.path.dirname(os.path.abspath(__file__))

SW, SH, TILE, CELL, RADIUS, PAN = 1920, 1080, 416, 16, 4, 24
COPY_TBPS = 7.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=1.0, help="least seconds per timed window")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--arms", default="", help="comma-separated arm names: time these alone (a kernel trace, say)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    pkg = os.path.dirname(HERE)
    sys.path.insert(0, os.path.join(pkg, "tools"))
    sys.path.insert(0, pkg)
    import zly
    import zly_model as zm

    B, cap, S = 64, 64, 8
    eng = zly.Engine(dtype=zly.DTYPE_BF16, model_w=TILE, model_h=TILE, max_batch=B, max_dets=cap, use_graph=True, warmup_runs=1,
                     flags=zly.FLAG_NO_HEAD_TENSOR | zly.FLAG_SINGLE_CHAIN)
    eng.track_enable(max_streams=S, max_tracks=64)
    eng.surfaces_enable(2 * S, SW * SH * 4)
    eng.camera_enable(S, cell=CELL, radius=RADIUS)
    eng.change_enable(S)
    lib, h = eng.lib, eng.h
    whole = zly.view_tight(zly.PIX_BGRA, SW, SH)
    pictures = zm.synth_frames(S, SW + PAN, SH, seed=21, rects=True)
    for s in range(S):
        for alt in (0, 1):                                   # slot s and slot S + s: the stream's picture, and the same PAN pixels further on
            pic = pictures[s][:, PAN * alt:PAN * alt + SW]
            eng.surface_define(s + S * alt, zly.PIX_BGRA, SW, SH)
            bgra = np.ascontiguousarray(np.concatenate([pic, np.full((SH, SW, 1), 255, np.uint8)], axis=2)).reshape(-1)
            eng.surface_update([(s + S * alt, 0, 0, bgra, whole)])
    eng.sync()
    # a table of tracks per stream for the apply to move: one tracked call on crafted slabs
    slabs = np.zeros((S, eng.slab_bytes), dtype=np.uint8)
    for s in range(S):
        slabs[s, :16].view(zly.SLAB_HDR_DTYPE)["n_kept"] = 16
        d = slabs[s, 16:].view(zly.DET_DTYPE)
        d["x"][:16], d["y"][:16], d["w"][:16], d["h"][:16], d["confidence"][:16] = np.linspace(0.1, 0.9, 16), 0.5, 0.03, 0.05, 0.9
    d_slabs = torch.from_numpy(slabs.reshape(-1)).cuda()
    torch.cuda.synchronize()
    eng.track_slabs(list(range(S)), d_slabs.data_ptr())
    eng.sync()
    tick = [0]

    def ids(n, alt=0):
        return (C.c_int32 * n)(*range(S * alt, S * alt + n))

    def a_camera(n, slots, streams):
        zly._check(lib, lib.zly_camera_surfaces(h, n, slots, streams, None))

    def b_camera_apply(n, slots, streams):
        zly._check(lib, lib.zly_camera_surfaces(h, n, slots, streams, None))
        zly._check(lib, lib.zly_camera_apply_tracks(h, n, streams, None))

    def c_change(n, slots, streams):
        zly._check(lib, lib.zly_change_surfaces(h, n, slots, streams, None))

    lines = [f"camera_bench: bf16 YOLOv8n {TILE} x {TILE}, max_dets {cap}, one engine (single chain), resident {SW} x {SH} BGRA surfaces, two pictures per stream "
             f"{PAN} pixels apart in turn; camera cells of {CELL}, radius {RADIUS}; change map at its defaults; windows of >= {a.window} s, {a.repeats} per arm, alternating",
             f"{'arm':<15}{'surfaces':>9}{'ms/frame (median)':>19}{'min':>9}{'max':>9}   windows (ms/frame)"]
    for n in (1, S):
        slots, streams = (ids(n, 0), ids(n, 1)), ids(n)

        def alternating(fn):
            def step():
                tick[0] ^= 1
                fn(n, slots[tick[0]], streams)
            return step

        arms = {"a_camera": alternating(a_camera), "b_camera_apply": alternating(b_camera_apply), "c_change": alternating(c_change)}
        if a.arms:
            arms = {k: v for k, v in arms.items() if k in a.arms.split(",")}
        steps_of = {}
        for k, step in arms.items():                         # warm-up, then a short timed run that sizes the arm's windows
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
        for r in range(a.repeats):
            for k in names[r % len(names):] + names[:r % len(names)]:
                step = arms[k]
                eng.sync()
                t0 = time.perf_counter()
                for _ in range(steps_of[k]):
                    step()
                eng.sync()                                   # ONE synchronise ends the window: the arms run ahead of the device inside it
                per[k].append((time.perf_counter() - t0) / (steps_of[k] * n) * 1e3)
        for k in sorted(names):
            v = per[k]
            lines.append(f"{k:<15}{n:>9}{float(np.median(v)):>19.4f}{min(v):>9.4f}{max(v):>9.4f}   " + " ".join(f"{x:.4f}" for x in v))
        if "a_camera" in per:
            bound = SW * SH * 4 / (COPY_TBPS * 1e12) * 1e3
            med = float(np.median(per["a_camera"]))
            hdr, _ = zly.parse_camera_record(eng.camera_read(0), RADIUS)
            lines.append(f"  ({n} surfaces: a_camera is {med / bound:.1f} x the {bound:.5f} ms that reading a frame's {SW * SH * 4} bytes once takes at {COPY_TBPS} TB/s; "
                         f"stream 0's last frame: shift ({int(hdr['sx_q4']) / 16:+.2f}, {int(hdr['sy_q4']) / 16:+.2f}) px, flags {int(hdr['flags'])}, "
                         f"sad_min {int(hdr['sad_min'])}, sad_zero {int(hdr['sad_zero'])}, n_applied {int(hdr['n_applied'])})")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    eng.close()


if __name__ == "__main__":
    main()
