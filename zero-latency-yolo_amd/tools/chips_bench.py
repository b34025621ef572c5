#!/usr/bin/env python3
"""chips_bench.py -- what cutting target chips on the GPU costs per frame (include/zly.h "Chips"), against doing without it.

On ONE engine (bf16 YOLOv8n 416 x 416, max_dets 64, no head tensor, one chain of launches) with 1920 x 1080 BGRA RESIDENT surfaces, for 1 and for 8
surfaces per call, 16 chips of 64 x 64 (BGR8) per frame, and targets of about 40 x 80 and about 300 x 600 pixels, it times, in ms per frame:

    a_chips     zly_chips_surfaces alone: the two chip kernels (and the one copy of the frame records)
    b_detect    zly_detect_surfaces alone                                                               (what an engine without the option costs)
    b_both      zly_detect_surfaces + zly_chips_surfaces                                                (b_both - b_detect: what the option costs)
    c_host      the only way to the same pixels without it: zly_read_slabs (a synchronisation), zly_surface_read of every surface (8 MB each), then
                the crop and the exact area resize on the host with numpy

The boxes the chips are cut for are hand-written slabs in a device buffer of the tool's (16 targets of the wanted size spread over the surface), so
that the target size is what the arm says; arm b_both's detector writes the engine's own slabs beside them, and arm c reads the same boxes from a host
copy after its zly_read_slabs.  The surfaces hold static pictures: their updates cost every arm the same and are not part of a step.  All arms run in
one process, alternating window by window; every arm is warmed up first; a window is steps of one arm bracketed by a synchronise and lasts at least
--window seconds (host clock); --repeats windows per arm show the spread.  Arm c synchronises in every step by its nature.

--detect-only times b_detect alone and needs nothing of the chips: with --package DIR (a package directory of another commit's build: its zly.py and
_build/) it is how detect alone is measured on the parent commit, in a process of its own, for the comparison DESIGN.md section 5 reports.

    python zero-latency-yolo_amd/tools/chips_bench.py [--window 1.0] [--repeats 5] [--warmup 30] [--detect-only] [--package DIR] [--out profiles/FILE.txt]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch        # noqa: F401  (the process uses torch's HIP runtime throughout, as the tests do)

HERE = os.path.dirname(os.path.abspath(__file__))

SW, SH, MODEL, CHIPS, CW, CH = 1920, 1080, 416, 16, 64, 64
TARGETS = ((40, 80), (300, 600))
DET_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("w", "<f4"), ("h", "<f4"), ("confidence", "<f4"),
                      ("class_id", "<i4"), ("track_id", "<u4"), ("pad_", "<u4"), ("timestamp", "<u8")])


def slab_of(tw, th, cap, scale):
    """one slab of CHIPS boxes whose scaled size is tw x th pixels, spread over the surface"""
    raw = np.zeros(16 + cap * 40, dtype=np.uint8)
    raw[:4] = np.array([CHIPS], dtype="<i4").view(np.uint8)
    d = raw[16:].view(DET_DTYPE)
    for k in range(CHIPS):
        cx = (tw / 2 + (SW - tw) * ((k * 7) % CHIPS) / (CHIPS - 1)) / SW
        cy = (th / 2 + (SH - th) * k / (CHIPS - 1)) / SH
        d[k]["x"], d[k]["y"], d[k]["w"], d[k]["h"], d[k]["confidence"] = cx, cy, tw / SW / scale, th / SH / scale, 0.9
    return raw


def axis_sums(a, axis, D):
    """the area filter of include/zly.h on one axis, exact in int64: the integral of the step function a over each content pixel's interval"""
    a = np.moveaxis(np.asarray(a, dtype=np.int64), axis, 0)
    S = a.shape[0]
    c = np.concatenate([np.zeros_like(a[:1]), np.cumsum(a, axis=0)])
    t = np.arange(D + 1, dtype=np.int64) * S
    q, r = t // D, t % D
    F = D * c[q] + r.reshape((-1,) + (1,) * (a.ndim - 1)) * a[np.minimum(q, S - 1)]
    return np.moveaxis(F[1:] - F[:-1], 0, axis)


def host_chip(bgra, x0, y0, rw, rh):
    crop = bgra[y0:y0 + rh, x0:x0 + rw, :3]
    T = rw * rh
    return ((axis_sums(axis_sums(crop, 1, CW), 0, CH) + (T >> 1)) // T).astype(np.uint8)


def rect_axis(x, w, scale, E):
    f = np.float32
    half = f(f(f(w) * f(scale)) * f(0.5))
    lo, hi = f(f(x) - half), f(f(x) + half)
    c = lambda v: (v if v < 1 else f(1)) if v > 0 else f(0)      # noqa: E731
    a, b = int(f(c(lo) * f(E))), int(f(c(hi) * f(E)))
    a = min(a, E - 1)
    return a, min(max(b, a + 1), E) - a


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=1.0, help="least seconds per timed window")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--detect-only", action="store_true")
    ap.add_argument("--package", default="", help="import zly (and load its _build/) from this package directory instead of this tool's own")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    pkg = os.path.abspath(a.package) if a.package else os.path.dirname(HERE)
    sys.path.insert(0, os.path.join(pkg, "tools"))
    sys.path.insert(0, pkg)
    import zly
    import zly_model as zm

    B, cap, S = 8, 64, 8
    eng = zly.Engine(dtype=zly.DTYPE_BF16, model_w=MODEL, model_h=MODEL, max_batch=B, max_dets=cap, use_graph=True, warmup_runs=1,
                     flags=zly.FLAG_NO_HEAD_TENSOR | zly.FLAG_SINGLE_CHAIN)
    eng.surfaces_enable(S, SW * SH * 4)
    lib, h = eng.lib, eng.h
    whole = zly.view_tight(zly.PIX_BGRA, SW, SH)
    pictures = zm.synth_frames(S, SW, SH, seed=21, rects=True)
    for s in range(S):
        eng.surface_define(s, zly.PIX_BGRA, SW, SH)
        bgra = np.ascontiguousarray(np.concatenate([pictures[s], np.full((SH, SW, 1), 255, np.uint8)], axis=2)).reshape(-1)
        eng.surface_update([(s, 0, 0, bgra, whole)])
    eng.sync()
    scale = 1.25
    if not a.detect_only:
        eng.chips_enable(chip_w=CW, chip_h=CH, max_chips=CHIPS, scale=scale, layout=zly.CHIP_BGR8)

    def ids(n):
        return (C.c_int32 * n)(*range(n))

    def b_detect(n, c_ids):
        zly._check(lib, lib.zly_detect_surfaces(h, n, c_ids, None, None, 0, None))

    lines = [f"chips_bench: bf16 YOLOv8n {MODEL} x {MODEL}, max_dets {cap}, one engine (single chain), resident {SW} x {SH} BGRA surfaces; {CHIPS} chips of "
             f"{CW} x {CH} BGR8 per frame, scale {scale}; windows of >= {a.window} s, {a.repeats} per arm, alternating" + (" [detect only]" if a.detect_only else ""),
             f"{'arm':<10}{'surfaces':>9}{'target':>10}{'ms/frame (median)':>19}{'min':>9}{'max':>9}   windows (ms/frame)"]
    host_slabs = np.zeros(B * eng.slab_bytes, dtype=np.uint8)
    surf_host = np.zeros(SW * SH * 4, dtype=np.uint8)
    for n in (1, S):
        c_ids = ids(n)
        for tw, th in (TARGETS if not a.detect_only else TARGETS[:1]):
            slab = slab_of(tw, th, cap, scale)
            dets = slab[16:].view(DET_DTYPE)[:CHIPS]
            rects = [rect_axis(d["x"], d["w"], scale, SW) + rect_axis(d["y"], d["h"], scale, SH) for d in dets]
            d_slabs = torch.from_numpy(np.tile(slab, n)).cuda()
            torch.cuda.synchronize()

            def a_chips():
                zly._check(lib, lib.zly_chips_surfaces(h, n, c_ids, d_slabs.data_ptr(), 0, None, None))

            def b_both():
                b_detect(n, c_ids)
                a_chips()

            def c_host():
                zly._check(lib, lib.zly_read_slabs(h, n, host_slabs.ctypes.data))
                for s in range(n):
                    zly._check(lib, lib.zly_surface_read(h, s, surf_host.ctypes.data, surf_host.nbytes))
                    img = surf_host.reshape(SH, SW, 4)
                    for x0, rw, y0, rh in rects:
                        host_chip(img, x0, y0, rw, rh)

            arms = {"b_detect": lambda: b_detect(n, c_ids)}
            if not a.detect_only:
                arms.update({"a_chips": a_chips, "b_both": b_both, "c_host": c_host})
            steps_of = {}
            for k, step in arms.items():                     # warm-up, then a short timed run that sizes the arm's windows
                for _ in range(a.warmup if k != "c_host" else 2):
                    step()
                eng.sync()
                t0 = time.perf_counter()
                reps = 20 if k != "c_host" else 2
                for _ in range(reps):
                    step()
                eng.sync()
                steps_of[k] = max(reps, int(a.window / ((time.perf_counter() - t0) / reps) * 1.15) + 1)
            per = {k: [] for k in arms}
            names = list(arms)
            for r in range(a.repeats):
                for k in names[r % len(names):] + names[:r % len(names)]:
                    eng.sync()
                    t0 = time.perf_counter()
                    for _ in range(steps_of[k]):
                        arms[k]()
                    eng.sync()                               # ONE synchronise ends the window: the enqueue-only arms run ahead of the device inside it
                    per[k].append((time.perf_counter() - t0) / (steps_of[k] * n) * 1e3)
            for k in sorted(names):
                v = per[k]
                lines.append(f"{k:<10}{n:>9}{f'{tw}x{th}':>10}{float(np.median(v)):>19.4f}{min(v):>9.4f}{max(v):>9.4f}   " + " ".join(f"{x:.4f}" for x in v))
            if not a.detect_only:
                sizes = sorted({(rw, rh) for _, rw, _, rh in rects})
                lines.append(f"  (rectangles of {sizes[0][0]} x {sizes[0][1]} to {sizes[-1][0]} x {sizes[-1][1]} pixels)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    eng.close()


if __name__ == "__main__":
    main()
