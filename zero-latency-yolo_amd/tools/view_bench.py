#!/usr/bin/env python3
"""view_bench.py -- what a frame view costs on the device path (include/zly.h zly_frame_view).

On ONE engine (bf16 YOLOv8n 416 x 416, batch 64 by default) it times, with bench.py's block structure (warm-up, then consecutive timed blocks
bracketed by a synchronize; the median block counts):

    tight   zly_detect_device       on `batch` tight model-sized BGR frames
    view    zly_detect_device_view  on `batch` model-sized windows of `batch` 1920 x 1080 BGR surfaces with a padded row pitch
                                    (3 * 1920 + 128), one window per surface around its centre -- the same number of pixel bytes

The two legs alternate block by block, so that clock ramps and neighbours on the box hit both alike.  It also reports the device time of the
front launch of either leg from the engine's production sampling (zly_get_stats: every 16th call is bracketed by events around the front
kernel), and checks that both legs give the same slabs (the windows hold the tight frames' pixels).

    python zero-latency-yolo_amd/tools/view_bench.py [--batch 64] [--steps 400] [--warmup 40] [--blocks 10] [--out FILE]
"""
import argparse
import json
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
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=400, help="timed steps per leg")
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    B, S = a.batch, a.size
    W, H, pitch = 1920, 1080, 1920 * 3 + 128
    x0, y0 = (W - S) // 2, (H - S) // 2

    frames = zm.synth_frames(B, S, S, seed=11, rects=True)                      # [B][S][S][3]
    tight = np.ascontiguousarray(frames).reshape(-1)
    surf = np.random.default_rng(5).integers(0, 256, (B, H, pitch), dtype=np.uint8)
    surf[:, y0:y0 + S, 3 * x0:3 * (x0 + S)] = frames.reshape(B, S, 3 * S)
    surf = surf.reshape(-1)
    whole = zly.FrameView()
    whole.fmt, whole.w, whole.h = zly.PIX_BGR, W, H
    whole.pitch[0] = pitch
    views = []
    for i in range(B):
        v = zly.view_crop(whole, x0, y0, S, S)
        v.off[0] += i * H * pitch
        views.append(v)
    d_tight = torch.from_numpy(tight).cuda()
    d_surf = torch.from_numpy(surf).cuda()
    torch.cuda.synchronize()

    eng = zly.Engine(dtype=zly.DTYPE_BF16, model_w=S, model_h=S, max_batch=B, max_dets=128, use_graph=True, warmup_runs=1,
                     flags=zly.FLAG_NO_HEAD_TENSOR | zly.FLAG_SINGLE_CHAIN)
    cviews = (zly.FrameView * B)(*views)
    lib, h = eng.lib, eng.h

    def step_tight():
        zly._check(lib, lib.zly_detect_device(h, B, d_tight.data_ptr(), S, S, None, 0, None))

    def step_view():
        zly._check(lib, lib.zly_detect_device_view(h, B, d_surf.data_ptr(), surf.nbytes, cviews, None, 0, None))

    # same pixels -> same slabs
    step_tight(); want = eng.read_slabs(B)
    step_view(); got = eng.read_slabs(B)
    fields = ["x", "y", "w", "h", "confidence", "class_id"]
    same = all(int(hw["n_kept"]) == int(hg["n_kept"]) and dw[fields].tobytes() == dg[fields].tobytes() for (hw, dw), (hg, dg) in zip(want, got))
    if not same:
        raise SystemExit("view_bench: the view leg's slabs differ from the tight leg's")

    def front_ms(step, calls=160):
        """mean device ms of the front launch per call (per batch), from the engine's sampled phase timing"""
        s0 = eng.stats()
        for _ in range(calls):
            step()
        eng.sync()
        s1 = eng.stats()
        fr = s1["sampled_frames"] - s0["sampled_frames"]
        return (s1["sampled_preprocess_ms"] - s0["sampled_preprocess_ms"]) / fr * B if fr else float("nan")

    legs = {"tight": step_tight, "view": step_view}
    for step in legs.values():
        for _ in range(a.warmup):
            step()
    eng.sync()
    per = {k: [] for k in legs}
    for b in range(a.blocks):
        n = a.steps // a.blocks + (1 if b < a.steps % a.blocks else 0)
        for k in (("tight", "view") if b % 2 == 0 else ("view", "tight")):
            eng.sync()
            t0 = time.perf_counter()
            for _ in range(n):
                legs[k]()
            eng.sync()
            per[k].append((time.perf_counter() - t0) / n * 1e3)
    res = {"tool": "view_bench", "batch": B, "size": S, "surface": [W, H], "pitch": pitch, "window_origin": [x0, y0],
           "steps_per_leg": a.steps, "blocks": a.blocks, "slabs_equal": same,
           "front_kernel": eng.op_kernels(B)[1]}
    for k in legs:
        res[f"{k}_ms_per_step"] = round(float(np.median(per[k])), 5)
        res[f"{k}_blocks_ms_per_step"] = [round(x, 5) for x in per[k]]
        res[f"{k}_frames_per_s"] = round(B / float(np.median(per[k])) * 1e3, 1)
    res["view_over_tight"] = round(res["view_ms_per_step"] / res["tight_ms_per_step"], 4)
    res["tight_front_launch_ms"] = round(front_ms(step_tight), 5)
    res["view_front_launch_ms"] = round(front_ms(step_view), 5)
    res["tight_front_launch_ms_profile_ops"] = round(float(eng.profile_ops(d_tight.data_ptr(), B, S, S, reps=20)[1]), 5)      # an event pair per launch, no graph
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
