#!/usr/bin/env python3
"""area_bench.py -- what the area-average resize filter (include/zly.h ZLY_FLAG_AREA) costs on the device path.

Two engines in one process (bf16 YOLOv8n 416 x 416, bench.py's flags), the plain one and the same with ZLY_FLAG_AREA, at batch 64 and at batch 1,
on device-resident frames of three shapes:

    bgra1080   1920 x 1080 BGRA   (a desktop capture: 8.3 MB per frame)
    nv12_1080  1920 x 1080 NV12   (a decoder surface: 3.1 MB per frame)
    bgr_model  model-sized BGR    (the pre-pass is then the identity: what it costs where it buys nothing)

Per shape the two engines alternate block by block (warm-up, then consecutive timed blocks bracketed by a synchronize; the median block counts),
so that clock ramps and neighbours on the box hit both alike.  Reported per shape and batch size:

    plain / area ms per step, and their difference
    front phase of either engine: device ms of everything the engine books as "preprocess" (zly_get_stats: every 16th call is bracketed by
        events) -- the front kernel on the plain engine, the pre-pass plus the front kernel on the area engine
    prepass_ms    the pre-pass alone: the area engine's front phase minus the front phase of the plain engine on MODEL-SIZED BGR frames of the
                  same batch size, which is the launch the area engine's front kernel is (same kernel, same input size)
    prepass_gbs   the source bytes of the batch divided by prepass_ms
    copy_gbs      a device-to-device copy of the same source bytes (torch copy_, events, median of 20), as bytes copied per second -- a copy
                  reads AND writes them, the pre-pass only reads them -- timed in the same run; prepass_share = prepass_gbs / copy_gbs

    python zero-latency-yolo_amd/tools/area_bench.py [--steps 200] [--warmup 20] [--blocks 10] [--out FILE]
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


def _frames(shape, B, S):
    """(u8 device tensor of B frames, fmt, w, h)"""
    if shape == "bgr_model":
        f = zm.synth_frames(min(B, 8), S, S, seed=11, rects=True)
        return np.ascontiguousarray(np.stack([f[i % len(f)] for i in range(B)])).reshape(-1), zly.PIX_BGR, S, S
    W, H = 1920, 1080
    base = zm.synth_frames(min(B, 4), W, H, seed=13, rects=True)
    if shape == "bgra1080":
        one = [np.concatenate([b, np.full((H, W, 1), 255, np.uint8)], axis=2).reshape(-1) for b in base]
        fmt = zly.PIX_BGRA
    else:
        # luma from the picture's green channel, flat chroma: the bytes' values do not change what the kernels cost
        one = [np.concatenate([b[:, :, 1].reshape(-1), np.full(W * H // 2, 128, np.uint8)]) for b in base]
        fmt = zly.PIX_NV12_BT601
    return np.ascontiguousarray(np.concatenate([one[i % len(one)] for i in range(B)])), fmt, W, H


def _copy_gbs(d):
    """bytes copied per second of a device-to-device copy of d (GB/s), median of 20"""
    dst = torch.empty_like(d)
    for _ in range(3):
        dst.copy_(d)
    ts = []
    for _ in range(20):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        dst.copy_(d)
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    del dst
    return d.numel() / (float(np.median(ts)) * 1e-3) / 1e9


def _front_ms(eng, step, B, calls=160):
    """mean device ms per call of what the engine books as preprocess, from its sampled phase timing"""
    s0 = eng.stats()
    for _ in range(calls):
        step()
    eng.sync()
    s1 = eng.stats()
    fr = s1["sampled_frames"] - s0["sampled_frames"]
    return (s1["sampled_preprocess_ms"] - s0["sampled_preprocess_ms"]) / fr * B if fr else float("nan")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200, help="timed steps per leg")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--batches", default="64,1")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    S = a.size
    lines = []
    for B in [int(x) for x in a.batches.split(",")]:
        base_flags = zly.FLAG_NO_HEAD_TENSOR | zly.FLAG_SINGLE_CHAIN
        engines = {"plain": zly.Engine(dtype=zly.DTYPE_BF16, model_w=S, model_h=S, max_batch=B, max_dets=128, use_graph=True, warmup_runs=1, flags=base_flags),
                   "area": zly.Engine(dtype=zly.DTYPE_BF16, model_w=S, model_h=S, max_batch=B, max_dets=128, use_graph=True, warmup_runs=1,
                                      flags=base_flags | zly.FLAG_AREA)}
        plain_model_front = None
        for shape in ("bgr_model", "bgra1080", "nv12_1080"):          # bgr_model first: its plain front phase is the front kernel every pre-pass figure subtracts
            host, fmt, w, h = _frames(shape, B, S)
            d = torch.from_numpy(host).cuda()
            torch.cuda.synchronize()
            legs = {k: (lambda e=e: e.detect_device(d.data_ptr(), B, w, h, fmt=fmt)) for k, e in engines.items()}
            for k, step in legs.items():
                for _ in range(a.warmup):
                    step()
                engines[k].sync()
            per = {k: [] for k in legs}
            for b in range(a.blocks):
                n = a.steps // a.blocks + (1 if b < a.steps % a.blocks else 0)
                for k in (("plain", "area") if b % 2 == 0 else ("area", "plain")):
                    engines[k].sync()
                    t0 = time.perf_counter()
                    for _ in range(n):
                        legs[k]()
                    engines[k].sync()
                    per[k].append((time.perf_counter() - t0) / n * 1e3)
            res = {"tool": "area_bench", "batch": B, "size": S, "shape": shape, "frame": [w, h], "source_bytes": int(host.nbytes),
                   "steps_per_leg": a.steps, "blocks": a.blocks, "front_kernel": engines["area"].op_kernels(B)[1]}
            for k in legs:
                res[f"{k}_ms_per_step"] = round(float(np.median(per[k])), 5)
                res[f"{k}_blocks_ms_per_step"] = [round(x, 5) for x in per[k]]
            res["area_minus_plain_ms_per_step"] = round(res["area_ms_per_step"] - res["plain_ms_per_step"], 5)
            front = {k: _front_ms(engines[k], legs[k], B) for k in legs}
            if shape == "bgr_model":
                plain_model_front = front["plain"]
            res["plain_front_phase_ms"] = round(front["plain"], 5)
            res["area_front_phase_ms"] = round(front["area"], 5)
            res["front_kernel_alone_ms"] = round(plain_model_front, 5)
            pre = front["area"] - plain_model_front
            res["prepass_ms"] = round(pre, 5)
            res["prepass_gbs"] = round(host.nbytes / (pre * 1e-3) / 1e9, 1) if pre > 0 else None
            res["copy_gbs"] = round(_copy_gbs(d), 1)
            res["prepass_share_of_copy"] = round(res["prepass_gbs"] / res["copy_gbs"], 3) if res["prepass_gbs"] else None
            line = json.dumps(res)
            print(line, flush=True)
            lines.append(line)
            del d
            torch.cuda.empty_cache()
        for e in engines.values():
            e.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
