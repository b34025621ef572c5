#!/usr/bin/env python3
"""pixfmt_bench.py -- what a frame's pixel format costs on the device path (include/zly.h ZLY_PIX_*).

On ONE engine (bf16 YOLOv8n 416 x 416, batch 64 by default, captured graphs, bench.py's engine flags) it runs zly_detect_device_fmt on `batch`
model-sized frames resident in HBM, once per format, the same synthetic pictures in every format:

    bgr                 the headline path (12-byte quad loads)
    nv12, i420          YUV 4:2:0 made from the pictures by a float transform (only the content of the requests matters here)
    rgb, bgra, rgba     the pictures' bytes permuted / padded with a fourth byte
    yuy2, uyvy          packed YUV 4:2:2 (capture cards, UVC devices) holding the nv12 frame's samples, each chroma row twice: 2 bytes per pixel, one
                        load per pixel, and exactly nv12's pixels after conversion, so that everything behind the front launch does nv12's work

The formats alternate block by block (bench.py's block structure: warm-up, then timed blocks bracketed by a synchronize, the median block counts),
so that clock ramps and neighbours on the box hit all alike.  Per format it reports the step time and the device time of the FRONT launch from the
engine's production sampling (zly_get_stats: every 16th call is bracketed by events around the front kernel).  ZLY_LIB selects the library, so
the same command measures another build of the engine on the same box (give it --formats it knows).

    python zero-latency-yolo_amd/tools/pixfmt_bench.py [--formats bgr,nv12,rgb,bgra,rgba] [--batch 64] [--steps 400] [--blocks 10] [--out FILE]
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

FORMATS = {"bgr": zly.PIX_BGR, "nv12": zly.PIX_NV12_BT601, "i420": zly.PIX_I420_BT601, "rgb": zly.PIX_RGB, "bgra": zly.PIX_BGRA, "rgba": zly.PIX_RGBA,
           "yuy2": zly.PIX_YUY2_BT601, "uyvy": zly.PIX_UYVY_BT601, "yuy2_709": zly.PIX_YUY2_BT709, "uyvy_709": zly.PIX_UYVY_BT709}


def to_format(bgr, name):
    """[B][S][S][3] BGR pictures -> flat u8 buffer of B tight frames of the named format"""
    B, H, W, _ = bgr.shape
    if name == "bgr":
        return np.ascontiguousarray(bgr).reshape(-1)
    if name == "rgb":
        return np.ascontiguousarray(bgr[..., ::-1]).reshape(-1)
    if name in ("bgra", "rgba"):
        out = np.empty((B, H, W, 4), np.uint8)
        out[..., :3] = bgr if name == "bgra" else bgr[..., ::-1]
        out[..., 3] = np.random.default_rng(3).integers(0, 256, (B, H, W), dtype=np.uint8)
        return out.reshape(-1)
    f = bgr.astype(np.float32)
    b, g, r = f[..., 0], f[..., 1], f[..., 2]
    y = 16 + 0.257 * r + 0.504 * g + 0.098 * b
    u8 = lambda a: np.clip(np.rint(a), 0, 255).astype(np.uint8)     # noqa: E731
    if name.startswith(("yuy2", "uyvy")):                          # chroma = nv12's (the mean of each 2 x 2 block) on both rows; Y0 U Y1 V or U Y0 V Y1
        cb = np.repeat((128 - 0.148 * r - 0.291 * g + 0.439 * b).reshape(B, H // 2, 2, W // 2, 2).mean(axis=(2, 4)), 2, axis=1)
        cr = np.repeat((128 + 0.439 * r - 0.368 * g - 0.071 * b).reshape(B, H // 2, 2, W // 2, 2).mean(axis=(2, 4)), 2, axis=1)
        yy = u8(y).reshape(B, H, W // 2, 2)
        order = [yy[..., 0], u8(cb), yy[..., 1], u8(cr)] if name.startswith("yuy2") else [u8(cb), yy[..., 0], u8(cr), yy[..., 1]]
        return np.ascontiguousarray(np.stack(order, axis=-1)).reshape(-1)
    cb = (128 - 0.148 * r - 0.291 * g + 0.439 * b).reshape(B, H // 2, 2, W // 2, 2).mean(axis=(2, 4))
    cr = (128 + 0.439 * r - 0.368 * g - 0.071 * b).reshape(B, H // 2, 2, W // 2, 2).mean(axis=(2, 4))
    chroma = np.stack([u8(cb), u8(cr)], axis=-1) if name == "nv12" else np.stack([u8(cb), u8(cr)], axis=1)
    return np.concatenate([u8(y).reshape(B, -1), chroma.reshape(B, -1)], axis=1).reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--formats", default="bgr,nv12,rgb,bgra,rgba")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=400, help="timed steps per format")
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    B, S = a.batch, a.size
    names = [n for n in a.formats.split(",") if n]
    pictures = zm.synth_frames(B, S, S, seed=11, rects=True)
    dev = {}
    for n in names:
        host = to_format(pictures, n)
        assert host.nbytes == B * zly.frame_bytes(FORMATS[n], S, S), n
        dev[n] = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    eng = zly.Engine(dtype=zly.DTYPE_BF16, model_w=S, model_h=S, max_batch=B, max_dets=128, use_graph=True, warmup_runs=1,
                     flags=zly.FLAG_NO_HEAD_TENSOR | zly.FLAG_SINGLE_CHAIN)
    lib, h = eng.lib, eng.h

    def step(n):
        zly._check(lib, lib.zly_detect_device_fmt(h, FORMATS[n], B, dev[n].data_ptr(), S, S, None, 0, None))

    def front_ms(n, calls=320):
        """mean device ms of the front launch per call (per batch), from the engine's sampled phase timing"""
        s0 = eng.stats()
        for _ in range(calls):
            step(n)
        eng.sync()
        s1 = eng.stats()
        fr = s1["sampled_frames"] - s0["sampled_frames"]
        return (s1["sampled_preprocess_ms"] - s0["sampled_preprocess_ms"]) / fr * B if fr else float("nan")

    for n in names:
        for _ in range(a.warmup):
            step(n)
    eng.sync()
    per = {n: [] for n in names}
    for b in range(a.blocks):
        k = a.steps // a.blocks + (1 if b < a.steps % a.blocks else 0)
        for n in (names if b % 2 == 0 else names[::-1]):
            eng.sync()
            t0 = time.perf_counter()
            for _ in range(k):
                step(n)
            eng.sync()
            per[n].append((time.perf_counter() - t0) / k * 1e3)
    res = {"tool": "pixfmt_bench", "lib": os.environ.get("ZLY_LIB", "default"), "batch": B, "size": S, "steps_per_format": a.steps, "blocks": a.blocks,
           "front_kernel": eng.op_kernels(B)[1], "formats": {}}
    for n in names:
        med = float(np.median(per[n]))
        res["formats"][n] = {"ms_per_step": round(med, 5), "frames_per_s": round(B / med * 1e3, 1),
                             "blocks_ms_per_step": [round(x, 5) for x in per[n]]}
    for rep in range(2):                                    # twice, in opposite orders: the spread of the sampled front-launch time itself
        for n in (names if rep == 0 else names[::-1]):
            res["formats"][n].setdefault("front_launch_ms", []).append(round(front_ms(n), 5))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
