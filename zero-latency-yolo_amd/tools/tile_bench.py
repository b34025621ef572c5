#!/usr/bin/env python3
"""tile_bench.py -- what merging a surface's tiles costs on the device path (include/zly.h "Tiles": zly_merge_slabs behind zly_detect_device_view).

On ONE engine at the headline configuration (bf16 YOLOv8n 416 x 416, max_dets 64, no head tensor, one chain of launches) it times, with bench.py's
block structure (warm-up, then consecutive timed blocks bracketed by a synchronize; the median block counts):

    t8              zly_detect_device_view on the 8 overlapping 416 x 416 tiles of one 1472 x 768 surface       (the unmerged step)
    t8_merge        the same + zly_merge_slabs, one group
    t8_merge_track  the same + zly_track_slabs on the merged slab, one stream
    t64             zly_detect_device_view on the 64 tiles of 8 such surfaces
    t64_merge       the same + zly_merge_slabs, 8 groups of 8 tiles
    t64_merge_track the same + zly_track_slabs on the 8 merged slabs, 8 streams
    merge_M*        zly_merge_slabs alone on crafted slabs of about 50, 512 and exactly 4096 candidates in one group (8, 8 and 64 tiles), back to
                    back in one stream: the table upload and the launch, with nothing to hide behind

The legs of one group alternate block by block, so that clock ramps and neighbours on the box hit all alike.  Writes one text file.

    python zero-latency-yolo_amd/tools/tile_bench.py [--steps 300] [--warmup 40] [--blocks 10] [--legs t8,t8_merge] [--out profiles/FILE.txt]
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

SW, SH, TILE, OVERLAP = 1472, 768, 416, 64        # 4 x 2 tiles


def crafted_slabs(tiles, cap, per_tile, n_objects, seed):
    """u8 [len(tiles)][slab_bytes]: random objects on the tiles' surface; a tile stores the part it sees of the first per_tile objects it sees"""
    rng = np.random.default_rng(seed)
    W, H = tiles[0].W, tiles[0].H
    cx, cy = rng.uniform(0, W, n_objects), rng.uniform(0, H, n_objects)
    bw, bh = rng.uniform(.05, .5, n_objects) * tiles[0].w, rng.uniform(.05, .5, n_objects) * tiles[0].h
    cls = rng.integers(0, 4, n_objects)
    sb = zly.SLAB_HDR_DTYPE.itemsize + cap * zly.DET_DTYPE.itemsize
    raw = np.zeros((len(tiles), sb), dtype=np.uint8)
    for i, t in enumerate(tiles):
        x0, x1 = np.maximum(cx - bw / 2, t.x0), np.minimum(cx + bw / 2, t.x0 + t.w)
        y0, y1 = np.maximum(cy - bh / 2, t.y0), np.minimum(cy + bh / 2, t.y0 + t.h)
        vis = np.flatnonzero((x1 - x0 > 2) & (y1 - y0 > 2))
        conf = rng.uniform(.3, .99, len(vis))
        order = sorted(range(len(vis)), key=lambda k: (cls[vis[k]], -conf[k]))[:min(per_tile, cap)]
        d = raw[i, 16:].view(zly.DET_DTYPE)
        for k, j in enumerate(order):
            o = vis[j]
            d[k]["x"], d[k]["y"] = ((x0[o] + x1[o]) / 2 - t.x0) / t.w, ((y0[o] + y1[o]) / 2 - t.y0) / t.h
            d[k]["w"], d[k]["h"] = (x1[o] - x0[o]) / t.w, (y1[o] - y0[o]) / t.h
            d[k]["confidence"], d[k]["class_id"] = conf[j], cls[o]
        raw[i, :16].view(zly.SLAB_HDR_DTYPE)["n_kept"] = len(order)
    return raw


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300, help="timed steps per leg")
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--legs", default="", help="comma-separated subset of the legs")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    B, cap = 64, 64
    grid = zly.tile_grid(SW, SH, TILE, TILE, OVERLAP, OVERLAP)
    assert len(grid) == 8
    surfaces = np.ascontiguousarray(zm.synth_frames(8, SW, SH, seed=11, rects=True))          # 8 clients' surfaces, one behind the other
    d_buf = torch.from_numpy(surfaces.reshape(-1)).cuda()
    views, tiles = [], []
    for g in range(8):
        surf = zly.view_tight(zly.PIX_BGR, SW, SH)
        surf.off[0] = g * SW * SH * 3
        for t in grid:
            views.append(zly.view_crop(surf, t.x0, t.y0, t.w, t.h))
            tiles.append(zly.tile(t.x0, t.y0, t.w, t.h, SW, SH, group=g))
    eng = zly.Engine(dtype=zly.DTYPE_BF16, model_w=TILE, model_h=TILE, max_batch=B, max_dets=cap, use_graph=True, warmup_runs=1,
                     flags=zly.FLAG_NO_HEAD_TENSOR | zly.FLAG_SINGLE_CHAIN)
    eng.track_enable(max_streams=8, max_tracks=64)
    lib, h = eng.lib, eng.h
    d_out = torch.zeros(8 * eng.slab_bytes, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    cv, ct = (zly.FrameView * B)(*views), (zly.Tile * B)(*tiles)
    cfg = zly.merge_config()
    streams = (C.c_int32 * 8)(*range(8))

    def detect(n):
        zly._check(lib, lib.zly_detect_device_view(h, n, d_buf.data_ptr(), d_buf.numel(), cv, None, 0, None))

    def merged(n, track):
        detect(n)
        zly._check(lib, lib.zly_merge_slabs(h, n, ct, n // 8, C.byref(cfg), None, d_out.data_ptr(), 0, None))
        if track:
            zly._check(lib, lib.zly_track_slabs(h, n // 8, streams, d_out.data_ptr(), None))

    # the merge alone: a fresh engine that has made no call merges caller-made slabs
    alone = zly.Engine(dtype=zly.DTYPE_BF16, model_w=64, model_h=64, max_batch=B, max_dets=cap, use_graph=False, warmup_runs=0)
    big_grid = zly.tile_grid(8 * 352 + 64, 8 * 352 + 64, TILE, TILE, OVERLAP, OVERLAP)
    assert len(big_grid) == 64
    crafted = {"merge_M50": crafted_slabs(grid, cap, 7, 60, 1), "merge_M512": crafted_slabs(grid, cap, 64, 3000, 2),
               "merge_M4096": crafted_slabs(big_grid, cap, 64, 40000, 3)}
    d_src = {k: torch.from_numpy(v).cuda() for k, v in crafted.items()}
    c_tiles = {k: (zly.Tile * len(v))(*(grid if len(v) == 8 else big_grid)) for k, v in crafted.items()}
    d_alone = torch.zeros(alone.slab_bytes, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def merge_alone(k):
        zly._check(lib, lib.zly_merge_slabs(alone.h, len(crafted[k]), c_tiles[k], 1, C.byref(cfg), d_src[k].data_ptr(), d_alone.data_ptr(), 0, None))

    groups = [
        (eng, {"t8": lambda: detect(8), "t8_merge": lambda: merged(8, False), "t8_merge_track": lambda: merged(8, True)}),
        (eng, {"t64": lambda: detect(64), "t64_merge": lambda: merged(64, False), "t64_merge_track": lambda: merged(64, True)}),
        (alone, {k: (lambda k=k: merge_alone(k)) for k in crafted}),
    ]
    if a.legs:
        groups = [(e, {k: v for k, v in g.items() if k in a.legs.split(",")}) for e, g in groups]
        groups = [(e, g) for e, g in groups if g]
    detect(64)
    kept = [int(hd["n_kept"]) for hd, _ in eng.read_slabs(64)]
    merged(64, False)
    eng.sync()
    mk = np.frombuffer(d_out.cpu().numpy().tobytes(), dtype=np.uint8).reshape(8, eng.slab_bytes)
    mh = [mk[g, :16].view(zly.SLAB_HDR_DTYPE)[0] for g in range(8)]
    lines = [f"tile_bench: bf16 YOLOv8n {TILE} x {TILE}, max_dets {cap}, one engine (single chain), device path on views of {SW} x {SH} surfaces "
             f"({len(grid)} tiles of {TILE}, overlap {OVERLAP}); merge: IoS at 0.5; {a.steps} steps per leg in {a.blocks} blocks, median block",
             f"detections per tile of the 64 synthetic tiles: min {min(kept)}, median {int(np.median(kept))}, max {max(kept)}; per surface: "
             f"candidates {[int(x['n_candidates']) for x in mh]}, merged {[int(x['n_kept']) for x in mh]}",
             f"{'leg':<18}{'tiles':>6}{'ms/step':>10}{'tiles/s':>11}{'over first leg':>16}   blocks (ms/step)"]
    for e, legs in groups:
        if e is eng:
            eng.track_reset(-1, 1)
        for step in legs.values():
            for _ in range(a.warmup):
                step()
        e.sync()
        per = {k: [] for k in legs}
        names = list(legs)
        for b in range(a.blocks):
            n = a.steps // a.blocks + (1 if b < a.steps % a.blocks else 0)
            for k in names[b % len(names):] + names[:b % len(names)]:
                e.sync()
                t0 = time.perf_counter()
                for _ in range(n):
                    legs[k]()
                e.sync()
                per[k].append((time.perf_counter() - t0) / n * 1e3)
        base = float(np.median(per[names[0]]))
        for k in names:
            nt = 8 if k.startswith("t8") else 64 if k.startswith("t64") else len(crafted[k])
            ms = float(np.median(per[k]))
            over = f"{(ms - base) * 1e3:>+13.1f} us" if e is eng else f"{'':>16}"
            lines.append(f"{k:<18}{nt:>6}{ms:>10.4f}{nt / ms * 1e3:>11.0f}{over}   " + " ".join(f"{x:.4f}" for x in per[k]))
    for k in crafted:
        merge_alone(k)
        alone.sync()
        hd = d_alone.cpu().numpy()[:16].view(zly.SLAB_HDR_DTYPE)[0]
        lines.append(f"{k}: {int(hd['n_candidates'])} candidates, {int(hd['n_kept'])} survivors")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    alone.close()
    eng.close()


if __name__ == "__main__":
    main()
