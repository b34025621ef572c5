"""How many of the Detect tail's 16-anchor waves survive its early-out -- i.e. run the box half, and with ZLY_TAIL_BOX the box branch's second conv --
on the benchmark's frames: the class logits of a ZLY_FLAG_DUMP_LOGITS engine (the kernel's own fp32 values), cut into the kernel's tiles (16 consecutive
anchors of one level of one frame) and compared with its skip_logit (csrc/head_skip.h: logit(conf_thr) - 1e-2 but for a term that matters next to conf_thr = 1).
usage: surviving_waves.py [thresholds=0.5,0.25,0.1,0.05] [frames=64] [size=416] [scale=n]"""
import math, os, sys
import numpy as np
sys.path[:0] = [os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."), os.path.dirname(os.path.abspath(__file__))]
import zly, zly_model as zm

arg = sys.argv[1:] + [""] * 4
thrs = [float(x) for x in (arg[0] or "0.5,0.25,0.1,0.05").split(",")]
n, size, scale = int(arg[1] or 64), int(arg[2] or 416), arg[3] or "n"
path = None
if scale != "n":
    spec = zm.build_spec(scale)
    path = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"yolov8{scale}_synth.zlyw")
    zm.write_zlyw(path, spec, zm.synth_weights(spec))
B = min(n, 16)
e = zly.Engine(path, model_w=size, model_h=size, max_batch=B, max_dets=64, warmup_runs=0, flags=zly.FLAG_DUMP_LOGITS)
frames = zm.synth_frames(n, size, size, seed=1, rects=False)
tiles = {t: [0, 0, 0] for t in thrs}
passing = {t: 0 for t in thrs}
total = [0, 0, 0]
for f0 in range(0, n, B):
    e.detect_batch(list(frames[f0:f0 + B]))
    for i in range(min(B, n - f0)):
        for l in range(3):
            z = e.tap(f"model.22.cv3.{l}.2", i).reshape(e.nc, -1).max(axis=0)          # best class logit per anchor
            pad = (-len(z)) % 16
            zt = np.concatenate([z, np.full(pad, -np.inf, np.float32)]).reshape(-1, 16).max(axis=1)
            total[l] += len(zt)
            for t in thrs:
                skip = -math.log((1.0 - t) / t + 4.0 * 2.0 ** -24) - 1e-2             # csrc/head_skip.h
                tiles[t][l] += int((zt >= skip).sum())
                passing[t] += int((z >= skip).sum())
e.close()
for t in thrs:
    s = sum(tiles[t]); tot = sum(total)
    print(f"conf {t}: {s} of {tot} waves survive ({s / tot:.4f}; P3 {tiles[t][0] / total[0]:.4f}, P4 {tiles[t][1] / total[1]:.4f}, P5 {tiles[t][2] / total[2]:.4f}), "
          f"{passing[t] / n:.1f} anchors per frame at or above the skip logit", flush=True)
