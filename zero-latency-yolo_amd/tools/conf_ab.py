"""The headline steps (three ZLY_FLAG_SINGLE_CHAIN engines fed alternate batch-64 steps, as multi_engine.py and bench.py run them) at a given
confidence threshold, which bench.py does not expose: ZLY_TAIL_BOX=0 against the automatic mode, arms alternating, to place ZLY_TAIL_BOX_MIN_CONF.
Also prints what the engine passes at that threshold: candidates per frame and kept detections per frame of the last step.
usage: conf_ab.py [thresholds=0.5,0.25,0.1,0.05] [steps=200] [rounds=1] [size=416] [batch=64] [scale=n]"""
import os, sys, time
import numpy as np, torch
sys.path[:0] = [os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."), os.path.dirname(os.path.abspath(__file__))]
import zly, zly_model as zm


def run(conf, tail_box, steps, size, B, path, n_eng=3, warmup=20):
    if tail_box is None:
        os.environ.pop("ZLY_TAIL_BOX", None)
    else:
        os.environ["ZLY_TAIL_BOX"] = tail_box
    os.environ["ZLY_TAIL_BOX_MIN_CONF"] = "0"              # the arm under test is the mode itself, whatever the floor's default
    flags = zly.FLAG_NO_HEAD_TENSOR | zly.FLAG_SINGLE_CHAIN
    engs = [zly.Engine(path, model_w=size, model_h=size, dtype=zly.DTYPE_BF16, max_batch=B, max_dets=64, conf_thr=conf, warmup_runs=2, flags=flags) for _ in range(n_eng)]
    took = sum(k.startswith("(computed in the Detect tail") for k in engs[0].op_kernels(B))
    frames = torch.from_numpy(zm.synth_frames(4 * B, size, size, seed=1, rects=False)).cuda()
    sets = [frames[i * B:(i + 1) * B] for i in range(4)]
    slabs = [[torch.zeros(B * e.slab_bytes, dtype=torch.uint8, device="cuda") for _ in range(3)] for e in engs]
    torch.cuda.synchronize()

    def go(k0, n):
        for k in range(k0, k0 + n):
            i = k % n_eng
            engs[i].detect_device(sets[k % 4].data_ptr(), B, size, size, d_slabs_ptr=slabs[i][(k // n_eng) % 3].data_ptr(), tag0=k)
        for e in engs:
            e.sync()
    go(0, warmup); torch.cuda.synchronize()
    t0 = time.perf_counter(); go(warmup, steps); torch.cuda.synchronize(); dt = time.perf_counter() - t0
    last = (warmup + steps - 1)
    got = zly.parse_slabs(slabs[last % n_eng][(last // n_eng) % 3].cpu().numpy(), B, engs[0].max_dets)
    cand = float(np.mean([int(h["n_candidates"]) for h, _ in got])); kept = float(np.mean([int(h["n_kept"]) for h, _ in got]))
    for e in engs:
        e.close()
    return B * steps / dt, took, cand, kept


if __name__ == "__main__":
    arg = sys.argv[1:] + [""] * 6
    thrs = [float(x) for x in (arg[0] or "0.5,0.25,0.1,0.05").split(",")]
    steps, rounds, size, B, scale = int(arg[1] or 200), int(arg[2] or 1), int(arg[3] or 416), int(arg[4] or 64), arg[5] or "n"
    path = None
    if scale != "n":
        spec = zm.build_spec(scale)
        path = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"yolov8{scale}_synth.zlyw")
        zm.write_zlyw(path, spec, zm.synth_weights(spec))
    for thr in thrs:
        for r in range(rounds):
            for name, tb in (("dense", "0"), ("tail", None)):
                fps, took, cand, kept = run(thr, tb, steps, size, B, path)
                print(f"conf {thr} round {r + 1} {name}: {fps:.1f} frames/s, {B / fps * 1e3:.5f} ms per step, {took} levels in the tail, "
                      f"{cand:.1f} candidates / {kept:.1f} kept per frame", flush=True)
