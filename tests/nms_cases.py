"""Candidate frames for nms_kernel (csrc/kernels_post.hip), the expected slab bytes from the CPU oracle, and a restatement of the
kernel's per-frame dispatch (TEST INFRASTRUCTURE).

tests/test_nms_cases.py checks, without a GPU, that the table below holds every path and boundary it claims and that the helpers bite;
tests/test_gpu_nms_batched.py launches the shipped kernel on the table through tests/cpp/nms_probe.hip.

A frame is what decode leaves for one workgroup: `n` live Cand records in arrival order (a random permutation), every one with a unique
anchor, pad_ = 0, a class below nc and a confidence in (0, 1] -- among them 1.0, the smallest normal float and exact ties.  What lies
behind the count in the candidate buffer (an earlier call's records) is added by build_batch().
"""
from collections import namedtuple

import numpy as np

from oracle_lib import DET_DTYPE

CAND_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("w", "<f4"), ("h", "<f4"), ("conf", "<f4"),
                       ("cls", "<i4"), ("anchor", "<i4"), ("pad_", "<i4")])          # zly::Cand (csrc/zly_internal.h), 32 bytes
HDR_DTYPE = np.dtype([("n_kept", "<i4"), ("n_candidates", "<i4"), ("flags", "<u4"), ("frame_tag", "<u4")])   # zly_slab_header
SLAB_OVERFLOW = 1
SLAB_FILL = 0xAB                 # what the slab buffer holds before the launch: every byte the kernel does not write keeps it
TAG0 = 0xFFFFFFF0                # frame f carries tag0 + f: wraps through 0 inside a batch of more than 16 frames
TINY = np.finfo(np.float32).tiny

# the kernel's dispatch constants (csrc/kernels_post.hip)
WAVE_CAP = 128                   # NMS_WAVE_CAP: a frame of at most this many candidates runs in one wave
SEG_CLASS = 64                   # a class segment held by one wave in registers (`fast = sh_misc[0] <= 64`)
BIG_CLASS = 128                  # NMS_BIG_CLASS: a class above it is resolved by the whole workgroup in blocks of 64


def lds_cap(N):
    """CAP: NMS_LDS_CAP = 1024 for models of up to 4096 anchors, 2 * NMS_LDS_CAP above (launch_nms picks the instantiation by N)"""
    return 1024 if N <= 4096 else 2048


Frame = namedtuple("Frame", "name cand n")                     # cand: CAND_DTYPE [n], the live records in arrival order
Path = namedtuple("Path", "label medium big")                  # medium: a class of 65..128 present; big: a class of more than 128
Case = namedtuple("Case", "name N nc iou_thr cap frame want")  # want: the path label the case was built for
Group = namedtuple("Group", "key N nc iou_thr cap cases")      # one batched launch: its cases share N, nc, iou_thr and cap


def nms_path(counts_per_class, n, N, force_general=False):
    """The path nms_kernel<CAP> takes for a frame of n candidates with this per-class histogram, restated from csrc/kernels_post.hip:
    `n <= NMS_WAVE_CAP && !force_general` (128) -> nms_wave; else `n <= CAP` (lds_cap(N): 1024 or 2048 by template instantiation) and
    the largest class `<= 64` -> class segments in registers; else nms_general, in LDS when `n <= CAP` and in global memory beyond.
    Inside nms_general a class of more than NMS_BIG_CLASS (128) is walked by the whole workgroup, one of 2..128 by a single wave
    (65..128 is the range only this path sees).  The path cannot be observed on the GPU: this is how the suite knows what it covered."""
    n = min(int(n), N)
    counts = np.asarray(counts_per_class)
    mx = int(counts.max()) if counts.size else 0
    medium = bool(((counts > SEG_CLASS) & (counts <= BIG_CLASS)).any())
    big = bool((counts > BIG_CLASS).any())
    if n <= WAVE_CAP and not force_general:
        return Path("one_wave", False, False)
    if n > lds_cap(N):
        return Path("global", medium, big)
    if mx <= SEG_CLASS:
        return Path("segments", False, False)
    return Path("lds_general", medium, big)


def histogram(frame, nc):
    return np.bincount(frame.cand["cls"][:frame.n], minlength=nc)


# ---------------------------------------------------------------------------------------------------
# frame generators
# ---------------------------------------------------------------------------------------------------
def _grid_box(k):
    """box k of a family of pairwise disjoint boxes (cells of 1/128, boxes a quarter of a cell), away from the unit square of the random ones"""
    k = np.asarray(k)
    g = np.float32(128.0)
    return ((k % 128 + np.float32(0.5)) / g, np.float32(2.0) + (k // 128 + np.float32(0.5)) / g, np.float32(0.25) / g, np.float32(0.25) / g)


def _mixed_conf(rng, m):
    """confidences in (0, 1]: half on a grid of 1/32 (exact ties), half anywhere; 1.0, the smallest normal float and one forced tie where they fit"""
    c = np.where(rng.random(m) < 0.5, np.ceil(rng.random(m) * 32) / 32, 1.0 - rng.random(m) * 0.999).astype(np.float32)
    c = np.maximum(c, TINY)
    if m >= 4:
        c[0], c[1], c[2] = 1.0, TINY, c[3]
    return c


def _ordered_conf(m, ties=()):
    """strictly decreasing with the sorted position p (1.0 first, the smallest normal float last), equal inside each (lo, hi) range of `ties`"""
    p = np.arange(m, dtype=np.float64)
    for lo, hi in ties:
        p[lo:hi] = lo
    c = (1.0 - p / (m + 1)).astype(np.float32)
    if m >= 2 and not any(hi >= m for _, hi in ties):
        c[m - 1] = TINY
    return c


def make_frame(name, seed, N, specs):
    """specs: [(class, m, mode, arg)].  Modes:
      random     m / 4 objects in the unit square with sides up to arg (default 0.3: a crowd overlaps across objects; 0.04: objects stay apart), every
                 candidate a jittered copy of one object: IoUs on both sides of the threshold
      identical  one box m times (the first in order suppresses the rest)
      disjoint   m pairwise disjoint boxes (all kept)
      cluster    arg distinct disjoint boxes, candidate i on box i % arg: exactly min(arg, m) are kept
      ordered    arg = (loc, ties): confidences strictly decreasing with the sorted position p, box = disjoint box loc(p) (loc None: random boxes)
      rows       arg = [(x, y, w, h, conf)], verbatim
    Anchors are unique and random, so exact confidence ties are broken by the anchor in an order unrelated to arrival."""
    rng = np.random.default_rng(seed)
    parts, loc0 = [], 0
    for cls, m, mode, arg in specs:
        p = np.zeros(m, dtype=CAND_DTYPE)
        p["cls"] = cls
        if mode == "rows":
            rows = np.asarray(arg, dtype=np.float32).reshape(m, 5)
            p["x"], p["y"], p["w"], p["h"], p["conf"] = rows.T
        else:
            ordered = mode == "ordered"
            loc = arg[0] if ordered else None
            p["conf"] = _ordered_conf(m, arg[1]) if ordered else _mixed_conf(rng, m)
            if mode == "random" or (ordered and loc is None):
                side = 0.3 if (ordered or arg is None) else arg
                # objects with several candidates each, jittered in place and size: IoUs on both sides of the threshold, chains of kept boxes
                k = max(1, -(-m // 4))
                ox, oy, ow, oh = rng.uniform(0.1, 0.9, k), rng.uniform(0.1, 0.9, k), rng.uniform(side / 3, side, k), rng.uniform(side / 3, side, k)
                o = rng.integers(0, k, m)
                p["x"], p["y"] = ox[o] + ow[o] * rng.uniform(-0.2, 0.2, m), oy[o] + oh[o] * rng.uniform(-0.2, 0.2, m)
                p["w"], p["h"] = ow[o] * rng.uniform(0.75, 1.25, m), oh[o] * rng.uniform(0.75, 1.25, m)
            else:
                if mode == "identical":
                    k = np.zeros(m, dtype=np.int64)
                elif mode == "disjoint":
                    k = np.arange(m)
                elif mode == "cluster":
                    k = np.arange(m) % arg
                elif ordered:
                    k = np.array([loc(q) for q in range(m)], dtype=np.int64)
                else:
                    raise ValueError(mode)
                p["x"], p["y"], p["w"], p["h"] = _grid_box(loc0 + k)
                loc0 += int(k.max()) + 1 if m else 0
        parts.append(p)
    cand = np.concatenate(parts) if parts else np.zeros(0, dtype=CAND_DTYPE)
    n = len(cand)
    assert n <= N, (name, n, N)
    cand["anchor"] = rng.choice(N, n, replace=False)
    cand["pad_"] = 0
    cand = cand[rng.permutation(n)]
    assert n == 0 or (cand["conf"] > 0).all() and (cand["conf"] <= 1).all()
    return Frame(name, np.ascontiguousarray(cand), n)


def spread(n, classes):
    """n candidates over the given classes, as evenly as they go"""
    classes = list(classes)
    q, r = divmod(n, len(classes))
    return {c: q + (1 if i < r else 0) for i, c in enumerate(classes) if q + (1 if i < r else 0) > 0}


def frame_random(name, seed, N, sizes, side=None):
    """random boxes, mixed confidences; sizes: {class: candidates}"""
    return make_frame(name, seed, N, [(c, m, "random", side) for c, m in sizes.items()])


def frame_layout(name, seed, N, sizes, mode, arg=None):
    return make_frame(name, seed, N, [(c, m, mode, arg) for c, m in sizes.items()])


# the pair of tests/test_oracle_kat.py::test_nms_strict_greater_keeps_iou_equal_to_threshold: the threshold cases use its float32 IoU
PAIR = [(.5, .5, .2, .2, .9), (.6, .5, .2, .2, .8)]


def iou_f32(a, b):
    """calculateIoU on (cx, cy, w, h) boxes, every operation rounded to float32 in the kernel's (and the oracle's) order"""
    f = np.float32
    ax, ay, aw, ah = [f(v) for v in a[:4]]
    bx, by, bw, bh = [f(v) for v in b[:4]]
    ox = min(ax + aw / f(2), bx + bw / f(2)) - max(ax - aw / f(2), bx - bw / f(2))
    oy = min(ay + ah / f(2), by + bh / f(2)) - max(ay - ah / f(2), by - bh / f(2))
    inter = f(max(ox, f(0))) * f(max(oy, f(0)))
    uni = f(f(aw * ah) + f(bw * bh)) - inter
    return f(inter / uni) if uni > 0 else f(0)


def pair_iou():
    return iou_f32(PAIR[0], PAIR[1])


def frame_edge(name, seed, N, filler):
    """class 0: the pair whose IoU is the threshold, three zero-width boxes on the pair's first box (IoU 0 with everything: union 0 or
    overlap 0); class 1: three identical boxes (IoU 1); `filler` specs bring the frame onto the wanted path without touching the pair
    (class 0 fillers are disjoint boxes far away)"""
    zero_w = [(.5, .5, 0., .2, .7), (.5, .5, 0., .2, .7), (.5, .5, 0., 0., .6)]
    return make_frame(name, seed, N, [(0, 2, "rows", PAIR), (0, 3, "rows", zero_w), (1, 3, "identical", None)] + filler)


def _edge_fillers(N):
    cap = lds_cap(N)
    return {"one_wave": [(2, 40, "random", None)],
            "segments": [(c, 50, "random", None) for c in range(2, 8)],
            "lds_general": [(0, 150, "disjoint", None), (2, 70, "random", None)],
            "global": [(0, cap // 2, "disjoint", None), (2, cap // 2, "random", 0.04), (3, 64, "random", None)]}


def _kept_fillers(N, kept):
    """frames with exactly `kept` survivors on each path ('cluster': min(arg, m) kept per class)"""
    cap = lds_cap(N)
    q, r = divmod(kept, 4)
    return {"one_wave": [(0, 120, "cluster", kept)],
            "segments": [(c, 60, "cluster", q + (1 if c < r else 0)) for c in range(4)],
            "lds_general": [(0, 400, "cluster", kept)],
            "global": [(0, cap + 50, "cluster", kept)]}


# ---------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------
def _dead_block(p):
    return p - 128 if 128 <= p < 192 else p          # sorted positions 128..191 (the third block of 64) repeat the boxes of 0..63


def _build_big(N):
    """groups for a model of N anchors (3549: CAP 1024; 8400: CAP 2048)"""
    CAP = lds_cap(N)
    seed = [N * 1000]

    def sd():
        seed[0] += 1
        return seed[0]

    d = []                                            # the default launch: nc = 80, iou_thr = 0.45, cap = N (nothing is cut off)

    def add(want, frame):
        d.append((want, frame))

    # one wave
    for n in (0, 1, 2, 63, 64, 65, 127, 128):
        add("one_wave", frame_random(f"ow_single_class_{n}", sd(), N, {3: n} if n else {}))
        add("one_wave", frame_random(f"ow_spread_{n}", sd(), N, spread(n, range(79, -1, -1)) if n else {}))   # n <= 80: all classes distinct
    add("one_wave", make_frame("ow_class_spans_60_70_identical", sd(), N, [(0, 60, "random", None), (1, 11, "identical", None), (2, 40, "random", None)]))
    add("one_wave", make_frame("ow_class_spans_60_70_random", sd(), N, [(0, 60, "random", None), (1, 11, "random", 0.6), (2, 57, "random", None)]))
    add("one_wave", frame_layout("ow_identical_128", sd(), N, {5: 128}, "identical"))
    add("one_wave", frame_layout("ow_disjoint_128", sd(), N, {5: 128}, "disjoint"))
    add("one_wave", make_frame("ow_ties_straddle_63_64", sd(), N, [(7, 128, "ordered", (None, [(60, 68)]))]))
    # class segments in registers
    add("segments", frame_random("seg_129_classes_of_64_64_1", sd(), N, {0: 64, 1: 64, 2: 1}))
    add("segments", frame_random("seg_512_in_40_classes", sd(), N, spread(512, range(0, 80, 2))))
    add("segments", frame_random("seg_cap_minus_1", sd(), N, spread(CAP - 1, range(CAP // 64 + 4))))
    add("segments", frame_random("seg_cap_in_classes_of_64", sd(), N, {c: 64 for c in range(CAP // 64)}))
    add("segments", frame_layout("seg_cap_in_classes_of_64_identical", sd(), N, {c: 64 for c in range(79, 79 - CAP // 64, -1)}, "identical"))
    # general path in LDS
    for L in (65, 128, 129, 192, 193):
        add("lds_general", frame_random(f"lds_largest_class_{L}", sd(), N, {2: L, 0: 30, 5: 64, 9: 1}))
    add("lds_general", make_frame("lds_disjoint_129_last_block_of_one", sd(), N, [(2, 129, "disjoint", None), (0, 10, "random", None)]))
    add("lds_general", make_frame("lds_disjoint_193_last_block_of_one", sd(), N, [(79, 193, "disjoint", None), (0, 10, "random", None)]))
    add("lds_general", frame_random("lds_n_130", sd(), N, {1: 66, 0: 64}))
    add("lds_general", frame_random("lds_n_513", sd(), N, {4: 300, 6: 100, 7: 64, 8: 49}))
    add("lds_general", frame_random("lds_n_cap_minus_1", sd(), N, {0: CAP - 201, 1: 120, 2: 80}, side=0.06))
    add("lds_general", frame_random("lds_n_cap", sd(), N, {0: CAP - 100, 3: 100}))
    add("lds_general", frame_random("lds_n_cap_one_class", sd(), N, {0: CAP}, side=0.04))
    add("lds_general", make_frame("lds_crowd_identical", sd(), N, [(0, 300, "identical", None), (1, 20, "random", None)]))
    add("lds_general", make_frame("lds_crowd_disjoint_63_survivors_per_block", sd(), N,
                                  [(0, 200, "ordered", (lambda p: p - (1 if p % 64 == 5 else 0), []))]))
    add("lds_general", make_frame("lds_crowd_block_without_survivor", sd(), N, [(0, 260, "ordered", (_dead_block, [])), (3, 70, "random", None)]))
    add("lds_general", frame_random("lds_crowded_medium_small", sd(), N, {0: 400, 1: 100, 2: 70, 3: 64, 4: 10, 5: 1}, side=0.08))
    # global memory
    add("global", frame_random("glb_cap_plus_1_one_class", sd(), N, {0: CAP + 1}, side=0.04))
    add("global", frame_random("glb_cap_plus_1_in_80_classes", sd(), N, spread(CAP + 1, range(80))))
    add("global", frame_layout("glb_cap_plus_1_disjoint", sd(), N, {3: CAP + 1}, "disjoint"))
    rest = CAP + CAP // 2 - (CAP // 2 + 37) - 120 - 64
    add("global", frame_random("glb_1p5_cap_mix", sd(), N, {0: CAP // 2 + 37, 1: 120, 2: 64, **spread(rest, range(3, 80))}))
    add("global", frame_random("glb_1p5_cap_one_class", sd(), N, {41: CAP + CAP // 2}))
    add("global", frame_random("glb_all_anchors_in_80_classes", sd(), N, spread(N, range(80))))
    add("global", frame_random("glb_all_anchors_one_class", sd(), N, {0: N}))
    rest = N - N // 2 - 128 - 129 - 65 - 64
    add("global", frame_random("glb_all_anchors_mix", sd(), N, {0: N // 2, 1: 128, 2: 129, 3: 65, 4: 64, **spread(rest, range(5, 80))}))
    add("global", make_frame("glb_crowd_block_without_survivor", sd(), N, [(0, CAP + 200, "ordered", (_dead_block, []))]))

    groups = [("default", 80, np.float32(0.45), N, d)]
    # nc = 65 (one class in the second 64-lane round of the class scans) and nc = 1024 (the kernel's limit), each on every path
    groups.append(("nc65", 65, np.float32(0.45), N, [
        ("one_wave", frame_random("nc65_ow", sd(), N, {64: 30, 0: 20})),
        ("segments", frame_random("nc65_seg", sd(), N, {64: 64, 0: 40, 33: 60})),
        ("lds_general", frame_random("nc65_lds", sd(), N, {64: 200, 0: 70})),
        ("global", frame_random("nc65_glb", sd(), N, {64: CAP // 2, 0: CAP // 2 + 1, 63: 100}))]))
    groups.append(("nc1024", 1024, np.float32(0.45), N, [
        ("one_wave", frame_random("nc1024_ow_classes_0_and_1023", sd(), N, {0: 64, 1023: 64})),
        ("one_wave", frame_random("nc1024_ow_128_distinct_classes", sd(), N, {8 * i + 7: 1 for i in range(128)})),
        ("segments", frame_random("nc1024_seg", sd(), N, {1023: 64, 0: 64, 512: 10, 64: 3, 63: 5})),
        ("lds_general", frame_random("nc1024_lds", sd(), N, {1023: 150, 0: 66, 500: 3})),
        ("global", frame_random("nc1024_glb", sd(), N, {1023: CAP, 0: 40}))]))
    # the threshold: IoU == iou_thr exactly (strict >: kept), one ulp either side, 0.0 and 1.0 -- on every path
    t = pair_iou()
    edge = [(want, frame_edge(f"edge_{want}", sd(), N, f)) for want, f in _edge_fillers(N).items()]
    for key, thr in (("thr_eq", t), ("thr_below", np.nextafter(t, np.float32(0))), ("thr_above", np.nextafter(t, np.float32(1))),
                     ("thr_0", np.float32(0.0)), ("thr_1", np.float32(1.0))):
        groups.append((key, 80, thr, N, edge))
    # the slab capacity: cap = 1, n_kept == cap and n_kept == cap + 1 -- on every path
    groups.append(("cap1", 80, np.float32(0.45), 1, edge))
    kept = []
    for k in (100, 101):
        kept += [(want, make_frame(f"kept_{k}_{want}", sd(), N, f)) for want, f in _kept_fillers(N, k).items()]
    groups.append(("cap100", 80, np.float32(0.45), 100, kept))
    return [_group(key, N, nc, thr, cap, cases) for key, nc, thr, cap, cases in groups]


def _build_small(N):
    """tiny candidate buffers whose frames are full (n == N): the kernel's `lane < N` guards, frames packed N records apart"""
    s = [N * 1000 + 500]

    def sd():
        s[0] += 1
        return s[0]

    cases = [(None, frame_random(f"full_one_class_{N}", sd(), N, {3: N})),
             (None, frame_random(f"full_spread_{N}", sd(), N, spread(N, range(80)))),
             (None, frame_random(f"empty_{N}", sd(), N, {})),
             (None, frame_layout(f"full_identical_{N}", sd(), N, {0: N}, "identical"))]
    if N > 1:
        cases.append((None, frame_random(f"half_{N}", sd(), N, {1: N // 2})))
    if N == 200:
        cases += [(None, frame_random("full_two_classes_of_100_200", sd(), N, {0: 100, 1: 100})),
                  (None, frame_random("n_128_of_200", sd(), N, {0: 100, 1: 28})),
                  (None, frame_random("n_129_of_200", sd(), N, {0: 65, 1: 64}))]
    return [_group("default", N, 80, np.float32(0.45), N, cases)]


def _group(key, N, nc, thr, cap, cases):
    out = []
    for want, fr in cases:
        p = nms_path(histogram(fr, nc), fr.n, N)
        out.append(Case(f"{key}/{fr.name}", N, nc, np.float32(thr), cap, fr, want or p.label))
    return Group(key, N, nc, np.float32(thr), cap, out)


BIG_N = (3549, 8400)            # 416 x 416 and 640 x 640 models: the two LDS-capacity instantiations
SMALL_N = (1, 64, 65, 200)
_tables = {}


def table(N):
    """the groups (batched launches) for N anchors; built once"""
    if N not in _tables:
        _tables[N] = _build_big(N) if N in BIG_N else _build_small(N)
    return _tables[N]


def all_cases(N):
    return [c for g in table(N) for c in g.cases]


# ---------------------------------------------------------------------------------------------------
# expected slab bytes
# ---------------------------------------------------------------------------------------------------
_oracle = None


def _default_oracle():
    global _oracle
    if _oracle is None:
        import oracle_lib
        _oracle = oracle_lib.Oracle()
    return _oracle


def oracle_kept(frame, iou_thr, oracle=None):
    """the frame's live candidates, sorted by anchor (the oracle's stable sort then breaks exact ties by the lower anchor: the kernel's
    rule), through the CPU oracle's NMS -> kept detections in output order"""
    live = frame.cand[:frame.n]
    live = live[np.argsort(live["anchor"], kind="stable")]
    dets = np.zeros(len(live), dtype=DET_DTYPE)
    for k in ("x", "y", "w", "h"):
        dets[k] = live[k]
    dets["confidence"], dets["class_id"] = live["conf"], live["cls"]
    return (oracle or _default_oracle()).nms(dets, float(np.float32(iou_thr)))


def slab_from_dets(kept, n_candidates, cap, tag, fill=SLAB_FILL):
    """slab bytes: header, the first min(n_kept, cap) detections (track_id, pad_, timestamp 0), the fill byte behind them"""
    buf = np.full(HDR_DTYPE.itemsize + cap * DET_DTYPE.itemsize, fill, dtype=np.uint8)
    hdr = buf[:HDR_DTYPE.itemsize].view(HDR_DTYPE)
    hdr["n_kept"], hdr["n_candidates"] = len(kept), n_candidates
    hdr["flags"] = SLAB_OVERFLOW if len(kept) > cap else 0
    hdr["frame_tag"] = int(tag) & 0xFFFFFFFF
    m = min(len(kept), cap)
    out = np.zeros(m, dtype=DET_DTYPE)
    for k in ("x", "y", "w", "h", "confidence", "class_id"):
        out[k] = kept[k][:m]
    buf[HDR_DTYPE.itemsize:HDR_DTYPE.itemsize + m * DET_DTYPE.itemsize] = out.view(np.uint8)
    return buf


def oracle_slab(frame, cap, tag, iou_thr, oracle=None, fill=SLAB_FILL):
    return slab_from_dets(oracle_kept(frame, iou_thr, oracle), frame.n, cap, tag, fill)


_kept_cache = {}


def case_slab(case, tag, oracle=None, fill=SLAB_FILL):
    """oracle_slab of a table case; the oracle's quadratic work is done once per (frame, threshold)"""
    key = (case.N, case.frame.name, float(case.iou_thr))
    if key not in _kept_cache:
        _kept_cache[key] = oracle_kept(case.frame, case.iou_thr, oracle)
    return slab_from_dets(_kept_cache[key], case.frame.n, case.cap, tag, fill)


# ---------------------------------------------------------------------------------------------------
# the candidate buffer of a batched launch, with its history
# ---------------------------------------------------------------------------------------------------
def build_batch(frames, N, stale, seed=0):
    """-> (cand CAND_DTYPE [len(frames)][N], counts int32): frame f's live records at cand[f, :n], and behind them
    stale = "hostile": plausible records that would change the result if one were read as live -- class 0 or a class live in the frame,
                       a confidence above every live one, a box over the whole image, half with pad_ = 0 and half with pad_ = 1;
    stale = "next":    the live records of the next frame of the batch, repeated up to N (what a crowded earlier call leaves)"""
    rng = np.random.default_rng(seed)
    cand = np.zeros((len(frames), N), dtype=CAND_DTYPE)
    counts = np.array([fr.n for fr in frames], dtype=np.int32)
    for f, fr in enumerate(frames):
        n, t = fr.n, N - fr.n
        cand[f, :n] = fr.cand[:n]
        if t == 0:
            continue
        if stale == "hostile":
            tail = np.zeros(t, dtype=CAND_DTYPE)
            tail["x"] = tail["y"] = 0.5
            tail["w"] = tail["h"] = 1.0
            tail["conf"] = 1.5
            tail["cls"] = rng.choice(np.unique(np.concatenate([[0], fr.cand["cls"][:n]])), t)
            tail["anchor"] = rng.integers(0, N, t)
            tail["pad_"] = np.arange(t) & 1
        elif stale == "next":
            nx = frames[(f + 1) % len(frames)]
            tail = np.resize(nx.cand[:nx.n], t) if nx.n else np.zeros(t, dtype=CAND_DTYPE)
        else:
            raise ValueError(stale)
        cand[f, n:] = tail
    return cand, counts
