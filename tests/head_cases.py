"""Crafted Detect heads for head_fused_kernel (csrc/kernels_head.hip): the case table, the weight crafting, the lane map, the population
counters and the expected values (TEST INFRASTRUCTURE).

tests/test_head_cases.py checks, without a GPU, that the table holds every tie class and boundary it claims, that the population conditions
hold on the CPU stand-in and that the helpers bite; tests/test_gpu_head_boundaries.py runs the engines on the crafted files.

A case is a ZLYW weight file: zm.synth_weights with the six final 1x1 convs (model.22.cv2.L.2, model.22.cv3.L.2) replaced.
  * UNIFORM: zero weights, bias only.  Every anchor of a level has logits equal to the (fp32) bias vector bit for bit, so the head tensor is
    closed_loop_ref.decode64 of the biases whatever the engine computed upstream.  A file's three levels carry three configurations.
  * GRADED: per level z = b + alpha (w . a): the synthetic filter scaled, so that logits are spread across anchors around logit(thr).  What
    is expected comes from the engine's own head tensor; populations() shows that a run really had empty, mixed and near-threshold tiles.

The lane map (kernels_head.hip): class ch = c * 16 + kq * 4 + r lives in channel tile c, lane quarter kq = lane >> 4, accumulator row r;
the arg-max runs over (c, r) inside a lane and then across the quarters by __shfl_xor 16 and 32."""
import functools
import os
from collections import namedtuple

import numpy as np

import zly_model as zm

F32 = np.float32
U24 = 2.0 ** -24
MODEL_W, MODEL_H = 160, 128              # maps of 20 x 16, 10 x 8, 5 x 4: 420 anchors, tiles that straddle rows, a partial last tile on P5
STRIDES = (8, 16, 32)
TILE = 16                                # anchors of one wave
K_VALUES = (2, 8, 18, 34, 100, 1000)     # thresholds 1 - k 2^-24
FAR = F32(-30.0)                         # a class that takes no part: score 9e-14
BACKGROUND = F32(-3.0)                   # classes below every threshold of the tie cases (score 0.047)
REQUEST_SIZES = ((200, 150), (96, 64), (160, 128))      # request frames (w, h): stretched to the model size by the front kernel


def level_dims(w=MODEL_W, h=MODEL_H):
    """[(map width, map height)] of P3, P4, P5"""
    return [(w // s, h // s) for s in STRIDES]


def level_slices(w=MODEL_W, h=MODEL_H):
    """anchor ranges of the three levels in the head tensor's N axis"""
    out, o = [], 0
    for mw, mh in level_dims(w, h):
        out.append(slice(o, o + mw * mh))
        o += mw * mh
    return out


def request_frames(n, seed=71, sizes=REQUEST_SIZES):
    """n noise frames [h][w][3] u8, their sizes cycling through `sizes`"""
    return [np.ascontiguousarray(zm.synth_frames(1, *sizes[i % len(sizes)], seed=seed + i, rects=False)[0]) for i in range(n)]


# ---------------------------------------------------------------------------------------------------
# thresholds, the early-out bound, fp32 sigmoid
# ---------------------------------------------------------------------------------------------------
def thr_of_k(k):
    """1 - k 2^-24: exact in fp32 (the spacing of [0.5, 1) is 2^-24)"""
    t = F32(1.0 - k * U24)
    assert float(t) == 1.0 - k * U24
    return t


def logit64(p):
    p = float(p)
    return float(np.log(p / (1.0 - p)))


def skip_logit(thr):
    """csrc/head_skip.h restated (tests/test_head_skip.py holds the two together)"""
    thr = F32(thr)
    if not thr > 0:
        return F32(-3.0e38)
    t = min(float(thr), 1.0)
    return F32(-np.log((1.0 - t) / t + 4.0 * U24) - 1e-2)


def skip_logit_margin_only(thr):
    """the bound before head_skip.h: logit(thr) - 1e-2, with its two special cases"""
    t = float(F32(thr))
    return F32(-3.0e38) if t <= 0.0 else F32(15.0) if t >= 1.0 else F32(np.log(t / (1.0 - t)) - 1e-2)


def score_ieee(z):
    """float32(1 / (float32(1) + float32(exp(-z)))): the fp32 engine's sigmoid, IEEE operations"""
    z = np.asarray(z, dtype=np.float32)
    with np.errstate(over="ignore"):
        e = np.exp(-z.astype(np.float64)).astype(np.float32)
        return F32(1.0) / (F32(1.0) + e)


def _ordered(v):
    b = int(np.asarray(v, dtype=np.float32).view(np.int32))
    return b if b >= 0 else -(b & 0x7fffffff)


def _from_ordered(k):
    return np.array([k if k >= 0 else ((-k) | 0x80000000)], dtype=np.uint32).view(np.float32)[0]


def lowest_passing_z(thr, score=score_ieee):
    """the lowest fp32 logit whose score is >= thr under `score` (monotone), by bisection over the fp32 values in [-100, 100]"""
    thr = F32(thr)
    lo, hi = _ordered(F32(-100.0)), _ordered(F32(100.0))
    assert not score(_from_ordered(lo)) >= thr and score(_from_ordered(hi)) >= thr, thr
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if score(_from_ordered(mid)) >= thr:
            hi = mid
        else:
            lo = mid
    return _from_ordered(hi)


# ---------------------------------------------------------------------------------------------------
# the lane map
# ---------------------------------------------------------------------------------------------------
def lane_of(ch):
    """class -> (channel tile c, lane quarter kq, accumulator row r)"""
    return ch // 16, (ch % 16) // 4, ch % 4


TIE_KINDS = ("same_lane_rows", "same_lane_tiles", "lanes_16_apart", "lanes_32_apart", "quarters_1_and_2", "high_class_in_low_lane")


def tie_kinds(a, b):
    """which of the kernel's tie decisions a tie between classes a and b goes through"""
    (ca, ka, _), (cb, kb, _) = lane_of(a), lane_of(b)
    out = set()
    if ka == kb:
        out.add("same_lane_rows" if ca == cb else "same_lane_tiles")
    else:
        if ka ^ kb == 1:
            out.add("lanes_16_apart")
        if ka ^ kb == 2:
            out.add("lanes_32_apart")
        if {ka, kb} == {1, 2}:
            out.add("quarters_1_and_2")
        hi, lo = max(a, b), min(a, b)
        if lane_of(hi)[1] < lane_of(lo)[1]:
            out.add("high_class_in_low_lane")
    return out


# ---------------------------------------------------------------------------------------------------
# uniform cases
# ---------------------------------------------------------------------------------------------------
# cls / box: the fp32 bias vectors [nc] / [64]; want_cls: the class every passing anchor must carry; passes: whether the level's anchors
# are candidates at the file's conf_thr (None: decided by the engine's own head tensor -- tiny and denormal scores)
Level = namedtuple("Level", "name cls box want_cls passes tied")
UniformFile = namedtuple("UniformFile", "key nc conf_thr levels")


def dfl_peaked(mu=1.25, offset=0.0):
    """box biases of a discretised Gaussian of mean mu bins on every side (multiples of 1/64: representable next to an offset of 3e4)"""
    bins = np.arange(16, dtype=np.float64)
    one = np.round(-0.5 * (bins - mu) ** 2 * 64.0) / 64.0 + offset
    return np.tile(one, 4).astype(np.float32)


def dfl_sides(*sides):
    """four sides (l, t, r, b), each a list of bins that share +60 while the others sit at -60, or None for all bins equal"""
    out = np.empty((4, 16), dtype=np.float32)
    for i, s in enumerate(sides):
        out[i] = 0.0 if s is None else -60.0
        if s is not None:
            out[i, list(s)] = 60.0
    return out.reshape(64)


def _cls(nc, at, fill=BACKGROUND):
    v = np.full(nc, fill, dtype=np.float32)
    for ch, z in at.items():
        v[ch] = z
    return v


def tie_level(name, classes, z=1.0, nc=80, box=None, fill=BACKGROUND, passes=True):
    classes = tuple(classes)
    return Level(name, _cls(nc, {c: z for c in classes}, fill), dfl_peaked() if box is None else box, min(classes), passes, classes)


@functools.lru_cache(maxsize=1)
def uniform_table():
    L, files = tie_level, []
    files.append(UniformFile("ties_a", 80, 0.25, (L("rows_0_1", (0, 1)), L("tiles_2_18", (2, 18)), L("lanes16_1_4", (1, 4)))))
    files.append(UniformFile("ties_b", 80, 0.25, (L("lanes32_1_8", (1, 8)), L("quarters_5_9", (5, 9)), L("high_low_17_5", (17, 5)))))
    files.append(UniformFile("ties_c", 80, 0.25, (L("high_low_64_13", (64, 13)), L("three_way_7_22_41", (7, 22, 41)), L("all_equal", range(80)))))
    # saturation: z = 20 and z = 30 both score 1.0f, the lower class wins although its logit is the smaller one
    sat = Level("saturated_3_40", _cls(80, {3: 20.0, 40: 30.0}), dfl_sides(None, None, None, None), 3, True, (3, 40))
    files.append(UniformFile("saturation_dfl", 80, 0.25, (sat, L("dfl_bin0_zero_area", (9,), box=dfl_sides([0], [0], [0], [0])),
                                                        L("dfl_bin15", (70,), box=dfl_sides([15], [15], [15], [15])))))
    files.append(UniformFile("dfl", 80, 0.25, (L("dfl_two_equal_bins", (33,), box=dfl_sides([3, 4], [3, 4], [3, 4], [3, 4])),
                                             L("dfl_offset_3e4", (12,), box=dfl_peaked(5.0, 3.0e4)),
                                             L("dfl_mixed_sides", (79,), box=dfl_sides([0], [15], [3, 4], None)))))
    # conf_thr 1.0: score 1.0f passes, 1 - 2^-23 (z = 16) does not; 0.0: a score of exactly 0 leaves the class at -1 and never passes
    files.append(UniformFile("conf_one", 80, 1.0, (L("z20", (6,), z=20.0), L("z16", (21,), z=16.0, passes=False), L("z30", (50,), z=30.0))))
    files.append(UniformFile("conf_zero", 80, 0.0, (L("z-120_score_0", range(80), z=-120.0, passes=False),
                                                  L("z-80_tiny", range(80), z=-80.0, passes=None), L("z-88_denormal", range(80), z=-88.0, passes=None))))
    # nc not a multiple of 4 or 16: the zero-padded rows have z = 0, score 0.5, far above the real classes' 0.047, and must never win
    for nc in (1, 3, 17, 64):
        files.append(UniformFile(f"nc{nc}", nc, 0.04, (L("all_-3", range(nc), z=-3.0, nc=nc), L("last_class", (nc - 1,), z=-2.5, nc=nc),
                                                      L("first_class", (0,), z=-2.5, nc=nc))))
    return tuple(files)


EQUALITY_BIASES = (("s0.047", -3.0, (0, 1)), ("s0.5", 0.0, (2, 18)), ("s0.9", 2.2, (17, 5)))       # threshold-at-equality levels: name, bias, tied classes
K_FILES = ((2, 8, 18), (34, 100, 1000))                                                           # the k values that share a file
K_TIED = {2: (1, 4), 8: (1, 8), 18: (5, 9), 34: (64, 13), 100: (0, 1), 1000: (7, 22, 41)}


def equality_file():
    """conf_thr is set per engine: the score s of a level's tied classes, its fp32 neighbours"""
    return UniformFile("equality", 80, None, tuple(tie_level(n, cls, z=z, fill=FAR) for n, z, cls in EQUALITY_BIASES))


def k_file(ks, z_of_k):
    """levels whose tied classes sit at z_of_k[k], the lowest logit that still scores 1 - k 2^-24 on the engine the file is for"""
    return UniformFile("k_" + "_".join(str(k) for k in ks), 80, None, tuple(tie_level(f"k{k}", K_TIED[k], z=z_of_k[k], fill=FAR) for k in ks))


LADDER_OFFSETS = tuple(sorted(set(range(-20, 21)) | {s * (1 << j) for j in range(5, 24) for s in (-1, 1)}, reverse=True))      # fp32 steps


def ladder_file(ks):
    """80 classes at a ladder of logits around the IEEE prediction of the lowest passing one: 41 rungs one fp32 step apart, then doubling
    distances up to 2^23 steps (several units of z), highest first.  The dump engine's head tensor tells which rungs pass on ITS arithmetic."""
    assert len(LADDER_OFFSETS) == 79
    levels = []
    for k in ks:
        z0 = lowest_passing_z(thr_of_k(k))
        rungs = np.array([_from_ordered(_ordered(z0) + o) for o in LADDER_OFFSETS] + [FAR], dtype=np.float32)
        levels.append(Level(f"ladder_k{k}", rungs, dfl_peaked(), None, None, ()))
    return UniformFile("ladder_" + "_".join(str(k) for k in ks), 80, 0.5, tuple(levels))


def pick_from_ladder(rungs, scores, thr):
    """the lowest rung whose score is >= thr; every rung above it must pass and one below it must fail (else the ladder missed the edge)"""
    rungs, scores = np.asarray(rungs, dtype=np.float32)[:79], np.asarray(scores, dtype=np.float32)[:79]
    ok = scores >= F32(thr)
    n = int(ok.sum())
    assert 0 < n < 79 and ok[:n].all() and not ok[n:].any(), f"thr {float(thr):.9g}: rungs passing {np.flatnonzero(ok).tolist()} of {rungs.tolist()}"
    return rungs[n - 1]


@functools.lru_cache(maxsize=4)
def _base(scale, nc):
    spec = zm.build_spec(scale, nc=nc)
    return spec, zm.synth_weights(spec)


def craft_uniform(f, scale="n"):
    """-> (spec, weights): the synthetic model with the six final convs of file f"""
    spec, base = _base(scale, f.nc)
    by_name = {c.name: c for c in spec.convs}
    w = dict(base)
    for l, lv in enumerate(f.levels):
        for br, bias in ((2, lv.box), (3, lv.cls)):
            c = by_name[f"model.22.cv{br}.{l}.2"]
            assert bias.shape == (c.cout,) and bias.dtype == np.float32, (c.name, bias.shape)
            w[c.name] = (np.zeros((c.cout, c.cin, 1, 1), dtype=np.float32), bias.copy())
    return spec, w


def write_uniform(path, f, scale="n"):
    spec, w = craft_uniform(f, scale)
    zm.write_zlyw(path, spec, w)
    return path


def uniform_head(f, w=MODEL_W, h=MODEL_H):
    """the float64 head tensor [4 + nc][N] every engine must produce for file f: decode64 of the biases"""
    import closed_loop_ref as cl
    box, cls = [], []
    for lv, (mw, mh) in zip(f.levels, level_dims(w, h)):
        box.append(np.broadcast_to(lv.box.astype(np.float64)[:, None, None], (64, mh, mw)))
        cls.append(np.broadcast_to(lv.cls.astype(np.float64)[:, None, None], (f.nc, mh, mw)))
    return cl.decode64(box, cls)


# ---------------------------------------------------------------------------------------------------
# the decode, restated, with the two mistakes a kernel could make and the early-out as a parameter
# ---------------------------------------------------------------------------------------------------
def decode_head(head, conf_thr, tie="lowest", cmp="ge"):
    """kernels_head.hip's arg-max and threshold on a head tensor [4 + nc][N] (fp32 comparisons) -> (class [N], best score [N], pass [N]).
    tie = "highest" and cmp = "gt" are the two wrong kernels the helpers must catch."""
    s = np.asarray(head, dtype=np.float32)[4:]
    best = s.max(0)
    if tie == "lowest":
        cls = s.argmax(0)                                        # first of the maxima: a running strict > from class 0 up
    else:
        cls = s.shape[0] - 1 - s[::-1].argmax(0)
    cls = np.where(best > 0, cls, -1)                            # best starts at 0.0f: a score of exactly 0 never becomes the class
    thr = F32(conf_thr)
    ok = (best >= thr) if cmp == "ge" else (best > thr)
    return cls, best, ok & (cls >= 0)


def early_out(z_levels, bound):
    """[N] bool: the anchors whose 16-anchor tile survives the production early-out: some anchor of the tile has a class logit >= bound.
    z_levels: per level [nc, hw] class logits of one frame"""
    out = []
    for z in z_levels:
        zmax = np.asarray(z, dtype=np.float32).max(0)
        keep = np.zeros(zmax.shape, dtype=bool)
        for t in range(0, len(zmax), TILE):
            keep[t:t + TILE] = (zmax[t:t + TILE] >= F32(bound)).any()
        out.append(keep)
    return np.concatenate(out)


def model_outcome(z_levels, conf_thr, tie="lowest", cmp="ge", bound=None, score=score_ieee):
    """a Python engine on one frame's class logits -> (classes of the candidates in anchor order, n_candidates); bound: the early-out's
    skip_logit (None: an engine that writes the head tensor and skips nothing)"""
    z = np.concatenate([np.asarray(v, dtype=np.float32) for v in z_levels], axis=1)
    head = np.concatenate([np.zeros((4, z.shape[1]), np.float32), score(z)])
    cls, _, ok = decode_head(head, conf_thr, tie, cmp)
    if bound is not None:
        ok = ok & early_out(z_levels, bound)
    return cls[ok], int(ok.sum())


def uniform_logits(f, w=MODEL_W, h=MODEL_H):
    return [np.repeat(lv.cls[:, None], mw * mh, axis=1) for lv, (mw, mh) in zip(f.levels, level_dims(w, h))]


def check_uniform_outcome(f, passes, classes, n_candidates, w=MODEL_W, h=MODEL_H):
    """what a frame of file f must give: `passes` (per level: are its anchors candidates), every candidate of a level carrying the level's
    want_cls -- as a multiset over the frame, the levels' classes being distinct -- and n_candidates the passing levels' anchors"""
    want = {}
    for lv, p, (mw, mh) in zip(f.levels, passes, level_dims(w, h)):
        if p:
            want[lv.want_cls] = want.get(lv.want_cls, 0) + mw * mh
    got = {int(c): int(k) for c, k in zip(*np.unique(np.asarray(classes, dtype=np.int64), return_counts=True))}
    assert n_candidates == sum(want.values()), f"{f.key}: {n_candidates} candidates, expected {sum(want.values())} ({want})"
    assert got == want, f"{f.key}: candidate classes {got}, expected {want}"


# ---------------------------------------------------------------------------------------------------
# graded cases
# ---------------------------------------------------------------------------------------------------
GRADED_THRESHOLDS = (F32(0.25), F32(0.9), thr_of_k(18))
GRADED_CLASSES = (5, 33, 64)             # the class that carries level 0 / 1 / 2: lane quarters 1, 0, 0, channel tiles 0, 2, 4
GRADED_PASS_FRACTION = 0.04              # of the anchors of levels 0 and 2 on the stand-in: 0.96^16 = 52 % of their tiles stay empty
Population = namedtuple("Population", "tiles empty mixed near window")
MIN_EMPTY, MIN_MIXED, MIN_NEAR, MIN_WINDOW = 0.25, 0.25, 50, 20


def is_high(thr):
    return 1.0 - float(thr) < 1e-4


def graded_weights(spec, base, ref, thr):
    """-> weights with the three cv3.L.2 convs replaced, chosen on the stand-in `ref` (an oracle/yolov8_ref.py model of `base` after a
    forward over the case's images):
      * levels 0 and 2: class GRADED_CLASSES[l] keeps its synthetic filter (alpha = 1), its bias puts GRADED_PASS_FRACTION of the anchors at
        or above logit(thr): about half of the tiles have no passing anchor and end in the early-out, the other half mix lanes above and
        below the bound;
      * level 1: the filter scaled so that the logits of class GRADED_CLASSES[1] have a standard deviation of two fp32 score steps around
        logit(thr) -- scores on both sides of the threshold and on it; at the high threshold a deviation of a 7.4th of the window [lowest
        passing logit, logit(thr)) around a point one deviation above its lower end: five anchors of six pass although no logit of their
        tile reaches logit(thr) (6.4 deviations away), the sixth scores one step below the threshold;
      * every other class: zero filter, bias FAR.
    The box branch keeps its synthetic filters: a box depends on the anchor's inputs."""
    thr = F32(thr)
    lg = logit64(thr)
    by_name = {c.name: c for c in spec.convs}
    w = dict(base)
    for l, ch in enumerate(GRADED_CLASSES):
        name = f"model.22.cv3.{l}.2"
        c = by_name[name]
        w0, _ = base[name]
        a = ref.taps[f"model.22.cv3.{l}.1"].double().numpy()                                          # [F, c3, h, w]
        t = np.einsum("c,fchw->fhw", ref.w[name][0][ch, :, 0, 0].double().numpy(), a).reshape(-1)
        if l != 1:
            alpha, b = 1.0, lg - float(np.quantile(t, 1.0 - GRADED_PASS_FRACTION))
        else:
            if is_high(thr):
                lo = float(lowest_passing_z(thr))
                sigma = (lg - lo) / 7.4
                centre = lo + sigma
            else:
                centre, sigma = lg, 2.0 * float(np.spacing(thr)) / (float(thr) * (1.0 - float(thr)))
            alpha = sigma / float(t.std())
            b = centre - alpha * float(t.mean())
        wn = np.zeros_like(w0)
        wn[ch] = (w0[ch].astype(np.float64) * alpha).astype(np.float32)
        bn = np.full(c.cout, FAR, dtype=np.float32)
        bn[ch] = F32(b)
        w[name] = (wn, bn)
    return w


def write_graded(workdir, oracle, scale="n"):
    """the graded files, chosen on the bf16 stand-in over the three request frames as the front kernel stretches them (the CPU oracle's
    preprocess is bit-exact with it) -> ({float(thr): path}, frames, images [3, 3, MODEL_H, MODEL_W] as a torch tensor)"""
    import torch
    import yolov8_ref
    frames = request_frames(3)
    images = torch.from_numpy(np.stack([oracle.preprocess(fr, MODEL_W, MODEL_H)[1] for fr in frames]))
    spec, base = _base(scale, 80)
    base_path = os.path.join(str(workdir), f"graded_base_{scale}.zlyw")
    zm.write_zlyw(base_path, spec, base)
    ref = yolov8_ref.load(base_path, "bf16")
    ref.forward(images)
    paths = {}
    for thr in GRADED_THRESHOLDS:
        paths[float(thr)] = os.path.join(str(workdir), f"graded_{scale}_{float(thr):.9g}.zlyw")
        zm.write_zlyw(paths[float(thr)], spec, graded_weights(spec, base, ref, thr))
    return paths, frames, images


def populations(frames, thr, w=MODEL_W, h=MODEL_H):
    """frames: per frame (the engine's own head [4 + nc][N] fp32, its class-logit taps per level [nc, mh, mw]) -> Population over the
    16-anchor tiles of every level of every frame (a tile is what a wave owns):
      empty / mixed: tiles without a passing anchor / with passing and non-passing anchors (pass: the head's best score >= thr, class >= 0);
      near: anchors whose best score is within 2 fp32 steps of thr;
      window: anchors that pass while no class logit of their tile reaches logit(thr) in float64."""
    thr = F32(thr)
    lg = logit64(thr)
    tiles = empty = mixed = near = window = 0
    for head, cls_taps in frames:
        _, best, ok = decode_head(head, thr)
        near += int((np.abs(best.astype(np.float64) - float(thr)) <= 2.0 * float(np.spacing(thr))).sum())
        for sl, z in zip(level_slices(w, h), cls_taps):
            zmax = np.asarray(z, dtype=np.float64).reshape(z.shape[0], -1).max(0)
            p = ok[sl]
            assert len(zmax) == len(p)
            for t in range(0, len(p), TILE):
                tiles += 1
                k, n = int(p[t:t + TILE].sum()), len(p[t:t + TILE])
                empty += k == 0
                mixed += 0 < k < n
                if not (zmax[t:t + TILE] >= lg).any():
                    window += k
    return Population(tiles, int(empty), int(mixed), near, window)


def check_populations(pop, thr):
    assert pop.empty >= MIN_EMPTY * pop.tiles and pop.mixed >= MIN_MIXED * pop.tiles and pop.near >= MIN_NEAR, (float(thr), pop)
    if is_high(thr):
        assert pop.window >= MIN_WINDOW, (float(thr), pop)
