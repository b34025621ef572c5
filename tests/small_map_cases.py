"""The smallest and thinnest maps a model size allows: shapes, configurations and the expected kernel coverage of tests/test_gpu_small_maps.py, and the
stand-in faults of tests/test_small_map_cases.py.  TEST INFRASTRUCTURE (imported by tests/ only; not a conftest).

zly_create accepts any model_w / model_h that are positive multiples of 32.  A side of 32 gives maps of one row or one column at P5 and, at 32 x 32, a
1 x 1 map; the planners have no floor on the map size, so such maps reach the tiled kernels with a tile larger than the map, 3 x 3 convs whose upper and
lower taps are padding at every pixel, stride 2 from two rows to one, Upsample from one pixel, pool windows of radius 2 / 4 / 6 on one pixel, Detect
levels of 1, 2 or 4 anchors inside a 16-anchor MFMA tile and M = n H W below one pixel tile.  On a one-row map in batch-linear NHWC row y - 1 of frame f
IS the row of frame f - 1: a wrong out-of-range test reads real data there, which only a per-element check on the engine's own inputs notices.

Sizes are (w, h) as everywhere in the suite; maps are written rows x columns."""
import contextlib

import numpy as np
import torch
import torch.nn.functional as F

import yolov8_ref
import zly_model as zm

# ---------------------------------------------------------------------------------------------------
# shapes
# ---------------------------------------------------------------------------------------------------
# (w, h): (P3, P4, P5 maps as rows x columns, what the shape is for)
SHAPES = {
    (32, 32): ("4x4 2x2 1x1", "the 1 x 1 map: Upsample from one pixel, pools on one pixel, levels of 16 / 4 / 1 anchors, N = 21"),
    (64, 32): ("4x8 2x4 1x2", "a one-row P5; stride 2 from two rows to one; the Upsample source has two columns"),
    (32, 64): ("8x4 4x2 2x1", "a one-column P5"),
    (96, 32): ("4x12 2x6 1x3", "one side at sppf_fused_ok's H < 3 || W < 3 refusal"),
    (32, 96): ("12x4 6x2 3x1", "the other side at that refusal"),
    (96, 96): ("12x12 6x6 3x3", "the smallest map sppf_fused_kernel accepts"),
    (416, 32): ("4x52 2x26 1x13", "long tile loops along the row while the rows are degenerate: the neighbour-frame row hazard on 13-pixel rows"),
    (32, 416): ("52x4 26x2 13x1", "long tile loops along the column while the columns are degenerate"),
    (64, 64): ("8x8 4x4 2x2", "in the suite under no-fusion / fp32 / batch 1; here through the fused and tiled kernels at batch 3"),
}
ONE_ROW = (416, 32)       # the shape the issue's single-orientation cases use: P3 is 4 rows by 52 columns, P5 1 by 13
THIN = [(32, 32), (64, 32), ONE_ROW]

SEED = 31                 # frames of every case: zm.synth_frames(n, w, h, seed=SEED, rects=False), at the model's size


def maps(w, h):
    """[(rows, columns)] of P3, P4, P5"""
    return [(h // s, w // s) for s in (8, 16, 32)]


def n_anchors(w, h):
    return sum(r * c for r, c in maps(w, h))


def frames_of(n, w, h):
    """the first n of the shape's 64 frames (the thresholds below are chosen over all 64)"""
    return np.ascontiguousarray(zm.synth_frames(64, w, h, seed=SEED, rects=False)[:n])


def images_of(frames):
    """what the oracle's preprocess gives for frames of the model's own size: RGB / 255 as fp32 [n, 3, h, w]"""
    return torch.from_numpy(np.ascontiguousarray(frames[..., ::-1])).permute(0, 3, 1, 2).to(torch.float32) / 255.0


# The confidence threshold per shape, chosen ON THE CPU from the oracle's own head (oracle/yolov8_ref.py in bf16 mode, the synthetic YOLOv8n weights, the 64
# frames of frames_of(64, w, h)): the largest multiple of 1/64 that leaves every one of the 64 frames at least MIN_CANDIDATES + 2 anchors whose best class
# score is at least 0.03 above it (0.03 > the 2e-2 the suite allows between the bf16 engine's scores and the oracle's).  choose_conf_thr() recomputes
# it; tests/test_small_map_cases.py asserts that the table says what it computes (to one step of 1/64: the oracle's last bits depend on the CPU).
# YOLOv8-s (other weights) has entries of its own by the same rule.  The GPU tests assert the count on the engine's own head, so that no detection
# comparison is one of empty slabs.
MIN_CANDIDATES = 4
CONF_THR = {              # {(scale, w, h): thr}; multiples of 1/64, exact in fp32
    ("n", 32, 32): 0.09375, ("n", 32, 64): 0.125, ("n", 32, 96): 0.140625, ("n", 32, 416): 0.1875, ("n", 64, 32): 0.125, ("n", 64, 64): 0.15625,
    ("n", 96, 32): 0.140625, ("n", 96, 96): 0.234375, ("n", 416, 32): 0.1875,
    ("s", 32, 32): 0.078125, ("s", 32, 64): 0.109375, ("s", 32, 96): 0.125, ("s", 32, 416): 0.171875, ("s", 64, 32): 0.109375, ("s", 64, 64): 0.171875,
    ("s", 96, 32): 0.125, ("s", 96, 96): 0.25, ("s", 416, 32): 0.1875,
}


def choose_conf_thr(ref, w, h, n=64):
    with torch.no_grad():
        head = ref.forward(images_of(frames_of(n, w, h))).numpy()
    best = np.sort(head[:, 4:].max(1), axis=1)[:, ::-1]          # [n, N] best class score per anchor, descending
    kth = float(best[:, MIN_CANDIDATES + 1].min()) - 0.03
    return float(np.floor(kth * 64) / 64)


def candidates(head, thr):
    """anchors of one head tensor [4 + nc, N] whose best class score reaches thr"""
    return int((np.asarray(head)[4:].max(0) >= thr).sum())


# ---------------------------------------------------------------------------------------------------
# configurations
# ---------------------------------------------------------------------------------------------------
MIN_SWITCHES = dict(ZLY_LDS_MIN_TILES="1", ZLY_STREAM_MIN_GROUPS="1", ZLY_PAIR_MIN_TILES="1", ZLY_WS_MIN_TILES="1")      # as tests/test_gpu_closed_loop.py
TAIL_ENV = {"ZLY_WS_MIN_TILES": "1", "ZLY_LDS_MIN_TILES": "1"}                                                           # as tests/test_gpu_head_boundaries.py

# name -> (scale, dtype, flags by name, environment, n, entry)
#   entry "forward+batch": zly_forward, the checks, then zly_detect_batch on the same engine and the checks again with first_input
#   entry "device": zly_detect_device only (the front kernel runs), frames 0 and n - 1 checked, and a production-flags engine must give the same slabs
CONFIGS = {
    "a":      ("n", "bf16", ("NO_FUSION", "DUMP_LOGITS"), {}, 3, "forward+batch"),
    "b":      ("n", "fp32", ("DUMP_LOGITS",), {}, 3, "forward+batch"),
    "c":      ("n", "bf16", ("DUMP_LOGITS",), MIN_SWITCHES, 3, "forward+batch"),
    "c-ws1":  ("n", "bf16", ("DUMP_LOGITS",), dict(MIN_SWITCHES, ZLY_WS1="2", ZLY_WS1_MIN_PX="1"), 3, "forward+batch"),
    "c-pair": ("n", "bf16", ("DUMP_LOGITS",), dict(MIN_SWITCHES, ZLY_NO_C2F="1"), 3, "forward+batch"),
    "d1":     ("n", "bf16", ("DUMP_LOGITS",), {}, 1, "forward+batch"),
    "d4":     ("n", "bf16", ("DUMP_LOGITS",), {}, 4, "forward+batch"),
    "e":      ("n", "bf16", ("DUMP_LOGITS",), dict(MIN_SWITCHES, ZLY_SPPF_FUSED="1"), 3, "forward+batch"),
    "f":      ("n", "bf16", ("ASYNC_NMS", "DUMP_LOGITS"), {}, 64, "device"),
    "g":      ("s", "bf16", ("DUMP_LOGITS",), MIN_SWITCHES, 3, "forward+batch"),
    "g-c2f64": ("s", "bf16", ("DUMP_LOGITS",), dict(MIN_SWITCHES, ZLY_C2F64="1"), 3, "forward+batch"),
    "g6":     ("s", "bf16", ("DUMP_LOGITS",), MIN_SWITCHES, 6, "forward+batch"),
    "h":      ("n", "bf16", ("DUMP_LOGITS",), dict(TAIL_ENV, ZLY_TAIL_BOX="2"), 6, "forward+batch"),
}
# n = 6 in "g6" and "h": the Detect convs are launches of their own from batch 5 up, and a 4 x 8 map passes plan_ws's / conv_wsk_ok's pixel gate
# (n Ho Wo >= 169 ws_min_tiles, with ZLY_WS_MIN_TILES=1) from 6 frames up

ALL = sorted(SHAPES)
# (shape, configuration) pairs.  Not every pair: every shape one kernel per conv (a) and through the throughput kernels (c); the other configurations on
# the shapes where they meet MUST_REACH / MUST_SPAN below or take another path (e: both sides of sppf_fused_ok's refusal)
CASES = ([(s, "a") for s in ALL] + [(s, "b") for s in [(32, 32), (64, 32), (32, 64), ONE_ROW, (32, 416)]] +
         [(s, "c") for s in ALL] + [(s, "c-ws1") for s in [(32, 32), (64, 32), (32, 96), ONE_ROW, (32, 416)]] +
         [(s, "c-pair") for s in [(32, 32), (64, 32), (32, 64), ONE_ROW, (64, 64)]] +
         [(s, "d1") for s in [(32, 32), (64, 32), (32, 64), ONE_ROW]] + [(s, "d4") for s in [(32, 32), (64, 32), ONE_ROW, (32, 416)]] +
         [(s, "e") for s in [(96, 96), (96, 32), (32, 96), (32, 32)]] +
         [(s, "f") for s in [(32, 32), ONE_ROW, (32, 416)]] +
         [(s, "g") for s in THIN] + [(s, "g-c2f64") for s in THIN + [(32, 416)]] + [((64, 32), "g6")] +
         [(s, "h") for s in [(32, 32), (64, 32), ONE_ROW, (32, 416)]])


def case_id(case):
    (w, h), cfg = case
    return f"{w}x{h}-{cfg}"


# ---------------------------------------------------------------------------------------------------
# coverage: what a launch table says
# ---------------------------------------------------------------------------------------------------
# kernel family -> (prefix of its zly_op_kernel_name, smallest tile as (rows, columns) or the pixels of its smallest pixel tile), from the planners:
#   ws_plan / wsk_plan / ws_pair_tiles / pair_plan / c2f_plan search tiles from 4 x 8 up (ws_plan at stride 2: 2 x 8 output pixels), c2f64_plan from 4 x 6;
#   plan_lds cuts the map into 4 PT x 16 tiles; the stream and direct kernels and conv1x1_ws_kernel walk pixel tiles of M = n H W: 16 PT pixels per wave
#   (one MFMA tile at least), 64 PT per workgroup of the direct kernel, 16 .. 256 for conv1x1_ws_kernel; the merged Detect launch and the Detect tail
#   work on 16-anchor MFMA tiles of one level; sppf_fused_kernel holds the whole map (3 x 3 at least), the pool kernels too (any size);
#   stem_fused_kernel works on fixed 16 x 32 tiles of model.0's map; stem_model1_kernel on tiles of model.1's map, planned 8 x 26 (or a divisor of the
#   width from 13 up) and halved for small launches down to 4 rows and, for widths that are multiples of 8, 8 columns.
FAMILIES = {
    "conv3x3_lds_kernel":       ("conv3x3_lds_kernel<", (4, 16)),
    "conv3x3_ws_kernel":        ("conv3x3_ws_kernel<", (4, 8)),
    "conv3x3_ws_kernel S=2":    ("conv3x3_ws_kernel<S=2", (2, 8)),
    "conv3x3_ws_pair_kernel":   ("conv3x3_ws_pair_kernel<", (4, 8)),
    "conv3x3_wsk_kernel":       ("conv3x3_wsk_kernel<", (4, 8)),
    "conv1x1_stream_kernel":    ("conv1x1_stream_kernel<", 16),
    "conv1x1_ws_kernel":        ("conv1x1_ws_kernel<NK", 16),
    "conv1x1_ws_kernel dual":   ("conv1x1_ws_kernel<dual-source", 16),
    "c2f_kernel<16>":           ("c2f_kernel<C=16", (4, 8)),
    "c2f_kernel<32>":           ("c2f_kernel<C=32", (4, 8)),
    "c2f64_kernel":             ("c2f_kernel<C=64", (4, 6)),
    "bottleneck_pair_kernel":   ("bottleneck_pair_kernel<", (4, 8)),
    "stem_model1_kernel":       ("stem_model1_kernel", (4, 8)),
    "stem_fused_kernel":        ("stem_fused_kernel", (16, 32)),
    "sppf_pool16_kernel":       ("sppf_pool16_kernel", (3, 3)),
    "sppf_pool_kernel":         ("sppf_pool_kernel", (3, 3)),
    "sppf_fused_kernel":        ("sppf_fused_kernel<", (3, 3)),
    "conv_igemm_kernel":        ("conv_igemm_kernel<", 64),
    "conv_igemm_kernel split-K": ("conv_igemm_kernel<", 16),
    "conv_igemm_multi_kernel":  ("conv_igemm_multi_kernel<", 16),
    "head_fused_kernel":        ("head_fused_kernel", 16),
    "head_fused_kernel + box conv": ("head_fused_kernel", 16),
}


def out_map(op_name, w, h):
    """(rows, columns) of the map an op of the plan writes (Detect tail ops: the level's map), None for preprocess / nms"""
    if op_name.startswith("detect.tail.P"):
        lvl = int(op_name[len("detect.tail.P")]) - 3
        return maps(w, h)[lvl]
    if not op_name.startswith("model."):
        return None
    parts = op_name.split(".")
    idx = int(parts[1])
    if idx == 22:
        return maps(w, h)[int(parts[3])]
    s = {0: 2, 1: 4, 2: 4, 3: 8, 4: 8, 5: 16, 6: 16, 7: 32, 8: 32, 9: 32, 12: 16, 15: 8, 16: 16, 18: 16, 19: 32, 21: 32}[idx]
    return (h // s, w // s)


def families_of(kernel_name):
    out = []
    for fam, (prefix, _) in FAMILIES.items():
        if not kernel_name.startswith(prefix):
            continue
        if fam == "conv_igemm_kernel split-K" and "KSPLIT=4" not in kernel_name:
            continue
        if fam == "conv_igemm_kernel" and "KSPLIT=1>" not in kernel_name:
            continue
        if fam == "conv3x3_ws_kernel" and "<S=2" in kernel_name:
            continue
        if fam == "head_fused_kernel + box conv" and "(+ box conv" not in kernel_name:
            continue
        out.append(fam)
    return out


def below_tile(fam, rows, cols, n):
    """is an n-frame launch on a rows x cols map smaller than the family's smallest tile: in at least one axis, or in pixels M = n rows cols
    (Detect tail and merged Detect launch: the anchors of one frame's level)"""
    t = FAMILIES[fam][1]
    if isinstance(t, tuple):
        return rows < t[0] or cols < t[1]
    if fam.startswith(("head_fused_kernel", "conv_igemm_multi_kernel")):
        return rows * cols < t
    return n * rows * cols < t


def spanned_by_tile(fam, rows, cols):
    """does ONE smallest tile of a spatially tiled family span the map in at least one axis (the map is no larger than the tile there)"""
    t = FAMILIES[fam][1]
    return isinstance(t, tuple) and (rows <= t[0] or cols <= t[1])


def reached(op_names, kernel_names, w, h, n):
    """a launch table's ({family: maps 'RxC' below its smallest tile it reaches}, {family: maps that one smallest tile spans in an axis})"""
    below, spanned = {}, {}
    per_level_tails = sum(k.startswith("head_fused_kernel") for k in kernel_names) == 3
    for op, k in zip(op_names, kernel_names):
        m = out_map(op.split("+")[0], w, h)
        if m is None:
            continue
        ms = [m]
        if k.startswith("head_fused_kernel") and not per_level_tails:
            ms = maps(w, h)                                       # one tail launch for the three levels
        for fam in families_of(k):
            if fam == "stem_model1_kernel":
                ms = [(h // 4, w // 4)]                           # booked on model.0's op; its tiles are tiles of model.1's map
            for r, c in ms:
                if below_tile(fam, r, c, n):
                    below.setdefault(fam, set()).add(f"{r}x{c}")
                if spanned_by_tile(fam, r, c):
                    spanned.setdefault(fam, set()).add(f"{r}x{c}")
    return {f: sorted(v) for f, v in below.items()}, {f: sorted(v) for f, v in spanned.items()}


# Derived from the planners, confirmed on the MI355X, frozen.  tests/test_gpu_small_maps.py::test_coverage_is_recorded builds the same tables from
# op_kernels of every engine it made and fails where they stop holding:
#   MUST_REACH[family][case] = maps below the family's smallest tile on which that case must reach it;
#   CANNOT_REACH[family] = why NO case reaches it on a map below its smallest tile.  If a planner change moves such a map into one of these kernels the
#     test fails until a shape is added for it here;
#   MUST_SPAN[family][case] = for the tiled families of CANNOT_REACH that a listed shape can reach at all: the maps that one smallest tile spans in an
#     axis (a 4 x 8 map at 100 % utilisation) on which that case must reach it -- the closest these shapes get to them.
MUST_REACH = {
    "conv3x3_lds_kernel": {"32x32-c": ["1x1", "2x2", "4x4"], "64x32-c": ["1x2", "2x4", "4x8"], "32x64-c": ["2x1", "4x2", "8x4"], "96x96-c": ["3x3", "6x6"],
                           "416x32-c": ["1x13", "2x26"], "32x416-c": ["13x1", "26x2", "52x4"], "416x32-f": ["2x26"], "32x416-f": ["13x1", "26x2", "52x4"],
                           "32x32-g": ["1x1", "2x2", "4x4"]},
    "conv1x1_ws_kernel": {"32x32-c-ws1": ["1x1", "2x2"], "64x32-c-ws1": ["1x2"], "32x96-c-ws1": ["3x1"]},
    "conv1x1_ws_kernel dual": {"32x32-c-ws1": ["2x2"]},           # model.12.cv1: Upsample from the 1 x 1 map + Concat, M = 12
    "c2f_kernel<32>": {"32x32-c": ["4x4"], "32x64-c": ["8x4"], "32x416-c": ["52x4"], "32x32-d1": ["4x4"], "32x32-d4": ["4x4"], "32x32-f": ["4x4"],
                       "32x416-f": ["52x4"]},
    "c2f64_kernel": {"32x32-g-c2f64": ["4x4"], "32x416-g-c2f64": ["52x4"]},
    "bottleneck_pair_kernel": {"32x32-c-pair": ["4x4"], "32x64-c-pair": ["8x4"]},
    "stem_fused_kernel": {"32x32-a": ["16x16"], "32x64-a": ["32x16"], "32x416-a": ["208x16"]},
    "sppf_pool16_kernel": {"32x32-c": ["1x1"], "64x32-c": ["1x2"], "32x64-c": ["2x1"], "416x32-c": ["1x13"], "32x416-c": ["13x1"], "32x32-e": ["1x1"],
                           "96x32-e": ["1x3"], "32x96-e": ["3x1"]},
    "sppf_pool_kernel": {"32x32-b": ["1x1"], "64x32-b": ["1x2"], "32x32-f": ["1x1"], "416x32-f": ["1x13"], "32x416-f": ["13x1"]},
    "conv_igemm_kernel": {"32x32-a": ["4x4"], "32x32-b": ["1x1", "2x2", "4x4"], "64x32-b": ["1x2", "2x4"], "32x64-b": ["2x1", "4x2"]},
    "conv_igemm_kernel split-K": {"32x32-a": ["1x1", "2x2"], "32x32-d1": ["1x1", "2x2"], "64x32-d1": ["1x2", "2x4"], "32x64-d1": ["2x1", "4x2"],
                                  "416x32-d1": ["1x13"], "32x32-d4": ["1x1"]},
    "conv_igemm_multi_kernel": {"32x32-d1": ["1x1"], "32x32-d4": ["1x1"], "64x32-d4": ["1x2"], "416x32-d4": ["1x13"], "32x416-d4": ["13x1"], "32x32-c": ["1x1"]},
    "head_fused_kernel": {"32x32-c": ["1x1", "2x2"], "64x32-c": ["1x2", "2x4"], "32x64-c": ["2x1", "4x2"], "32x32-d1": ["1x1", "2x2"], "32x32-f": ["1x1", "2x2"],
                          "416x32-f": ["1x13"], "32x416-f": ["13x1"]},
    "head_fused_kernel + box conv": {"32x32-h": ["1x1", "2x2"], "64x32-h": ["1x2", "2x4"], "416x32-h": ["1x13"], "32x416-h": ["13x1"]},
}
_UTIL = ("a map below a 4 x 8 tile in an axis is covered to at most 75 % (3 of 4 rows, 6 of 8 columns) and the listed maps of three rows or six columns are "
         "thin in the other axis too: util < 0.7 refuses every one of them")
CANNOT_REACH = {
    "conv3x3_ws_kernel": "plan_ws: " + _UTIL,
    "conv3x3_ws_kernel S=2": "plan_ws: " + _UTIL + "; the 2 x 6 map of 96 x 32 (75 % of a 2 x 8 tile) fails n Ho Wo >= 169 ws_min_tiles at n = 3",
    "conv3x3_ws_pair_kernel": "conv_ws_pair_plan takes a pair only where both convs plan as conv3x3_ws_kernel; plan_ws: " + _UTIL,
    "conv3x3_wsk_kernel": "conv_wsk_ok: " + _UTIL,
    "conv1x1_stream_kernel": "plan_stream: M / (16 PT) whole pixel groups x channel blocks < stream_min_groups refuses every M below one pixel group, "
                             "whatever ZLY_STREAM_MIN_GROUPS says (1 at least)",
    "c2f_kernel<16>": "no gate: model.2's map is w / 4 x h / 4, 8 x 8 pixels at least, never below the 4 x 8 tile",
    "stem_model1_kernel": "no gate: model.1's map is w / 4 x h / 4, 8 x 8 pixels at least, never below a 4 x 8 tile (the planned 4 x 13 tile of a small "
                          "launch is wider than the 8-column map of every 32-wide shape)",
    "sppf_fused_kernel": "sppf_fused_ok: H < 3 || W < 3 refuses; the pool kernels and the two convs run instead (configuration e asserts which)",
}
MUST_SPAN = {
    "conv3x3_ws_kernel": {"64x32-h": ["4x8"], "416x32-h": ["4x52"]},
    "conv3x3_ws_kernel S=2": {"64x32-h": ["4x8"]},
    "conv3x3_wsk_kernel": {"64x32-h": ["4x8"], "416x32-h": ["4x52"]},
    "conv3x3_ws_pair_kernel": {"64x32-g6": ["4x8"], "416x32-g": ["4x52"]},
    "c2f_kernel<16>": {"32x32-c": ["8x8"], "32x416-f": ["104x8"]},
    "stem_model1_kernel": {"32x32-c": ["8x8"], "32x32-f": ["8x8"], "32x416-f": ["104x8"]},
    "sppf_fused_kernel": {"96x96-e": ["3x3"]},
}


# ---------------------------------------------------------------------------------------------------
# stand-in faults that matter on exactly these maps (tests/test_small_map_cases.py)
# ---------------------------------------------------------------------------------------------------
def halo_from_neighbour_frame(x):
    """x [F, C, H, W] padded for a 3 x 3 conv as a kernel with a wrong vertical out-of-range test sees batch-linear NHWC: row -1 of frame f is the last
    row of frame f - 1, row H of frame f is row 0 of frame f + 1 (zeros outside the tensor, zeros left and right)"""
    f, c, h, w = x.shape
    top = torch.cat([torch.zeros_like(x[:1, :, -1:]), x[:-1, :, -1:]], 0)
    bottom = torch.cat([x[1:, :, :1], torch.zeros_like(x[:1, :, :1])], 0)
    return F.pad(torch.cat([top, x, bottom], 2), (1, 1, 0, 0))


def upsample_from_next(t):
    """nearest Upsample x 2 reading source pixel (y >> 1, (x >> 1) + 1), clamped in the last column"""
    w = t.shape[3]
    idx = torch.clamp(torch.arange(2 * w) // 2 + 1, max=w - 1)
    return t.repeat_interleave(2, dim=2)[..., idx]


@contextlib.contextmanager
def first_upsample_replaced(fn):
    """oracle/yolov8_ref.py's first Upsample (into model.12.cv1) computed by fn; the second one as it is"""
    real, calls = yolov8_ref.F.interpolate, []

    def patched(t, scale_factor=2, mode="nearest"):
        calls.append(1)
        return fn(t) if len(calls) == 1 else real(t, scale_factor=scale_factor, mode=mode)
    yolov8_ref.F.interpolate = patched
    try:
        yield
    finally:
        yolov8_ref.F.interpolate = real
