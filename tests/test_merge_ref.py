"""CPU tests of the tile merge's rule (include/zly.h, "Tiles"): the numpy oracle tests/merge_ref.py on the hand cases of tests/merge_cases.py,
whose expected survivors are written out by hand; zly_tile_grid through ctypes against the oracle's integers; the struct sizes.  The
perturbation tests show, in the manner of tests/test_parity_helpers_bite.py, that the hand cases notice a rule with >= in place of > and a rule
without the tie-break -- the same cases hold the GPU to the byte in tests/test_gpu_merge.py.
"""
import ctypes as C
import os

import numpy as np
import pytest

import merge_cases as mc
import merge_ref
import zly

HAND = mc.hand_cases()


def _oracle(case, **perturb):
    before = np.full((case.n_groups, mc.slab_bytes(case.cap)), mc.POISON, dtype=np.uint8)
    return merge_ref.merge_slabs(mc.case_raw(case), case.tiles, case.n_groups, case.cap, case.metric, case.thr, mc.TAG0, before, **perturb)


@pytest.mark.parametrize("case", HAND, ids=[c.name for c in HAND])
def test_oracle_on_hand_case(case):
    got, want = _oracle(case), mc.hand_expected(case)
    assert np.array_equal(got, want), (case.name, np.flatnonzero(got != want)[:8].tolist())


def test_hand_cases_cover_what_the_issue_lists():
    names = {c.name for c in HAND}
    for must in ("seam_duplicate_removed_by_iou", "cut_box_kept_by_iou", "cut_box_removed_by_ios", "iou_equal_to_threshold_kept",
                 "iou_one_ulp_above_threshold_removed", "different_classes_never_suppress", "tie_broken_by_slab_index", "tie_broken_by_position",
                 "chain_b_dies_c_lives", "source_n_kept_above_cap", "source_n_kept_negative_is_empty", "merged_count_above_cap", "empty_group",
                 "group_minus_1_left_out", "interleaved_groups", "zero_area_boxes_survive", "whole_surface_beside_quarters"):
        assert must in names, must
    over = next(c for c in HAND if c.name == "source_n_kept_above_cap")
    hdr = _oracle(over)[0, :16].view(zly.SLAB_HDR_DTYPE)[0]
    assert (int(hdr["n_kept"]), int(hdr["n_candidates"]), int(hdr["flags"])) == (8, 8, zly.SLAB_OVERFLOW)         # the source's flag, not the merged count
    many = next(c for c in HAND if c.name == "merged_count_above_cap")
    hdr = _oracle(many)[0, :16].view(zly.SLAB_HDR_DTYPE)[0]
    assert (int(hdr["n_kept"]), int(hdr["n_candidates"]), int(hdr["flags"])) == (12, 12, zly.SLAB_OVERFLOW)


def _failing(**perturb):
    return {c.name for c in HAND if not np.array_equal(_oracle(c, **perturb), mc.hand_expected(c))}


def test_a_rule_with_greater_or_equal_fails_the_hand_cases():
    bad = _failing(strict=False)
    assert {"iou_equal_to_threshold_kept", "ios_equal_to_threshold_kept", "zero_area_boxes_survive"} <= bad, bad


def test_a_rule_without_the_tie_break_fails_the_hand_cases():
    bad = _failing(tie_break=False)
    assert {"tie_broken_by_slab_index", "tie_broken_by_slab_index_swapped", "tie_broken_by_position", "tie_of_signed_zeros", "merged_count_above_cap"} <= bad, bad


def test_vector_measure_is_the_scalar_measure():
    """merge_group's inner loop runs measure() over float32 arrays; both must round alike, zero-area and disjoint boxes included"""
    rng = np.random.default_rng(5)
    n = 400
    b = [rng.uniform(.2, .8, n).astype(np.float32), rng.uniform(.2, .8, n).astype(np.float32),
         rng.uniform(0, .4, n).astype(np.float32), rng.uniform(0, .4, n).astype(np.float32)]
    b[2][:20] = 0
    b[3][10:30] = 0
    for a in ((np.float32(.5), np.float32(.5), np.float32(.3), np.float32(.2)), (np.float32(.4), np.float32(.6), np.float32(0), np.float32(.2))):
        for metric in (merge_ref.IOU, merge_ref.IOS):
            vec = merge_ref.measure_many(a, tuple(b), metric)
            one = np.array([merge_ref.measure(a, (b[0][k], b[1][k], b[2][k], b[3][k]), metric) for k in range(n)], dtype=np.float32)
            assert np.array_equal(vec.view(np.uint32), one.view(np.uint32))
            assert (vec == 0).sum() > 20 and (a[2] == 0 or (vec > 0).sum() > 50)


def test_scenes_hold_what_they_are_meant_to():
    """on the oracle: every scene has exactly the candidate count it names, and candidates are suppressed and survive in it"""
    suppressed = 0
    for (sc, target), name in zip(mc.SCENE_PARAMS, mc.SCENE_IDS):
        st = mc.scene_stats(sc, target)
        if target is not None:
            assert st["M"] == target, name
        assert len(mc.scene_tiles(sc)) * sc.cap <= merge_ref.MAX_CANDIDATES
        if st["M"] > 2:
            assert 0 < st["kept"] < st["M"], (name, st)
        suppressed += st["M"] - st["kept"]
    assert suppressed > 500
    sizes = sorted(t for sc in mc.SCENES for t in sc.targets if t is not None)
    for edge in (64, 128, 256, 512, 1024, 2048):
        assert {edge - 1, edge, edge + 1} <= set(sizes), edge                    # a block of 64 sorted positions, a power of two of the sort
    assert sizes[0] == 0 and sizes[-1] == merge_ref.MAX_CANDIDATES == zly.MERGE_MAX_CANDIDATES


# ---- zly_tile_grid ---------------------------------------------------------------------------------------------------------------
_GRID_BUF = (zly.Tile * 4096)()


def _grid(W, H, tw, th, ox, oy, even):
    """zly_tile_grid in one call: the tiles as tuples, None for ZLY_ERR_INVALID_ARGUMENT (which must leave the count alone)"""
    lib = zly.load_library()
    n = C.c_int32(-1)
    rc = lib.zly_tile_grid(W, H, tw, th, ox, oy, even, _GRID_BUF, len(_GRID_BUF), C.byref(n))
    if rc != zly.OK:
        assert rc == zly.ERR_INVALID_ARGUMENT and n.value == -1
        return None
    assert 1 <= n.value <= len(_GRID_BUF)
    return [(t.group, t.x0, t.y0, t.w, t.h, t.W, t.H) for t in _GRID_BUF[:n.value]]


@pytest.mark.parametrize("tile,overlap", [((8, 8), (0, 0)), ((8, 6), (3, 1)), ((16, 12), (15, 4)), ((5, 7), (2, 6)), ((40, 40), (8, 8)), ((2, 2), (1, 0))])
def test_tile_grid_against_the_oracle_for_every_small_surface(tile, overlap):
    for even in (0, 1):
        for W in range(1, 41):
            for H in range(1, 41):
                got, want = _grid(W, H, tile[0], tile[1], overlap[0], overlap[1], even), merge_ref.tile_grid(W, H, tile[0], tile[1], overlap[0], overlap[1], bool(even))
                assert got == want, (W, H, tile, overlap, even, got, want)


def test_tile_grid_properties_and_refusals():
    # every tile full-sized and inside; the tiles cover the surface; even grids have even origins
    for W, H, t, o, even in ((1920, 1080, 640, 128, 1), (3840, 2160, 416, 64, 1), (101, 77, 32, 5, 0), (128, 96, 80, 32, 1)):
        tiles = merge_ref.tile_grid(W, H, t, t, o, o, bool(even))
        assert _grid(W, H, t, t, o, o, even) == tiles
        cover = np.zeros((H, W), dtype=bool)
        for g, x0, y0, w, h, sw, sh in tiles:
            assert (g, w, h, sw, sh) == (0, min(t, W), min(t, H), W, H) and x0 >= 0 and y0 >= 0 and x0 + w <= W and y0 + h <= H
            assert not even or (x0 % 2 == 0 and y0 % 2 == 0)
            cover[y0:y0 + h, x0:x0 + w] = True
        assert cover.all()
    assert len(merge_ref.tile_grid(3840, 2160, 640, 640, 128, 128)) == 8 * 4
    assert zly.tile_grid(128, 96, 80, 80, 32, 32)[3].x0 == 48 and [(t.x0, t.y0) for t in zly.tile_grid(128, 96, 80, 80, 32, 32, even=True)] == [(0, 0), (48, 0), (0, 16), (48, 16)]
    for bad in ((0, 8, 4, 4, 0, 0, 0), (8, 0, 4, 4, 0, 0, 0), (1 << 24, 8, 4, 4, 0, 0, 0), (8, 1 << 24, 4, 4, 0, 0, 0), (8, 8, 0, 4, 0, 0, 0), (8, 8, 4, -1, 0, 0, 0),
                (8, 8, 4, 4, 4, 0, 0), (8, 8, 4, 4, 0, 5, 0), (8, 8, 4, 4, -1, 0, 0), (9, 8, 4, 4, 0, 0, 1), (8, 8, 3, 4, 0, 0, 1), (8, 8, 4, 5, 0, 0, 1), (8, 7, 16, 16, 0, 0, 1)):
        assert _grid(*bad) is None and merge_ref.tile_grid(*bad[:6], bool(bad[6])) is None, bad
    lib = zly.load_library()
    out, n = (zly.Tile * 2)(), C.c_int32(-1)
    assert lib.zly_tile_grid((1 << 24) - 1, 2, 1, 2, 0, 0, 0, None, 0, C.byref(n)) == zly.OK and n.value == (1 << 24) - 1        # the count alone
    n.value = -1
    assert lib.zly_tile_grid(8, 8, 4, 4, 0, 0, 0, out, 2, None) == zly.ERR_INVALID_ARGUMENT
    assert lib.zly_tile_grid(8, 8, 4, 4, 0, 0, 0, None, 2, C.byref(n)) == zly.ERR_INVALID_ARGUMENT and n.value == -1
    assert lib.zly_tile_grid(8, 8, 4, 4, 0, 0, 0, out, -1, C.byref(n)) == zly.ERR_INVALID_ARGUMENT
    # a capacity below the count: the first tiles are written, the count is reported
    assert lib.zly_tile_grid(8, 8, 4, 4, 0, 0, 0, out, 2, C.byref(n)) == zly.OK and n.value == 4 and [(t.x0, t.y0) for t in out] == [(0, 0), (4, 0)]


def test_struct_sizes_and_defaults():
    assert C.sizeof(zly.Tile) == 28 and C.sizeof(zly.MergeConfig) == 8
    c = zly.merge_config()
    assert (c.metric, c.thr) == (zly.MERGE_IOS, 0.5) and (zly.MERGE_IOU, zly.MERGE_IOS) == (merge_ref.IOU, merge_ref.IOS) == (0, 1)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "zly.h")).read()
    assert "#define ZLY_MERGE_MAX_CANDIDATES 4096" in hdr and "#define ZLY_MERGE_IOU 0" in hdr and "#define ZLY_MERGE_IOS 1" in hdr
    # every argument error of a merge is refused before the device is touched: without an engine the call answers NOT_INITIALIZED
    lib = zly.load_library()
    assert lib.zly_merge_slabs(None, 1, None, 1, None, None, None, 0, None) == zly.ERR_NOT_INITIALIZED
    assert lib.zly_read_merged(None, 1, None) == zly.ERR_NOT_INITIALIZED
    assert lib.zly_detect_tiled(None, None, 0, None, 1, None, None, None, 0, None) == zly.ERR_NOT_INITIALIZED
