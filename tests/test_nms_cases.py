"""tests/nms_cases.py without a GPU: the case table holds every NMS path and boundary it claims (measured by nms_path on the frames'
actual per-class histograms), the expected-slab builder agrees with an independent numpy NMS, and the helpers bite."""
import numpy as np
import pytest

import nms_cases as nc_
from nms_cases import BIG_N, SMALL_N, all_cases, histogram, lds_cap, nms_path, oracle_slab, table
from oracle_lib import DET_DTYPE


def _paths(N):
    return [(c, histogram(c.frame, c.nc), nms_path(histogram(c.frame, c.nc), c.frame.n, N)) for c in all_cases(N)]


def test_nms_path_restates_the_dispatch():
    for N, cap in ((3549, 1024), (4096, 1024), (4097, 2048), (8400, 2048)):
        assert lds_cap(N) == cap
        assert nms_path([128], 128, N).label == "one_wave" and nms_path([128], 128, N, force_general=True) == ("lds_general", True, False)
        assert nms_path([64, 64, 1], 129, N).label == "segments" and nms_path([65, 64], 129, N) == ("lds_general", True, False)
        assert nms_path([129], 129, N) == ("lds_general", False, True) and nms_path([128, 129], 257, N) == ("lds_general", True, True)
        assert nms_path([64] * (cap // 64), cap, N).label == "segments" and nms_path([64] * (cap // 64) + [1], cap + 1, N).label == "global"
        assert nms_path([cap], cap, N).label == "lds_general" and nms_path([cap + 1], cap + 1, N) == ("global", False, True)
    assert nms_path([2048], 2048, 3549).label == "global" and nms_path([60] * 3, 180, 100).label == "one_wave"     # the kernel clamps n to N
    assert nms_path([], 0, 8400).label == "one_wave" and nms_path([0] * 80, 0, 8400, force_general=True).label == "segments"


@pytest.mark.parametrize("N", BIG_N + SMALL_N)
def test_frames_are_well_formed(N):
    seen = set()
    for g in table(N):
        assert 1 <= len(g.cases) <= 64 and 1 <= g.nc <= 1024 and g.cap >= 1
        for c in g.cases:
            fr = c.frame
            assert c.name not in seen and (c.N, c.nc, c.cap) == (N, g.nc, g.cap) and c.iou_thr == g.iou_thr
            seen.add(c.name)
            assert fr.cand.dtype == nc_.CAND_DTYPE and len(fr.cand) == fr.n <= N
            assert len(np.unique(fr.cand["anchor"])) == fr.n and (fr.n == 0 or (0 <= fr.cand["anchor"].min() and fr.cand["anchor"].max() < N))
            assert not fr.cand["pad_"].any() and (fr.n == 0 or (0 <= fr.cand["cls"].min() and fr.cand["cls"].max() < c.nc))
            assert ((fr.cand["conf"] > 0) & (fr.cand["conf"] <= 1)).all()
            assert nms_path(histogram(fr, c.nc), fr.n, N).label == c.want, c.name          # the path the case was built for
    if N in BIG_N:
        conf = np.concatenate([c.frame.cand["conf"] for c in all_cases(N)])
        assert (conf == 1.0).any() and (conf == nc_.TINY).any()
        ties = 0
        for c in all_cases(N):
            k = np.stack([c.frame.cand["cls"].astype(np.float64), c.frame.cand["conf"].astype(np.float64)], axis=1)
            ties += len(k) - len(np.unique(k, axis=0))
        assert ties > 100                                       # exact (class, confidence) ties: the anchor decides
        arrival = [c.frame for c in all_cases(N) if c.frame.n > 100]
        assert all((np.diff(fr.cand["anchor"]) < 0).any() for fr in arrival)        # arrival order is not anchor order


@pytest.mark.parametrize("N", BIG_N)
def test_table_covers_every_path_cell(N):
    cells = set()
    for c, h, p in _paths(N):
        cells.add(p.label)
        if p.label == "lds_general":
            cells |= {"lds_general/medium"} if p.medium else set()
            cells |= {"lds_general/big"} if p.big else set()
    assert cells == {"one_wave", "segments", "lds_general", "lds_general/medium", "lds_general/big", "global"}
    # ... and inside every launch whose cases were built per path, neighbouring workgroups take different paths
    for g in table(N):
        assert len({c.want for c in g.cases}) == 4, g.key
    # force_general: no frame stays on the one-wave path
    assert all(nms_path(h, c.frame.n, N, force_general=True).label != "one_wave" for c, h, p in _paths(N))


@pytest.mark.parametrize("N", BIG_N)
def test_table_holds_every_boundary(N):
    CAP = lds_cap(N)
    P = _paths(N)

    def on(label):
        return [(c, h) for c, h, p in P if p.label == label]

    ow, seg, lds, glb = on("one_wave"), on("segments"), on("lds_general"), on("global")
    assert {0, 1, 2, 63, 64, 65, 127, 128} <= {c.frame.n for c, _ in ow}
    for n in (63, 64, 65, 127, 128):                            # a single class, and spread over many
        assert any(c.frame.n == n and h.max() == n for c, h in ow) and any(c.frame.n == n and h.max() <= 2 for c, h in ow)
    assert any(c.frame.n == 64 and h.max() == 1 for c, h in ow) and any(c.frame.n == 128 and h.max() == 1 for c, h in ow)      # all classes distinct
    assert any(c.nc == 1024 and h[0] > 0 and h[1023] > 0 for c, h in ow)
    assert any(h[0] == 60 and h[1] == 11 for c, h in ow)        # class 1 holds the sorted positions 60..70
    assert {129, 512, CAP - 1, CAP} <= {c.frame.n for c, _ in seg}
    assert any((h == 1).any() and (h == 64).any() for c, h in seg)
    assert any((h == 64).sum() == CAP // 64 and c.frame.n == CAP for c, h in seg)
    assert any((h > 0).sum() > 8 for c, h in seg)
    assert {65, 80, 1024} <= {c.nc for c, _ in seg} and any(c.nc == 65 and h[64] > 0 for c, h in seg) and any(c.nc == 1024 and h[1023] > 0 for c, h in seg)
    assert {65, 128, 129, 192, 193} <= {int(h.max()) for c, h in lds}
    assert {130, 513, CAP - 1, CAP} <= {c.frame.n for c, _ in lds}
    assert any((h > 128).any() and ((h > 64) & (h <= 128)).any() and ((h > 0) & (h <= 64)).any() for c, h in lds)
    assert any(int(h.max()) % 64 == 1 for c, h in lds)          # a last block of one member
    assert {CAP + 1, N} <= {c.frame.n for c, _ in glb} and any(1.4 * CAP < c.frame.n < 1.6 * CAP for c, _ in glb)
    for n in (CAP + 1, N):
        assert any(c.frame.n == n and (h > 0).sum() == 1 for c, h in glb) and any(c.frame.n == n and (h > 0).sum() == 80 for c, h in glb)
    assert any((h > 128).any() and ((h > 64) & (h <= 128)).any() and ((h > 1) & (h <= 64)).any() for c, h in glb)
    assert {65, 1024} <= {c.nc for c, _ in lds} and {65, 1024} <= {c.nc for c, _ in glb}
    # thresholds and capacities: each on all four paths
    t = nc_.pair_iou()
    for g in table(N):
        if g.key != "default" and not g.key.startswith("nc"):
            assert {c.want for c in g.cases} == {"one_wave", "segments", "lds_general", "global"}, g.key
    thr = {g.key: g.iou_thr for g in table(N)}
    assert thr["thr_eq"] == t and thr["thr_below"] == np.nextafter(t, np.float32(0)) and thr["thr_above"] == np.nextafter(t, np.float32(1))
    assert thr["thr_0"] == 0.0 and thr["thr_1"] == 1.0
    assert {g.key: g.cap for g in table(N)}["cap1"] == 1


def test_threshold_pair_is_the_oracles(oracle):
    a, b = nc_.PAIR
    t = nc_.pair_iou()
    assert np.float32(oracle.iou(a[:4], b[:4])) == t and 0 < t < 1
    for g in table(3549):
        if not g.key.startswith("thr_"):
            continue
        for c in g.cases:                                       # the pair's second box survives exactly when IoU > thr fails
            kept = nc_.oracle_kept(c.frame, c.iou_thr, oracle)
            k0 = kept[kept["class_id"] == 0]
            b_kept = bool(((k0["x"] == np.float32(b[0])) & (k0["w"] == np.float32(b[2]))).any())
            assert b_kept == (g.key in ("thr_eq", "thr_above", "thr_1")), c.name
            zero_w = int((k0["w"] == 0).sum())
            assert zero_w == 3                                  # zero-width boxes: IoU 0, never suppressed -- not even at iou_thr = 0


@pytest.mark.parametrize("N", BIG_N)
def test_capacity_cases_hit_the_cap_exactly(N, oracle):
    for g in table(N):
        if g.key == "cap100":
            kept = sorted(len(nc_.oracle_kept(c.frame, c.iou_thr, oracle)) for c in g.cases)
            assert kept == [100] * 4 + [101] * 4                # n_kept == cap and n_kept > cap on each of the four paths
        if g.key == "cap1":
            assert all(len(nc_.oracle_kept(c.frame, c.iou_thr, oracle)) > 1 for c in g.cases)
    blocks = {c.frame.name: nc_.oracle_kept(c.frame, c.iou_thr, oracle) for c in table(N)[0].cases if "crowd" in c.frame.name}
    assert len(blocks["lds_crowd_identical"][blocks["lds_crowd_identical"]["class_id"] == 0]) == 1        # the first kills all
    assert len(blocks["lds_crowd_disjoint_63_survivors_per_block"]) == 63 * 3 + 7                         # no block's survivors are a multiple of 4
    k = blocks["lds_crowd_block_without_survivor"]
    assert len(k[k["class_id"] == 0]) == 260 - 64                                                          # the third block dies by the first


# ---------------------------------------------------------------------------------------------------
# oracle_slab against an independent NMS, and the helpers' bite
# ---------------------------------------------------------------------------------------------------
def _numpy_nms(cand, thr):
    """greedy class-aware NMS in float32: order by (class asc, confidence desc, anchor asc), suppress on IoU > thr"""
    c = cand[np.lexsort((cand["anchor"], -cand["conf"].astype(np.float64), cand["cls"]))]
    dead = np.zeros(len(c), dtype=bool)
    for i in range(len(c)):
        if dead[i]:
            continue
        for j in range(i + 1, len(c)):
            if not dead[j] and c["cls"][j] == c["cls"][i] and nc_.iou_f32(list(c[i])[:4], list(c[j])[:4]) > np.float32(thr):
                dead[j] = True
    return c[~dead]


def _small_frames():
    return [nc_.frame_random("small_one_class", 1, 3549, {2: 40}),
            nc_.frame_random("small_three_classes", 2, 3549, {0: 20, 7: 15, 79: 9}),
            nc_.frame_layout("small_identical", 3, 3549, {4: 12}, "identical"),
            nc_.frame_layout("small_cluster", 4, 3549, {1: 30, 2: 30}, "cluster", 7),
            nc_.frame_edge("small_edge", 5, 3549, [(2, 10, "random", None)])]


@pytest.mark.parametrize("cap", [1, 16, 64])
def test_oracle_slab_agrees_with_numpy_nms(oracle, cap):
    for i, fr in enumerate(_small_frames()):
        thr = np.float32(0.45) if i < 4 else nc_.pair_iou()
        slab = oracle_slab(fr, cap, 0xFFFFFFFE + i, thr, oracle)
        want = _numpy_nms(fr.cand, thr)
        assert 0 < len(want) < fr.n or fr.name == "small_edge"
        hdr = slab[:16].view(nc_.HDR_DTYPE)[0]
        assert (hdr["n_kept"], hdr["n_candidates"], hdr["flags"], hdr["frame_tag"]) == (len(want), fr.n, int(len(want) > cap), (0xFFFFFFFE + i) & 0xFFFFFFFF)
        m = min(len(want), cap)
        dets = slab[16:16 + 40 * m].view(DET_DTYPE)
        for a, b in (("x", "x"), ("y", "y"), ("w", "w"), ("h", "h"), ("confidence", "conf"), ("class_id", "cls")):
            assert np.array_equal(dets[a].view(np.uint32), want[b][:m].view(np.uint32)), (fr.name, a)
        assert not dets["track_id"].any() and not dets["pad_"].any() and not dets["timestamp"].any()
        assert (slab[16 + 40 * m:] == nc_.SLAB_FILL).all() and len(slab) == 16 + 40 * cap


def test_helpers_bite(oracle):
    fr = _small_frames()[0]
    thr = np.float32(0.45)
    base = oracle_slab(fr, 64, 7, thr, oracle)
    assert np.array_equal(base, oracle_slab(fr, 64, 7, thr, oracle))
    # one suppression flipped: the first suppressed candidate (in sorted order) is moved away from everything
    kept = nc_.oracle_kept(fr, thr, oracle)
    order = np.lexsort((fr.cand["anchor"], -fr.cand["conf"].astype(np.float64), fr.cand["cls"]))
    lost = [i for i in order if not ((kept["x"] == fr.cand["x"][i]) & (kept["y"] == fr.cand["y"][i]) & (kept["confidence"] == fr.cand["conf"][i])).any()]
    moved = fr.cand.copy()
    moved["x"][lost[0]] += 5.0
    assert not np.array_equal(base, oracle_slab(nc_.Frame("flip", moved, fr.n), 64, 7, thr, oracle))
    # a stale candidate counted in: the hostile tail's first record read as live
    cand, counts = nc_.build_batch([fr], 3549, "hostile", seed=1)
    assert counts[0] == fr.n and np.array_equal(cand[0, :fr.n], fr.cand)
    one_more = nc_.Frame("stale", cand[0, :fr.n + 1].copy(), fr.n + 1)
    got = oracle_slab(one_more, 64, 7, thr, oracle)
    assert not np.array_equal(base[16:], got[16:]) and not np.array_equal(base[:16], got[:16])
    # a frame tag off by one, a cap off by one, another fill byte
    assert not np.array_equal(base, oracle_slab(fr, 64, 8, thr, oracle))
    assert np.array_equal(base[:12], oracle_slab(fr, 64, 8, thr, oracle)[:12])
    assert not np.array_equal(base, oracle_slab(fr, 64, 7, thr, oracle, fill=0))
    n_kept = int(base[:4].view(np.int32)[0])
    assert oracle_slab(fr, n_kept, 7, thr, oracle)[8] == 0 and oracle_slab(fr, n_kept - 1, 7, thr, oracle)[8] == 1      # overflow only above the cap


def test_build_batch_tails():
    frames = [c.frame for c in table(3549)[0].cases[:6]]
    for stale in ("hostile", "next"):
        cand, counts = nc_.build_batch(frames, 3549, stale, seed=3)
        assert cand.shape == (6, 3549) and list(counts) == [f.n for f in frames]
        for f, fr in enumerate(frames):
            assert np.array_equal(cand[f, :fr.n], fr.cand)
            tail = cand[f, fr.n:]
            if stale == "hostile":
                live = set(fr.cand["cls"].tolist()) | {0}
                assert set(tail["cls"].tolist()) <= live and (tail["conf"] > 1.0).all() and (tail["w"] == 1).all()
                assert 0 < (tail["pad_"] == 0).sum() and abs(int((tail["pad_"] == 0).sum()) - int((tail["pad_"] == 1).sum())) <= 1
            else:
                nx = frames[(f + 1) % 6]
                assert nx.n == 0 or np.array_equal(tail[:min(nx.n, len(tail))], nx.cand[:min(nx.n, len(tail))])
