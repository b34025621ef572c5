"""c2f_kernel (run on the MI355X box: pytest -m gpu) at the smallest tile shapes at which its pixel enumerations can go wrong.  cv1 walks the
(TH+4) x (TW+4) patch as ring tiles (the 2-pixel halo: y1 only) followed by interior tiles (y0 | y1), and cv2 takes the bottleneck's output from
the registers of conv B's epilogue, at most four pixel tiles per wave -- per-pixel arithmetic does not depend on the tiling, so an engine with a
forced tile shape (ZLY_C2F_TILE, read per engine at create) must give the BITS of the engine with the planned shapes, on every tap of the four
fused blocks (FLAG_DUMP_LOGITS exposes the LDS-resident ones) and on the head tensor.  What the shapes are for:
  * 416 x 416, n = 4, tile 4 x 8: the minimal tile.  The ring (4*12 + 4*4 = 64 pixels) is larger than the interior (32), its segments are shorter
    than 16 pixels, so one MFMA tile spans top rows, bottom rows and side columns; every launch has more tiles than workgroups (model.2: 1352,
    model.4 / model.15: 364), so the persistent loop and the prefetch across tiles run;
  * 352 x 288, n = 3, tile 5 x 11: ragged 88 x 72 and 44 x 36 maps, partial tiles on the right and bottom edges; 55 pixels per tile is no multiple
    of 16, so the lanes past the tile (clamped indices, nothing stored) are exercised;
  * 320 x 256, n = 2, tile 7 x 9 against the planned tile: the dual-source cv1 of model.15 on 40 x 32 maps.
Each engine is also checked per element against float64 on its own inputs (tests/closed_loop_ref.py, all 63 convs), and a forced-tile engine
without the dump flag must give the same head bits.

Those tiles give every wave at most one pixel tile of conv B / cv2, so a second test forces tiles LARGER than the planned ones: there a wave carries
the results of two or three pixel tiles in registers (the selects on the wave-uniform tile count), cv2's fragments are requested one tile ahead and
rotated.  What the LDS budget and the staging registers allow (c2f_plan) decides the shapes:
  * 352 x 288, n = 2, tile 13 x 26, 16 waves: the back half of model.4 has 22 pixel tiles per workgroup tile, two for waves 0..5, on ragged maps
    (the headline's shape); model.15's whole block does not fit the LDS with a tile of more than 16 pixel tiles and runs unfused;
  * 416 x 416, n = 2, ZLY_C2F32_NW=8, tile 12 x 13: 10 pixel tiles on 8 waves in the back half AND in model.15 (ring tiles, y0 map, dual source);
  * 416 x 416, n = 2, ZLY_C2F32_NW=8, tile 16 x 17: 17 pixel tiles on 8 waves in the back half, three for wave 0 (model.15 unfused again).
Each case asserts that ceil(TH * TW / 16) exceeds NW (twice NW in the last), so that it cannot silently fall back to one tile per wave."""
import re

import numpy as np
import pytest

import zly
import zly_model as zm
from closed_loop_ref import check_closed_loop, lds_resident_from_kernels

pytestmark = pytest.mark.gpu

C2F_TAPS = ("model.2.cv1", "model.2.m.0.cv2", "model.2.cv2", "model.4.cv1", "model.4.m.0.cv2", "model.4.m.1.cv2", "model.4.cv2",
            "model.15.cv1", "model.15.m.0.cv2", "model.15.cv2")
LDS_RESIDENT = {"model.2.m.0.cv1", "model.4.m.0.cv1", "model.4.m.1.cv1", "model.15.m.0.cv1"}


def _engine(monkeypatch, tile, w, h, n, flags, nw=None, fused=4):
    for k in ("ZLY_C2F_TILE", "ZLY_C2F32_NW"):
        monkeypatch.delenv(k, raising=False)
    if tile:
        monkeypatch.setenv("ZLY_C2F_TILE", tile)
    if nw:
        monkeypatch.setenv("ZLY_C2F32_NW", str(nw))
    e = zly.Engine(model_w=w, model_h=h, max_batch=n, warmup_runs=0, flags=flags)
    kernels = e.op_kernels(n)
    assert sum("c2f_kernel" in k for k in kernels) == fused, (tile, kernels)
    return e


def _tile_of(kernel_name):
    """'c2f_kernel<C=32,NW=16,bottleneck+cv2,13x26 tiles>' -> (13, 26)"""
    m = re.search(r",(\d+)x(\d+) tiles>", kernel_name)
    assert m, kernel_name
    return int(m.group(1)), int(m.group(2))


@pytest.mark.parametrize("w,h,n,tile", [(416, 416, 4, "4,8"), (352, 288, 3, "5,11"), (320, 256, 2, "7,9")])
def test_forced_tile_gives_the_planned_tiles_bits(monkeypatch, w, h, n, tile):
    frames = zm.synth_frames(n, w, h, seed=37, rects=False)
    want_tile = tuple(int(v) for v in tile.split(","))
    # the engine with the planned tile shapes: the reference bits (and itself against float64)
    ref = _engine(monkeypatch, None, w, h, n, zly.FLAG_DUMP_LOGITS)
    x = np.stack([ref.preprocess(f) for f in frames])
    planned = [_tile_of(k) for k in ref.op_kernels(n) if "c2f_kernel" in k]
    want_head = ref.forward(x)
    want = {nm: [ref.tap(nm, i) for i in range(n)] for nm in C2F_TAPS}
    lds = lds_resident_from_kernels(ref, n)
    assert lds == LDS_RESIDENT, lds
    assert len(check_closed_loop(ref, zly.DEFAULT_WEIGHTS, (0, n - 1), lds_resident=lds)) == 63
    ref.close()
    # the forced shape, dumps on
    e = _engine(monkeypatch, tile, w, h, n, zly.FLAG_DUMP_LOGITS)
    forced = [_tile_of(k) for k in e.op_kernels(n) if "c2f_kernel" in k]
    assert all(t == want_tile for t in forced), forced
    assert any(t != want_tile for t in planned), planned                # the two engines really tile differently
    got_head = e.forward(x)
    for nm in C2F_TAPS:
        for i in range(n):
            g = e.tap(nm, i)
            assert g.shape == want[nm][i].shape and np.array_equal(g, want[nm][i]), (nm, i, float(np.mean(g != want[nm][i])))
            assert np.isfinite(g).all() and np.abs(g).max() > 0, (nm, i)
    assert np.array_equal(got_head, want_head)
    lds = lds_resident_from_kernels(e, n)
    assert lds == LDS_RESIDENT, lds
    assert len(check_closed_loop(e, zly.DEFAULT_WEIGHTS, (0, n - 1), lds_resident=lds)) == 63
    e.close()
    # ... and without the dumps (the intermediates stay in LDS / registers): the same head
    e = _engine(monkeypatch, tile, w, h, n, 0)
    assert np.array_equal(e.forward(x), want_head)
    with pytest.raises(zly.ZlyError):
        e.tap("model.15.m.0.cv2", 0)
    e.close()


M24_TAPS = tuple(t for t in C2F_TAPS if not t.startswith("model.15."))


@pytest.mark.parametrize("w,h,n,nw,tile,rounds,fused", [(352, 288, 2, 16, "13,26", 2, 3), (416, 416, 2, 8, "12,13", 2, 4), (416, 416, 2, 8, "16,17", 3, 3)])
def test_several_pixel_tiles_per_wave_carried_to_cv2(monkeypatch, w, h, n, nw, tile, rounds, fused):
    frames = zm.synth_frames(n, w, h, seed=41, rects=False)
    th, tw = (int(v) for v in tile.split(","))
    assert -(-th * tw // 16) > (rounds - 1) * nw                       # some wave has `rounds` pixel tiles of conv B / cv2
    ref = _engine(monkeypatch, None, w, h, n, zly.FLAG_DUMP_LOGITS)      # planned shapes: one pixel tile per wave at most
    x = np.stack([ref.preprocess(f) for f in frames])
    assert all(-(-a * b // 16) <= 16 for a, b in (_tile_of(k) for k in ref.op_kernels(n) if "c2f_kernel<C=32" in k))
    taps = C2F_TAPS if fused == 4 else M24_TAPS
    want_head = ref.forward(x)
    want = {nm: [ref.tap(nm, i) for i in range(n)] for nm in taps}
    ref.close()
    for flags in (zly.FLAG_DUMP_LOGITS, 0):
        e = _engine(monkeypatch, tile, w, h, n, flags, nw=None if nw == 16 else nw, fused=fused)
        carried = [k for k in e.op_kernels(n) if k.startswith("c2f_kernel<C=32") and "bottleneck+cv2" in k]      # back half (+ whole block)
        assert len(carried) == fused - 2 and all(_tile_of(k) == (th, tw) and f"NW={nw}," in k for k in carried), carried
        got_head = e.forward(x)
        if flags:
            for nm in taps:
                for i in range(n):
                    g = e.tap(nm, i)
                    assert g.shape == want[nm][i].shape and np.array_equal(g, want[nm][i]), (nm, i, float(np.mean(g != want[nm][i])))
            assert len(check_closed_loop(e, zly.DEFAULT_WEIGHTS, (0, n - 1), lds_resident=lds_resident_from_kernels(e, n))) == 63
        else:                                                            # block outputs reach HBM without the dumps too
            for nm in ("model.4.cv2",) + (("model.15.cv2",) if fused == 4 else ()):
                assert np.array_equal(e.tap(nm, n - 1), want[nm][n - 1]), nm
        if fused == 4:                                                   # every launch up to the head computes the same bits
            assert np.array_equal(got_head, want_head)
        e.close()
