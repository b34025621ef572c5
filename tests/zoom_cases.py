"""Hand-made tables for the zoom regions' plan (include/zly.h, "Zoom regions") with the regions they must give, WRITTEN BY HAND from the rule -- the
arithmetic is in the comments -- and seeded random tables.  Shared by the oracle's own test (test_zoom_ref.py), the test of the stand-alone CPU
program (test_zoom_plan.py) and the GPU test (test_gpu_zoom.py).

A case is (name, Table, Config, W, H, expected) with expected = [(x0, y0, slot)] * K, slot = -1 for a fallback; a region's w, h are step 1's rw, rh.
Unless a case says otherwise: a 640 x 480 surface, K = 3 regions of 208 x 208, max_age = 2, any class -- so rw = rh = 208, xmax = 432, ymax = 272,
the fallback is (216, 136), and a region spans 208/640 = 0.325 of the width and 208/480 = 0.4333 of the height.
"""
import numpy as np

from zoom_ref import Config, F, Table

W0, H0 = 640, 480
CFG0 = Config(regions=3, region_w=208, region_h=208, max_age=2, class_id=-1)
FB0 = (216, 136, -1)
UP, DOWN = F(np.inf), F(-np.inf)


def _f(bits):
    return np.array(bits, dtype=np.uint32).view(np.float32)[()]


# A prediction that tells "the product is rounded first" from a fused multiply-add.  x = 0.5060128 (0x3f018a0e), vx = 0.0020134549 (0x3b03f42b) and
# dtf = 3: fl(vx * 3) = 0.0060403645, and x + that rounds to px = 0.51205313 (0x3f0315ea); the exact x + vx * 3 lies just beyond the midpoint to the
# next float, so an fma gives 0x3f0315eb.  On a surface 1203 wide: px * 1203 = 615.99994 -> cx = 615 -> 511 -> x0 = 510; the fma's 616.00000 ->
# cx = 616 -> x0 = 512.  The velocity is what the motion tracker gets from a box born at FUSED_X1 and matched three frames later at FUSED_X2
# (vx = fl(fl(x2 - x1) / 3), the first match taking the whole residual), which is how the GPU test builds the table.
FUSED_X1, FUSED_X2, FUSED_VX = _f(0x3efffc63), _f(0x3f018a0e), _f(0x3b03f42b)
FUSED_W, FUSED_SIZE, FUSED_X0, FUSED_X0_IF_FUSED = 1203, 0.02, 510, 512


def _table(frame_no, slots, T=64):
    """slots: dicts of Table.add's arguments, keyed 'slot' for their index (default: in order); the rest of the T slots are free"""
    t = Table(frame_no=frame_no)
    for _ in range(T):
        t.add(0, 0, 0, 0, live=False, id=0)
    for i, s in enumerate(slots):
        s = dict(s)
        k = s.pop("slot", i)
        s.setdefault("last_seen", frame_no)
        s.setdefault("id", 100 + k)
        t.live[k] = s.get("live", True)
        t.box[k] = (F(s["x"]), F(s["y"]), F(s["w"]), F(s["h"]))
        t.cls[k], t.id[k], t.last_seen[k] = s.get("cls", 0), s["id"], s["last_seen"] & 0xFFFFFFFF
        t.vx[k], t.vy[k] = F(s.get("vx", 0)), F(s.get("vy", 0))
    return t


def hand_cases():
    cases = []

    def add(name, t, expected, cfg=CFG0, W=W0, H=H0):
        assert len(expected) == cfg.regions
        cases.append((name, t, cfg, W, H, expected))

    # no eligible slot at all: three fallbacks
    add("none", _table(5, []), [FB0, FB0, FB0])

    # left border, top border, bottom-right corner.  Areas ascending with the slot, so the order is 0, 1, 2.
    #   slot 0 (0.01, 0.5): cx = int(6.4) = 6 -> max(6 - 104, 0) = 0; cy = 240 -> 136
    #   slot 1 (0.5, 0.01): cx = 320 -> 216; cy = int(4.8) = 4 -> 0
    #   slot 2 (0.99, 0.99): cx = int(633.6) = 633 -> 529 -> xmax 432; cy = int(475.2) = 475 -> 371 -> ymax 272
    add("left-top-corner_br", _table(3, [dict(x=0.01, y=0.5, w=0.05, h=0.05), dict(x=0.5, y=0.01, w=0.06, h=0.05), dict(x=0.99, y=0.99, w=0.07, h=0.05)]),
        [(0, 136, 0), (216, 0, 1), (432, 272, 2)])
    # right border, bottom border, top-left corner
    add("right-bottom-corner_tl", _table(3, [dict(x=0.99, y=0.5, w=0.05, h=0.05), dict(x=0.5, y=0.99, w=0.06, h=0.05), dict(x=0.005, y=0.005, w=0.07, h=0.05)]),
        [(432, 136, 0), (216, 272, 1), (0, 0, 2)])
    # top-right and bottom-left corners, and the centre: (0.5, 0.5) -> (320 - 104, 240 - 104)
    add("corner_tr-corner_bl-centre", _table(3, [dict(x=0.99, y=0.01, w=0.05, h=0.05), dict(x=0.01, y=0.99, w=0.06, h=0.05), dict(x=0.5, y=0.5, w=0.07, h=0.05)]),
        [(432, 0, 0), (0, 272, 1), (216, 136, 2)])

    # odd W and H: 641 x 479 -> xmax = 433 & ~1 = 432, ymax = 271 & ~1 = 270; fallback (433 // 2 = 216, 271 // 2 = 135 -> 134)
    #   (0.99, 0.99): cx = int(634.59) = 634 -> 530 -> 432; cy = int(474.21) = 474 -> 370 -> 270
    add("odd-surface", _table(3, [dict(x=0.99, y=0.99, w=0.05, h=0.05)]), [(432, 270, 0), (216, 134, -1), (216, 134, -1)], W=641, H=479)

    # a surface smaller than the region: 101 x 77 -> rw = 100, rh = 76, xmax = ymax = 0: one possible origin.  Slot 0 (w * 101 = 50.5 <= 100 fits) gets it;
    # slot 1 (larger area, so later) lies inside [0, 100/101] x [0, 76/77] and is covered
    add("small-surface", _table(3, [dict(x=0.7, y=0.3, w=0.5, h=0.1), dict(x=0.5, y=0.5, w=0.5, h=0.5)]), [(0, 0, 0), (0, 0, -1), (0, 0, -1)], W=101, H=77)

    # ties in age and area are broken by the slot index: slots 5, 2, 9 -> 2, 5, 9
    #   slot 2 (0.2, 0.2): cx = 128 -> 24, cy = 96 -> 0;  slot 5 (0.8, 0.2): cx = 512 -> 408;  slot 9 (0.2, 0.8): cy = 384 -> 280 -> 272
    add("tie-by-slot", _table(3, [dict(slot=5, x=0.8, y=0.2, w=0.05, h=0.05), dict(slot=2, x=0.2, y=0.2, w=0.05, h=0.05), dict(slot=9, x=0.2, y=0.8, w=0.05, h=0.05)]),
        [(24, 0, 2), (408, 0, 5), (24, 272, 9)])
    # age goes before area: slot 1 (age 0, large) before slot 0 (age 1, small)
    add("age-before-area", _table(4, [dict(x=0.2, y=0.2, w=0.02, h=0.02, last_seen=3), dict(x=0.8, y=0.8, w=0.2, h=0.2)]), [(408, 272, 1), (24, 0, 0), FB0])
    # +0 and -0 areas tie (as bit patterns -0 would come first): slot order
    add("zero-areas", _table(3, [dict(x=0.2, y=0.2, w=0.0, h=0.05), dict(x=0.8, y=0.8, w=-0.0, h=0.05)]), [(24, 0, 0), (408, 272, 1), FB0])

    # covered: slot 0's region (216, 136) spans x in [0.3375, 0.6625], y in [0.2833, 0.7167]; slot 1 (0.6, 0.6, 0.1 x 0.1) lies inside
    add("covered", _table(3, [dict(x=0.5, y=0.5, w=0.05, h=0.05), dict(x=0.6, y=0.6, w=0.1, h=0.1)]), [(216, 136, 0), FB0, FB0])
    # ... and the edges of coverage to the ulp.  The probe (slot 1) is 0.0625 wide, so its half width 0.03125 and the sums below are exact.
    a, b = F(F(216) / F(640)), F(F(424) / F(640))
    half = F(0.03125)
    #   upper edge exactly on the region's: covered
    add("covered-hi-at", _table(3, [dict(x=0.5, y=0.5, w=0.05, h=0.05), dict(x=F(b - half), y=0.5, w=0.0625, h=0.0625)]), [(216, 136, 0), FB0, FB0])
    #   one ulp beyond: its own region.  px = 0.63125 + 1 ulp -> px * 640 = 404.00003 -> cx = 404 -> 300
    add("covered-hi-miss", _table(3, [dict(x=0.5, y=0.5, w=0.05, h=0.05), dict(x=F(np.nextafter(b, UP) - half), y=0.5, w=0.0625, h=0.0625)]),
        [(216, 136, 0), (300, 136, 1), FB0])
    #   lower edge exactly on the region's: covered
    add("covered-lo-at", _table(3, [dict(x=0.5, y=0.5, w=0.05, h=0.05), dict(x=F(a + half), y=0.5, w=0.0625, h=0.0625)]), [(216, 136, 0), FB0, FB0])
    #   one ulp short: px = 0.36875 - 1 ulp -> px * 640 = 235.99998 -> cx = 235 -> 131 -> 130
    add("covered-lo-miss", _table(3, [dict(x=0.5, y=0.5, w=0.05, h=0.05), dict(x=F(np.nextafter(a, DOWN) + half), y=0.5, w=0.0625, h=0.0625)]),
        [(216, 136, 0), (130, 136, 1), FB0])

    # a box exactly as large as a region is eligible, one ulp larger is not.  512 x 512, regions of 128: w = 0.25 -> 0.25 * 512 = 128 <= 128;
    # (0.5, 0.5) -> 256 - 64 = 192; the fallback is (192, 192) too -- the slot tells them apart
    c128 = Config(regions=3, region_w=128, region_h=128, max_age=2, class_id=-1)
    add("fits-exactly", _table(3, [dict(x=0.5, y=0.5, w=0.25, h=0.25), dict(x=0.1, y=0.1, w=np.nextafter(F(0.25), UP), h=0.1), dict(x=0.9, y=0.9, w=0.1, h=np.nextafter(F(0.25), UP))]),
        [(192, 192, 0), (192, 192, -1), (192, 192, -1)], cfg=c128, W=512, H=512)

    # max_age = 2: age 2 is zoomed, age 3 is not
    add("max-age", _table(10, [dict(x=0.2, y=0.2, w=0.05, h=0.05, last_seen=8), dict(x=0.8, y=0.8, w=0.04, h=0.04, last_seen=7)]), [(24, 0, 0), FB0, FB0])
    # the class filter
    add("class-filter", _table(3, [dict(x=0.2, y=0.2, w=0.05, h=0.05, cls=0), dict(x=0.8, y=0.8, w=0.05, h=0.05, cls=2)]), [(408, 272, 1), FB0, FB0],
        cfg=Config(regions=3, region_w=208, region_h=208, max_age=2, class_id=2))
    # frame_no has wrapped: F = 1, last_seen = 2^32 - 1 -> age 2, dtf = 3; px = 0.25 + 0.03125 * 3 = 0.34375 -> 220 -> 116.  last_seen = 2^32 - 2: age 3
    add("frame-no-wraps", _table(1, [dict(x=0.25, y=0.5, w=0.05, h=0.05, vx=0.03125, last_seen=0xFFFFFFFF), dict(x=0.8, y=0.8, w=0.04, h=0.04, last_seen=0xFFFFFFFE)]),
        [(116, 136, 0), FB0, FB0])
    # predictions outside [0, 1] and a NaN velocity: the origin stays inside the surface.  px = 1.15 -> 1 -> 640 - 104 -> 432; NaN -> 0; -0.15 -> 0
    # (slot 2's extent starts below 0: slot 1's region at x0 = 0 does not cover it)
    add("outside-and-nan", _table(3, [dict(x=0.9, y=0.5, w=0.04, h=0.04, vx=0.25), dict(x=0.5, y=0.5, w=0.05, h=0.05, vx=np.nan), dict(x=0.1, y=0.5, w=0.06, h=0.06, vx=-0.25)]),
        [(432, 136, 0), (0, 136, 1), (0, 136, 2)])

    # the product of the prediction is rounded before the sum (FUSED_* above): x0 = 510, not the 512 of an fma.  1203 x 480: xmax = 994, fallback
    # ((1203 - 208) // 2 = 497 -> 496, 136)
    add("product-rounded-first", _table(6, [dict(x=FUSED_X2, y=0.5, w=FUSED_SIZE, h=FUSED_SIZE, vx=FUSED_VX, last_seen=4)]),
        [(FUSED_X0, 136, 0), (496, 136, -1), (496, 136, -1)], W=FUSED_W)

    # a full table of 64: slot s at ((2 (s % 8) + 1) / 16, (2 (s // 8) + 1) / 16), (s + 8) / 1024 on a side -- all exact; the order is the slots'.
    #   slot 0 (40, 30 px) -> (0, 0), spanning x <= 0.325, y <= 0.4333: covers slots 1 (x = 0.1875) and 2 (0.3125 + 0.0049)
    #   slot 3 (x = 0.4375 -> 280 -> 176) -> (176, 0), spanning x in [0.275, 0.6]: covers slot 4 (0.5625 +- 0.0059)
    #   slot 5 (x = 0.6875 -> 440 -> 336) -> (336, 0)
    add("full-table", _table(7, [dict(x=(2 * (s % 8) + 1) / 16, y=(2 * (s // 8) + 1) / 16, w=(s + 8) / 1024, h=(s + 8) / 1024) for s in range(64)]),
        [(0, 0, 0), (176, 0, 3), (336, 0, 5)])
    return cases


def random_case(rng, engine_cfg=False):
    """a seeded table -> (Table, Config, W, H); engine_cfg: the GPU test's fixed config and surfaces of at most 640 x 480"""
    T = 64
    if engine_cfg:
        cfg, W, H = CFG0, int(rng.integers(2, 641)), int(rng.integers(2, 481))
    else:
        cfg = Config(regions=int(rng.integers(1, 16)), region_w=2 * int(rng.integers(1, 400)), region_h=2 * int(rng.integers(1, 400)),
                     max_age=int(rng.integers(0, 4)), class_id=int(rng.integers(-1, 3)))
        W, H = int(rng.integers(2, 2000)), int(rng.integers(2, 1200))
    frame_no = int(rng.choice([0, 1, 2, 7, 1000, 0xFFFFFFFF, 0xFFFFFFFE]))
    t = Table(frame_no=frame_no)
    grid = int(rng.choice([0, 16, 64]))                       # coarse positions and sizes make ties and exact edges common
    for s in range(T):
        x, y = rng.uniform(-0.1, 1.1, 2)
        w, h = rng.uniform(0, 0.5, 2) * rng.choice([1, 0.2])
        vx, vy = rng.uniform(-0.2, 0.2, 2) * rng.choice([0, 1])
        if grid:
            x, y, w, h = (np.round(v * grid) / grid for v in (x, y, w, h))
        t.add(x, y, w, h, cls=int(rng.integers(0, 3)), id=int(rng.integers(1, 1 << 32)), last_seen=(frame_no - int(rng.integers(0, 5))) & 0xFFFFFFFF,
              vx=vx, vy=vy, live=bool(rng.random() < 0.7))
    return t, cfg, W, H
