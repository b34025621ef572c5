"""The chips' rules as the product's own text computes them on a CPU: tests/cpp/test_chip_rules.cpp compiles csrc/chip_device.h -- the rectangle,
the selection predicate, the slab offsets and the per-format sample addresses the two kernels execute -- with the host checks of csrc/chip_rules.h,
and cuts chips pixel by pixel through that addressing.  Compared byte for byte with the numpy oracle (tests/chip_ref.py) for all twelve formats,
tight and through pitched views in a poisoned buffer; no sample address may leave its plane's extent.  No GPU, no library."""
import os
import subprocess

import numpy as np
import pytest

import chip_cases as cc
import chip_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TARGET = "zero-latency-yolo_amd/_build/test_chip_rules"
INVALID_ARGUMENT, INVALID_INPUT = 2, 203
CAP = 8


def _program():
    path = os.path.join(ROOT, TARGET)
    if not os.path.exists(path):
        subprocess.run(["make", "-C", ROOT, TARGET], check=True, stdout=subprocess.DEVNULL)
    return path


def _bits(v):
    return "%x" % int(np.array(v, dtype=np.float32).view(np.uint32))


def _run(lines):
    p = subprocess.run([_program(), "run"], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    return p.stdout.splitlines()


def _case_line(tmp, k, buf, view, slab, cap, cfg, flags=0):
    bp, sp = os.path.join(tmp, f"buf{k}.bin"), os.path.join(tmp, f"slab{k}.bin")
    np.asarray(buf, dtype=np.uint8).tofile(bp)
    np.asarray(slab, dtype=np.uint8).tofile(sp)
    fmt, w, h, off, pitch = view
    return (f"case {bp} {flags} {fmt} {w} {h} {off[0]} {off[1]} {off[2]} {pitch[0]} {pitch[1]} {pitch[2]} {sp} {cap} "
            f"{cfg.chip_w} {cfg.chip_h} {cfg.max_chips} {cfg.class_id} {_bits(cfg.scale)} {cfg.layout}")


def _parse(lines, pos):
    """one case's output from lines[pos:] -> (result, next position); result: ("refused", rc) or (hdr, recs, chips, violations)"""
    if lines[pos].startswith("refused"):
        return ("refused", int(lines[pos].split()[1])), pos + 1
    hdr = tuple(int(v) for v in lines[pos].split()[1:])
    n = hdr[0]
    recs = [ln.split()[1:] for ln in lines[pos + 1:pos + 1 + n]]
    chips = [bytes.fromhex(ln.split()[1]) if len(ln.split()) > 1 else b"" for ln in lines[pos + 1 + n:pos + 1 + 2 * n]]
    assert lines[pos + 1 + 2 * n].startswith("violations")
    return (hdr, recs, chips, int(lines[pos + 1 + 2 * n].split()[1])), pos + 2 + 2 * n


def _check_against_oracle(result, slab, cap, bgr, cfg):
    hdr, recs, chips, violations = result
    assert violations == 0
    sb, po, st, cb = cr.layout(cfg)
    want = cr.chip_slabs(slab[None], [bgr], cfg, np.zeros((1, sb), dtype=np.uint8), cap=cap)[0]
    wh = want[:16].view(cr.HDR_DTYPE)[0]
    assert hdr == (int(wh["n_chips"]), int(wh["n_eligible"]), int(wh["frame_tag"]), int(wh["flags"]))
    wr = want[16:16 + 32 * hdr[0]].view(cr.REC_DTYPE)
    for j in range(hdr[0]):
        r = recs[j]
        got = (int(r[0]), int(r[1]), int(r[2]), int(r[3], 16), int(r[4]), int(r[5]), int(r[6]), int(r[7]))
        w = wr[j]
        assert got == (int(w["det"]), int(w["class_id"]), int(w["track_id"]), int(np.array(w["confidence"]).view(np.uint32)),
                       int(w["x0"]), int(w["y0"]), int(w["w"]), int(w["h"]))
        assert chips[j] == want[po + j * st:po + j * st + cb].tobytes(), (j, got)


def _boxes(W, H, scale, odd):
    """boxes whose rectangles cover the frame's corners, odd and even origins, one pixel, the whole frame, and a few that cross the borders"""
    r = [(0, 0, W, H), (0, 0, 1, 1), (W - 1, H - 1, 1, 1), (W // 3, H // 3, max(W // 2, 1), max(H // 4, 1))]
    if odd and W > 3 and H > 3:
        r += [(1, 1, W - 2, H - 2), (3, 1, min(5, W - 3), min(3, H - 1))]
    dets = [cc.box(x0, y0, rw, rh, W, H, scale, conf=0.9 - 0.05 * k, cls=k % 2, track=50 + k) for k, (x0, y0, rw, rh) in enumerate(r)]
    dets.append((1.2, -0.1, 0.7, 0.9, 0.3, 1, 77))                 # crosses two borders
    return dets[:CAP]


@pytest.mark.parametrize("layout", [cr.BGR8, cr.RGB_F32])
def test_every_format_tight_and_pitched(tmp_path, layout):
    lines, expect = [], []
    k = 0
    for fmt in cc.ALL_FORMATS:
        for (w, h) in (cc.legal(fmt, 23, 13), (2, 2)) + (() if fmt in cc.F420 else ((2, 1),)) + (((1, 1),) if fmt in cc.FPK else ()):
            f, bgr = cc.frame(fmt, w, h, seed=w * 7 + h)
            cfg = cr.Config(chip_w=5, chip_h=4, max_chips=CAP, class_id=-1, scale=1.25, layout=layout)
            slab = cr.make_slab(_boxes(w, h, cfg.scale, odd=True), cap=CAP, frame_tag=900 + k, fill=0xEE)
            pbuf, pview = cc.pitched(f, fmt, w, h)
            lead = np.full(3, cc.POISON, dtype=np.uint8)
            for buf, view in ((f, cc.tight_view(fmt, w, h)), (np.concatenate([lead, pbuf]), cc.shifted(pview, 3))):
                lines.append(_case_line(str(tmp_path), k, buf, view, slab, CAP, cfg))
                expect.append((slab, bgr, cfg))
                k += 1
    out = _run(lines)
    pos, odd_seen = 0, 0
    for slab, bgr, cfg in expect:
        res, pos = _parse(out, pos)
        assert res[0] != "refused", res
        _check_against_oracle(res, slab, CAP, bgr, cfg)
        odd_seen += sum(1 for r in res[1] if int(r[4]) & 1 and int(r[5]) & 1)
    assert pos == len(out) and odd_seen > 24                        # odd x0 and y0 on every format, 4:2:0 and 4:2:2 among them


def test_selection_and_class_filter(tmp_path):
    w, h = 16, 12
    f, bgr = cc.frame(0, w, h, seed=1)
    dets = [cc.box(2 * k, k, 4, 3, w, h, 1.0, conf=0.9 - 0.1 * k, cls=[0, 0, 1, 2, 2, 2][k], track=k + 1) for k in range(6)]
    cases = [(cr.make_slab(dets, cap=CAP, frame_tag=5), cr.Config(chip_w=3, chip_h=3, max_chips=4, class_id=-1, scale=1.0)),
             (cr.make_slab(dets, cap=CAP), cr.Config(chip_w=3, chip_h=3, max_chips=2, class_id=2, scale=1.0)),
             (cr.make_slab(dets, cap=CAP), cr.Config(chip_w=3, chip_h=3, max_chips=3, class_id=2, scale=1.0)),
             (cr.make_slab(dets, cap=CAP), cr.Config(chip_w=3, chip_h=3, max_chips=4, class_id=9, scale=1.0)),
             (cr.make_slab(dets + dets[:2], cap=CAP, n_kept=30, flags=1), cr.Config(chip_w=3, chip_h=3, max_chips=8, scale=4.0)),
             (cr.make_slab(dets, cap=CAP, n_kept=-2), cr.Config(chip_w=3, chip_h=3, max_chips=8, scale=1.0))]
    out = _run([_case_line(str(tmp_path), k, f, cc.tight_view(0, w, h), s, CAP, c) for k, (s, c) in enumerate(cases)])
    pos = 0
    counts = []
    for s, c in cases:
        res, pos = _parse(out, pos)
        _check_against_oracle(res, s, CAP, bgr, c)
        counts.append(res[0][:2])
    assert counts == [(4, 6), (2, 3), (3, 3), (0, 0), (8, 8), (0, 0)]


def test_rectangle_arithmetic_is_not_contracted(tmp_path):
    """boxes whose rectangle an fma in lo / hi would move by a pixel: the program's text rounds every operation (tests/test_chip_ref.py holds the first by hand)"""
    f, bgr = cc.frame(0, 1920, 2, seed=9)
    bits = lambda u: float(np.array(u, dtype=np.uint32).view(np.float32))      # noqa: E731
    dets = [(bits(1058274016), 0.5, bits(1050864689), 0.5, 0.9, 0, 1), (bits(1064584439), 0.5, bits(1042313654), 0.5, 0.8, 0, 2)]
    cfg = cr.Config(chip_w=4, chip_h=2, max_chips=4, scale=1.25)
    slab = cr.make_slab(dets, cap=CAP)
    res, _ = _parse(_run([_case_line(str(tmp_path), 0, f, cc.tight_view(0, 1920, 2), slab, CAP, cfg)]), 0)
    _check_against_oracle(res, slab, CAP, bgr, cfg)
    assert [(int(r[4]), int(r[6])) for r in res[1]] == [(728, 763), (1643, 277)]


def test_refusals(tmp_path):
    w, h = 8, 6
    f, _ = cc.frame(0, w, h, seed=2)
    slab = cr.make_slab([], cap=CAP)
    ok = cr.Config(chip_w=4, chip_h=4, max_chips=CAP)
    tv = cc.tight_view(0, w, h)
    bad_cfgs = [cr.Config(chip_w=0), cr.Config(chip_w=257), cr.Config(chip_h=0), cr.Config(chip_h=257), cr.Config(max_chips=0), cr.Config(max_chips=CAP + 1),
                cr.Config(max_chips=CAP, class_id=-2), cr.Config(max_chips=CAP, scale=0.99), cr.Config(max_chips=CAP, scale=4.5),
                cr.Config(max_chips=CAP, scale=float("nan")), cr.Config(max_chips=CAP, scale=float("inf")), cr.Config(max_chips=CAP, layout=2),
                cr.Config(max_chips=CAP, layout=-1)]
    lines = [_case_line(str(tmp_path), k, f, tv, slab, CAP, c) for k, c in enumerate(bad_cfgs)]
    want = [INVALID_ARGUMENT] * len(bad_cfgs)
    k = len(lines)
    bad_views = [((5, w, h, tv[3], tv[4]), INVALID_ARGUMENT),                                   # an unknown format
                 ((0, 0, h, tv[3], tv[4]), INVALID_INPUT), ((0, w, -1, tv[3], tv[4]), INVALID_INPUT),
                 ((1, 7, 6, [0, 48, 0], [7, 8, 0]), INVALID_INPUT),                               # an odd 4:2:0 width
                 ((10, 7, 6, [0, 0, 0], [14, 0, 0]), INVALID_INPUT),                              # an odd 4:2:2 width
                 ((0, w, h, tv[3], [3 * w - 1, 0, 0]), INVALID_INPUT),                            # a pitch below the row's bytes
                 ((0, w, h, [1, 0, 0], tv[4]), INVALID_INPUT),                                    # one byte more than the buffer holds
                 ((0, 16385, 1, tv[3], [3 * 16385, 0, 0]), INVALID_INPUT)]                        # wider than ZLY_AREA_MAX_DIM (and than the buffer)
    for v, rc in bad_views:
        lines.append(_case_line(str(tmp_path), k, f, v, slab, CAP, ok))
        want.append(rc)
        k += 1
    # a frame above ZLY_AREA_MAX_DIM that its buffer does hold: the size limit itself, on an engine without any resize flag
    wide = np.zeros(16386 * 3, dtype=np.uint8)
    lines.append(_case_line(str(tmp_path), k, wide, cc.tight_view(0, 16386, 1), slab, CAP, ok))
    want.append(INVALID_INPUT)
    lines.append(_case_line(str(tmp_path), k + 1, wide, cc.tight_view(0, 16384, 1), slab, CAP, ok))      # at the limit: accepted
    out = _run(lines)
    assert [int(ln.split()[1]) for ln in out[:len(want)]] == want and all(ln.startswith("refused") for ln in out[:len(want)])
    assert out[len(want)].startswith("hdr 0 0")
    # the call's own arguments: n, the view array, the source
    calls = [("call 1 4 1 0 0", 0), ("call 4 4 1 1 0", 0), ("call 1 4 1 0 1", 0), ("call 0 4 1 0 0", 2), ("call 5 4 1 0 0", 2), ("call -1 4 1 0 0", 2),
             ("call 1 4 0 0 0", 2), ("call 1 4 1 0 2", 2), ("call 1 4 1 0 -1", 2), ("call 1 4 1 1 1", 2)]
    assert _run([c for c, _ in calls]) == [f"rc {rc}" for _, rc in calls]


def test_layout_equals_the_oracle():
    shapes = [(64, 64, 16, 0), (1, 1, 1, 0), (1, 1, 1, 1), (33, 17, 7, 0), (33, 17, 7, 1), (256, 256, 64, 1), (5, 1, 8, 0)]
    out = _run([f"layout {w} {h} {m} {lay}" for w, h, m, lay in shapes])
    for ln, (w, h, m, lay) in zip(out, shapes):
        assert tuple(int(v) for v in ln.split()[1:]) == cr.layout(cr.Config(chip_w=w, chip_h=h, max_chips=m, layout=lay))


def test_wide_rectangle_crosses_staging_chunks(tmp_path):
    """a rectangle wider than a staging chunk, from an odd origin: the row ranges the cut kernel stages stay inside the planes for every family"""
    lines, expect = [], []
    for k, fmt in enumerate((0, 17, cc.F420[0], cc.F420[1], cc.F422[0])):
        w, h = 2300, 2
        f, bgr = cc.frame(fmt, w, h, seed=40 + k)
        cfg = cr.Config(chip_w=7, chip_h=2, max_chips=2, scale=1.0)
        slab = cr.make_slab([cc.box(1, 0, 2299, 2, w, h, 1.0), cc.box(1019, 1, 1022, 1, w, h, 1.0)], cap=CAP)
        pbuf, pview = cc.pitched(f, fmt, w, h, pad=1, lead=1)
        lines.append(_case_line(str(tmp_path), k, pbuf, pview, slab, CAP, cfg))
        expect.append((slab, bgr, cfg))
    out = _run(lines)
    pos = 0
    for slab, bgr, cfg in expect:
        res, pos = _parse(out, pos)
        _check_against_oracle(res, slab, CAP, bgr, cfg)
