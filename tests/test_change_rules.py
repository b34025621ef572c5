"""The change map's rules as the product's own text computes them on a CPU: tests/cpp/test_change_rules.cpp compiles csrc/change_device.h -- the
granule loads and the luma the sums kernel executes, the cells, the predicates and the windows -- with the host twin of csrc/change_rules.h, and
is compared with the numpy oracle (tests/change_ref.py) for all twelve formats, tight and through pitched views in a poisoned buffer, over
sequences of frames; no needed sample address of the sums pass may lie outside its plane's extent.  No GPU, no library."""
import os
import subprocess

import numpy as np
import pytest

import change_cases as cs
import change_ref as chr_
import chip_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TARGET = "zero-latency-yolo_amd/_build/test_change_rules"
INVALID_INPUT = 203


def _program():
    path = os.path.join(ROOT, TARGET)
    if not os.path.exists(path):
        subprocess.run(["make", "-C", ROOT, TARGET], check=True, stdout=subprocess.DEVNULL)
    return path


def _run(lines):
    p = subprocess.run([_program()], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    return p.stdout.splitlines()


def _cfg_line(c):
    return f"cfg {c.cell} {c.threshold_q4} {c.max_active_permille} {c.max_peaks} {c.window_w} {c.window_h}"


def _frame_line(tmp, k, stream, buf, view):
    path = os.path.join(tmp, f"buf{k}.bin")
    np.asarray(buf, dtype=np.uint8).tofile(path)
    fmt, w, h, off, pitch = view
    return f"frame {stream} {fmt} {w} {h} {off[0]} {off[1]} {off[2]} {pitch[0]} {pitch[1]} {pitch[2]} {path}"


def _parse(lines, pos):
    """one frame's output from lines[pos:] -> (result, next position)"""
    if lines[pos].startswith("refused"):
        return ("refused", int(lines[pos].split()[1])), pos + 1
    t = lines[pos].split()
    assert t[0] == "hdr" and t[9] == "outside"
    hdr, outside = tuple(int(v) for v in t[1:9]), int(t[10])
    S = [int(v) for v in lines[pos + 1].split()[1:]]
    A = [int(v) for v in lines[pos + 2].split()[1:]]
    pos += 3
    peaks = []
    while pos < len(lines) and lines[pos].startswith("peak"):
        peaks.append(tuple(int(v) for v in lines[pos].split()[1:]))
        pos += 1
    plan = None
    if pos < len(lines) and lines[pos].startswith("plan"):
        v = [int(x) for x in lines[pos].split()[1:]]
        plan = [tuple(v[i:i + 6]) for i in range(0, len(v), 6)]
        pos += 1
    return (hdr, outside, S, A, peaks, plan), pos


def _expect(result, stream_ref, bgr, cfg, suppress=()):
    hdr, outside, S, A, peaks, _ = result
    rec = np.zeros(chr_.layout(cfg)[0], dtype=np.uint8)
    wh, wp, wa = stream_ref.frame(bgr, cfg, rec, suppress)
    assert outside == 0
    assert S == chr_.sums(bgr, cfg.cell)[0].reshape(-1).tolist()
    assert hdr == tuple(int(wh[k]) for k in ("n_cells", "n_active", "n_peaks", "flags", "gw", "gh", "step", "pad"))
    assert A == wa.reshape(-1).tolist()
    assert peaks == [p + (0,) for p in wp]
    return wh, wp


KINDS = ["new", "blocks", "same", "flat", "blocks", "new"]


@pytest.mark.parametrize("fmt", cc.ALL_FORMATS)
def test_every_format_tight_and_pitched_over_a_sequence(tmp_path, fmt):
    """per format a sequence of six frames on two streams: stream 0 takes them tight, stream 1 through pitched views between poisoned bytes; at the
    sizes of the issue that the format allows, rounded up where it needs even ones"""
    lines, wants, k = [], [], 0
    for (w0, h0), C in zip(cs.SIZES, (8, 8, 8, 16, 32, 64, 32)):
        w, h = cs.legal_size(fmt, w0, h0)
        cfg = chr_.Config(cell=C, threshold_q4=8, max_active_permille=600, max_peaks=4, window_w=min(64, max(w & ~1, 2)), window_h=min(48, max(h & ~1, 2)))
        lines += [_cfg_line(cfg), "reset -1"]
        refs = [chr_.Stream(), chr_.Stream()]
        steps = KINDS if w * h <= 101 * 77 else KINDS[:3]
        for f, bgr in cs.film(fmt, w, h, steps, seed=5):
            pbuf, pview = cc.pitched(f, fmt, w, h)
            lines += [_frame_line(str(tmp_path), k, 0, f, cc.tight_view(fmt, w, h)), _frame_line(str(tmp_path), k + 1, 1, pbuf, pview)]
            wants += [(refs[0], bgr, cfg), (refs[1], bgr, cfg)]
            k += 2
    out = _run(lines)
    pos, n_peaks, n_flags = 0, 0, set()
    for ref, bgr, cfg in wants:
        result, pos = _parse(out, pos)
        wh, wp = _expect(result, ref, bgr, cfg)
        n_peaks += len(wp)
        n_flags.add(int(wh["flags"]))
    assert pos == len(out) and n_peaks >= 4 and n_flags >= {0, chr_.FIRST, chr_.GLOBAL}, (n_peaks, n_flags)


def test_hand_cases_thresholds_windows_and_the_fill(tmp_path):
    """the hand cases of tests/test_change_ref.py through the host twin, and the fill of a plan with the plan's track regions as initial suppression"""
    lines, wants, k = [], [], 0

    def add(cfg, frames, plan=None):
        nonlocal k
        lines.extend([_cfg_line(cfg), "reset -1"])
        ref = chr_.Stream()
        for i, bgr in enumerate(frames):
            h, w = bgr.shape[:2]
            last = i == len(frames) - 1
            if plan is not None and last:
                lines.append("plan %d " % len(plan) + " ".join("%d %d %d %d %d %d" % tuple(int(v) for v in r) for r in plan))
            lines.append(_frame_line(str(tmp_path), k, 0, bgr.reshape(-1), cc.tight_view(0, w, h)))
            wants.append((ref, bgr, cfg, plan if last else None))
            k += 1

    g = cs.gray
    f1 = g(64, 64, 0)
    for j, (y, x) in enumerate(((1, 1), (1, 33), (33, 1), (33, 33))):
        f1[y, x] = 10 + j
    add(chr_.Config(cell=32, threshold_q4=0, max_active_permille=1000, max_peaks=15, window_w=2, window_h=2), [g(64, 64), f1])
    f2 = g(101, 77)
    f2[5, 100] = 50
    add(chr_.Config(cell=32, threshold_q4=0, max_active_permille=1000, max_peaks=2, window_w=40, window_h=40), [g(101, 77), f2])
    for v in (128, 129):
        f3 = g(8, 8)
        f3[3, 4] = v
        add(chr_.Config(cell=8, threshold_q4=32, max_active_permille=1000, max_peaks=1, window_w=8, window_h=8), [g(8, 8), f3])
    add(chr_.Config(cell=64, threshold_q4=4080, max_active_permille=1000, window_w=64, window_h=64), [g(64, 64, 0), g(64, 64, 255)])
    f4, f5 = g(64, 64), g(64, 64)
    f4[0, 0] = 255
    f5[0, 0] = f5[0, 40] = 255
    for f in (f4, f5):
        add(chr_.Config(cell=32, threshold_q4=0, max_active_permille=250, window_w=32, window_h=32), [g(64, 64), f])
    f6 = g(128, 32)
    for cx, v in enumerate((40, 90, 20, 70)):
        f6[3, 32 * cx + 3] = v
    dt = [("x0", "<i4"), ("y0", "<i4"), ("w", "<i4"), ("h", "<i4"), ("slot", "<i4"), ("track_id", "<u4")]
    for slots in ([-1, -1, -1], [3, -1, -1], [3, 4, 5], [-1, 3, -1]):
        plan = np.zeros(3, dtype=dt)
        plan["w"], plan["h"], plan["x0"], plan["slot"] = 32, 32, [32, 48, 96], slots          # fallbacks at x0 = 48 would be the centred window
        plan["track_id"] = [9 if s >= 0 else 0 for s in slots]
        add(chr_.Config(cell=32, threshold_q4=0, max_active_permille=1000, max_peaks=2, window_w=32, window_h=32), [g(128, 32), f6], plan)
    out = _run(lines)
    pos, filled = 0, 0
    for ref, bgr, cfg, plan in wants:
        result, pos = _parse(out, pos)
        sup = chr_.track_rects(plan) if plan is not None else ()
        _, wp = _expect(result, ref, bgr, cfg, sup)
        if plan is not None:
            want = chr_.fill(plan, wp)
            assert result[5] == [tuple(int(v) for v in r) for r in want]
            filled += int((want["slot"] == -2).sum())
    assert pos == len(out) and filled >= 4


def test_refusals(tmp_path):
    """more than ZLY_CHANGE_MAX_CELLS cells, and a view whose last row leaves the buffer"""
    f = np.zeros(1024 * 520 * 3, dtype=np.uint8)
    lines = ["cfg 8 32 250 3 64 64", _frame_line(str(tmp_path), 0, 0, f, cc.tight_view(0, 1024, 520)),            # 128 x 65 = 8320 cells
             _frame_line(str(tmp_path), 1, 0, f, cc.tight_view(0, 1024, 512)),                                      # 8192: accepted
             _frame_line(str(tmp_path), 2, 0, f[:-1], cc.tight_view(0, 1024, 520))]
    out = _run(lines)
    r0, pos = _parse(out, 0)
    r1, pos = _parse(out, pos)
    r2, pos = _parse(out, pos)
    assert r0 == ("refused", INVALID_INPUT) and r1[0][0] == 8192 and r2 == ("refused", INVALID_INPUT)
