"""csrc/surface_rules.h on its own, without a GPU: tests/cpp/test_surface_rules.cpp includes the rule headers and nothing of the engine, keeps a
store in host memory and runs a script of defines, updates and detect-view requests.  For every update it prints the verdict and the job and band
tables and executes the band table on host arrays, row by row and item by item as the patch kernel walks it.  Here the executed store is
compared with the numpy oracle (tests/surface_ref.py), the bands are checked to tile the rectangles exactly once, and every refusal is asked for.
The entry points' null-engine and bad-argument answers come from libzly.so itself, before it touches a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import surface_ref as sr
import zly

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TARGET = "zero-latency-yolo_amd/_build/test_surface_rules"
POISON = 0xEE
OK, ARG, INPUT = 0, zly.ERR_INVALID_ARGUMENT, zly.ERR_INVALID_INPUT


def band_bytes():
    text = open(os.path.join(ROOT, "zero-latency-yolo_amd", "csrc", "surface_device.h")).read()
    return int(re.search(r"#define\s+ZLY_SURFACE_BAND_BYTES\s+(\d+)", text).group(1))


def _program():
    path = os.path.join(ROOT, TARGET)
    if not os.path.exists(path):
        subprocess.run(["make", "-C", ROOT, TARGET], check=True, stdout=subprocess.DEVNULL)
    return path


class Script:
    """collects commands, runs the program once, hands back one parsed answer per command"""

    def __init__(self, tmp_path):
        self.dir, self.lines, self.kinds, self.files = tmp_path, [], [], 0

    def store(self, n, each):
        self.lines.append(f"store {n} {each}"); self.kinds.append("store")

    def define(self, s, fmt, w, h):
        self.lines.append(f"define {s} {fmt} {w} {h}"); self.kinds.append("define")

    def update(self, rects):
        """rects: (s, x0, y0, fmt, w, h, bytes or None)"""
        path = self.dir / f"px{self.files}.bin"
        self.files += 1
        blob = [np.asarray(r[6], dtype=np.uint8).reshape(-1) if r[6] is not None else np.zeros(sr.frame_bytes(r[3], r[4], r[5]), np.uint8) for r in rects]
        (np.concatenate(blob) if blob else np.zeros(0, np.uint8)).tofile(path)
        self.lines.append(f"update {len(rects)} {path}")
        self.lines += [f"{r[0]} {r[1]} {r[2]} {r[3]} {r[4]} {r[5]}" for r in rects]
        self.kinds.append("update")

    def views(self, items):
        """items: s or (s, x0, y0, w, h)"""
        with_rois = 1 if items and isinstance(items[0], tuple) else 0
        self.lines.append(f"views {len(items)} {with_rois}")
        self.lines += [" ".join(str(v) for v in it) if with_rois else str(it) for it in items]
        self.kinds.append(("views", len(items)))

    def dump(self, s):
        path = self.dir / f"dump{self.files}.bin"
        self.files += 1
        self.lines.append(f"dump {s} {path}"); self.kinds.append(("dump", path))

    def run(self):
        path = self.dir / "script.txt"
        path.write_text("\n".join(self.lines) + "\n")
        r = subprocess.run([_program(), str(path)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        out, answers = r.stdout.splitlines(), []
        i = 0
        for kind in self.kinds:
            head = out[i].split(); i += 1
            if kind == "store":
                answers.append(dict(rc=int(head[1]), stride=int(head[2]), total=int(head[3])))
            elif kind == "define":
                answers.append(dict(rc=int(head[1])))
            elif kind == "update":
                a = dict(rc=int(head[1]), jobs=[], bands=[])
                if a["rc"] != 0:
                    a["error"] = out[i][len("error "):]; i += 1
                else:
                    nj, nb, a["pixel_bytes"], a["stage_bytes"] = (int(v) for v in head[2:6])
                    a["jobs"] = [tuple(int(v) for v in out[i + k].split()[1:]) for k in range(nj)]; i += nj
                    a["bands"] = [tuple(int(v) for v in out[i + k].split()[1:]) for k in range(nb)]; i += nb
                    a["covers"] = [int(v) for v in out[i].split()[1:]]; i += 1
                    a["exec"] = out[i].split()[1:]; i += 1
                answers.append(a)
            elif kind[0] == "views":
                a = dict(rc=int(head[1]), views=[])
                if a["rc"] == 0:
                    n = kind[1]
                    a["views"] = [tuple(int(v) for v in out[i + k].split()[1:]) for k in range(n)]; i += n
                answers.append(a)
            else:
                answers.append(dict(bytes=np.fromfile(kind[1], dtype=np.uint8)))
        assert i == len(out), out[i:]
        return answers


def _size(fmt):
    _, _, ex, ey = sr.FORMATS[fmt]
    return (38 if ex else 37), (30 if ey else 29)


def _disjoint_rects(fmt, w, h, rng, count):
    _, _, ex, ey = sr.FORMATS[fmt]
    sx, sy = (2 if ex else 1), (2 if ey else 1)
    out = []
    for _ in range(count * 20):
        rw, rh = int(rng.integers(1, 9)) * sx, int(rng.integers(1, 7)) * sy
        if rw > w or rh > h:
            continue
        r = (int(rng.integers(0, (w - rw) // sx + 1)) * sx, int(rng.integers(0, (h - rh) // sy + 1)) * sy, rw, rh)
        if all(sr.disjoint(r, o) for o in out):
            out.append(r)
        if len(out) == count:
            break
    return out


def _check_tables(a, rects, fmt, total):
    """jobs: one per (rectangle, plane); bands tile every job once: same bytes, no store byte twice, none outside"""
    want_bytes = sum(sr.frame_bytes(fmt, r[2], r[3]) for r in rects)
    assert len(a["jobs"]) == sum(len(sr.planes(fmt, r[2], r[3])) for r in rects)
    assert sum(rb * rows for _, _, rb, rows, _ in a["jobs"]) == want_bytes
    assert sum(rb * rows for _, _, rb, rows, _ in a["bands"]) == want_bytes
    hit_dst, hit_src = np.zeros(total, np.uint8), np.zeros(a["pixel_bytes"], np.uint8)
    for src, dst, rb, rows, pitch in a["bands"]:
        assert rows >= 1 and (rows == 1 or rows * rb <= band_bytes())
        for r in range(rows):
            hit_dst[dst + r * pitch:dst + r * pitch + rb] += 1
            hit_src[src + r * rb:src + (r + 1) * rb] += 1
    assert hit_dst.max() == 1 and int(hit_dst.sum()) == want_bytes and hit_src.max() == 1 and int(hit_src.sum()) == want_bytes
    assert a["exec"] == ["same", "0"], a["exec"]
    assert a["stage_bytes"] == a["pixel_bytes"] + 32 * len(a["bands"]) and a["pixel_bytes"] % 16 == 0


def test_standalone_selftest():
    r = subprocess.run([_program(), "selftest"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and " updates, 0 failed" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.parametrize("fmt", sr.ALL_FORMATS)
def test_executed_tables_match_the_oracle(fmt, tmp_path):
    rng = np.random.default_rng(7 + fmt)
    w, h = _size(fmt)
    fb = sr.frame_bytes(fmt, w, h)
    sc = Script(tmp_path)
    sc.store(3, fb + 3)
    sc.define(1, fmt, w, h)
    calls = [[(0, 0, w, h)]] + [_disjoint_rects(fmt, w, h, rng, 12) for _ in range(4)]
    pixels = [[rng.integers(0, 256, sr.frame_bytes(fmt, r[2], r[3]), dtype=np.uint8) for r in call] for call in calls]
    for call, px in zip(calls, pixels):
        sc.update([(1, r[0], r[1], fmt, r[2], r[3], p) for r, p in zip(call, px)])
        for s in (0, 1, 2):
            sc.dump(s)
    ans = sc.run()
    stride, total = ans[0]["stride"], ans[0]["total"]
    assert ans[0]["rc"] == OK and stride % zly.SURFACE_ALIGN == 0 and stride >= fb + 3 and total == 3 * stride and ans[1]["rc"] == OK
    surface = np.full(fb, POISON, dtype=np.uint8)
    k = 2
    for ci, (call, px) in enumerate(zip(calls, pixels)):
        a = ans[k]; k += 1
        assert a["rc"] == OK, a
        assert a["covers"] == [1 if sr.covers(w, h, *r) else 0 for r in call]
        _check_tables(a, call, fmt, total)
        for r, p in zip(call, px):
            sr.apply(surface, fmt, w, h, r[0], r[1], p, r[2], r[3])
        for s in (0, 1, 2):
            got = ans[k]["bytes"]; k += 1
            assert got.size == stride
            if s == 1:
                assert np.array_equal(got[:fb], surface), (fmt, ci)
                assert (got[fb:] == POISON).all()
            else:
                assert (got == POISON).all(), (fmt, ci, s)


def test_bands_at_the_band_constant(tmp_path):
    """a job of rows x row_bytes gets ceil(rows / max(1, BAND // row_bytes)) bands: heights one below, at and one above a band's rows, rows longer
    than a band, and a keyframe whose bytes lie on either side of a multiple of the band size"""
    B = band_bytes()
    sc, want = Script(tmp_path), []
    sc.store(1, 4 * 4100 * 12)
    cases = []
    for w in (40, 1024, 4096, 4100):
        per = max(1, B // (4 * w))
        for rows in sorted({1, per - 1, per, per + 1, 2 * per, 2 * per + 1} - {0}):
            if 4 * w * rows <= 4 * 4100 * 12:
                cases.append((w, rows, -(-rows // per)))
    for w, rows, _ in cases:
        sc.define(0, sr.PIX_BGRA, w, rows)
        sc.update([(0, 0, 0, sr.PIX_BGRA, w, rows, None)])
    ans = sc.run()
    for i, (w, rows, nb) in enumerate(cases):
        a = ans[2 + 2 * i]
        assert a["rc"] == OK and len(a["jobs"]) == 1 and len(a["bands"]) == nb, (w, rows, nb, len(a["bands"]))
        assert sum(b[3] for b in a["bands"]) == rows and a["exec"] == ["same", "0"]


def test_every_refusal(tmp_path):
    sc, want = Script(tmp_path), []

    def expect(rc, text=None):
        want.append((rc, text))

    sc.store(0, 100); expect(ARG)
    sc.store(4, 0); expect(ARG)
    sc.store(2, 1 << 56); expect(ARG)                       # 2 x 2^56 bytes: beyond what a view's offset addresses
    sc.store(1 << 20, (1 << 36) + 1); expect(ARG)
    sc.store(1, 1 << 56); expect(OK)                        # exactly the largest store (the program does not allocate it)
    sc.store(4, 37 * 29 * 3 + 1000); expect(OK)
    sc.store(4, 4096); expect(ARG)                          # twice
    sc.define(4, sr.PIX_BGR, 8, 8); expect(ARG)
    sc.define(-1, sr.PIX_BGR, 8, 8); expect(ARG)
    sc.define(0, 5, 8, 8); expect(ARG)                      # unknown format
    sc.define(0, sr.PIX_BGR, 0, 8); expect(INPUT)
    sc.define(0, sr.PIX_NV12_BT601, 9, 8); expect(INPUT)
    sc.define(0, sr.PIX_I420_BT601, 8, 7); expect(INPUT)
    sc.define(0, sr.PIX_YUY2_BT601, 7, 8); expect(INPUT)
    sc.define(0, sr.PIX_BGR, 38, 29); expect(OK)            # 3306 bytes <= 4223
    sc.define(0, sr.PIX_BGRA, 37, 29); expect(INPUT)        # 4292 bytes: above max_bytes_each
    sc.define(0, sr.PIX_BGR, 37, 29); expect(OK)
    sc.define(1, sr.PIX_NV12_BT709, 38, 30); expect(OK)
    sc.define(2, sr.PIX_UYVY_BT601, 38, 29); expect(OK)
    sc.views([0]); expect(INPUT, None)                      # not valid: no keyframe yet
    sc.views([3]); expect(ARG)                              # not defined
    sc.views([4]); expect(ARG)
    B, N, U = sr.PIX_BGR, sr.PIX_NV12_BT709, sr.PIX_UYVY_BT601
    for rects, rc, text in (
            ([(0, 36, 28, B, 2, 1, None)], ARG, "not inside"),
            ([(0, -1, 0, B, 2, 1, None)], ARG, "not inside"),
            ([(0, 0, 0, B, 38, 29, None)], ARG, "not inside"),
            ([(1, 1, 0, N, 2, 2, None)], ARG, "even"),
            ([(1, 0, 1, N, 2, 2, None)], ARG, "even"),
            ([(2, 1, 0, U, 2, 1, None)], ARG, "even"),
            ([(1, 0, 0, N, 3, 2, None)], INPUT, "invalid frame view"),      # the source view itself is illegal
            ([(0, 0, 0, sr.PIX_RGB, 2, 2, None)], ARG, "is not the surface's"),
            ([(0, 0, 0, 5, 2, 2, None)], ARG, "unknown pixel format"),
            ([(3, 0, 0, B, 2, 2, None)], ARG, "not defined"),
            ([(4, 0, 0, B, 2, 2, None)], ARG, "out of range"),
            ([(0, 0, 0, B, 4, 4, None), (0, 3, 3, B, 2, 2, None)], ARG, "overlaps rectangle 0"),
            ([(0, 0, 0, B, 4, 4, None), (1, 0, 0, N, 4, 4, None), (0, 5, 5, B, 2, 2, None), (1, 2, 2, N, 2, 2, None)], ARG, "rectangle 3: overlaps rectangle 1"),
            ([(0, 10, 10, B, 4, 4, None), (0, 0, 0, B, 2, 2, None), (0, 12, 8, B, 2, 3, None)], ARG, "rectangle 2: overlaps rectangle 0"),     # the later one begins higher up
            ([(0, 0, 0, B, 20, 20, None), (1, 0, 0, N, 2, 2, None), (0, 5, 5, B, 1, 1, None)], ARG, "rectangle 2: overlaps rectangle 0"),        # contained
            ([(0, 30, 3, B, 3, 1, None), (0, 0, 0, B, 37, 4, None)], ARG, "rectangle 1: overlaps rectangle 0"),
            ([], ARG, "a call takes 1..1024"),
            ([(0, i % 37, i // 37, B, 1, 1, None) for i in range(1025)], ARG, "1025 rectangles")):
        sc.update(rects); expect(rc, text)
    sc.update([(0, i % 37, i // 37, B, 1, 1, None) for i in range(1024)]); expect(OK)       # the most a call takes; the same cell of two SURFACES does not overlap
    sc.update([(0, 0, 0, B, 4, 4, None), (1, 0, 0, N, 4, 4, None), (2, 0, 0, U, 4, 4, None)]); expect(OK)
    sc.update([(0, 4, 0, B, 4, 4, None), (0, 0, 4, B, 8, 1, None), (0, 0, 0, B, 4, 4, None), (0, 8, 0, B, 1, 5, None), (0, 0, 5, B, 8, 2, None)]); expect(OK)      # touching, in any order
    sc.views([0]); expect(INPUT)                            # 1024 pixels are not a keyframe
    sc.update([(0, 0, 0, B, 37, 29, None)]); expect(OK)
    sc.views([0]); expect(OK)
    sc.views([(0, 36, 28, 2, 1)]); expect(ARG)
    sc.define(0, B, 37, 29); expect(OK)
    sc.views([0]); expect(INPUT)                            # redefining invalidates
    ans = sc.run()
    assert len(ans) == len(want)
    for i, (a, (rc, text)) in enumerate(zip(ans, want)):
        assert a["rc"] == rc, (i, sc.kinds[i], a, rc)
        if text:
            assert text in a["error"], (i, a["error"])


def test_detect_views_are_crops_of_the_tight_view_in_the_slot(tmp_path):
    lib = zly.load_library()
    sc = Script(tmp_path)
    each = sr.frame_bytes(sr.PIX_I420_BT601, 38, 30) + 7
    sc.store(3, each)
    cfg = [(0, sr.PIX_BGR, 20, 15), (1, sr.PIX_I420_BT601, 38, 30), (2, sr.PIX_YUY2_BT709, 38, 21)]
    for s, fmt, w, h in cfg:
        sc.define(s, fmt, w, h)
    sc.update([(s, 0, 0, fmt, w, h, None) for s, fmt, w, h in cfg])
    sc.views([2, 0, 1, 1])
    rois = [(0, 3, 5, 7, 9), (1, 2, 4, 8, 6), (2, 4, 1, 2, 3), (1, 0, 0, 38, 30)]
    sc.views(rois)
    ans = sc.run()
    stride = ans[0]["stride"]
    assert stride == -(-each // zly.SURFACE_ALIGN) * zly.SURFACE_ALIGN
    by_slot = {s: (fmt, w, h) for s, fmt, w, h in cfg}

    def expected(s, roi=None):
        fmt, w, h = by_slot[s]
        v = zly.view_tight(fmt, w, h)
        if roi:
            v = zly.view_crop(v, *roi)
        np_ = len(sr.planes(fmt, w, h))
        return (v.fmt, v.w, v.h) + tuple(int(v.off[p]) + s * stride if p < np_ else s * stride for p in range(3)) + tuple(int(v.pitch[p]) for p in range(3))

    whole, cropped = ans[-2], ans[-1]
    assert whole["rc"] == OK and cropped["rc"] == OK
    for got, s in zip(whole["views"], [2, 0, 1, 1]):
        assert got[:9] == expected(s) and got[9] <= (s + 1) * stride
    for got, r in zip(cropped["views"], rois):
        assert got[:9] == expected(r[0], r[1:]) and got[9] <= (r[0] + 1) * stride


def test_entry_points_answer_before_touching_a_device():
    lib = zly.load_library()
    n = C.c_int32(0)
    one = (C.c_int32 * 1)(0)
    assert lib.zly_surfaces_enable(None, 4, 1 << 20) == zly.ERR_NOT_INITIALIZED
    assert lib.zly_surface_define(None, 0, zly.PIX_BGR, 8, 8) == zly.ERR_NOT_INITIALIZED
    assert lib.zly_surface_update(None, 0, None, None, None, None) == zly.ERR_NOT_INITIALIZED
    assert lib.zly_surface_read(None, 0, None, 0) == zly.ERR_NOT_INITIALIZED
    assert lib.zly_detect_surfaces(None, 1, one, None, None, 0, None) == zly.ERR_NOT_INITIALIZED
    assert lib.zly_detect_delta(None, 0, None, None, None, None, 1, one, None, 0, C.byref(n)) == zly.ERR_NOT_INITIALIZED
    assert b"Engine not running" in lib.zly_last_error()
    assert zly.SURFACE_MAX_RECTS == int(re.search(r"#define\s+ZLY_SURFACE_MAX_RECTS\s+(\d+)", open(os.path.join(ROOT, "include", "zly.h")).read()).group(1))
    assert C.sizeof(zly.SurfaceRect) == 12 and C.sizeof(zly.Roi) == 16
