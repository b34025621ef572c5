"""The moves of the resident surfaces (include/zly.h "Resident surfaces", MOVES) without a GPU: tests/cpp/test_surface_moves.cpp includes the rule
headers and nothing of the engine, keeps a store and a bounce buffer in host memory and runs a script of defines, keyframes and move calls.  For
every call it prints the verdict, the phases and the tables, and executes each launch's bands item by item as the kernels walk them -- in table
order, in reverse and in a seeded shuffle.  Here the executed store is compared with the numpy oracle (tests/surface_move_ref.py), the phases and
bands are held to their invariants, and every refusal is asked for.  The entry points' null-engine answers come from libzly.so itself, before it
touches a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import surface_move_ref as mr
import surface_ref as sr
import zly

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TARGET = "zero-latency-yolo_amd/_build/test_surface_moves"
SOURCES = ("tests/cpp/test_surface_moves.cpp", "zero-latency-yolo_amd/csrc/surface_rules.h", "zero-latency-yolo_amd/csrc/surface_device.h")
POISON = 0xEE
OK, ARG, INPUT = 0, zly.ERR_INVALID_ARGUMENT, zly.ERR_INVALID_INPUT


def band_bytes():
    text = open(os.path.join(ROOT, "zero-latency-yolo_amd", "csrc", "surface_device.h")).read()
    return int(re.search(r"#define\s+ZLY_SURFACE_BAND_BYTES\s+(\d+)", text).group(1))


def _program():
    path = os.path.join(ROOT, TARGET)
    if not os.path.exists(path) or any(os.path.getmtime(os.path.join(ROOT, s)) > os.path.getmtime(path) for s in SOURCES):
        subprocess.run(["make", "-C", ROOT, TARGET], check=True, stdout=subprocess.DEVNULL)
    return path


class Script:
    """collects commands, runs the program once, hands back one parsed answer per command"""

    def __init__(self, tmp_path):
        self.dir, self.lines, self.kinds, self.files = tmp_path, [], [], 0

    def _file(self, stem):
        self.files += 1
        return self.dir / f"{stem}{self.files}.bin"

    def store(self, n, each):
        self.lines.append(f"store {n} {each}"); self.kinds.append("store")

    def define(self, s, fmt, w, h):
        self.lines.append(f"define {s} {fmt} {w} {h}"); self.kinds.append("define")

    def keyframe(self, s, px):
        path = self._file("key")
        np.asarray(px, dtype=np.uint8).tofile(path)
        self.lines.append(f"keyframe {s} {path}"); self.kinds.append("keyframe")

    def bounce(self, nbytes):
        self.lines.append(f"bounce {nbytes}"); self.kinds.append("bounce")

    def moves(self, ms, null=False):
        """ms: (s, sx, sy, dx, dy, w, h) each"""
        self.lines.append(f"{'moves_null' if null else 'moves'} {len(ms)}")
        if not null:
            self.lines += [" ".join(str(v) for v in m) for m in ms]
        self.kinds.append("moves")

    def dump(self, s):
        path = self._file("dump")
        self.lines.append(f"dump {s} {path}"); self.kinds.append(("dump", path))

    def run(self):
        path = self.dir / "script.txt"
        path.write_text("\n".join(self.lines) + "\n")
        r = subprocess.run([_program(), str(path)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        out, answers = r.stdout.splitlines(), []
        i = 0

        def take(n, name):
            nonlocal i
            rows = [out[i + k].split() for k in range(n)]
            assert all(r[0] == name for r in rows), (name, rows[:2])
            i += n
            return [tuple(int(v) for v in r[1:]) for r in rows]

        for kind in self.kinds:
            head = out[i].split(); i += 1
            if kind == "store":
                answers.append(dict(rc=int(head[1]), stride=int(head[2]), total=int(head[3])))
            elif kind in ("define", "keyframe", "bounce"):
                assert head[0] == kind
                answers.append(dict(rc=int(head[1])))
            elif kind == "moves":
                a = dict(rc=int(head[1]))
                if a["rc"] != 0:
                    a["error"] = out[i][len("error "):]; i += 1
                else:
                    nph, naj, nab, nbj, nbb, a["table_bytes"] = (int(v) for v in head[2:8])
                    n_moves = 0
                    while out[i + n_moves].startswith("move "):
                        n_moves += 1
                    a["moves"] = take(n_moves, "move")                       # (index, phase, via)
                    a["phases"] = take(nph, "phase")                         # (first, count, a_first, a_count, b_first, b_count, bounce_bytes)
                    a["ajobs"] = take(naj, "ajob")                           # (src, dst, to_bounce, row_bytes, rows, src_pitch, dst_pitch)
                    a["abands"] = take(nab, "aband")
                    a["bjobs"] = take(nbj, "bjob")                           # (src, dst, row_bytes, rows, pitch)
                    a["bbands"] = take(nbb, "bband")
                    a["exec"] = out[i].split()[1:]; i += 1
                answers.append(a)
            else:
                answers.append(dict(bytes=np.fromfile(kind[1], dtype=np.uint8)))
        assert i == len(out), out[i:]
        return answers


def _size(fmt):
    _, _, ex, ey = sr.FORMATS[fmt]
    return (38 if ex else 37), (30 if ey else 29)


def _steps(fmt):
    _, _, ex, ey = sr.FORMATS[fmt]
    return (2 if ex else 1), (2 if ey else 1)


def _need(fmt, m):
    """a self-overlapping move's bytes in the bounce buffer: every (move, plane) job starts 16-byte aligned"""
    return sum(-(-(rows * rb) // 16) * 16 for rows, rb, *_ in sr.planes(fmt, m[4], m[5]))


def _random_moves(fmt, w, h, rng, count):
    """seeded legal moves up to half the surface on a side: most calls hold self-overlapping moves, conflicts of every kind and an identity"""
    stx, sty = _steps(fmt)
    out = []
    while len(out) < count:
        mw, mh = int(rng.integers(1, w // 2 // stx + 1)) * stx, int(rng.integers(1, h // 2 // sty + 1)) * sty
        pos = lambda lim, st: int(rng.integers(0, lim // st + 1)) * st
        sx, sy = pos(w - mw, stx), pos(h - mh, sty)
        kind = int(rng.integers(0, 8))
        if kind == 0:
            dx, dy = sx, sy                                                  # an identity
        elif kind <= 3:                                                      # near its source: overlaps itself
            dx = min(max(sx + int(rng.integers(-2, 3)) * stx, 0), w - mw)
            dy = min(max(sy + int(rng.integers(-2, 3)) * sty, 0), h - mh)
        else:
            dx, dy = pos(w - mw, stx), pos(h - mh, sty)
        out.append((sx, sy, dx, dy, mw, mh))
    return out


def _check_phases(a, fmt, moves, bounce):
    """moves: (sx, sy, dx, dy, w, h) of ONE surface"""
    n = len(moves)
    assert [m[0] for m in a["moves"]] == list(range(n))
    phase_of, via = [m[1] for m in a["moves"]], [m[2] for m in a["moves"]]
    # consecutive runs in call order
    assert all(phase_of[i] <= phase_of[i + 1] for i in range(n - 1))
    at = 0
    for k, (first, count, *_rest) in enumerate(a["phases"]):
        assert first == at and count >= 1 and all(phase_of[i] == k for i in range(first, first + count))
        at += count
    assert at == n
    # self-overlapping moves, and only they, go through the bounce buffer; identity moves appear in no table
    for m, v in zip(moves, via):
        assert v == (0 if mr.identity(m) else 2 if mr.self_overlaps(m) else 1), (m, v)
    assert len(a["ajobs"]) == sum(len(sr.planes(fmt, m[4], m[5])) for m, v in zip(moves, via) if v)
    assert len(a["bjobs"]) == sum(len(sr.planes(fmt, m[4], m[5])) for m, v in zip(moves, via) if v == 2)
    assert sum(j[2] for j in a["ajobs"]) == len(a["bjobs"])
    live = lambda first, count: [i for i in range(first, first + count) if via[i]]
    for k, (first, count, _af, _ac, _bf, _bc, used) in enumerate(a["phases"]):
        ids = live(first, count)
        # no two moves in a phase conflict
        assert not any(mr.conflicts(moves[i], moves[j]) for x, i in enumerate(ids) for j in ids[x + 1:]), (k, ids)
        assert used == sum(_need(fmt, moves[i]) for i in ids if via[i] == 2) and used <= bounce
        if k:
            # the first move of a later phase conflicts with a move of the phase before it, or found no room in the bounce buffer
            pf, pc, *_r, pused = a["phases"][k - 1]
            opener = moves[first]
            assert via[first] != 0
            assert any(mr.conflicts(moves[i], opener) for i in live(pf, pc)) or (via[first] == 2 and pused + _need(fmt, opener) > bounce), (k, opener)


def _check_bands(a, fmt, moves, total, bounce):
    """the bands tile each job exactly once; no destination byte appears twice in a launch; launch A reads no byte that it writes"""
    B = band_bytes()
    via = [m[2] for m in a["moves"]]
    want = sum(sr.frame_bytes(fmt, m[4], m[5]) for m, v in zip(moves, via) if v)
    assert sum(j[3] * j[4] for j in a["ajobs"]) == want == sum(b[3] * b[4] for b in a["abands"])
    want_b = sum(sr.frame_bytes(fmt, m[4], m[5]) for m, v in zip(moves, via) if v == 2)
    assert sum(j[2] * j[3] for j in a["bjobs"]) == want_b == sum(b[2] * b[3] for b in a["bbands"])
    for _first, _count, af, ac, bf, bc, used in a["phases"]:
        wr_store, wr_bounce, rd = np.zeros(total, np.uint8), np.zeros(bounce, np.uint8), np.zeros(total, np.uint8)
        for src, dst, tb, rb, rows, sp, dp in a["abands"][af:af + ac]:
            assert rows >= 1 and (rows == 1 or rows * rb <= B)
            for r in range(rows):
                rd[src + r * sp:src + r * sp + rb] = 1
                (wr_bounce if tb else wr_store)[dst + r * dp:dst + r * dp + rb] += 1
        assert wr_store.max(initial=0) <= 1 and wr_bounce.max(initial=0) <= 1 and not (rd & wr_store).any()
        assert int(wr_bounce.sum()) == sum(b[2] * b[3] for b in a["bbands"][bf:bf + bc]) and (bc > 0) == (used > 0)
        rd_bounce, wr2 = np.zeros(bounce, np.uint8), np.zeros(total, np.uint8)
        for src, dst, rb, rows, pitch in a["bbands"][bf:bf + bc]:
            assert rows >= 1 and (rows == 1 or rows * rb <= B)
            for r in range(rows):
                rd_bounce[src + r * rb:src + (r + 1) * rb] += 1
                wr2[dst + r * pitch:dst + r * pitch + rb] += 1
        assert wr2.max(initial=0) <= 1 and np.array_equal(rd_bounce, wr_bounce)     # launch B scatters exactly what launch A gathered
    assert a["exec"] == ["same", "0"], a["exec"]
    assert a["table_bytes"] == 32 * (len(a["abands"]) + len(a["bbands"]))


def _crafted(fmt):
    """calls built to contain a read-after-write, a write-after-read and a write-after-write pair (even coordinates: legal for every format)"""
    raw = [(0, 0, 10, 0, 6, 6), (10, 0, 20, 10, 6, 6)]
    war = [(0, 10, 8, 10, 6, 6), (20, 20, 2, 12, 6, 6)]
    waw = [(0, 0, 20, 0, 6, 6), (30, 20, 22, 2, 6, 6)]
    for pair in (raw, war, waw):
        assert mr.conflicts(*pair) and not any(mr.self_overlaps(m) for m in pair)
    return [raw, war, waw, raw + war + waw, [(2, 2, 4, 4, 12, 10), (4, 4, 2, 2, 12, 10), (2, 2, 2, 2, 8, 8), (20, 2, 22, 2, 8, 20)]]


@pytest.mark.parametrize("fmt", sr.ALL_FORMATS)
def test_executed_moves_match_the_oracle(fmt, tmp_path):
    rng = np.random.default_rng(70 + fmt)
    w, h = _size(fmt)
    fb = sr.frame_bytes(fmt, w, h)
    bounce = 1536                                            # holds any one move of up to half the surface on a side, not two large ones
    sc = Script(tmp_path)
    sc.store(3, fb + 3)
    sc.define(1, fmt, w, h)
    key = rng.integers(0, 256, fb, dtype=np.uint8)
    sc.keyframe(1, key)
    sc.bounce(bounce)
    calls = _crafted(fmt) + [_random_moves(fmt, w, h, rng, 10) for _ in range(6)]
    for call in calls:
        assert all(mr.legal(fmt, w, h, m) and (not mr.self_overlaps(m) or _need(fmt, m) <= bounce) for m in call)
        sc.moves([(1,) + m for m in call])
        for s in (0, 1, 2):
            sc.dump(s)
    ans = sc.run()
    stride, total = ans[0]["stride"], ans[0]["total"]
    assert [a["rc"] for a in ans[:4]] == [OK] * 4
    surface = key.copy()
    k, phases_seen, kinds_seen = 4, 0, set()
    for ci, call in enumerate(calls):
        a = ans[k]; k += 1
        assert a["rc"] == OK, a
        _check_phases(a, fmt, call, bounce)
        _check_bands(a, fmt, call, total, bounce)
        phases_seen = max(phases_seen, len(a["phases"]))
        kinds_seen |= {m[2] for m in a["moves"]}
        mr.apply_moves(surface, fmt, w, h, call)
        for s in (0, 1, 2):
            got = ans[k]["bytes"]; k += 1
            assert got.size == stride
            if s == 1:
                assert np.array_equal(got[:fb], surface), (fmt, ci, np.flatnonzero(got[:fb] != surface)[:8])
                assert (got[fb:] == POISON).all()                            # the slack behind the frame
            else:
                assert (got == POISON).all(), (fmt, ci, s)                   # the neighbouring slots
    for ci in range(3):
        assert len(ans[4 + 4 * ci]["phases"]) == 2                           # each crafted pair is two phases
    assert phases_seen >= 3 and kinds_seen == {0, 1, 2} and not np.array_equal(surface, key)


def test_a_full_bounce_buffer_opens_the_next_phase(tmp_path):
    fmt, w, h = sr.PIX_BGR, 37, 29
    sc = Script(tmp_path)
    sc.store(1, sr.frame_bytes(fmt, w, h))
    sc.define(0, fmt, w, h)
    key = np.random.default_rng(5).integers(0, 256, sr.frame_bytes(fmt, w, h), dtype=np.uint8)
    sc.keyframe(0, key)
    sc.bounce(1024)
    call = [(0, 0, 1, 0, 16, 14), (0, 15, 1, 15, 16, 14), (20, 0, 21, 1, 4, 4), (30, 0, 30, 20, 5, 5)]      # 672 + 672 bytes: the second finds no room
    sc.moves([(0,) + m for m in call])
    sc.dump(0)
    sc.bounce(4096)
    sc.moves([(0,) + m for m in call])
    ans = sc.run()
    a, b = ans[4], ans[7]
    assert not any(mr.conflicts(x, y) for i, x in enumerate(call) for y in call[i + 1:])
    assert [p[:2] for p in a["phases"]] == [(0, 1), (1, 3)] and [p[6] for p in a["phases"]] == [672, 672 + 48]
    assert [p[:2] for p in b["phases"]] == [(0, 4)]                          # with room for both: one phase, two launches
    _check_phases(a, fmt, call, 1024); _check_bands(a, fmt, call, ans[0]["total"], 1024)
    _check_phases(b, fmt, call, 4096); _check_bands(b, fmt, call, ans[0]["total"], 4096)
    assert np.array_equal(ans[5]["bytes"][:key.size], mr.apply_moves(key.copy(), fmt, w, h, call))


def test_bands_at_the_band_constant(tmp_path):
    """a job of rows x row_bytes gets ceil(rows / max(1, BAND // row_bytes)) bands, on both paths: heights one below, at and one above a band's rows,
    and rows longer than a band on a surface 4100 wide"""
    B = band_bytes()
    fmt, w, h = sr.PIX_BGRA, 4100, 12
    fb = sr.frame_bytes(fmt, w, h)
    sc = Script(tmp_path)
    sc.store(2, fb)
    sc.define(1, fmt, w, h)
    key = np.random.default_rng(6).integers(0, 256, fb, dtype=np.uint8)
    sc.keyframe(1, key)
    sc.bounce(fb)
    calls = []
    for mw in (1024, 4096, 4099):
        per = max(1, B // (4 * mw))
        for rows in sorted({1, per - 1, per, per + 1, 2 * per, 2 * per + 1} - {0}):
            if rows + 1 <= h:
                calls.append(((0, 0, 1, 1, mw, rows), -(-rows // per)))              # overlaps itself: gathered, then scattered
                if 2 * rows <= h:
                    calls.append(((1, 0, 0, rows, mw, rows), -(-rows // per)))       # clear of itself: store -> store
    for m, _ in calls:
        sc.moves([(1,) + m])
    sc.dump(0); sc.dump(1)
    ans = sc.run()
    surface = key.copy()
    for (m, nb), a in zip(calls, ans[4:]):
        assert a["rc"] == OK and len(a["abands"]) == nb and len(a["bbands"]) == (nb if mr.self_overlaps(m) else 0), (m, nb)
        _check_phases(a, fmt, [m], fb); _check_bands(a, fmt, [m], ans[0]["total"], fb)
        mr.apply_moves(surface, fmt, w, h, [m])
    assert np.array_equal(ans[-1]["bytes"][:fb], surface) and (ans[-2]["bytes"] == POISON).all()


def test_every_refusal(tmp_path):
    sc, want = Script(tmp_path), []
    B, N, Y = sr.PIX_BGR, sr.PIX_NV12_BT709, sr.PIX_YUY2_BT601
    sc.store(5, 38 * 30 * 3)
    for s, fmt, w, h in ((0, B, 37, 29), (1, N, 38, 30), (2, Y, 38, 29)):
        sc.define(s, fmt, w, h)
        sc.keyframe(s, np.full(sr.frame_bytes(fmt, w, h), s + 1, np.uint8))
    sc.define(3, B, 8, 8)                                    # defined, never keyframed; slot 4 is not defined
    head = len(sc.kinds)

    def expect(ms, rc, text=None, null=False):
        sc.moves(ms, null=null); want.append((rc, text))

    good = (0, 0, 0, 10, 10, 4, 4)
    expect([good], ARG, "no bounce buffer")                 # before zly_surface_moves_enable
    sc.bounce(512); want.append(None)
    expect([good] * 2, ARG, "null argument", null=True)
    expect([], ARG, "a call takes 1..1024")
    expect([(0, i % 30, i // 30, i % 30, i // 30, 1, 1) for i in range(1025)], ARG, "1025 moves")
    for bad, rc, text in (
            ((5, 0, 0, 1, 1, 2, 2), ARG, "out of range"), ((-1, 0, 0, 1, 1, 2, 2), ARG, "out of range"),
            ((4, 0, 0, 1, 1, 2, 2), ARG, "not defined"),
            ((3, 0, 0, 1, 1, 2, 2), INPUT, "not valid"),
            ((0, 36, 0, 0, 0, 2, 1), ARG, "source"), ((0, 0, 0, 36, 28, 2, 2), ARG, "destination"),
            ((0, -1, 0, 0, 0, 2, 2), ARG, "source"), ((0, 0, 0, 0, -1, 2, 2), ARG, "destination"),
            ((0, 0, 0, 5, 5, 0, 2), ARG, "source"), ((0, 0, 0, 5, 5, 2, 0), ARG, "source"), ((0, 0, 0, 0, 0, 38, 29), ARG, "source"),
            ((1, 1, 0, 10, 10, 2, 2), ARG, "even"), ((1, 0, 0, 10, 11, 2, 2), ARG, "even"), ((1, 0, 0, 10, 10, 3, 2), ARG, "even"), ((1, 0, 0, 10, 10, 2, 3), ARG, "even"),
            ((2, 0, 0, 11, 10, 2, 1), ARG, "even"), ((2, 1, 1, 10, 10, 2, 1), ARG, "even"),
            ((0, 0, 0, 1, 0, 30, 20), ARG, "bounce buffer")):              # 1800 bytes through a bounce buffer of 512
        expect([good, bad], rc, text)                       # behind a legal move: the whole call is refused
    for s in range(4):
        sc.dump(s); want.append(None)
    expect([(0, 0, 0, 0, 15, 37, 14)], OK)                  # larger than the bounce buffer, clear of itself: needs none
    expect([(0, 0, 0, 0, 0, 37, 29), (1, 0, 0, 0, 0, 38, 30)], OK)      # identities of any size
    expect([(0, i % 36, i // 36, i % 36 + 1, i // 36, 1, 1) for i in range(1024)], OK)     # the most a call takes
    expect([(0, 0, 0, 1, 1, 4, 4), (1, 0, 0, 2, 2, 4, 4), (2, 0, 0, 2, 1, 4, 4), (0, 0, 0, 1, 1, 4, 4)], OK)       # the same cells of three surfaces do not conflict
    ans = sc.run()[head:]
    assert len(ans) == len(want)
    for i, (a, w_) in enumerate(zip(ans, want)):
        if w_ is None:
            continue
        assert a["rc"] == w_[0], (i, a, w_)
        if w_[1]:
            assert w_[1] in a["error"], (i, a["error"])
    dumps = [a["bytes"] for a in ans if "bytes" in a]
    assert (dumps[0][:37 * 29 * 3] == 1).all() and (dumps[1][:38 * 30 * 3 // 2] == 2).all() and (dumps[2][:38 * 29 * 2] == 3).all() and (dumps[3] == POISON).all()
    assert ans[-3]["rc"] == OK and ans[-3]["ajobs"] == [] and ans[-3]["phases"] == [(0, 2, 0, 0, 0, 0, 0)]        # identities: no table, no launch
    assert [p[:2] for p in ans[-1]["phases"]] == [(0, 3), (3, 1)] and [m[2] for m in ans[-1]["moves"]] == [2, 2, 2, 2]


def test_entry_points_answer_before_touching_a_device():
    lib = zly.load_library()
    assert lib.zly_surface_moves_enable(None, 0) == zly.ERR_NOT_INITIALIZED
    assert lib.zly_surface_move(None, 0, None) == zly.ERR_NOT_INITIALIZED
    assert b"Engine not running" in lib.zly_last_error()
    assert zly.SURFACE_MAX_MOVES == int(re.search(r"#define\s+ZLY_SURFACE_MAX_MOVES\s+(\d+)", open(os.path.join(ROOT, "include", "zly.h")).read()).group(1))
    assert C.sizeof(zly.SurfaceMove) == 28
