"""The cases of tests/golden/frame_rules_parent.json and how one case is put to a libzly.so: the six entry points that answer on the host alone
(zly_frame_bytes, zly_view_bytes, zly_view_tight, zly_view_crop, zly_letterbox_geometry, zly_tile_grid; no device is touched, no engine made).

The golden file records what the library answered BEFORE these rules moved into csrc/frame_rules.h; tests/test_frame_rules_golden.py replays it
through the library of the tree.  It was written once, against a library built from the commit before the move:

    ZLY_LIB=<that commit's libzly.so> python3 tests/frame_rules_cases.py --record

and is not regenerated from the code under test: a change of a rule that is meant shows as a diff of the file, made by hand or by recording at
the last commit whose answers are still the wanted ones.

Layout of the file: {"messages": [...], "<family>": [[inputs, outputs], ...]}.  An output list starts with the return code and the index of the
zly_last_error text in "messages" (-1: the call did not fail); run_<family>(lib, inputs) returns the same list with the text itself.  The inputs of
a "crop" or "crop2" case start with the index of their surface among the "surface" cases, in place of its ten fields.
"""
import ctypes as C
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zero-latency-yolo_amd"))
import zly  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "frame_rules_parent.json")
FAMILIES = ("frame", "surface", "crop", "crop2", "letterbox", "tiles")
I32MAX = 2**31 - 1
U64MAX = 2**64 - 1
KNOWN = (0, 1, 2, 3, 4, 10, 11, 12, 13, 16, 17, 18)
S = -7                                    # what every output is filled with before a call: a refused call must leave it


# ---- the library side -----------------------------------------------------------------------------------------------------------------------
def _view(fields=None):
    v = zly.FrameView()
    fmt, w, h, pad, o0, o1, o2, p0, p1, p2 = fields if fields is not None else [S] * 10
    v.fmt, v.w, v.h, v.pad_ = fmt, w, h, pad
    for i, (o, p) in enumerate(((o0, p0), (o1, p1), (o2, p2))):
        v.off[i] = o & U64MAX
        v.pitch[i] = p
    return v


def _fields(v):
    return [v.fmt, v.w, v.h, v.pad_, *[int(x) for x in v.off], *[int(x) for x in v.pitch]]


SENTINEL = _fields(_view())


def _status(lib, rc):
    return [rc, lib.zly_last_error().decode() if rc != zly.OK else ""]


def run_frame(lib, c):
    """[fmt, w, h] -> [rc, message of zly_view_tight, zly_frame_bytes, the tight view (None: left as it was), zly_view_bytes of it]"""
    fmt, w, h = c
    out = _view()
    rc = lib.zly_view_tight(fmt, w, h, C.byref(out))
    f = _fields(out)
    return [*_status(lib, rc), lib.zly_frame_bytes(fmt, w, h), None if f == SENTINEL else f, lib.zly_view_bytes(C.byref(out))]


def run_surface(lib, c):
    """the ten fields of a view -> [0, "", zly_view_bytes]"""
    return [0, "", lib.zly_view_bytes(C.byref(_view(c)))]


def _crop(lib, surface, rect, out):
    rc = lib.zly_view_crop(C.byref(surface), *rect, C.byref(out))
    return _status(lib, rc)


def _crop_result(lib, before, out):
    """what a crop wrote: None if nothing; else [w, h, off0, off1, off2], zly_view_bytes of it, and whether fmt, pad_ and the pitches are the surface's"""
    f = _fields(out)
    if f == SENTINEL:
        return [None, 0, True]
    return [f[1:3] + f[4:7], lib.zly_view_bytes(C.byref(out)), f[0] == before[0] and f[3] == before[3] and f[7:] == before[7:]]


def run_crop(lib, c):
    """[view fields, [x0, y0, w, h]] -> [rc, message, *_crop_result]"""
    surface, out = _view(c[0]), _view()
    st = _crop(lib, surface, c[1], out)
    assert _fields(surface) == _fields(_view(c[0]))          # the surface is read only
    return [*st, *_crop_result(lib, c[0], out)]


def run_crop2(lib, c):
    """[view fields, rect, rect of the first crop's result] -> the second crop's [rc, message, *_crop_result], made in place (out = its own surface)"""
    v = _view(c[0])
    st = _crop(lib, v, c[1], v)
    assert st[0] == zly.OK, st
    before = _fields(v)
    st = _crop(lib, v, c[2], v)
    if st[0] != zly.OK:
        return [*st, None if _fields(v) == before else _fields(v), 0, True]       # a refused crop leaves its output, here its surface, alone
    return [*st, *_crop_result(lib, c[0], v)]


def run_letterbox(lib, c):
    """[w, h, model_w, model_h, mask of null outputs] -> [rc, message, nw, nh, pad_x, pad_y] (a null or untouched output: S)"""
    w, h, mw, mh, nulls = c
    o = [C.c_int32(S) for _ in range(4)]
    rc = lib.zly_letterbox_geometry(w, h, mw, mh, *[None if nulls >> i & 1 else C.byref(o[i]) for i in range(4)])
    return [*_status(lib, rc), *[x.value for x in o]]


def run_tiles(lib, c):
    """[W, H, tile_w, tile_h, overlap_x, overlap_y, even, cap] -> [rc, message, n_out, the tiles written, nothing written behind them]
    the tiles: all of them up to four, else the first two, the last two and the first 16 hex digits of the SHA-256 of the array's bytes"""
    cap = c[7]
    tiles = (zly.Tile * (cap + 1))()
    C.memset(tiles, 0xA5, C.sizeof(tiles))
    n = C.c_int32(S)
    rc = lib.zly_tile_grid(*c[:7], tiles, cap, C.byref(n))
    raw = bytes(tiles)
    ts = C.sizeof(zly.Tile)
    written = min(cap, n.value) if rc == zly.OK else 0
    tail_clean = raw[written * ts:] == b"\xa5" * (len(raw) - written * ts)
    rows = [[getattr(tiles[i], k) for k, _ in zly.Tile._fields_] for i in (range(written) if written <= 4 else (0, 1, written - 2, written - 1))]
    if written > 4:
        rows.append(hashlib.sha256(raw[:written * ts]).hexdigest()[:16])
    return [*_status(lib, rc), n.value, rows, tail_clean]


RUN = {"frame": run_frame, "surface": run_surface, "crop": run_crop, "crop2": run_crop2, "letterbox": run_letterbox, "tiles": run_tiles}


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------
def _planes(fmt, w, h):
    """rows and bytes per row of the planes of a known format (the generator's own arithmetic, used only to place pitches and offsets)"""
    if fmt in (1, 3):
        return [(h, w), (h // 2, w)]
    if fmt in (2, 4):
        return [(h, w), (h // 2, w // 2), (h // 2, w // 2)]
    return [(h, {0: 3, 16: 3, 17: 4, 18: 4}.get(fmt, 2) * w)]


def _surface(fmt, w, h, extra=0, base=0):
    """a w x h view of format fmt: every pitch its row's bytes + extra, the planes behind each other from byte `base`"""
    off, pitch, at = [0, 0, 0], [0, 0, 0], base
    for p, (rows, rb) in enumerate(_planes(fmt, w, h)):
        off[p], pitch[p] = at, rb + extra
        at += rows * (rb + extra)
    return [fmt, w, h, 0, *off, *pitch]


def frame_inputs():
    sizes = [(v, v) for v in (0, -1, 1, 2, 3, 4, 416, 417, 32768, I32MAX)]
    sizes += [(1920, 1080), (416, 417), (417, 416), (2, 1), (1, 2), (2, 3), (3, 2), (4, 0), (0, 4), (-1, 4), (4, -1),
              (I32MAX, 2), (2, I32MAX), (I32MAX - 1, I32MAX - 1), (32768, I32MAX - 1), (I32MAX - 1, 32768)]
    return [[fmt, w, h] for fmt in range(-1, 21) for w, h in sizes]


W0, H0 = 64, 48
RECTS = [
    [0, 0, 32, 24], [0, 0, W0, H0],                                                  # at the origin; the whole surface
    [8, 6, 32, 24],                                                                  # interior, all even
    [9, 6, 32, 24], [8, 7, 32, 24], [8, 6, 31, 24], [8, 6, 32, 23],                  # odd x0, y0, w, h, one at a time
    [32, 24, 32, 24],                                                                # flush against the bottom-right corner
    [-1, 0, 32, 24], [0, -1, 32, 24], [33, 24, 32, 24], [32, 25, 32, 24],            # one pixel past each edge ...
    [-2, 0, 32, 24], [0, -2, 32, 24], [34, 24, 32, 24], [32, 26, 32, 24],            # ... and the even rectangle nearest to it
    [8, 6, 0, 24], [8, 6, 32, 0], [8, 6, -1, 24], [8, 6, 32, -2],                    # zero and negative sizes
    [2, 0, I32MAX, 24], [I32MAX, 0, 2, 24], [0, 2, 32, I32MAX], [0, I32MAX - 1, 32, 2], [I32MAX - 1, I32MAX - 1, 2, 2],     # x0 + w, y0 + h past INT32_MAX
]
SECOND = [[4, 2, 16, 12], [0, 0, 32, 24], [16, 12, 16, 12], [3, 2, 16, 12], [4, 1, 16, 12], [18, 2, 16, 12]]      # of the 32 x 24 result of RECTS[2]


def standard_surfaces():
    return [_surface(fmt, W0, H0, extra) for fmt in KNOWN for extra in (0, 1, 64)]


def invalid_surfaces():
    """views at and just inside each limit of the validity rule (include/zly.h), per known format and plane; views of unknown formats"""
    out = []
    for fmt in KNOWN:
        tight = _surface(fmt, W0, H0)
        for p, (rows, rb) in enumerate(_planes(fmt, W0, H0)):
            v = list(tight); v[7 + p] = rb - 1; out.append(v)                        # a pitch one byte below its row
            reach = -(-(2**31 - rb) // (rows - 1))                                   # the least pitch whose extent reaches 2^31
            for pitch in (reach - 1, reach):
                v = list(tight); v[7 + p] = pitch; out.append(v)
            ext = (rows - 1) * rb + rb
            for off in (U64MAX - ext, U64MAX - ext + 1, U64MAX):                     # the last offset that fits, the first that does not
                v = list(tight); v[4 + p] = off; out.append(v)
    for fmt in (-1, 5, 9, 14, 15, 19, 20, I32MAX):
        v = _surface(0, W0, H0); v[0] = fmt; out.append(v)
    out += [_surface(1, 63, 48), _surface(2, 64, 47), _surface(10, 63, 48), _surface(10, 64, 47), _surface(0, 0, 48), _surface(0, 64, -1)]
    return out


def crop_inputs():
    return [[s, r] for s in standard_surfaces() for r in RECTS] + [[s, [0, 0, 2, 2]] for s in invalid_surfaces()]


def crop2_inputs():
    return [[s, RECTS[2], r] for s in standard_surfaces() for r in SECOND]


def letterbox_inputs():
    req = [(1, 1), (2, 1), (416, 416), (1920, 1080), (1080, 1920), (16384, 16384), (I32MAX, I32MAX), (I32MAX, 1), (1, I32MAX)]
    out = [[w, h, mw, mh, 0] for w, h in req for mw, mh in ((416, 416), (640, 384), (1, 1))]
    out += [[0, 1080, 416, 416, 0], [1920, 0, 416, 416, 0], [1920, 1080, 0, 416, 0], [1920, 1080, 416, 0, 0], [-1, 1080, 416, 416, 0],
            [1920, 1080, 416, -416, 0], [0, 0, 0, 0, 0]]
    out += [[1920, 1080, 416, 416, m] for m in (1, 2, 4, 8, 15)] + [[0, 1080, 416, 416, 15], [1920, 1080, 0, 0, 1]]
    return out


def _axis_count(extent, tile, overlap, even):
    """the generator's own count of one axis (None: refused), used only to choose the caps"""
    if extent < 1 or extent >= 2**24 or tile < 1 or overlap < 0 or overlap >= tile or (even and (extent | tile) & 1):
        return None
    return 1 if tile >= extent else -(-(extent - tile) // (tile - overlap)) + 1


def tiles_inputs():
    out, seen = [], set()

    def add(W, H, tw, th, ox, oy, even):
        nx, ny = _axis_count(W, tw, ox, even), _axis_count(H, th, oy, even)
        count = None if nx is None or ny is None or nx * ny > I32MAX else nx * ny
        caps = [0] if count is None else [0] + ([min(3, count - 1)] if count > 1 else []) + ([count] if count < 4096 else [])
        for cap in caps:
            key = (W, H, tw, th, ox, oy, even, cap)
            if key not in seen:
                seen.add(key); out.append(list(key))

    for extent in (1, 2, 415, 416, 417, 1920, 2**24 - 1, 2**24):
        for tile in (0, 1, 416, extent + 1):
            for overlap in (-1, 0, 32, tile - 1, tile):
                for even in (0, 1):
                    add(extent, 416, tile, 416, overlap, 0, even)                    # the x axis alone (one row of tiles) ...
                    if extent in (417, 1920):
                        add(416, extent, 416, tile, 0, overlap, even)                # ... the y axis alone (the same rule: two extents)
    for even in (0, 1):                                                              # both axes
        add(1920, 1080, 416, 416, 32, 32, even); add(1920, 1080, 640, 384, 0, 64, even); add(417, 415, 416, 416, 32, 0, even)
        add(2**24 - 1, 2**24 - 1, 1, 1, 0, 0, even); add(2**24 - 2, 2**24 - 2, 416, 416, 415, 415, even)      # too many tiles
        add(2**24 - 2, 2**24 - 2, 512, 512, 0, 0, even)                              # 32768 x 32768: the most that fit
    return out


INPUTS = {"frame": frame_inputs, "surface": lambda: standard_surfaces() + invalid_surfaces(), "crop": crop_inputs, "crop2": crop2_inputs,
          "letterbox": letterbox_inputs, "tiles": tiles_inputs}


# ---- the file -------------------------------------------------------------------------------------------------------------------------------
def load():
    """{family: [(inputs, outputs with the message text)]}"""
    g = json.load(open(GOLDEN))
    msgs = g["messages"]
    surfaces = [i for i, _ in g["surface"]]
    return {fam: [([surfaces[i[0]], *i[1:]] if fam.startswith("crop") else i, [o[0], msgs[o[1]] if o[1] >= 0 else "", *o[2:]]) for i, o in g[fam]]
            for fam in FAMILIES}


def record(path):
    lib = zly.load_library()
    msgs, doc = [""], {}
    surfaces = INPUTS["surface"]()
    for fam in FAMILIES:
        rows = []
        for c in INPUTS[fam]():
            o = json.loads(json.dumps(RUN[fam](lib, c)))
            if o[1] not in msgs:
                msgs.append(o[1])
            rows.append([[surfaces.index(c[0]), *c[1:]] if fam.startswith("crop") else c, [o[0], msgs.index(o[1]) if o[0] != zly.OK else -1, *o[2:]]])
        doc[fam] = rows
    with open(path, "w") as f:
        f.write('{"messages": ' + json.dumps(msgs) + ",\n")
        for k, fam in enumerate(FAMILIES):
            f.write(f'"{fam}": [\n' + ",\n".join(json.dumps(r, separators=(",", ":")) for r in doc[fam]) + "\n]" + (",\n" if k + 1 < len(FAMILIES) else "}\n"))
    print(f"{path}: " + ", ".join(f"{fam} {len(doc[fam])}" for fam in FAMILIES) + f"; {len(msgs) - 1} messages, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    if sys.argv[1:2] != ["--record"]:
        sys.exit(__doc__)
    record(sys.argv[2] if len(sys.argv) > 2 else GOLDEN)
