"""The camera motion's rules as the product's own text computes them on a CPU: tests/cpp/test_camera_rules.cpp compiles csrc/camera_device.h -- the
window, the order of the candidates, the fit, the shift, LOST and step A -- with the host twin of csrc/camera_rules.h (and the change map's host twin
for the sums), and is compared with the numpy oracle (tests/camera_ref.py): the whole record of a stream after every frame, reset and apply, the
table's untouched entries included.  No GPU, no library."""
import os
import subprocess

import numpy as np
import pytest

import camera_cases as cs
import camera_ref as cam
import chip_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TARGET = "zero-latency-yolo_amd/_build/test_camera_rules"
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


def _frame_line(tmp, k, stream, buf, view):
    path = os.path.join(tmp, f"buf{k}.bin")
    np.asarray(buf, dtype=np.uint8).tofile(path)
    fmt, w, h, off, pitch = view
    return f"frame {stream} {fmt} {w} {h} {off[0]} {off[1]} {off[2]} {pitch[0]} {pitch[1]} {pitch[2]} {path}"


def _record(lines, pos):
    """the record the program printed at lines[pos], lines[pos + 1] -> u8 [REC_BYTES]"""
    t, sad = lines[pos].split(), lines[pos + 1].split()
    assert t[0] == "hdr" and sad[0] == "sad" and len(t) == 21 and len(sad) == 1 + cam.SAD_ROOM, (lines[pos], len(sad))
    hdr = np.zeros(1, dtype=cam.HDR_DTYPE)
    names = ("flags", "step", "gw", "gh", "dx", "dy", "fx", "fy", "sx_q4", "sy_q4", "n_lost", "n_applied", "sad_min", "sad_zero", "pend_x_q4", "pend_y_q4")
    for name, v in zip(names, t[1:17]):
        hdr[name] = int(v)
    hdr["pad"] = [int(v) for v in t[17:21]]
    return np.concatenate([hdr.view(np.uint8), np.array([int(v) for v in sad[1:]], dtype=np.uint64).view(np.uint8)])


def _same(got, want, what):
    assert np.array_equal(got, want), (what, got[:96].view(cam.HDR_DTYPE)[0], want[:96].view(cam.HDR_DTYPE)[0], np.flatnonzero(got != want)[:8])


@pytest.mark.parametrize("fmt", cs.FORMATS)
def test_pans_of_five_formats_tight_and_pitched(tmp_path, fmt):
    """per format a pan of five frames (whole cells, sub-cell shifts, a jump beyond the radius) at 200 x 120 and C = 8, R = 4, then three frames at
    72 x 72 with R = 4 -- gw = gh = 2R + 1, a window of one cell -- on the same streams (FIRST: the table keeps the larger geometry's entries);
    stream 0 takes them tight, stream 1 through pitched views between poisoned bytes"""
    cfg = cam.Config(cell=8, radius=4, max_residual_q4=200)
    lines, wants, k = [f"cfg {cfg.cell} {cfg.radius} {cfg.max_residual_q4}"], [], 0
    refs, recs = [cam.Stream(), cam.Stream()], [np.zeros(cam.REC_BYTES, np.uint8) for _ in range(2)]
    flags = set()
    for (w, h, shifts) in ((200, 120, [(8, -16), (6, 4), (-2, 10), (60, 0)]), (72, 72, [(4, 2), (-8, 0)])):
        for bgr in cs.pan(w, h, shifts, 2, seed=fmt + w):
            f, img = cs.as_format(fmt, bgr)
            pbuf, pview = cc.pitched(f, fmt, w, h)
            lines += [_frame_line(str(tmp_path), k, 0, f, cc.tight_view(fmt, w, h)), _frame_line(str(tmp_path), k + 1, 1, pbuf, pview)]
            for s in (0, 1):
                flags.add(int(refs[s].frame(img, cfg, recs[s])["flags"]))
                wants.append(recs[s].copy())
            k += 2
    out = _run(lines)
    assert len(out) == 2 * len(wants)
    for i, want in enumerate(wants):
        _same(_record(out, 2 * i), want, (fmt, i))
    assert flags >= {0, cam.FIRST}, flags


def test_every_cell_and_radius_flags_reset_and_apply(tmp_path):
    """BGR: every cell size at 200 x 120 (200 x 136 at C = 64, whose grid must be three cells high) and every radius 1..4 at 72 x 72 (radius 8 at
    272 x 272 and C = 16: 17 x 17 cells); unrelated frames (LOST), a shift of R cells (CLIPPED), a reset between frames, and step A on a track table
    with live and dead slots, after a frame and after a reset"""
    lines, wants, k = [], [], 0
    flags = set()

    def run(cfg, w, h, shifts, seed, script):
        """script: per frame of the pan, what follows it: None, "reset" or "apply" """
        nonlocal k
        lines.extend([f"cfg {cfg.cell} {cfg.radius} {cfg.max_residual_q4}", "reset 3"])
        ref, rec = cam.Stream(), wants[-1][1].copy() if wants else np.zeros(cam.REC_BYTES, np.uint8)
        ref.n_lost, ref.n_applied = (int(rec[:96].view(cam.HDR_DTYPE)[0][n]) for n in ("n_lost", "n_applied"))
        ref.reset(rec)
        rng = np.random.default_rng(seed)
        for bgr, then in zip(cs.pan(w, h, shifts, 1, seed), script):
            lines.append(_frame_line(str(tmp_path), k, 3, bgr.reshape(-1), cc.tight_view(0, w, h)))
            flags.add(int(ref.frame(bgr, cfg, rec)["flags"]))
            wants.append(("rec", rec.copy()))
            k += 1
            if then == "reset":
                lines.append("reset 3")
                ref.reset(rec)
            elif then in ("apply", "reset+apply"):
                if then == "reset+apply":
                    lines.append("reset 3")
                    ref.reset(rec)
                x, y = rng.random(64, dtype=np.float32), rng.random(64, dtype=np.float32)
                live = (rng.random(64) < 0.6).astype(np.uint32)
                lines.append("tracks 3 64 " + " ".join(f"{int(live[t])} {int(x[t:t + 1].view(np.uint32)[0])} {int(y[t:t + 1].view(np.uint32)[0])}" for t in range(64)))
                lines.append("apply 3")
                ref.apply(x, y, live, rec)
                wants.append(("xy", np.stack([x.view(np.uint32), y.view(np.uint32)], axis=1).reshape(-1).copy()))
                wants.append(("rec", rec.copy()))

    for C in cam.CELLS:
        run(cam.Config(cell=C, radius=1, max_residual_q4=4080), 200, 136 if C == 64 else 120, [(C, 0), (3, -5)], 20 + C, [None, "apply", None])
    for R in (1, 2, 3, 4):
        run(cam.Config(cell=8, radius=R, max_residual_q4=4080), 72, 72, [(8 * R, 0), (-3, 2), (1, 1)], 30 + R, [None, "apply", "reset", "reset+apply"])
    run(cam.Config(cell=16, radius=8, max_residual_q4=4080), 272, 272, [(-37, 50), (128, -128)], 40, [None, None, "apply"])
    run(cam.Config(cell=8, radius=4, max_residual_q4=16), 200, 120, [(8, 8), (90, 70), (0, 8)], 41, ["apply", None, None, "apply"])      # the jump: LOST
    out = _run(lines)
    pos = 0
    for kind, want in wants:
        if kind == "xy":
            t = out[pos].split()
            assert t[0] == "xy" and [int(v) for v in t[1:]] == want.tolist()
            pos += 1
        else:
            _same(_record(out, pos), want, pos)
            pos += 2
    assert pos == len(out) and flags >= {0, cam.FIRST, cam.CLIPPED, cam.LOST | cam.CLIPPED}, flags          # the jump's best match lies at the rim


def test_refusals(tmp_path):
    """a grid below 2R + 1 cells on either axis (72 x 40 at C = 8 is 9 x 5 cells: legal up to R = 2), more than ZLY_CHANGE_MAX_CELLS cells, and a view
    whose last row leaves the buffer"""
    f = np.zeros(1024 * 520 * 3, dtype=np.uint8)
    lines = ["cfg 8 4 64",
             _frame_line(str(tmp_path), 0, 0, f[:64 * 72 * 3], cc.tight_view(0, 64, 72)),        # 8 x 9 cells
             _frame_line(str(tmp_path), 1, 0, f[:64 * 72 * 3], cc.tight_view(0, 72, 64)),        # 9 x 8
             _frame_line(str(tmp_path), 2, 0, f[:65 * 65 * 3], cc.tight_view(0, 65, 65)),        # 9 x 9: accepted
             _frame_line(str(tmp_path), 3, 0, f, cc.tight_view(0, 1024, 520)),                   # 128 x 65 = 8320 cells
             _frame_line(str(tmp_path), 4, 0, f[:65 * 65 * 3 - 1], cc.tight_view(0, 65, 65))]
    out = _run(lines)
    assert out[0] == out[1] == out[4] == out[5] == f"refused {INVALID_INPUT}" and out[2].startswith("hdr 1 1 9 9 ")
    small = np.zeros(72 * 40 * 3, dtype=np.uint8)
    out = _run([ln for R in (1, 2, 3, 4) for ln in (f"cfg 8 {R} 64", _frame_line(str(tmp_path), 5, 0, small, cc.tight_view(0, 72, 40)))] +
               ["cfg 64 1 64", _frame_line(str(tmp_path), 6, 0, f[:200 * 120 * 3], cc.tight_view(0, 200, 120))])
    assert [ln.split()[0] for ln in out] == ["hdr", "sad", "hdr", "sad", "refused", "refused", "refused"]
