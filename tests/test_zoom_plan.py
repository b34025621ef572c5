"""The plan of the zoom regions as the product's own text computes it on a CPU: tests/cpp/test_zoom_plan.cpp compiles csrc/zoom_device.h -- the
functions the plan kernel executes -- through the host twin of csrc/zoom_rules.h.  Compared with regions written by hand, with the numpy oracle on
seeded random tables, and (the per-plane offset arithmetic the kernel patches descriptors with) against zly_view_crop's own for all twelve formats.
No GPU, no library."""
import os
import subprocess

import numpy as np

import zoom_ref
from zoom_cases import hand_cases, random_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TARGET = "zero-latency-yolo_amd/_build/test_zoom_plan"


def _program():
    path = os.path.join(ROOT, TARGET)
    if not os.path.exists(path):
        subprocess.run(["make", "-C", ROOT, TARGET], check=True, stdout=subprocess.DEVNULL)
    return path


def _bits(v) -> str:
    return "%x" % int(np.array(v, dtype=np.float32).view(np.uint32))


def run_plans(cases):
    """cases: (Table, Config, W, H) each -> one REGION_DTYPE array per case, from the program"""
    lines = [str(len(cases))]
    for t, cfg, W, H in cases:
        lines.append(f"{t.T} {cfg.regions} {cfg.region_w} {cfg.region_h} {cfg.max_age} {cfg.class_id} {W} {H} {t.frame_no & 0xFFFFFFFF}")
        for s in range(t.T):
            x, y, w, h = t.box[s]
            lines.append(f"{int(t.live[s])} {t.cls[s]} {t.id[s]} {t.last_seen[s]} {_bits(x)} {_bits(y)} {_bits(w)} {_bits(h)} {_bits(t.vx[s])} {_bits(t.vy[s])}")
    p = subprocess.run([_program(), "plan"], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr
    rows = [tuple(int(v) for v in ln.split()) for ln in p.stdout.splitlines()]
    out, k = [], 0
    for _, cfg, _, _ in cases:
        out.append(np.array(rows[k:k + cfg.regions], dtype=zoom_ref.REGION_DTYPE))
        k += cfg.regions
    assert k == len(rows)
    return out


def test_hand_cases():
    cases = hand_cases()
    got = run_plans([(t, cfg, W, H) for _, t, cfg, W, H, _ in cases])
    for (name, t, cfg, W, H, expected), g in zip(cases, got):
        rw, rh, _, _ = zoom_ref.size(cfg, W, H)
        want = [(x0, y0, rw, rh, slot, t.id[slot] if slot >= 0 else 0) for x0, y0, slot in expected]
        assert [tuple(int(v) for v in r) for r in g] == want, name


def test_random_tables_equal_the_oracle():
    rng = np.random.default_rng(2024)
    cases = [random_case(rng) for _ in range(3000)]
    got = run_plans(cases)
    n_zoomed = n_covered = 0
    for i, ((t, cfg, W, H), g) in enumerate(zip(cases, got)):
        want, covered = zoom_ref.plan(t, cfg, W, H, with_covered=True)
        assert g.tobytes() == want.tobytes(), (i, cfg, W, H, g, want)
        n_zoomed += int((want["slot"] >= 0).sum())
        n_covered += len(covered)
    assert n_zoomed > 3000 and n_covered > 300          # the tables exercise the choice, not only the fallback


def test_plane_offsets_equal_view_crop():
    p = subprocess.run([_program(), "offsets"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and p.stdout.startswith("offsets ok "), p.stdout + p.stderr
    assert int(p.stdout.split()[2]) > 12 * 2 * 500


def test_selftest():
    p = subprocess.run([_program(), "selftest"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and p.stdout.rstrip().endswith("selftest ok"), p.stdout + p.stderr
