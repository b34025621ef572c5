"""The pre-pass kernel's per-axis footprint arithmetic (csrc/area_device.h: area_span, area_weight -- __host__ __device__, so the host compiler
takes them as they are) against the oracle tests/area_ref.py: tests/cpp/test_area_footprint.cpp prints i0, i1, w(i0), w(i1) and the weights' sum
for (S, D, d) triples; compared for the pairs of tests/test_area_ref.py at d = 0, D - 1 and 50 seeded d, and for every d of every small pair."""
import os
import subprocess

import numpy as np
import pytest

import area_ref as ar

PAIRS = ar.PAIRS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TARGET = "zero-latency-yolo_amd/_build/test_area_footprint"


def _run(triples):
    path = os.path.join(ROOT, TARGET)
    if not os.path.exists(path):
        subprocess.run(["make", "-C", ROOT, TARGET], check=True, stdout=subprocess.DEVNULL)
    out = {}
    for a in range(0, len(triples), 2000):                 # a few command lines, not one per triple
        args = [str(v) for t in triples[a:a + 2000] for v in t]
        r = subprocess.run([path] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr
        for line in r.stdout.splitlines():
            v = [int(x) for x in line.split()]
            out[tuple(v[:3])] = tuple(v[3:])
    assert len(out) == len(set(triples))
    return out


@pytest.mark.parametrize("S,D", PAIRS)
def test_footprints_of_the_large_pairs(S, D):
    ds = sorted({0, D - 1, *np.random.default_rng(S * 131 + D).integers(0, D, 50).tolist()})
    got = _run([(S, D, d) for d in ds])
    for d in ds:
        assert got[(S, D, d)] == (*ar.footprint(S, D, d), S), (S, D, d)


def test_footprints_of_every_small_pair():
    triples = [(S, D, d) for S in range(1, 13) for D in range(1, 13) for d in range(D)]
    got = _run(triples)
    for S, D, d in triples:
        assert got[(S, D, d)] == (*ar.footprint(S, D, d), S), (S, D, d)


def test_extremes_fit_int32():
    """S = D = 16384 (ZLY_AREA_MAX_DIM) at the last index: the largest products of the arithmetic, 2^28"""
    M = ar.MAX_DIM
    got = _run([(M, M, M - 1), (M, 1, 0), (1, M, M - 1), (M, M - 1, M - 2)])
    for (S, D, d), v in got.items():
        assert v == (*ar.footprint(S, D, d), S), (S, D, d)
