"""The Detect tail's early-out bound (csrc/head_skip.h, HeadArgs::skip_logit) is SAFE: no class logit below it scores conf_thr or more.

tests/cpp/test_head_skip.cpp prints the bound exactly as launch_head_fused computes it.  For every threshold below, EVERY fp32 logit z in
[bound - 1, bound) is scored (the sigmoid is monotone, so lower logits score no higher) and no score may reach the threshold:
  * in IEEE fp32 arithmetic, float32(1 / (float32(1) + float32(exp(-z)))): the fp32 engine's expf and divide;
  * with e = exp(-z) and the quotient each moved one fp32 step either way: the bf16 engine's v_exp_f32 and v_rcp_f32 are good to one ulp
    each and cannot be run here, so all four moved scans stand in for them.
The same scan shows why the bound changed: under the earlier logit(thr) - 1e-2 a logit that passes exists from thr = 1 - 34 * 2^-24 up."""
import os
import subprocess

import numpy as np
import pytest

import head_cases as hc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TARGET = "zero-latency-yolo_amd/_build/test_head_skip"
F32 = np.float32
THRESHOLDS = [F32(0.05), F32(0.5), F32(0.9)] + [hc.thr_of_k(k) for k in hc.K_VALUES]
CHUNK = 1 << 22


def _bits(v):
    return int(np.asarray(v, dtype=np.float32).view(np.uint32))


@pytest.fixture(scope="module")
def bounds():
    """{threshold bits: bound (fp32)} from the C++ header, through the host binary (built on demand; `make host` builds it)"""
    path = os.path.join(ROOT, TARGET)
    if not os.path.exists(path):
        subprocess.run(["make", "-C", ROOT, TARGET], check=True, stdout=subprocess.DEVNULL)
    extra = [F32(0.0), F32(-1.0), F32(1.0), F32(2.0), F32(0.25)]
    r = subprocess.run([path] + [f"{_bits(t):08x}" for t in THRESHOLDS + extra], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    out = {}
    for line in r.stdout.split("\n"):
        if line:
            tb, bb, _ = line.split()
            out[int(tb, 16)] = np.array([int(bb, 16)], dtype=np.uint32).view(np.float32)[0]
    return out


def _ordered(v):
    """fp32 -> int64 key that grows with the value (the bit pattern, mirrored for negative values)"""
    b = np.asarray(v, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.where(b >= 0, b, -(b & 0x7fffffff))


def _from_ordered(k):
    k = np.asarray(k, dtype=np.int64)
    return np.where(k >= 0, k, (-k) | 0x80000000).astype(np.uint32).view(np.float32)


def _every_f32(lo, hi):
    """every fp32 value in [lo, hi), in chunks"""
    k0, k1 = int(_ordered(F32(lo))), int(_ordered(F32(hi)))
    for a in range(k0, k1, CHUNK):
        yield _from_ordered(np.arange(a, min(a + CHUNK, k1), dtype=np.int64))


def _best_scores(z):
    """-> (largest IEEE score, largest score over the four moved scans) of the fp32 logits z"""
    e = np.exp(-z.astype(np.float64)).astype(np.float32)
    one = F32(1.0)
    ieee = (one / (one + e)).max()
    moved = F32(0.0)
    for e_to in (F32(-np.inf), F32(np.inf)):
        em = np.maximum(np.nextafter(e, e_to), F32(0.0))
        q = one / (one + em)
        for q_to in (F32(-np.inf), F32(np.inf)):
            moved = max(moved, np.nextafter(q, q_to).max())
    return ieee, moved


def _scan(lo, hi):
    ieee, moved = F32(0.0), F32(0.0)
    for z in _every_f32(lo, hi):
        a, b = _best_scores(z)
        ieee, moved = max(ieee, a), max(moved, b)
    return ieee, moved


@pytest.mark.parametrize("thr", THRESHOLDS, ids=lambda t: f"{float(t):.9g}")
def test_no_logit_below_the_bound_reaches_the_threshold(bounds, thr):
    bound = bounds[_bits(thr)]
    assert bound == hc.skip_logit(thr) or abs(float(bound) - float(hc.skip_logit(thr))) <= float(np.spacing(bound)), (bound, hc.skip_logit(thr))
    ieee, moved = _scan(bound - F32(1.0), bound)
    print(f"thr {float(thr):.9g}: bound {float(bound):.6f}; largest score below it {float(ieee):.9g} (IEEE), {float(moved):.9g} (e and quotient moved one step)")
    assert ieee < thr, (float(thr), float(bound), float(ieee))
    assert moved < thr, (float(thr), float(bound), float(moved))


@pytest.mark.parametrize("k", hc.K_VALUES)
def test_the_earlier_margin_is_unsafe_exactly_where_the_analysis_says(k):
    """logit(thr) - 1e-2, scanned the same way: a passing logit lies below it for k <= 34 and none does for k >= 100"""
    thr = hc.thr_of_k(k)
    old = hc.skip_logit_margin_only(thr)
    ieee, _ = _scan(old - F32(1.0), old)
    assert (ieee >= thr) == (k <= 34), (k, float(old), float(ieee))


def test_bound_at_the_edges(bounds):
    assert bounds[_bits(F32(0.0))] == F32(-3.0e38) and bounds[_bits(F32(-1.0))] == F32(-3.0e38)      # keeps everything
    # thr >= 1 is the formula's own limit: below the z >= 16.6 a score of 1.0f needs, and no special case
    assert bounds[_bits(F32(1.0))] == bounds[_bits(F32(2.0))]
    assert 15.0 < bounds[_bits(F32(1.0))] < 16.0
    # away from 1 the bound is the earlier one but for 4 * 2^-24 * thr / (1 - thr): 2.4e-7 at 0.5, the seventh digit
    for t in (F32(0.25), F32(0.5), F32(0.9)):
        moved, step = float(hc.skip_logit_margin_only(t)) - float(bounds[_bits(t)]), float(np.spacing(np.abs(bounds[_bits(t)])))
        assert -step <= moved <= 4 * 2.0 ** -24 * float(t) / (1 - float(t)) + 2 * step, (float(t), moved)
    ks = [bounds[_bits(hc.thr_of_k(k))] for k in sorted(hc.K_VALUES)]
    assert all(a > b for a, b in zip(ks, ks[1:]))                                # monotone in the threshold
