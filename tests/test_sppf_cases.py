"""tests/sppf_cases.py on the CPU: the direct-window reference against two independent forms, the integer-domain model of the fast kernels
against the reference, proof that the case table catches the mistakes it was built for, and the CPU floor of closed_loop_ref's bound on the
fused kernel's inputs.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import closed_loop_ref as cl
import sppf_cases as sc
import sppf_fused_ref as fr
from sppf_cases import BF16, FP32

TABLES = {"pool16": sc.pool16_table, "six_pass_bf16": lambda: sc.six_pass_table(BF16), "six_pass_fp32": lambda: sc.six_pass_table(FP32)}


def test_table_covers_shapes_layouts_and_patterns():
    p16 = sc.pool16_table()
    assert {(c.H, c.W) for c in p16} == {(h, w) for h in range(1, 17) for w in range(1, 17)} and all(c.pool16 for c in p16)
    assert {(c.c, c.cs) for c in sc.all_cases()} == set(sc.LAYOUTS)
    assert {c.n for c in p16} == {1, 2, 16}
    for dtype in (BF16, FP32):
        six = sc.six_pass_table(dtype)
        assert not any(c.pool16 for c in six)
        assert {(17, 16), (16, 17), (20, 20), (1, 40), (40, 1), (40, 40), (41, 41)} <= {(c.H, c.W) for c in six}
        assert any(c.n == 17 and c.H <= 16 and c.W <= 16 and not c.six_pass for c in six)
        assert 3 * 41 * 41 * 32 <= 160 * 1024 < 3 * sc.REFUSED_SHAPE[0] * sc.REFUSED_SHAPE[1] * 32
    fams = {dt: set() for dt in (BF16, FP32)}
    names = {dt: set() for dt in (BF16, FP32)}
    for c in sc.all_cases():
        bits, infos = sc.case_maps(c)
        assert not sc.is_nan(bits, c.dtype).any()
        if c.H * c.W >= 9:                                                      # (a map of a few pixels has too few states to be unlike all others)
            flat = bits.reshape(c.n, -1, c.c)
            for f in range(c.n):
                for g in range(0, c.c, 8):                                          # no two channels of one 16-byte group share a map ...
                    assert len({flat[f, :, ch].tobytes() for ch in range(g, g + 8)}) == 8, (c.name, f, g)
                for ch in range(c.c):                                               # ... and no channel has its neighbour frames' map
                    assert f == 0 or flat[f, :, ch].tobytes() != flat[f - 1, :, ch].tobytes(), (c.name, f, ch)
        for row in infos:
            for i in row:
                fams[c.dtype].add(i.family)
                names[c.dtype].add(i.pattern)
    assert fams[BF16] == fams[FP32] == set(sc.FAMILIES)
    assert names[BF16] == set(sc.OTHERS[BF16]) | {"impulse"} and names[FP32] == set(sc.OTHERS[FP32]) | {"impulse"}


@pytest.mark.parametrize("table", list(TABLES))
def test_direct_windows_equal_chained_pools_and_torch(table):
    """the reference (direct windows of radius 2, 4, 6) = three chained radius-2 pools = torch's max_pool2d chained three times.  Against torch
    numerically (its zero sign is whatever its compare leaves); against the chained form bit for bit, which includes the zero rule; and the
    zero rule itself once more from its definition."""
    for c in TABLES[table]():
        bits, _ = sc.case_maps(c)
        ref = sc.case_reference(c)
        for a, b in zip(ref, sc.ref_pools_chained(bits, c.dtype)):
            assert np.array_equal(a, b), c.name
        t = torch.from_numpy(sc.to_f64(bits, c.dtype)).permute(0, 3, 1, 2)
        for k in range(3):
            t = F.max_pool2d(t, 5, 1, 2)
            assert np.array_equal(t.permute(0, 2, 3, 1).numpy(), sc.to_f64(ref[k], c.dtype)), (c.name, k)
        sign = 1 << (sc.width(c.dtype) - 1)
        for k, r in enumerate(sc.RADII):
            zero = sc.to_f64(ref[k], c.dtype) == 0
            for f, y, x, ch in zip(*np.nonzero(zero)):
                win = bits[f, max(y - r, 0):y + r + 1, max(x - r, 0):x + r + 1, ch]
                assert int(ref[k][f, y, x, ch]) == (0 if (win == 0).any() else sign), (c.name, k, f, y, x, ch)


@pytest.mark.parametrize("table", list(TABLES))
def test_integer_domain_model_equals_reference(table):
    """T, integer max over the window with the smallest integer outside the map, T again: what sppf_pool16_kernel and sppf_fused_kernel do"""
    for c in TABLES[table]():
        for a, b in zip(sc.t_pools(sc.case_maps(c)[0], c.dtype), sc.case_reference(c)):
            assert np.array_equal(a, b), c.name


def test_integer_order_is_the_reference_order_for_every_bf16_pair():
    """All 65282 non-NaN (65536 - 2 x 127 NaNs) bf16 patterns, ordered as the reference orders them (by value; -0 below +0), have strictly increasing T.  Two
    patterns therefore compare under T as under the reference -- for every one of the 65282^2 pairs, without enumerating them -- and the
    integer max of any window selects the reference's pattern.  The padding integer lies below all of them; T(-inf) is its upper neighbour
    but 0x7f patterns (the negative NaNs) apart."""
    pats = sc.NON_NAN_BF16
    assert len(pats) == 65282
    v = sc.to_f64(pats, BF16)
    order = np.lexsort((pats == 0, v))                                           # by value, then -0 (0x8000) before +0 (0x0000)
    t = sc.sortable(pats[order], BF16)
    assert (np.diff(t) > 0).all()
    assert (np.diff(v[order]) >= 0).all() and (np.diff(v[order]) == 0).sum() == 1
    assert np.array_equal(sc.unsortable(t, BF16), pats[order])                  # an involution
    assert t.min() == sc.t_of_minus_inf(BF16) == -0x8000 + 0x7f and sc.sortable(np.array([0x8000, 0x0000]), BF16).tolist() == [-1, 0]
    # the same for fp32 on the neighbourhoods the table uses
    p32 = np.array([0xff800000, 0xff7fffff, 0xbf800001, 0xbf800000, 0xbf7fffff, 0x80800000, 0x807fffff, 0x80000001, 0x80000000,
                    0x00000000, 0x00000001, 0x007fffff, 0x00800000, 0x3f7fffff, 0x3f800000, 0x3f800001, 0x7f7fffff, 0x7f800000], dtype=np.uint32)
    assert (np.diff(sc.sortable(p32, FP32)) > 0).all() and (np.diff(sc.to_f64(p32, FP32)) >= 0).all()


def test_impulse_fills_exactly_the_clipped_squares():
    seen = set()
    for c in sc.all_cases():
        ref = sc.case_reference(c)
        for f, row in enumerate(sc.case_maps(c)[1]):
            for ch, info in enumerate(row):
                if info.family != "impulse":
                    continue
                py, px = info.pos
                seen.add((py == 0, px == 0, py == c.H - 1, px == c.W - 1, min(py, px, c.H - 1 - py, c.W - 1 - px)))
                for k, r in enumerate(sc.RADII):
                    want = np.full((c.H, c.W), info.floor, dtype=ref[k].dtype)
                    want[max(py - r, 0):py + r + 1, max(px - r, 0):px + r + 1] = info.peak
                    assert np.array_equal(ref[k][f, :, :, ch], want), (c.name, f, ch, info)
    assert {d for *_, d in seen} >= set(range(8))                                # distances 0 .. 7 from a border all occur


def test_ramp_maximum_is_the_far_edge_of_the_window():
    checked = 0
    for c in sc.all_cases():
        bits, infos = sc.case_maps(c)
        ref = sc.case_reference(c)
        y, x = np.mgrid[0:c.H, 0:c.W]
        for f, row in enumerate(infos):
            for ch, info in enumerate(row):
                if info.pattern not in ("ramp+x", "ramp-x", "ramp+y", "ramp-y"):
                    continue
                m = bits[f, :, :, ch]
                for k, r in enumerate(sc.RADII):
                    far = {"ramp+x": m[y, np.minimum(x + r, c.W - 1)], "ramp-x": m[y, np.maximum(x - r, 0)],
                           "ramp+y": m[np.minimum(y + r, c.H - 1), x], "ramp-y": m[np.maximum(y - r, 0), x]}[info.pattern]
                    assert np.array_equal(ref[k][f, :, :, ch], far), (c.name, f, ch, info.pattern, k)
                checked += 1
    assert checked > 500


# ---------------------------------------------------------------------------------------------------
# the table bites: every mutant of the reference differs from it on the case family that was built against it
# ---------------------------------------------------------------------------------------------------
def _swap_halfwords(pools, c):
    return [p.reshape(*p.shape[:3], c.c // 2, 2)[..., ::-1].reshape(p.shape) for p in pools]


def _rotate_groups(pools, c):
    return [np.roll(p.reshape(*p.shape[:3], c.c // 8, 8), -1, axis=3).reshape(p.shape) for p in pools]


def _previous_frame(pools, c):
    return [np.concatenate([p[:1], p[:-1]]) for p in pools]


MUTANTS = {
    # name: (mutant(case, bits) -> pools, families that must catch it)
    "third_pool_radius_5": (lambda c, b: sc.ref_pools(b, c.dtype, radii=(2, 4, 5)), {"impulse", "ramp"}),
    "short_left": (lambda c, b: sc.ref_pools(b, c.dtype, short="left"), {"impulse", "ramp"}),
    "short_right": (lambda c, b: sc.ref_pools(b, c.dtype, short="right"), {"impulse", "ramp"}),
    "short_top": (lambda c, b: sc.ref_pools(b, c.dtype, short="top"), {"impulse", "ramp"}),
    "short_bottom": (lambda c, b: sc.ref_pools(b, c.dtype, short="bottom"), {"impulse", "ramp"}),
    "zero_padding": (lambda c, b: sc.ref_pools(b, c.dtype, pad_value=0.0), {"allneg", "impulse", "denormal"}),
    "raw_int_compare_without_flip": (lambda c, b: sc.t_pools(b, c.dtype, flip=False), {"allneg", "ramp", "ulp", "denormal"}),
    "halfwords_of_a_dword_swapped": (lambda c, b: _swap_halfwords(sc.case_reference(c), c), set(sc.FAMILIES)),
    "channel_groups_rotated": (lambda c, b: _rotate_groups(sc.case_reference(c), c), set(sc.FAMILIES)),
    "frame_read_one_early": (lambda c, b: _previous_frame(sc.case_reference(c), c), set(sc.FAMILIES)),
}
# every seventh shape of the pool16 table (all layouts and batch sizes occur), and the six-pass tables
BITE_CASES = sc.pool16_table()[::7] + sc.six_pass_table(BF16) + sc.six_pass_table(FP32)[:12]


@pytest.mark.parametrize("name", list(MUTANTS))
def test_table_catches_mutant(name):
    mutant, must_catch = MUTANTS[name]
    caught, n_cases = set(), 0
    for c in BITE_CASES:
        bits, infos = sc.case_maps(c)
        diff = np.zeros((c.n, c.c), dtype=bool)
        for a, b in zip(mutant(c, bits), sc.case_reference(c)):
            diff |= (a != b).any(axis=(1, 2))
        if name == "channel_groups_rotated" and c.c == 8 or name == "frame_read_one_early" and c.n == 1:
            assert not diff.any()                                               # one group / one frame: nothing to confuse
        n_cases += bool(diff.any())
        caught |= {infos[f][ch].family for f, ch in zip(*np.nonzero(diff))}
    print(f"{name}: differs on {n_cases} of {len(BITE_CASES)} cases, in families {sorted(caught)}")
    assert must_catch <= caught, (name, sorted(must_catch - caught))


def test_equivalent_mutants_are_equivalent():
    """Two mutants change nothing, on ANY map without NaN -- asserted here on the whole table, -inf-floor impulses included:
      * replicate padding: a window that reaches over a border already holds the border pixel it would be padded with, and max is idempotent.
        (sppf_pool16_kernel's clamped column reads and the fused kernel's "the centre again" reads rest on exactly this.)
      * the padding integer T(-inf) = 0x807f in place of 0x8000: every window holds its own centre, and no non-NaN value lies below -inf, so the
        padding never wins either way; where a window holds nothing but -inf the result is -inf both times.  Only a negative NaN could tell them
        apart, and NaN is outside the contract.  No test can see this one; the kernels' 0x8000 is the safe choice, not an observable one."""
    for c in sc.all_cases():
        bits = sc.case_maps(c)[0]
        ref = sc.case_reference(c)
        for a, b, r in zip(sc.ref_pools(bits, c.dtype, mode="edge"), sc.t_pools(bits, c.dtype, pad=sc.t_of_minus_inf(c.dtype)), ref):
            assert np.array_equal(a, r) and np.array_equal(b, r), c.name


# ---------------------------------------------------------------------------------------------------
# the fused kernel's inputs: closed_loop_ref's bound holds on the CPU with its usual margin
# ---------------------------------------------------------------------------------------------------
def _silu_bf16_bits(t):
    return sc.bf16_rne_bits((t * torch.sigmoid(t)).numpy())                      # oracle/yolov8_ref.py: y * sigmoid(y), then bf16


@pytest.mark.parametrize("cout", [256, 128])
def test_fused_inputs_keep_the_closed_loop_bound_on_the_cpu(cout):
    """torch's fp32 conv2d (what oracle/yolov8_ref.py computes), bf16-rounded, on the inputs of tests/test_gpu_sppf.py against float64:
    within closed_loop_ref's bound, and 16 x the measured accumulation floor <= C_ACC, as test_closed_loop_ref.py asserts for model shapes."""
    w1, b1, w2, b2 = sc.fused_weights(cout=cout)
    floors, worst, zero_seen = [], 0.0, set()
    for H, W in sc.FUSED_MAPS:
        for n in sc.FUSED_N:
            xb = sc.fused_x(H, W, n)
            x32 = torch.from_numpy(fr.nchw64(xb, H, W)).float()
            y32 = F.conv2d(x32, torch.from_numpy(w1.copy())[:, :, None, None], torch.from_numpy(b1.copy()))
            yb = _silu_bf16_bits(y32).transpose(0, 2, 3, 1)                     # [n, H, W, c]
            y, bb = fr.conv64(xb, w1, b1, H, W)
            r1, f1 = fr.bound_ratio(yb.reshape(n, H * W, -1), y, bb, H, W)
            zero_seen |= set(np.unique(yb[..., list(sc.FUSED_ZERO_CHANNELS)]).tolist())
            assert (sc.to_f64(yb, BF16) < 0).mean() > 0.3                       # whole channels of small negatives
            cat = np.concatenate([yb] + sc.ref_pools(yb, BF16), axis=3).reshape(n, H * W, -1)
            c32 = torch.from_numpy(fr.nchw64(cat, H, W)).float()
            o32 = F.conv2d(c32, torch.from_numpy(w2.copy())[:, :, None, None], torch.from_numpy(b2.copy()))
            ob = _silu_bf16_bits(o32).transpose(0, 2, 3, 1).reshape(n, H * W, -1)
            o, ob_b = fr.conv64(cat, w2, b2, H, W)
            r2, f2 = fr.bound_ratio(ob, o, ob_b, H, W)
            floors += [f1, f2]
            worst = max(worst, r1, r2)
    print(f"Cout {cout}: accumulation floor {max(floors):.3f} x 2^-24 B, worst |g - y| / bound {worst:.3f}")
    assert worst <= 1.0
    assert 16 * max(floors) <= cl.C_ACC
    assert zero_seen <= {0x0000, 0x8000} and zero_seen                           # the -100-bias channels are zeros of either sign
