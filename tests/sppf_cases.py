"""The SPPF pools' oracle and case table.  TEST INFRASTRUCTURE (numpy only; imported by tests/test_sppf_cases.py and tests/test_gpu_sppf.py).

The kernels under test (csrc/kernels_misc.hip: sppf_pool16_kernel, sppf_pool_kernel<bf16_t>, sppf_pool_kernel<float>; csrc/kernels_sppf.hip:
sppf_fused_kernel) compute three chained 5x5 stride-1 max pools of a map y.  The reference here does NOT chain: pool k is written as the direct
window of radius 2k (2, 4, 6) over y, clipped to the map (outside lies -inf, which no window's own centre is below), on the exact values --
bf16 and fp32 are exact in float64 -- and its result is a bit pattern of the input dtype.

Zero rule: a window whose maximum is numerically zero gives +0 if it holds a +0, else -0.  That is the order of the integer domain both fast
kernels pool in (T(x) = x ^ ((x >> 15) & 0x7fff) per half-word: T(-0) = -1 < T(+0) = 0).  NaN is outside the contract: the integer order puts
positive NaNs above +inf and negative NaNs below -inf while fp32 max drops them; the table holds none, and no test feeds one.

Every map of a case -- one per (frame, channel) -- is generated from its own seed and its own pattern, so that no two channels of an 8-channel
group (one 16-byte access) and no two frames share a map: a swapped channel pair, a rotated channel group or a wrong frame stride changes bits.
"""
import functools
from dataclasses import dataclass

import numpy as np

FP32, BF16 = 0, 1                                  # zly.DTYPE_FP32 / zly.DTYPE_BF16
SENTINEL = {BF16: 0xA5C3, FP32: 0xA5C3F00D}        # guard fill: a finite negative value that no generated map holds on purpose
RADII = (2, 4, 6)
HIP_ERROR_INVALID_VALUE = 1


# ---------------------------------------------------------------------------------------------------
# bit patterns <-> exact values
# ---------------------------------------------------------------------------------------------------
def bits_dtype(dtype):
    return np.uint16 if dtype == BF16 else np.uint32


def width(dtype):
    return 16 if dtype == BF16 else 32


def to_f64(bits, dtype):
    b = np.asarray(bits, dtype=np.uint32)
    if dtype == BF16:
        b = b << 16
    return np.ascontiguousarray(b).view(np.float32).astype(np.float64)


def from_f64(v, dtype):
    """exact for values that came from to_f64 of the same dtype (zero sign as numpy carries it)"""
    u = np.ascontiguousarray(np.asarray(v, dtype=np.float64).astype(np.float32)).view(np.uint32)
    return (u >> 16).astype(np.uint16) if dtype == BF16 else u


def is_nan(bits, dtype):
    b = np.asarray(bits, dtype=np.uint32) << (16 if dtype == BF16 else 0)
    return (b & 0x7fffffff) > 0x7f800000


def is_denormal(bits, dtype):
    b = np.asarray(bits, dtype=np.uint32) << (16 if dtype == BF16 else 0)
    return ((b & 0x7f800000) == 0) & ((b & 0x007fffff) != 0)


def widen(bits16):
    return np.asarray(bits16, dtype=np.uint32) << 16


# ---------------------------------------------------------------------------------------------------
# the reference: direct windows
# ---------------------------------------------------------------------------------------------------
def _window(a, r, pad, reduce, mode="constant", short=None):
    """a [n, H, W, c] -> reduce over the (2r + 1)^2 window of every pixel; outside the map lies `pad` (mode "edge": the border pixel).
    short: "left" / "right" / "top" / "bottom" drops the window's outermost column / row on that side (a mutant)."""
    n, H, W, c = a.shape
    ap = np.pad(a, ((0, 0), (r, r), (r, r), (0, 0)), mode="edge") if mode == "edge" else \
        np.pad(a, ((0, 0), (r, r), (r, r), (0, 0)), mode="constant", constant_values=pad)
    out = None
    for dy in range(-r + (short == "top"), r + 1 - (short == "bottom")):
        for dx in range(-r + (short == "left"), r + 1 - (short == "right")):
            s = ap[:, r + dy:r + dy + H, r + dx:r + dx + W, :]
            out = s.copy() if out is None else reduce(out, s, out=out)
    return out


def ref_pools(bits, dtype, radii=RADII, pad_value=-np.inf, mode="constant", short=None):
    """bits [n, H, W, c] -> [3][n, H, W, c] bit patterns of the windows of radius 2, 4, 6.  The keyword arguments make the mutants of
    tests/test_sppf_cases.py; the defaults are the reference."""
    bits = np.asarray(bits, dtype=bits_dtype(dtype))
    assert bits.ndim == 4 and not is_nan(bits, dtype).any()
    v = to_f64(bits, dtype)
    plus_zero = bits == 0
    sign = bits_dtype(dtype)(1 << (width(dtype) - 1))
    out = []
    for r in radii:
        m = _window(v, r, pad_value, np.maximum, mode, short)
        has_pz = _window(plus_zero, r, bool(pad_value == 0.0), np.logical_or, mode, short)
        res = from_f64(m, dtype)
        zero = m == 0.0
        res[zero] = np.where(has_pz[zero], 0, sign).astype(res.dtype)
        out.append(res)
    return out


def ref_pools_chained(bits, dtype):
    """the form the kernels use: three radius-2 pools, each of the one before"""
    out, cur = [], bits
    for _ in range(3):
        cur = ref_pools(cur, dtype, radii=(2,))[0]
        out.append(cur)
    return out


# ---------------------------------------------------------------------------------------------------
# a model of what the fast kernels do: T, integer max, T again
# ---------------------------------------------------------------------------------------------------
def sortable(bits, dtype, flip=True):
    """T(x) = x ^ ((x >> (w - 1)) & (2^(w-1) - 1)) as a SIGNED integer (int64 holds both widths); flip=False: the raw pattern as a signed integer"""
    w = width(dtype)
    u = np.asarray(bits).astype(np.int64)
    if flip:
        u = u ^ ((u >> (w - 1)) * ((1 << (w - 1)) - 1))
    return u - ((u >> (w - 1)) << w)


def unsortable(t, dtype, flip=True):
    w = width(dtype)
    u = np.asarray(t, dtype=np.int64) & ((1 << w) - 1)
    if flip:
        u = u ^ ((u >> (w - 1)) * ((1 << (w - 1)) - 1))
    return u.astype(bits_dtype(dtype))


def t_pools(bits, dtype, flip=True, pad=None):
    """pad: the integer that lies outside the map (default: the smallest one, 0x8000 per half-word -- below T(-inf) = 0x807f)"""
    w = width(dtype)
    t = sortable(bits, dtype, flip)
    pad = -(1 << (w - 1)) if pad is None else pad
    return [unsortable(_window(t, r, pad, np.maximum), dtype, flip) for r in RADII]


def t_of_minus_inf(dtype):
    return int(sortable(np.array([0xff80 if dtype == BF16 else 0xff800000]), dtype)[0])


# ---------------------------------------------------------------------------------------------------
# value patterns: name -> (family, generator(dtype, H, W, rng) -> bits [H, W])
# ---------------------------------------------------------------------------------------------------
ALL_BF16 = np.arange(65536, dtype=np.uint32)
NON_NAN_BF16 = ALL_BF16[~is_nan(ALL_BF16, BF16)].astype(np.uint16)              # 65282 patterns: 65536 - 2 x 127 NaNs
FINITE_BF16 = NON_NAN_BF16[(NON_NAN_BF16 & 0x7f80) != 0x7f80]
NEG_BF16 = NON_NAN_BF16[NON_NAN_BF16 >= 0x8000]                                # -0 .. -inf, the negative denormals among them


def _pick(dtype, pool16, H, W, rng):
    b = rng.choice(np.asarray(pool16, dtype=np.uint16), size=(H, W))
    return b if dtype == BF16 else widen(b)


def _uniform(dtype, H, W, rng):
    if dtype == BF16:
        return rng.choice(NON_NAN_BF16, size=(H, W))
    b = rng.integers(0, 1 << 32, size=(H, W), dtype=np.uint64).astype(np.uint32)
    bad = is_nan(b, FP32)
    b[bad] &= np.uint32(0xff800000)                                              # the few NaNs become the infinity of their sign
    return b


def _allneg(dtype, H, W, rng):
    b = rng.choice(NEG_BF16, size=(H, W)).astype(np.uint32)
    k = rng.integers(0, 4, size=(H, W))
    b = np.where(k == 0, rng.choice(np.array([0xff80, 0x8000, 0x8001, 0x807f, 0xff7f], dtype=np.uint32), size=(H, W)), b)
    if dtype == FP32:
        b = (b << 16) | np.where((b & 0x7f80) == 0x7f80, 0, rng.integers(0, 1 << 16, size=(H, W))).astype(np.uint32)
    return b.astype(bits_dtype(dtype))


def _ramp(kind, negate):
    def gen(dtype, H, W, rng):
        y, x = np.mgrid[0:H, 0:W]
        idx = {"x": x, "y": y, "xy": x + y}[kind]
        steps = int(idx.max()) + 1
        if dtype == BF16:
            vals = to_f64(rng.choice(FINITE_BF16[FINITE_BF16 != 0x8000], size=steps, replace=False), BF16)      # distinct values: one zero at most
        else:
            b = rng.integers(0, 1 << 32, size=2 * steps + 64, dtype=np.uint64).astype(np.uint32)
            b = b[((b & 0x7f800000) != 0x7f800000) & (b != 0x80000000)]
            vals = rng.choice(np.unique(to_f64(b, FP32)), size=steps, replace=False)
        v = np.sort(vals)[idx]
        return from_f64(-v if negate else v, dtype)
    return gen


def _zero_checker(dtype, H, W, rng):
    y, x = np.mgrid[0:H, 0:W]
    b = np.where((x + y + int(rng.integers(0, 2))) & 1, 0x8000, 0x0000).astype(np.uint32)
    return (b if dtype == BF16 else b << 16).astype(bits_dtype(dtype))


def _zero_checker_on_floor(dtype, H, W, rng):
    y, x = np.mgrid[0:H, 0:W]
    floor = rng.choice(NEG_BF16[(NEG_BF16 > 0x8000) & (NEG_BF16 < 0xff80)], size=(H, W)).astype(np.uint32)
    sx, sy = int(rng.integers(0, 3)), int(rng.integers(0, 3))
    knot = ((x + sx) % 3 == 0) & ((y + sy) % 3 == 0)
    b = np.where(knot, np.where(((x + sx) // 3 + (y + sy) // 3) & 1, 0x8000, 0x0000), floor).astype(np.uint32)
    return (b if dtype == BF16 else b << 16).astype(bits_dtype(dtype))


def _ulp32(dtype, H, W, rng):
    """fp32 only: neighbours one fp32 ulp apart -- around random finite values, across 0, across a binade, at the largest finite values"""
    assert dtype == FP32
    special = np.array([0x3f7fffff, 0x3f800000, 0x3f800001, 0xbf7fffff, 0xbf800000, 0xbf800001, 0x7f7ffffe, 0x7f7fffff, 0x7f800000,
                        0xff7ffffe, 0xff7fffff, 0xff800000, 0x00000001, 0x80000001, 0x00000000, 0x80000000, 0x007fffff, 0x00800000], dtype=np.uint32)
    base = np.uint32((int(rng.choice(FINITE_BF16[(FINITE_BF16 & 0x7fff) > 0x0100])) << 16) | 0x8000)
    near = (base + rng.integers(0, 3, size=(H, W)).astype(np.uint32)).astype(np.uint32)
    return np.where(rng.integers(0, 2, size=(H, W)) == 0, near, rng.choice(special, size=(H, W))).astype(np.uint32)


PATTERNS = {
    "uniform": ("uniform", _uniform),
    "allneg": ("allneg", _allneg),
    "ramp+x": ("ramp", _ramp("x", False)), "ramp+y": ("ramp", _ramp("y", False)), "ramp+xy": ("ramp", _ramp("xy", False)),
    "ramp-x": ("ramp", _ramp("x", True)), "ramp-y": ("ramp", _ramp("y", True)), "ramp-xy": ("ramp", _ramp("xy", True)),
    "zeros": ("zeros", _zero_checker),
    "zeros_on_floor": ("zeros", _zero_checker_on_floor),
    "ulp_across_0": ("ulp", lambda d, H, W, r: _pick(d, [0x8001, 0x8000, 0x0000, 0x0001], H, W, r)),
    "ulp_across_binade": ("ulp", lambda d, H, W, r: _pick(d, [0x3f7f, 0x3f80, 0x3f81] if r.integers(0, 2) else [0xbf7f, 0xbf80, 0xbf81], H, W, r)),
    "ulp_at_+inf": ("ulp", lambda d, H, W, r: _pick(d, [0x7f7e, 0x7f7f, 0x7f80], H, W, r)),
    "ulp_at_-inf": ("ulp", lambda d, H, W, r: _pick(d, [0xff7e, 0xff7f, 0xff80], H, W, r)),
    "denormal+": ("denormal", lambda d, H, W, r: _pick(d, np.arange(0x0000, 0x0080), H, W, r)),
    "denormal-": ("denormal", lambda d, H, W, r: _pick(d, np.arange(0x8000, 0x8080), H, W, r)),
    "ulp32": ("ulp", _ulp32),
}
OTHERS = {BF16: [k for k in PATTERNS if k != "ulp32"], FP32: list(PATTERNS)}
FAMILIES = ("uniform", "allneg", "impulse", "ramp", "zeros", "ulp", "denormal")
IMPULSE_FLOORS = (0xff80, 0xff7f)                      # -inf, the most negative finite value (bf16 patterns; widened for fp32)


def impulse_positions(H, W):
    """corners, edge midpoints, centre, and distance 2..7 from each border (at the other axis' middle); duplicates dropped, order kept"""
    my, mx = H // 2, W // 2
    pos = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, mx), (H - 1, mx), (my, 0), (my, W - 1), (my, mx)]
    for d in range(2, 8):
        pos += [(d, mx), (H - 1 - d, mx), (my, d), (my, W - 1 - d)]
    seen, out = set(), []
    for y, x in pos:
        if 0 <= y < H and 0 <= x < W and (y, x) not in seen:
            seen.add((y, x))
            out.append((y, x))
    return out


def impulse_map(dtype, H, W, pos, floor16, rng):
    peak = int(rng.choice(FINITE_BF16[FINITE_BF16 != 0xff7f]))                  # any finite value above the floor, negatives and zeros included
    b = np.full((H, W), floor16, dtype=np.uint32)
    b[pos] = peak
    return (b if dtype == BF16 else b << 16).astype(bits_dtype(dtype)), peak if dtype == BF16 else peak << 16


# ---------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    dtype: int
    H: int
    W: int
    c: int
    cs: int
    n: int
    six_pass: int = 0
    seed: int = 0
    refused: bool = False        # inside the probe's contract, beyond the launcher's range: hipErrorInvalidValue, buffer untouched

    @property
    def name(self):
        return f"{'bf16' if self.dtype == BF16 else 'fp32'}-{self.H}x{self.W}-c{self.c}of{self.cs}-n{self.n}" + ("-sixpass" if self.six_pass else "")

    @property
    def pool16(self):
        """what sppf_pool16_ok must say (csrc/kernels_misc.hip)"""
        return self.dtype == BF16 and self.H <= 16 and self.W <= 16 and not self.six_pass and self.n <= 16


@dataclass(frozen=True)
class MapInfo:
    pattern: str
    family: str
    pos: tuple = None            # impulses: (y, x), floor pattern, peak pattern
    floor: int = 0
    peak: int = 0


@functools.lru_cache(maxsize=None)
def case_maps(case):
    """-> (bits [n, H, W, c], infos [n][c]).  Even maps are impulses, odd maps walk the other patterns; both walks start at an offset taken
    from the case, so that over the table every pattern and every impulse position meets every kind of shape."""
    H, W = case.H, case.W
    bits = np.empty((case.n, H, W, case.c), dtype=bits_dtype(case.dtype))
    positions, others = impulse_positions(H, W), OTHERS[case.dtype]
    infos, off = [], case.seed + 7 * H + 3 * W
    for f in range(case.n):
        row = []
        for ch in range(case.c):
            m = f * case.c + ch
            rng = np.random.default_rng([case.seed, case.dtype, H, W, f, ch])
            if m % 2 == 0:
                i = m // 2 + off
                pos, floor = positions[i % len(positions)], IMPULSE_FLOORS[(i // len(positions)) % 2]
                bits[f, :, :, ch], peak = impulse_map(case.dtype, H, W, pos, floor, rng)
                row.append(MapInfo("impulse", "impulse", pos, floor if case.dtype == BF16 else floor << 16, peak))
            else:
                name = others[(m // 2 + off + f) % len(others)]
                fam, gen = PATTERNS[name]
                bits[f, :, :, ch] = gen(case.dtype, H, W, rng)
                row.append(MapInfo(name, fam))
        infos.append(row)
    assert not is_nan(bits, case.dtype).any()
    bits.setflags(write=False)
    return bits, infos


@functools.lru_cache(maxsize=None)
def case_reference(case):
    """computed once per case, shared, read-only"""
    out = ref_pools(case_maps(case)[0], case.dtype)
    for o in out:
        o.setflags(write=False)
    return tuple(out)


GUARD_FRAMES = 1


def case_buffer(case, pools=None):
    """the concat buffer [guard + n + guard][H*W][cs] as bit patterns: sentinel everywhere, the maps in channel block 0 of the n middle frames;
    with pools (3 x [n, H, W, c]) also blocks 1..3 -- the buffer a correct launch leaves behind"""
    g, hw = GUARD_FRAMES, case.H * case.W
    buf = np.full((case.n + 2 * g, hw, case.cs), SENTINEL[case.dtype], dtype=bits_dtype(case.dtype))
    buf[g:g + case.n, :, :case.c] = case_maps(case)[0].reshape(case.n, hw, case.c)
    if pools is not None:
        for k, p in enumerate(pools):
            buf[g:g + case.n, :, (k + 1) * case.c:(k + 2) * case.c] = np.asarray(p).reshape(case.n, hw, case.c)
    return buf


LAYOUTS = ((8, 32), (8, 40), (24, 96), (24, 104), (128, 512))
SIX_PASS_SMALL = ((1, 1), (1, 16), (16, 1), (2, 3), (3, 2), (5, 5), (7, 13), (13, 13), (16, 16), (3, 16), (16, 3), (11, 9))
SIX_PASS_LARGE = ((17, 16), (16, 17), (20, 20), (1, 40), (40, 1), (1, 300), (300, 1), (40, 40), (41, 41))      # 40 x 40: LDS above 64 KB; 41 x 41: the largest map
REFUSED_SHAPE = (42, 41)                                                          # 3 x 42 x 41 x 32 bytes of LDS: above the 160 KB the launcher accepts


@functools.lru_cache(maxsize=None)
def pool16_table():
    """sppf_pool16_kernel: every H x W with 1 <= H, W <= 16, layouts and batch sizes dealt round; n = 16, the launcher's last batch on this kernel,
    and the 128-channel layout of the model at a handful of shapes"""
    rot = ((8, 32, 2), (8, 40, 1), (24, 96, 2), (24, 104, 2), (8, 40, 2), (24, 96, 1))
    special = {(13, 13): (128, 512, 2), (16, 16): (128, 512, 1), (1, 1): (128, 512, 2), (3, 2): (128, 512, 1), (16, 1): (128, 512, 1),
               (11, 9): (24, 96, 16), (7, 13): (24, 104, 16), (16, 15): (8, 32, 16), (2, 16): (8, 40, 16), (1, 16): (24, 96, 16)}
    out = []
    for H in range(1, 17):
        for W in range(1, 17):
            c, cs, n = special.get((H, W), rot[(H * 5 + W) % len(rot)])
            out.append(Case(BF16, H, W, c, cs, n, seed=1))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def six_pass_table(dtype):
    """sppf_pool_kernel<bf16_t> / <float>: small maps through six_pass = 1, the maps beyond 16 x 16, and batch 17 (where the launcher leaves
    sppf_pool16_kernel) on small maps without the switch"""
    out = []
    for i, (H, W) in enumerate(SIX_PASS_SMALL):
        c, cs = LAYOUTS[i % 4]
        out.append(Case(dtype, H, W, c, cs, (1, 2)[i % 2], six_pass=1, seed=2))
    out.append(Case(dtype, 13, 13, 128, 512, 2, six_pass=1, seed=2))
    for i, (H, W) in enumerate(SIX_PASS_LARGE):
        c, cs = ((8, 32), (8, 40))[i % 2] if H * W > 400 else LAYOUTS[i % 4]
        out.append(Case(dtype, H, W, c, cs, (2, 1)[i % 2], seed=3))
    for (H, W), (c, cs) in (((13, 13), (8, 32)), ((16, 16), (24, 104)), ((3, 2), (24, 96)), ((9, 11), (8, 40))):
        out.append(Case(dtype, H, W, c, cs, 17, seed=4))
    return tuple(out)


def refused_cases():
    return tuple(Case(d, *REFUSED_SHAPE, 8, 32, 1, seed=5, refused=True) for d in (BF16, FP32))


def all_cases():
    return pool16_table() + six_pass_table(BF16) + six_pass_table(FP32)


# ---------------------------------------------------------------------------------------------------
# the fused kernel's inputs (tests/test_gpu_sppf.py; their CPU floor: tests/test_sppf_cases.py)
# ---------------------------------------------------------------------------------------------------
FUSED_MAPS = ((3, 3), (3, 58), (58, 3), (13, 13), (9, 11), (13, 7), (11, 16), (16, 11), (4, 44), (5, 35), (12, 14), (7, 25), (8, 22))
FUSED_COUT_SPLIT = ((256, 2), (256, 4), (128, 2))
FUSED_N = (1, 3)
FUSED_X_LAYOUTS = ((256, 0), (320, 32))                # (x_cs, x_co)
FUSED_OUT_LAYOUTS = ((0, 0), (64, 8))                  # (out_cs - Cout, out_co)
FUSED_CAT_CS = (512, 520)
FUSED_CIN, FUSED_C = 256, 128
FUSED_ZERO_CHANNELS = (5, 42, 77, 120)                 # cv1 bias -100: SiLU takes the whole channel to zero
SENTINEL16 = SENTINEL[BF16]


def bf16_rne_bits(x):
    u = np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_round(x):
    return to_f64(bf16_rne_bits(x), BF16).astype(np.float32)


@functools.lru_cache(maxsize=None)
def fused_weights(cin=FUSED_CIN, c=FUSED_C, cout=256):
    """(w1 [c][cin], b1 [c], w2 [cout][4c], b2 [cout]) fp32; the weights are bf16 values already, so the probe's packing rounds nothing"""
    rng = np.random.default_rng([9, cin, c, cout])
    w1 = bf16_round(rng.standard_normal((c, cin)) / np.sqrt(cin))
    b1 = np.linspace(-8.0, 4.0, c).astype(np.float32)             # whole channels of small negatives with many near-ties
    for ch in FUSED_ZERO_CHANNELS:
        if ch < c:
            b1[ch] = -100.0
    w2 = bf16_round(rng.standard_normal((cout, 4 * c)) / np.sqrt(4 * c))
    b2 = (0.1 * rng.standard_normal(cout)).astype(np.float32)
    for a in (w1, b1, w2, b2):
        a.setflags(write=False)
    return w1, b1, w2, b2


@functools.lru_cache(maxsize=None)
def fused_x(H, W, n, cin=FUSED_CIN):
    """x [n, H*W, cin] as bf16 bit patterns: normal(0, 1)"""
    rng = np.random.default_rng([10, H, W, n, cin])
    x = bf16_rne_bits(rng.standard_normal((n, H * W, cin)))
    x.setflags(write=False)
    return x
