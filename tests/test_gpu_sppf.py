"""The SPPF kernels as shipped, on crafted maps, against the exact reference of tests/sppf_cases.py (run on the MI355X box: pytest -m gpu).
The launches go through tests/cpp/sppf_probe.hip, which links the kernels_misc.o, kernels_sppf.o and weights.o of libzly.so itself.

Pools (launch_sppf_pool): sppf_pool16_kernel on every H x W up to 16 x 16, sppf_pool_kernel<bf16_t> and <float> on small maps (six_pass), on the
maps beyond 16 x 16 up to the largest the launcher takes (41 x 41; 40 x 40 needs LDS above 64 KB) and at batch 17, where the launcher leaves
sppf_pool16_kernel.  Every map is one of the table's patterns (all non-NaN bit patterns, all-negative maps with -inf / -0 / denormals, impulses
over -inf, ramps, +-0 checkerboards, neighbours one ulp apart, denormals).  Blocks 1..3 of the concat buffer must equal the reference bit for
bit; block 0, the guard channels beyond 4c and the guard frames on either side must come back byte for byte.  No tolerance anywhere.

Where a six-pass result is numerically zero or a denormal, fp32 max might have left other bits than the integer order of sppf_pool16_kernel
(the zero rule of sppf_cases.py); there the six-pass kernels are held to numerical equality by the case tests, and what the hardware did is
counted.  Measured on an MI355X: of 153220 such results of sppf_pool_kernel<bf16_t> and 149840 of sppf_pool_kernel<float>, none has other bits
than the reference -- v_max_f32 orders -0 below +0 and keeps denormals -- so the "same bits" comment in kernels_misc.hip stands as written,
and test_six_pass_zero_and_denormal_bits_as_measured asserts the zero count so that a change of that behaviour is noticed.

Fused block (launch_sppf_fused): cv1, the pools and cv2 in one launch, with the debug dump and without.  The dumped y against a float64 cv1
and `out` against a float64 cv2 over the dumped concat within closed_loop_ref's bf16 bound (imported; its CPU floor on these very inputs is
asserted in tests/test_sppf_cases.py), the dumped pools against the reference pools of the dumped y bit for bit, dump = 0 bit-identical to
dump = 1 with an untouched concat buffer, and not a byte outside the output view.  Maps from 3 x 3 to 3 x 58 / 58 x 3 (176 pixels is the limit).

Any HIP error ends the session (pytest.exit): it may be a GPU fault, and nothing more is started on that device.

Measured on an MI355X: the module's 121 tests take 5.3 to 6.6 s; slowest: test_pool16_kernel_bit_exact[1] 0.3 s (the first launch: it loads the
probe), the batch-17 six-pass case on 16 x 16 x 24 channels 0.10 s, a test_fused_kernel case (32 launches: 16 layouts with and without the dump)
0.07 to 0.11 s.  Worst |g - y| / bound of the fused kernel: 0.994 for cv1, 0.995 for cv2 (the half-ulp term; the CPU gives 0.995 on the same inputs).
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import sppf_cases as sc
import sppf_fused_ref as fr
from sppf_cases import BF16, FP32, SENTINEL16

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE_TARGET = "zero-latency-yolo_amd/_build/libsppf_probe.so"
ZERO_DENORMAL_STATS = {}            # kernel -> [elements held to numerical equality only, of those with other bits than the reference]


@pytest.fixture(scope="module")
def probe():
    """ctypes handle on the probe; built on demand (after `make` it is there: the target is part of `all`)"""
    path = os.path.join(ROOT, PROBE_TARGET)
    if not os.path.exists(path):
        subprocess.run(["make", "-C", ROOT, PROBE_TARGET], check=True, stdout=subprocess.DEVNULL)
    lib = C.CDLL(path)
    vp, i, sz = C.c_void_p, C.c_int, C.c_size_t
    lib.sppf_probe_pool.argtypes = [i, vp, sz, i, i, i, i, i, i, i, vp, vp]
    lib.sppf_probe_pool.restype = i
    lib.sppf_probe_fused.argtypes = [vp, sz, i, i, i, vp, vp, i, vp, vp, i, i, i, i, i, i, vp, sz, i, i, vp, sz, i, vp]
    lib.sppf_probe_fused.restype = i
    return lib


# ---------------------------------------------------------------------------------------------------
# pools
# ---------------------------------------------------------------------------------------------------
def _launch_pool(probe, case, buf=None):
    """-> (hip error code, buffer after, 1 if sppf_pool16_ok chose sppf_pool16_kernel)"""
    buf = np.ascontiguousarray(sc.case_buffer(case) if buf is None else buf)
    out = np.zeros_like(buf)
    kernel = C.c_int(-1)
    rc = probe.sppf_probe_pool(case.dtype, buf.ctypes.data, buf.nbytes, case.cs, case.c, case.n, case.H, case.W, case.six_pass, sc.GUARD_FRAMES,
                               out.ctypes.data, C.byref(kernel))
    return rc, out, kernel.value


def _where(case, got, want):
    d = np.argwhere(got != want)
    f, px, ch = (int(v) for v in d[0])
    y, x = divmod(px, case.W)
    g = sc.GUARD_FRAMES
    if not g <= f < g + case.n:
        place = f"guard frame {f}"
    elif ch >= 4 * case.c:
        place = f"frame {f - g}, guard channel {ch}"
    else:
        info = sc.case_maps(case)[1][f - g][ch % case.c]
        place = f"frame {f - g}, block {ch // case.c}, channel {ch % case.c} ({info.pattern}{' at ' + str(info.pos) if info.pos else ''})"
    return f"{case.name}: {len(d)} elements differ, first at {place}, pixel ({y}, {x}): got {int(got[f, px, ch]):#x} want {int(want[f, px, ch]):#x}"


def _check_pool(probe, case):
    rc, got, kernel = _launch_pool(probe, case)
    if rc != 0:
        pytest.exit(f"sppf_probe_pool: HIP error {rc} on {case.name}", returncode=3)
    assert kernel == int(case.pool16), f"{case.name}: sppf_pool16_ok said {kernel}"
    want = sc.case_buffer(case, sc.case_reference(case))
    if not case.pool16:
        # six-pass kernels: numerical equality where the result is a zero or a denormal, bits everywhere else
        g = sc.GUARD_FRAMES
        loose = np.zeros(want.shape, dtype=bool)
        blk = want[g:g + case.n, :, case.c:4 * case.c]
        loose[g:g + case.n, :, case.c:4 * case.c] = (sc.to_f64(blk, case.dtype) == 0) | sc.is_denormal(blk, case.dtype)
        assert np.array_equal(sc.to_f64(got[loose], case.dtype), sc.to_f64(want[loose], case.dtype)), \
            f"{case.name}: a zero or denormal result differs NUMERICALLY: " + _where(case, np.where(loose, got, want), want)
        st = ZERO_DENORMAL_STATS.setdefault("bf16" if case.dtype == BF16 else "fp32", [0, 0])
        st[0] += int(loose.sum())
        st[1] += int((got[loose] != want[loose]).sum())
        got = np.where(loose, want, got)
    assert np.array_equal(got, want), _where(case, got, want)


@pytest.mark.parametrize("H", range(1, 17))
def test_pool16_kernel_bit_exact(probe, H):
    """sppf_pool16_kernel on H x 1 .. H x 16: blocks 1..3 = the reference's bits; block 0, guard channels and guard frames untouched"""
    for case in sc.pool16_table():
        if case.H == H:
            _check_pool(probe, case)


@pytest.mark.parametrize("case", sc.six_pass_table(BF16) + sc.six_pass_table(FP32), ids=lambda c: c.name)
def test_six_pass_kernels_bit_exact(probe, case):
    """sppf_pool_kernel<bf16_t> / <float>, batch 17 (the launcher's switch between the two bf16 kernels) included"""
    _check_pool(probe, case)


def test_six_pass_zero_and_denormal_bits_as_measured(probe):
    """What fp32 max left where the result is a zero or a denormal (counted by the tests above; run alone, this test launches the cases it needs).
    On the MI355X the six-pass kernels give the reference's bits there too -- v_max_f32 orders -0 below +0 and keeps denormals -- so the
    "same bits" comment in kernels_misc.hip stands, and it is asserted here so that a change of that behaviour is noticed."""
    if not ZERO_DENORMAL_STATS:
        for case in sc.six_pass_table(BF16)[:6] + sc.six_pass_table(FP32)[:6]:
            _check_pool(probe, case)
    print("six-pass kernels, results that are zeros or denormals: " +
          ", ".join(f"{k}: {v[0]} elements, {v[1]} with other bits than the integer order gives" for k, v in sorted(ZERO_DENORMAL_STATS.items())))
    for k, v in ZERO_DENORMAL_STATS.items():
        assert v[0] > 1000, (k, v)
        assert v[1] == 0, f"{k}: {v[1]} of {v[0]} zero / denormal results have other bits than sppf_pool16_kernel would give"


def test_six_pass_equals_pool16_on_the_same_buffers(probe):
    """the two bf16 kernels on identical buffers, zeros and denormals included: compared with each other directly (bits)"""
    for case in sc.pool16_table()[5::37]:
        rc_a, a, ka = _launch_pool(probe, case)
        six = sc.Case(**{**case.__dict__, "six_pass": 1})
        rc_b, b, kb = _launch_pool(probe, six, sc.case_buffer(case))
        if rc_a != 0 or rc_b != 0:
            pytest.exit(f"sppf_probe_pool: HIP error {rc_a} / {rc_b} on {case.name}", returncode=3)
        assert (ka, kb) == (1, 0)
        assert np.array_equal(a, b), _where(case, b, a)


@pytest.mark.parametrize("case", sc.refused_cases(), ids=lambda c: c.name)
def test_map_beyond_the_lds_is_refused(probe, case):
    buf = sc.case_buffer(case)
    rc, got, kernel = _launch_pool(probe, case, buf)
    assert rc == sc.HIP_ERROR_INVALID_VALUE and kernel == 0
    assert got.tobytes() == buf.tobytes(), "a refused launch wrote to the buffer"


def test_pool_probe_rejects_what_the_kernels_must_not_see(probe):
    case = sc.Case(BF16, 5, 5, 8, 32, 1)
    buf = sc.case_buffer(case)
    out, k = np.zeros_like(buf), C.c_int(0)

    def run(**kw):
        a = dict(dtype=BF16, nbytes=buf.nbytes, cs=32, c=8, n=1, H=5, W=5, guard=1)
        a.update(kw)
        return probe.sppf_probe_pool(a["dtype"], buf.ctypes.data, a["nbytes"], a["cs"], a["c"], a["n"], a["H"], a["W"], 0, a["guard"], out.ctypes.data, C.byref(k))
    assert run(c=4) == -1 and run(c=12, cs=48) == -1           # c % 8
    assert run(cs=36) == -1                                     # cs % 8
    assert run(c=16) == -1                                      # cs < 4c
    assert run(n=0) == -1 and run(H=0) == -1 and run(W=-1) == -1
    assert run(n=2) == -1 and run(nbytes=buf.nbytes - 2) == -1 and run(dtype=FP32) == -1       # buffer size
    assert run(dtype=7) == -1
    assert probe.sppf_probe_pool(BF16, None, buf.nbytes, 32, 8, 1, 5, 5, 0, 1, out.ctypes.data, C.byref(k)) == -1
    assert not out.any()


# ---------------------------------------------------------------------------------------------------
# the fused block
# ---------------------------------------------------------------------------------------------------
def _launch_fused(probe, H, W, n, cout, split, x_cs, x_co, out_cs, out_co, cat_cs, dump, cin=sc.FUSED_CIN, c=sc.FUSED_C):
    """-> (hip error code, sppf_fused_ok's verdict, out [n, HW, out_cs], cat [n, HW, cat_cs], the out buffer as it went in)"""
    w1, b1, w2, b2 = sc.fused_weights(cin, c, cout)
    hw = H * W
    x = np.full((n, hw, x_cs), SENTINEL16, dtype=np.uint16)
    x[:, :, x_co:x_co + cin] = sc.fused_x(H, W, n, cin)
    out = np.full((n, hw, out_cs), SENTINEL16, dtype=np.uint16)
    cat = np.full((n, hw, cat_cs), SENTINEL16, dtype=np.uint16)
    ok = C.c_int(-1)
    rc = probe.sppf_probe_fused(x.ctypes.data, x.size, x_cs, x_co, cin, w1.ctypes.data, b1.ctypes.data, c, w2.ctypes.data, b2.ctypes.data, cout,
                                n, H, W, split, dump, out.ctypes.data, out.size, out_cs, out_co, cat.ctypes.data, cat.size, cat_cs, C.byref(ok))
    return rc, ok.value, out, cat


def _only_view_written(out, out_co, cout):
    return (out[:, :, :out_co] == SENTINEL16).all() and (out[:, :, out_co + cout:] == SENTINEL16).all()


@pytest.mark.parametrize("cout,split", sc.FUSED_COUT_SPLIT)
@pytest.mark.parametrize("H,W", sc.FUSED_MAPS)
def test_fused_kernel(probe, H, W, cout, split):
    """sppf_fused_kernel<8, 2> (Cout 256 split 4, Cout 128 split 2) and <8, 4> (Cout 256 split 2), every layout of the table"""
    w1, b1, w2, b2 = sc.fused_weights(cout=cout)
    worst, c = [0.0, 0.0], sc.FUSED_C
    for n in sc.FUSED_N:
        y64, yb64 = fr.conv64(sc.fused_x(H, W, n), w1, b1, H, W)
        cat_ref, pool_ref = {}, {}
        for x_cs, x_co in sc.FUSED_X_LAYOUTS:
            for out_extra, out_co in sc.FUSED_OUT_LAYOUTS:
                for cat_cs in sc.FUSED_CAT_CS:
                    lay = dict(x_cs=x_cs, x_co=x_co, out_cs=cout + out_extra, out_co=out_co, cat_cs=cat_cs)
                    tag = f"{H}x{W} n {n} Cout {cout} split {split} {lay}"
                    rc1, ok1, out1, cat1 = _launch_fused(probe, H, W, n, cout, split, dump=1, **lay)
                    rc0, ok0, out0, cat0 = (rc1, ok1, None, None) if rc1 != 0 else _launch_fused(probe, H, W, n, cout, split, dump=0, **lay)
                    if rc1 != 0 or rc0 != 0:
                        pytest.exit(f"sppf_probe_fused: HIP error {rc1} / {rc0} on {tag}", returncode=3)
                    assert ok1 == 1 and ok0 == 1, tag
                    # dump = 1: y against float64 cv1; pools against the reference of the dumped y; out against float64 cv2 of the dumped concat
                    assert (cat1[:, :, 4 * c:] == SENTINEL16).all() and _only_view_written(out1, out_co, cout), tag
                    dumped = np.ascontiguousarray(cat1[:, :, :4 * c])
                    assert not sc.is_nan(dumped, BF16).any(), tag
                    r, _ = fr.bound_ratio(dumped[:, :, :c], y64, yb64, H, W)
                    assert r <= 1.0, f"{tag}: dumped y is {r:.3g} x the bound from the float64 cv1"
                    worst[0] = max(worst[0], r)
                    yb = dumped[:, :, :c].reshape(n, H, W, c)
                    if yb.tobytes() not in pool_ref:                             # the same y comes back for every layout: one reference
                        pool_ref.clear()
                        pool_ref[yb.tobytes()] = sc.ref_pools(yb, BF16)
                    for k, p in enumerate(pool_ref[yb.tobytes()]):
                        got = dumped[:, :, (k + 1) * c:(k + 2) * c].reshape(n, H, W, c)
                        d = np.argwhere(got != p)
                        assert not len(d), f"{tag}: pool {k + 1} differs from the reference pool of the dumped y at {len(d)} elements, first (frame, y, x, channel) = {d[0].tolist()}: got {int(got[tuple(d[0])]):#x} want {int(p[tuple(d[0])]):#x}"
                    key = dumped.tobytes()
                    if key not in cat_ref:                                       # the same concat comes back for every layout: one float64 cv2
                        cat_ref.clear()
                        cat_ref[key] = fr.conv64(dumped, w2, b2, H, W)
                    o64, ob64 = cat_ref[key]
                    r, _ = fr.bound_ratio(np.ascontiguousarray(out1[:, :, out_co:out_co + cout]), o64, ob64, H, W)
                    assert r <= 1.0, f"{tag}: out is {r:.3g} x the bound from the float64 cv2 over the dumped concat"
                    worst[1] = max(worst[1], r)
                    # dump = 0: the same bits, and the concat buffer stays as it was
                    assert np.array_equal(out0, out1), f"{tag}: out differs between dump = 0 and dump = 1 at {int((out0 != out1).sum())} elements"
                    assert (cat0 == SENTINEL16).all(), f"{tag}: dump = 0 wrote to the concat buffer"
    print(f"{H}x{W} Cout {cout} split {split}: worst |g - y| / bound: cv1 {worst[0]:.3f}, cv2 {worst[1]:.3f}")


REFUSALS = {
    "3x59": dict(H=3, W=59), "H=2": dict(H=2, W=13), "Cin 128": dict(cin=128, x_cs=128), "c 64": dict(c=64), "x_cs 260": dict(x_cs=260),
    "split 3": dict(split=3), "Cout 128 split 4": dict(cout=128, split=4, out_cs=128), "Cout 384": dict(cout=384, out_cs=384),
}


@pytest.mark.parametrize("what", list(REFUSALS))
def test_fused_kernel_refusals(probe, what):
    a = dict(H=13, W=13, n=2, cout=256, split=2, x_cs=256, x_co=0, out_cs=256, out_co=0, cat_cs=512, dump=1)
    a.update(REFUSALS[what])
    rc, ok, out, cat = _launch_fused(probe, **a)
    assert ok == 0 and rc == sc.HIP_ERROR_INVALID_VALUE, (what, ok, rc)
    assert (out == SENTINEL16).all() and (cat == SENTINEL16).all(), f"{what}: a refused launch wrote to its buffers"


def test_fused_probe_rejects_buffers_smaller_than_their_views(probe):
    w1, b1, w2, b2 = sc.fused_weights()
    x = np.zeros((1, 9, 256), dtype=np.uint16)
    out = np.full((1, 9, 256), SENTINEL16, dtype=np.uint16)
    cat = np.full((1, 9, 512), SENTINEL16, dtype=np.uint16)
    ok = C.c_int(-1)

    def run(x_elems=x.size, x_co=0, out_elems=out.size, out_co=0, cat_cs=512, n=1):
        return probe.sppf_probe_fused(x.ctypes.data, x_elems, 256, x_co, 256, w1.ctypes.data, b1.ctypes.data, 128, w2.ctypes.data, b2.ctypes.data, 256,
                                      n, 3, 3, 2, 1, out.ctypes.data, out_elems, 256, out_co, cat.ctypes.data, cat.size, cat_cs, C.byref(ok))
    assert run(x_elems=x.size - 8) == -1 and run(x_co=8) == -1 and run(out_elems=out.size - 8) == -1 and run(out_co=8) == -1
    assert run(cat_cs=504) == -1 and run(n=2) == -1 and run(n=0) == -1
    assert (out == SENTINEL16).all() and (cat == SENTINEL16).all()
