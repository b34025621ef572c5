"""Closed-loop float64 reference for every conv of the YOLOv8 graph.  TEST INFRASTRUCTURE (imported by tests/ only; not a conftest).

The layer checks of test_gpu_parity.py compare an engine tensor with an oracle tensor computed from the ORACLE's upstream activations, so
the two chains drift apart and the bounds are loose (2^-5 of the range).  Here every conv is fed the engine's OWN tapped inputs -- exact
bf16 (or fp32) values, read back through zly_debug_tap -- through a float64 convolution.  Pools, nearest Upsample, Concat and the C2f
channel slices are selections and therefore exact.  The only legitimate difference between the engine's output g and the float64 result y
is then one final rounding plus fp32 accumulation noise, nothing accumulates from layer to layer, and the bound can be per element.

For one output element, with w = the weights as the engine holds them (csrc/weights.cpp: bf16 RNE of the file's values in the bf16 engine --
the fp8 file's values e4m3 * 2^exp are exact in bf16 -- and the fp32 values themselves in the fp32 engine), b the fp32 bias, x the tapped
inputs, r the tapped shortcut (or 0), everything in float64:

    p = b + sum w x          A = |b| + sum |w| |x|   (a conv of |x| with |w|)
    y = SiLU(p) + r          (y = p + r where the spec has no activation)
    B = A + |r|

    output stored as bf16:                                         |g - y| <= 2^-8  |y| + C_ACC 2^-24 B
    output stored as fp32 (the six final Detect logits; fp32 engine): |g - y| <= 2^-24 |y| + C_ACC 2^-24 B

Derivation.  Round-to-nearest-even to bf16 (8 significant bits) moves a value by at most half an ulp, which is at most 2^-8 |v|; truncation
reaches 2^-7 |v|, a second rounding ahead of the shortcut add reaches 2^-8 |SiLU(p)| + 2^-8 |y|: both are caught.  To fp32 the half ulp is
2^-24 |v|.  Everything ahead of the store happens in fp32 and is proportional to B: the accumulation order of the products (each partial sum is
bounded by A), the rounded p * (-log2 e) argument, v_exp_f32 and v_rcp_f32 at 1 ulp each (|SiLU'| <= 1.1 and |SiLU(p)| <= |p| <= A), the add of r.

C_ACC is NOT tuned on GPU results.  Its floor is measured against the reference alone, on the CPU: for every conv of every model and shape
the tests use, torch's fp32 CPU conv2d (what oracle/yolov8_ref.py computes) fed the same inputs, max over elements of
(|y32 - y| - rounding term)^+ / (2^-24 B)  (acc_floor() below; tests/test_closed_loop_ref.py asserts 16 x floor <= C_ACC on its shapes).
Measured maxima: see C_ACC_CPU_FLOOR (the oracle in bf16 mode, for the bf16 engine) and C_ACC_FP32_CPU_FLOOR (in fp32 mode, for the fp32
engine).  C_ACC = 16 x that, rounded up to a power of two; the 16 x is for what the CPU cannot show (MFMA's internal summation order and
rounding, the two approximate transcendentals).  The margin costs no sensitivity: with B / |y| between 10 and 75
on the synthetic weights (median per layer), 32 * 2^-24 * B is under 4 % of the half-ulp term.

Intermediates that cannot be tapped (the first conv of a bottleneck inside bottleneck_pair_kernel / c2f_kernel<16 / 32>, which stay in LDS
even with the dump flag): the reference chains both convs, mid = bf16_RNE(SiLU(p_A)) in float64.  A mid element is AMBIGUOUS when SiLU(p_A)
lies within 1.1 C_ACC 2^-24 A_A of a bf16 rounding tie; there, and only there, the engine may hold the neighbouring bf16 value.  Output
elements that depend on ambiguous mids get the extra allowance 1.1 sum |w_B| ulp(mid) over those mids (one more float64 conv of a masked map).
That path is taken only for a name whose tap call was refused, and the set of refused names must EQUAL the caller's `lds_resident`: a
tappable tensor can never be loosened silently.

The head rider (check_head_decode): zly_head_tensor against a float64 DFL-softmax / anchor / sigmoid decode of the engine's own six fp32
logits taps per frame, written out as in oracle/yolov8_ref.py::detect.  Tolerances measured like C_ACC (torch fp32 decode vs float64 decode
on the CPU, decode_floor() below), 16 x, rounded up to a power of two."""
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

import zly_model as zm

# Largest (|y32 - y| - rounding term)^+ / (2^-24 B) of torch's fp32 CPU conv2d, fed the same inputs, over every conv of: yolov8n / s at
# 64x64, 96x64, 352x288; n at 224x416, 416x416; s at 320x320, and with fp8 weights at 96x64 and 640x640; yolov8m at 320x320 / 352x288;
# yolov8l at 256x256; yolov8n with 1 / 4 / 17 / 64 classes at 416x416 (acc_floor()).
#   * the oracle in bf16 mode (stands in for the bf16 engine): 1.59, at the final 1x1 Detect convs (model.22.cv3.L.2), whose fp32 store hides nothing;
#   * the oracle in fp32 mode (stands in for the fp32 engine; n and s, the models that engine loads): 6.51, at 3x3 convs of 576 .. 1152 products --
#     fp32 inputs and weights carry 24-bit mantissas, so unlike in bf16 mode no product is exact in fp32, and a 2^-24 |y| store hides nothing anywhere.
# C_ACC = 16 x the floor of the engine's dtype, rounded up to a power of two.
#
# The smallest and thinnest maps (tests/small_map_cases.py: yolov8n at 32x32, 64x32, 32x64, 96x32, 32x96, 96x96, 416x32, 32x416 and 64x64, n = 3;
# tests/test_small_map_cases.py asserts the 16 x rule there) were measured with the stand-in built inside torch.backends.mkldnn.flags(enabled=False):
#   * bf16 mode: 0.52 (32x32) .. 1.12 (64x32), at the final 1x1 Detect convs model.22.cv2.L.2 -- below 1.59;
#   * fp32 mode: 2.26 (32x32) .. 4.13 (96x96), at model.1 / model.2 / model.4 / model.12 convs -- below 6.51;
#   * decode: at most 5.4e-5 px and 2.8e-8 -- below the decode floors.
# So the constants stay as they are.  Two observations about the STAND-IN there, neither of which says anything about an engine:
#   1. with torch's defaults (oneDNN on) the stand-in misses the 16 x rule at 32x32: at n >= 2 its floor is 6.3 - 6.9 (bf16 mode) and 9.4 - 9.9 (fp32 mode), at
#      the six final Detect convs -- oneDNN's choice of algorithm for those tiny batched convs (at n = 1 the floor is 0.28).  It produces no violation either
#      way, but a stand-in for these shapes is built with oneDNN off, where the plain CPU conv shows the figures above;
#   2. at n = 64 (32x32, all frames) torch's CPU conv shows floors of 8.8 with oneDNN and 24 without (bf16 mode), 13 and 111 (fp32 mode) -- its blocking over a
#      large batch of tiny maps sums in an order of its own; figures of 10.8 and 60 have been seen on another run.  The stand-in is not used at large n.  The
#      64-frame GPU cases need no stand-in -- their reference is float64 on the engine's own taps.
C_ACC_CPU_FLOOR, C_ACC_FP32_CPU_FLOOR = 1.59, 6.51
C_ACC = 32.0                  # bf16 engine
C_ACC_FP32_ENGINE = 128.0     # fp32 engine
# the oracle's torch fp32 decode vs the float64 decode of the same logits, same models and shapes (decode_floor()): boxes in px, scores absolute
DECODE_BOX_CPU_FLOOR, DECODE_SCORE_CPU_FLOOR = 8.7e-5, 6.0e-8
DECODE_BOX_TOL, DECODE_SCORE_TOL = 2.0 ** -9, 2.0 ** -19       # 16 x the floors (1.4e-3 px, 9.6e-7), rounded up to a power of two

EPS_BF16, EPS_F32 = 2.0 ** -8, 2.0 ** -24
SILU_LIP = 1.1                # max |SiLU'| = 1.0998...


class TapUnavailable(Exception):
    """what a stand-in engine's tap() raises for a tensor that stays in LDS (the engine raises zly.ZlyError)"""


def bf16_rne(v):
    """float64 array -> (nearest bf16 value, ties to even; ulp of the binade of v; distance of v to the nearest rounding tie), all float64.
    Done on the float64 value itself: a detour through fp32 would round twice."""
    v = np.asarray(v, dtype=np.float64)
    _, e = np.frexp(v)                                           # |v| = m 2^e, m in [0.5, 1): 8 significant bits -> spacing 2^(e - 8)
    ulp = np.ldexp(1.0, np.maximum(e, -125) - 8)
    s = v / ulp                                                  # exact (power of two)
    q = np.rint(s) * ulp                                         # rint: ties to even
    frac = s - np.floor(s)
    return q, ulp, np.abs(frac - 0.5) * ulp


def silu64(p):
    return p / (1.0 + np.exp(-p))


@functools.lru_cache(maxsize=8)
def _load_cached(path, mtime, fp32):
    meta, weights = zm.read_zlyw(path)
    w64 = {}
    for name, (w, b) in weights.items():
        wt = torch.from_numpy(np.array(w, dtype=np.float32))
        if not fp32:
            wt = wt.to(torch.bfloat16).to(torch.float32)         # == f32_to_bf16_rne of csrc/weights.cpp (finite values)
        w64[name] = (wt.to(torch.float64), torch.from_numpy(np.array(b, dtype=np.float32)).to(torch.float64))
    return meta, w64


def load_model(path, fp32=False):
    """(meta, {name: (w, b) as float64 tensors holding the values the engine computes with})"""
    return _load_cached(os.path.abspath(path), os.path.getmtime(path), bool(fp32))


def keeps_fp32(name):
    """the six final Detect convs store fp32 logits in either engine"""
    return name.startswith("model.22.") and name.endswith(".2")


class _Graph:
    """The wiring of oracle/yolov8_ref.py::forward over TAPPED tensors: inputs(name) -> (x, r), float64 [F, C, H, W], built from get()."""

    def __init__(self, meta, get):
        self.get = get
        self.n = tuple(meta["n_c2f"])
        self.names = [c.name for c in meta["convs"]]
        self.recipe = {}                                         # conv name -> (callable -> x, callable -> r or None)
        self.pair_of = {}                                        # m.i.cv2 -> its m.i.cv1
        n = self.n
        g = self._tap
        self._conv("model.0", lambda: get("images"))
        self._conv("model.1", g("model.0"))
        self._c2f("model.2", g("model.1"), n[0], True)
        self._conv("model.3", g("model.2.cv2"))
        self._c2f("model.4", g("model.3"), n[1], True)
        self._conv("model.5", g("model.4.cv2"))
        self._c2f("model.6", g("model.5"), n[2], True)
        self._conv("model.7", g("model.6.cv2"))
        self._c2f("model.8", g("model.7"), n[3], True)
        self._conv("model.9.cv1", g("model.8.cv2"))

        def sppf_in():
            y = get("model.9.cv1")
            p1 = F.max_pool2d(y, 5, 1, 2)
            p2 = F.max_pool2d(p1, 5, 1, 2)
            p3 = F.max_pool2d(p2, 5, 1, 2)
            return torch.cat([y, p1, p2, p3], 1)
        self._conv("model.9.cv2", sppf_in)
        up = lambda t: t.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)      # nearest, scale 2
        self._c2f("model.12", lambda: torch.cat([up(get("model.9.cv2")), get("model.6.cv2")], 1), n[4], False)
        self._c2f("model.15", lambda: torch.cat([up(get("model.12.cv2")), get("model.4.cv2")], 1), n[5], False)
        self._conv("model.16", g("model.15.cv2"))
        self._c2f("model.18", lambda: torch.cat([get("model.16"), get("model.12.cv2")], 1), n[6], False)
        self._conv("model.19", g("model.18.cv2"))
        self._c2f("model.21", lambda: torch.cat([get("model.19"), get("model.9.cv2")], 1), n[7], False)
        for lvl, feat in enumerate(("model.15.cv2", "model.18.cv2", "model.21.cv2")):
            for br in (2, 3):
                self._conv(f"model.22.cv{br}.{lvl}.0", g(feat))
                self._conv(f"model.22.cv{br}.{lvl}.1", g(f"model.22.cv{br}.{lvl}.0"))
                self._conv(f"model.22.cv{br}.{lvl}.2", g(f"model.22.cv{br}.{lvl}.1"))
        assert sorted(self.recipe) == sorted(self.names), sorted(set(self.names) ^ set(self.recipe))

    def _tap(self, name):
        return lambda: self.get(name)

    def _conv(self, name, x, r=None):
        self.recipe[name] = (x, r)

    def _c2f(self, prefix, src, n, shortcut):
        get = self.get
        self._conv(f"{prefix}.cv1", src)

        def part(i):
            """ys[i] of yolov8_ref.c2f: the two halves of cv1, then every bottleneck's output"""
            if i < 2:
                def half():
                    y = get(f"{prefix}.cv1")
                    c = y.shape[1] // 2
                    return y[:, :c] if i == 0 else y[:, c:]
                return half
            return lambda: get(f"{prefix}.m.{i - 2}.cv2")
        for i in range(n):
            self._conv(f"{prefix}.m.{i}.cv1", part(i + 1))
            self._conv(f"{prefix}.m.{i}.cv2", self._tap(f"{prefix}.m.{i}.cv1"), part(i + 1) if shortcut else None)
            self.pair_of[f"{prefix}.m.{i}.cv2"] = f"{prefix}.m.{i}.cv1"
        self._conv(f"{prefix}.cv2", lambda: torch.cat([part(i)() for i in range(n + 2)], 1))


def conv64(spec, w, b, x):
    """float64: (p = b + sum w x, A = |b| + sum |w| |x|)"""
    pad = spec.k // 2
    p = F.conv2d(x, w, b, stride=spec.stride, padding=pad)
    a = F.conv2d(x.abs(), w.abs(), b.abs(), stride=spec.stride, padding=pad)
    return p.numpy(), a.numpy()


def _finish(spec, p, a, r):
    y = silu64(p) if spec.act else p
    bb = a
    if r is not None:
        r = r.numpy()
        y = y + r
        bb = a + np.abs(r)
    return y, bb


def mid_of(model_path, name, x, fp32=False):
    """the chained reference's view of an untappable conv `name` on its (tapped) input x [F, C, H, W]: (mid = bf16_RNE(SiLU(p)) as float64,
    ambiguity mask, ulp(mid), neighbour = the bf16 value on the other side of the nearest rounding tie)"""
    meta, w64 = load_model(model_path, fp32)
    spec = {c.name: c for c in meta["convs"]}[name]
    p, a = conv64(spec, *w64[name], torch.as_tensor(np.asarray(x, dtype=np.float64)))
    return _mid(spec, p, a)


def _mid(spec, p, a):
    assert spec.act, spec.name
    s = silu64(p)
    mid, ulp, tie_dist = bf16_rne(s)
    amb = tie_dist <= SILU_LIP * C_ACC * EPS_F32 * a
    other = np.where(s >= mid, mid + ulp, mid - ulp)            # the tie nearest to s lies on the side of s
    return mid, amb, ulp, other


class Violation:
    def __init__(self, name, frame, count, total, worst, box, allowance):
        self.name, self.frame, self.count, self.total, self.worst, self.box, self.allowance = name, frame, count, total, worst, box, allowance

    def __str__(self):
        (c0, c1), (y0, y1), (x0, x1) = self.box
        return (f"{self.name}[frame {self.frame}]: {self.count} of {self.total} elements violate, worst |g - y| / bound = {self.worst:.3g}, "
                f"violators within c {c0}..{c1}, y {y0}..{y1}, x {x0}..{x1}" + (" (checked through the ambiguity allowance)" if self.allowance else ""))


def closed_loop(engine, model_path, frames, lds_resident=(), first_input=None, fp32=None):
    """-> (names checked, violations, stats).  engine: anything with tap(name, frame) -> float [C, H, W] that raises zly.ZlyError /
    TapUnavailable for a tensor it cannot expose; frames: frame indices of the last call; first_input: [len(frames), 3, H, W] to stand for
    the "images" tap (the detect path's front kernels never write that buffer); fp32: the engine's dtype (default: read from engine.cfg).
    stats[name] = (largest |g - y| / bound, largest (|g - y| - rounding term)^+ / (2^-24 B)): the second is what C_ACC bounds."""
    import zly
    if fp32 is None:
        fp32 = engine.cfg.dtype == zly.DTYPE_FP32 if hasattr(engine, "cfg") else bool(engine.fp32)
    meta, w64 = load_model(model_path, fp32)
    c_acc = C_ACC_FP32_ENGINE if fp32 else C_ACC
    specs = {c.name: c for c in meta["convs"]}
    frames = list(frames)
    cache, refused = {}, set()

    def get(name):
        if name in refused:
            raise TapUnavailable(name)
        if name not in cache:
            if name == "images" and first_input is not None:
                t = np.asarray(first_input, dtype=np.float64)
                assert t.shape[0] == len(frames) and t.shape[1] == 3, t.shape
            else:
                try:
                    t = np.stack([np.asarray(engine.tap(name, i), dtype=np.float64) for i in frames])
                except TapUnavailable:
                    refused.add(name)
                    raise
                except zly.ZlyError as exc:
                    if exc.code != zly.ERR_INVALID_ARGUMENT:
                        raise
                    refused.add(name)
                    raise TapUnavailable(name) from exc
            assert np.isfinite(t).all(), name
            cache[name] = torch.from_numpy(t)
        return cache[name]

    graph = _Graph(meta, get)
    for name in graph.names:                                     # find what the engine refuses before anything is checked
        try:
            get(name)
        except TapUnavailable:
            pass
    assert refused == set(lds_resident), f"taps refused {sorted(refused)}, expected LDS-resident {sorted(lds_resident)}"
    assert not (fp32 and refused), "the fp32 engine fuses nothing"
    for name in refused:
        assert ".m." in name and name.endswith(".cv1"), f"{name}: only the first conv of a bottleneck may be checked through its consumer"
    consumer_of = {v: k for k, v in graph.pair_of.items()}
    checked, violations, stats = [], [], {}
    for name in graph.names:
        if name in refused:
            continue                                             # checked through its consumer below
        spec = specs[name]
        fx, fr = graph.recipe[name]
        r = fr() if fr is not None else None
        extra = 0.0
        first = graph.pair_of.get(name)
        if first in refused:
            sa = specs[first]
            pa, aa = conv64(sa, *w64[first], graph.recipe[first][0]())
            mid, amb, ulp, _ = _mid(sa, pa, aa)
            x = torch.from_numpy(mid)
            extra = SILU_LIP * F.conv2d(torch.from_numpy(np.where(amb, ulp, 0.0)), w64[name][0].abs(), None, stride=spec.stride, padding=spec.k // 2).numpy()
        else:
            x = fx()
        p, a = conv64(spec, *w64[name], x)
        y, bb = _finish(spec, p, a, r)
        g = get(name).numpy()
        assert g.shape == y.shape, (name, g.shape, y.shape)
        rnd = (EPS_F32 if fp32 or keeps_fp32(name) else EPS_BF16) * np.abs(y)
        err = np.abs(g - y)
        bound = rnd + c_acc * EPS_F32 * bb + extra
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
        acc = np.clip(err - rnd - extra, 0, None) / np.where(bb > 0, EPS_F32 * bb, 1.0)
        stats[name] = (float(ratio.max()), float(acc.max()))
        for k, fi in enumerate(frames):
            bad = ratio[k] > 1.0
            if bad.any():
                idx = np.nonzero(bad)
                violations.append(Violation(name, fi, int(bad.sum()), bad.size, float(ratio[k].max()),
                                            tuple((int(i.min()), int(i.max())) for i in idx), first in refused))
        checked.append(name)
        if first in refused:
            checked.append(first)
    assert set(consumer_of) >= refused
    return checked, violations, stats


def check_closed_loop(engine, model_path, frames, lds_resident=(), first_input=None, fp32=None):
    """asserts the per-element bound for every conv of the model on the engine's own tapped inputs; returns the names checked"""
    checked, violations, _ = closed_loop(engine, model_path, frames, lds_resident, first_input, fp32)
    assert not violations, "closed-loop float64 check:\n  " + "\n  ".join(str(v) for v in violations)
    meta, _ = load_model(model_path, False)
    assert len(checked) == len(meta["convs"]), sorted(set(c.name for c in meta["convs"]) - set(checked))
    return checked


def lds_resident_from_kernels(engine, n):
    """the conv names a bf16 engine created with ZLY_FLAG_DUMP_LOGITS cannot expose after a call of batch size n, read off its kernel table
    (zly_op_kernel_name): the first conv of a bottleneck that runs in bottleneck_pair_kernel, or inside c2f_kernel<C=16 / 32> (the 64-channel
    C2f kernel and conv3x3_ws_pair_kernel write their intermediate map out with the dump flag)"""
    kern = {o["name"]: k for o, k in zip(engine.ops(), engine.op_kernels(n))}
    inside = "(fused into the C2f kernel at "
    out = set()
    for name, k in kern.items():
        if ".m." not in name or not name.endswith(".cv1"):
            continue
        lead = k[len(inside):-1] if k.startswith(inside) else name
        if k.startswith("bottleneck_pair_kernel<") or kern[lead].startswith(("c2f_kernel<C=16", "c2f_kernel<C=32")):
            out.add(name)
    return out


def acc_floor(engine, model_path, frames, fp32=False):
    """the CPU floor of C_ACC on a stand-in engine (oracle/yolov8_ref.py's taps): max over convs of (|y32 - y| - rounding term)^+ / (2^-24 B)"""
    _, _, stats = closed_loop(engine, model_path, frames, fp32=fp32)
    return max(v[1] for v in stats.values()), max(stats, key=lambda k: stats[k][1])


# ---------------------------------------------------------------------------------------------------
# head decode
# ---------------------------------------------------------------------------------------------------
def decode64(box_logits, cls_logits, reg_max=16, dtype=np.float64):
    """oracle/yolov8_ref.py::detect in `dtype`: box_logits / cls_logits = per level [4 * reg_max, h, w] / [nc, h, w] -> [4 + nc, N]"""
    boxes, clss, anchors, strides = [], [], [], []
    for lvl, (b, c) in enumerate(zip(box_logits, cls_logits)):
        h, w = b.shape[1], b.shape[2]
        boxes.append(np.asarray(b, dtype=dtype).reshape(4, reg_max, h * w))
        clss.append(np.asarray(c, dtype=dtype).reshape(c.shape[0], h * w))
        sy, sx = np.meshgrid(np.arange(h, dtype=dtype) + dtype(0.5), np.arange(w, dtype=dtype) + dtype(0.5), indexing="ij")
        anchors.append(np.stack([sx.reshape(-1), sy.reshape(-1)]))
        strides.append(np.full(h * w, (8, 16, 32)[lvl], dtype=dtype))
    box, cls, anc, st = np.concatenate(boxes, 2), np.concatenate(clss, 1), np.concatenate(anchors, 1), np.concatenate(strides)
    e = np.exp(box - box.max(1, keepdims=True))
    prob = e / e.sum(1, keepdims=True)                           # DFL: softmax over the bins, expectation
    dist = (prob * np.arange(reg_max, dtype=dtype).reshape(1, -1, 1)).sum(1)      # [4, N] = l, t, r, b
    x1y1, x2y2 = anc - dist[:2], anc + dist[2:]
    out_box = np.concatenate([(x1y1 + x2y2) / dtype(2), x2y2 - x1y1]) * st
    return np.concatenate([out_box, dtype(1) / (dtype(1) + np.exp(-cls))]).astype(dtype)


def _logit_taps(engine, frame):
    return ([engine.tap(f"model.22.cv2.{l}.2", frame) for l in range(3)], [engine.tap(f"model.22.cv3.{l}.2", frame) for l in range(3)])


def check_head_decode(engine, head, frame, reg_max=16):
    """head [4 + nc, N] (zly_head_tensor of `frame`) against the float64 decode of the engine's own six logits taps of that frame"""
    want = decode64(*_logit_taps(engine, frame), reg_max=reg_max)
    head = np.asarray(head, dtype=np.float64)
    assert head.shape == want.shape, (head.shape, want.shape)
    db, ds = np.abs(head[:4] - want[:4]), np.abs(head[4:] - want[4:])
    assert db.max() <= DECODE_BOX_TOL, f"head boxes of frame {frame}: {db.max():.3g} px from the float64 decode at anchor {int(db.max(0).argmax())} (row {int(db.max(1).argmax())})"
    assert ds.max() <= DECODE_SCORE_TOL, f"head scores of frame {frame}: {ds.max():.3g} from the float64 decode at anchor {int(ds.max(0).argmax())} (class {int(ds.max(1).argmax())})"


def decode_floor(engine, head, frame, reg_max=16):
    """CPU floor of the decode tolerances: the oracle's torch fp32 decode (head = row `frame` of YoloV8Ref.forward) vs the float64 decode
    of the same logits -> (box px, score)"""
    d = np.abs(np.asarray(head, dtype=np.float64) - decode64(*_logit_taps(engine, frame), reg_max=reg_max))
    return float(d[:4].max()), float(d[4:].max())


class StandIn:
    """oracle/yolov8_ref.py as an engine: its taps of the last forward() behind tap(name, frame); `hidden` names are refused like LDS-resident ones"""

    def __init__(self, ref, images, hidden=()):
        self.ref, self.hidden, self.fp32 = ref, set(hidden), ref.mode == "fp32"
        images = torch.as_tensor(images)
        self.head = ref.forward(images).numpy()
        self.images = ref._q(images)

    def tap(self, name, frame):
        if name in self.hidden:
            raise TapUnavailable(name)
        return (self.images if name == "images" else self.ref.taps[name])[frame].numpy()
