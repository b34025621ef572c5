"""The exact numpy oracle of the chips (include/zly.h, "Chips"), written from the header alone: float32 scalars with one rounding per operation for
the rectangle of step 4, the selection of steps 1-3 in slab order, the area resize of step 5 through tests/area_ref.py on the frame's BGR image,
and the chip slab of step 7 -- including what it must NOT write.

rect() is one detection's source rectangle, select() a slab's chosen detections, chip() one chip's pixels in the config's layout, and chip_slabs()
the bytes an output buffer must hold after a call, given what it held before.  Frames of other formats are first converted to BGR by their own
references (bgr_of): the header's rule, with every pixel's own chroma sample at its own position in the frame."""
from dataclasses import dataclass

import numpy as np

import area_ref as ar
import pixfmt_ref as pr
import yuv422_ref as y2
import yuv_ref as yr

F = np.float32
BGR8, RGB_F32 = 0, 1
MAX_DIM = ar.MAX_DIM

DET_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("w", "<f4"), ("h", "<f4"), ("confidence", "<f4"),
                      ("class_id", "<i4"), ("track_id", "<u4"), ("pad_", "<u4"), ("timestamp", "<u8")])
SLAB_HDR_DTYPE = np.dtype([("n_kept", "<i4"), ("n_candidates", "<i4"), ("flags", "<u4"), ("frame_tag", "<u4")])
HDR_DTYPE = np.dtype([("n_chips", "<i4"), ("n_eligible", "<i4"), ("frame_tag", "<u4"), ("flags", "<u4")])
REC_DTYPE = np.dtype([("det", "<i4"), ("class_id", "<i4"), ("track_id", "<u4"), ("confidence", "<f4"),
                      ("x0", "<i4"), ("y0", "<i4"), ("w", "<i4"), ("h", "<i4")])
assert DET_DTYPE.itemsize == 40 and SLAB_HDR_DTYPE.itemsize == 16 and HDR_DTYPE.itemsize == 16 and REC_DTYPE.itemsize == 32


@dataclass
class Config:
    """zly_chip_config"""
    chip_w: int = 64
    chip_h: int = 64
    max_chips: int = 16
    class_id: int = -1
    scale: float = 1.25
    layout: int = BGR8


def layout(cfg):
    """step 7 -> (slab_bytes, pixels_off, chip_stride, chip_bytes)"""
    pixels_off = -(-(HDR_DTYPE.itemsize + cfg.max_chips * REC_DTYPE.itemsize) // 256) * 256
    chip_bytes = cfg.chip_w * cfg.chip_h * (12 if cfg.layout == RGB_F32 else 3)
    stride = -(-chip_bytes // 16) * 16
    return pixels_off + cfg.max_chips * stride, pixels_off, stride, chip_bytes


def _c(v):
    """v > 0 ? (v < 1 ? v : 1) : 0 -- a NaN gives 0"""
    return (v if v < 1 else F(1)) if v > 0 else F(0)


def rect_axis(x, w, scale, E):
    """step 4, one axis -> (origin, length)"""
    with np.errstate(all="ignore"):
        x, w, scale = F(x), F(w), F(scale)
        e = F(w * scale)
        half = F(e * F(0.5))
        lo, hi = F(x - half), F(x + half)
        a = int(F(_c(lo) * F(E)))          # truncation; the product is in [0, E]
        b = int(F(_c(hi) * F(E)))
    a = min(a, E - 1)
    b = min(max(b, a + 1), E)
    return a, b - a


def rect(det, W, H, scale):
    """step 4 -> (x0, y0, rw, rh) of a detection (a DET_DTYPE record, or anything with x, y, w, h by name or in that order)"""
    try:
        x, y, w, h = det["x"], det["y"], det["w"], det["h"]
    except (TypeError, IndexError, KeyError, ValueError):
        x, y, w, h = det[:4]
    x0, rw = rect_axis(x, w, scale, W)
    y0, rh = rect_axis(y, h, scale, H)
    return x0, y0, rw, rh


def parse_slab(raw, cap):
    """one slab's bytes -> (header record, all cap detection records)"""
    raw = np.ascontiguousarray(raw, dtype=np.uint8).reshape(-1)
    assert raw.size == SLAB_HDR_DTYPE.itemsize + cap * DET_DTYPE.itemsize
    return raw[:16].view(SLAB_HDR_DTYPE)[0], raw[16:].view(DET_DTYPE)


def select(slab, cap, cfg):
    """steps 1-3 -> (n_eligible, [the selected detections' indices in slab order]); slab: one slab's bytes"""
    hdr, dets = parse_slab(slab, cap)
    K = min(max(int(hdr["n_kept"]), 0), cap)
    elig = [d for d in range(K) if cfg.class_id == -1 or int(dets[d]["class_id"]) == cfg.class_id]
    return len(elig), elig[:min(cfg.max_chips, len(elig))]


def bgr_of(fmt, frame, w, h):
    """the frame's BGR image by its format's reference (frame: the tight frame as the engine takes it)"""
    if fmt == 0:
        return np.asarray(frame, dtype=np.uint8).reshape(h, w, 3)
    if fmt in yr.YUV_FORMATS:
        return yr.yuv420_to_bgr(frame, w, h, fmt)
    if fmt in y2.FORMATS:
        return y2.to_bgr(frame, w, h, fmt)
    return pr.to_bgr(frame, w, h, fmt)


def chip_bgr(bgr, r, cfg):
    """step 5: u8 [chip_h][chip_w][3] B, G, R of the rectangle r = (x0, y0, rw, rh) of the frame's BGR image"""
    x0, y0, rw, rh = r
    H, W = bgr.shape[:2]
    assert 0 <= x0 and 0 <= y0 and rw >= 1 and rh >= 1 and x0 + rw <= W and y0 + rh <= H
    return ar.area_bgr(bgr[y0:y0 + rh, x0:x0 + rw, :3], cfg.chip_w, cfg.chip_h)


def chip(bgr, r, cfg):
    """steps 5-6: the chip's bytes in the config's layout, as a flat u8 array"""
    c = chip_bgr(bgr, r, cfg)
    if cfg.layout == RGB_F32:
        planes = np.stack([c[..., 2], c[..., 1], c[..., 0]]).astype(np.float32) / np.float32(255.0)
        return np.ascontiguousarray(planes).view(np.uint8).reshape(-1)
    return np.ascontiguousarray(c).reshape(-1)


def chip_slabs(raw_slabs, bgr_frames, cfg, before, cap=None):
    """the bytes of the n chip slabs after a call: raw_slabs u8 [n][slab bytes], bgr_frames the n frames' BGR images, before u8 [n][chip slab bytes]
    what the output buffer held.  Only the header, the n_chips records and the n_chips chips' own bytes differ from `before`."""
    n = len(bgr_frames)
    raw_slabs = np.ascontiguousarray(raw_slabs, dtype=np.uint8).reshape(n, -1)
    if cap is None:
        cap = (raw_slabs.shape[1] - SLAB_HDR_DTYPE.itemsize) // DET_DTYPE.itemsize
    slab_bytes, pixels_off, stride, chip_bytes = layout(cfg)
    out = np.array(before, dtype=np.uint8).reshape(n, slab_bytes).copy()
    for i in range(n):
        hdr, dets = parse_slab(raw_slabs[i], cap)
        n_elig, chosen = select(raw_slabs[i], cap, cfg)
        h = np.zeros(1, dtype=HDR_DTYPE)
        h["n_chips"], h["n_eligible"], h["frame_tag"], h["flags"] = len(chosen), n_elig, hdr["frame_tag"], 0
        out[i, :16] = h.view(np.uint8)
        H, W = bgr_frames[i].shape[:2]
        assert 1 <= W <= MAX_DIM and 1 <= H <= MAX_DIM
        for j, d in enumerate(chosen):
            r = rect(dets[d], W, H, cfg.scale)
            rec = np.zeros(1, dtype=REC_DTYPE)
            rec["det"], rec["class_id"], rec["track_id"], rec["confidence"] = d, dets[d]["class_id"], dets[d]["track_id"], dets[d]["confidence"]
            rec["x0"], rec["y0"], rec["w"], rec["h"] = r
            out[i, 16 + 32 * j:16 + 32 * (j + 1)] = rec.view(np.uint8)
            o = pixels_off + j * stride
            out[i, o:o + chip_bytes] = chip(bgr_frames[i], r, cfg)
    return out


def make_slab(dets, cap, n_kept=None, frame_tag=0, flags=0, n_candidates=0, fill=0):
    """one slab's bytes from hand-written detections: dets = [(x, y, w, h, confidence, class_id, track_id)]; records beyond them hold `fill` bytes"""
    raw = np.full(SLAB_HDR_DTYPE.itemsize + cap * DET_DTYPE.itemsize, fill, dtype=np.uint8)
    hdr = np.zeros(1, dtype=SLAB_HDR_DTYPE)
    hdr["n_kept"] = len(dets) if n_kept is None else n_kept
    hdr["n_candidates"], hdr["flags"], hdr["frame_tag"] = n_candidates, flags, frame_tag
    raw[:16] = hdr.view(np.uint8)
    rec = np.zeros(min(len(dets), cap), dtype=DET_DTYPE)
    for k, d in enumerate(dets[:cap]):
        d = tuple(d) + (1.0, 0, 0)[len(d) - 4:] if len(d) < 7 else d
        rec[k]["x"], rec[k]["y"], rec[k]["w"], rec[k]["h"], rec[k]["confidence"], rec[k]["class_id"], rec[k]["track_id"] = d
    raw[16:16 + rec.nbytes] = rec.view(np.uint8)
    return raw
