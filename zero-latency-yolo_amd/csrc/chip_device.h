// chip_device.h -- the arithmetic of the chips (include/zly.h "Chips"): step 4's source rectangle, the selection predicate, the chip slab's offsets
// and where a frame pixel's samples lie through a view, as the two kernels (kernels_chips.hip), the host side (chip_rules.h) and a stand-alone CPU
// program (tests/cpp/test_chip_rules.cpp) all compile it.  Nothing here includes a HIP header: a plain C++ compiler takes this file as it is.  Every
// float operation below is one IEEE fp32 operation, in the order written: each function that has one turns FP contraction off in its own body, as
// zoom_device.h does; a compiler without the pragma is given -ffp-contract=off (the Makefile).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ZLY_CHIP_HD __host__ __device__ inline
#else
#define ZLY_CHIP_HD inline
#endif
#if defined(__clang__)
#define ZLY_CHIP_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define ZLY_CHIP_NO_CONTRACT
#endif

namespace zly {

// The cut kernel's shape constants (kernels_chips.hip).  tests/test_gpu_chips.py parses them from this file: rectangle widths and heights one
// below, at and one above each of them are where the kernel changes path.
#define ZLY_CHIP_THREADS    256     // threads per workgroup = the widest chip (one thread per chip column)
#define ZLY_CHIP_CHUNK_PX   1020    // frame pixels of a row staged into LDS at once (even; 4 bytes each plus 15 of alignment slack = 256 lanes x 16 bytes)
#define ZLY_CHIP_BAND_ROWS  4       // chip rows per workgroup: a 64-row chip of a large target is the work of 16 workgroups

#define ZLY_CHIP_MAX_DIM    256     // chip_w, chip_h <= 256
#define ZLY_CHIP_HDR_BYTES  16      // sizeof(zly_chip_header)
#define ZLY_CHIP_REC_BYTES  32      // sizeof(zly_chip_rec)
#define ZLY_CHIP_ALIGN      256     // the pixels of a chip slab begin at a multiple of it

// the format families as the addressing below needs them (chip_rules.h: chip_frame_of derives a frame's family from the format table)
#define ZLY_CHIP_FAM_PACKED 0       // one plane, bpp bytes per pixel, bytes 0..2 are the pixel's
#define ZLY_CHIP_FAM_NV12   1       // Y plane + one plane of U, V pairs
#define ZLY_CHIP_FAM_I420   2       // Y plane + U plane + V plane
#define ZLY_CHIP_FAM_Y422   3       // one plane of 4-byte macropixels of two pixels

// What the kernels need of one frame of a call; the host fills it from the frame's (checked) view (chip_rules.h: chip_frame_of) and uploads it.
// ext[p]: the extent of plane p -- no byte at or beyond off[p] + ext[p] may be read.  88 bytes.
struct ChipFrame {
    uint64_t off[3];          // the view's plane offsets (planes the format does not have: 0)
    uint64_t ext[3];          // (rows - 1) * pitch + row bytes of each plane (0 for a plane the format does not have)
    int32_t  pitch[3];
    int32_t  W, H;            // the frame the slab's boxes are fractions of
    int32_t  fmt;             // ZLY_PIX_*
    int32_t  fam;             // ZLY_CHIP_FAM_*
    int32_t  bpp;             // bytes per pixel of plane 0 (packed 4:2:2: 2)
    int32_t  planes;
    int32_t  pad_;
};

// ---- step 4: the source rectangle, one axis.  x: the box's centre, w: its size (fractions of the extent E), scale: the config's ----
struct ChipSpan { int32_t o, n; };       // origin and length: 0 <= o, 1 <= n, o + n <= E
ZLY_CHIP_HD float chip_clamp01(float v) { return v > 0.0f ? (v < 1.0f ? v : 1.0f) : 0.0f; }      // a NaN gives 0
ZLY_CHIP_HD ChipSpan chip_rect_axis(float x, float w, float scale, int32_t E)
{
    ZLY_CHIP_NO_CONTRACT
    const float e = w * scale;
    const float half = e * 0.5f;
    const float lo = x - half;
    const float hi = x + half;
    int32_t a = (int32_t)(chip_clamp01(lo) * (float)E);
    int32_t b = (int32_t)(chip_clamp01(hi) * (float)E);
    a = a < E - 1 ? a : E - 1;
    b = b > a + 1 ? b : a + 1;
    b = b < E ? b : E;
    ChipSpan s;
    s.o = a; s.n = b - a;
    return s;
}

// ---- step 2: is a detection of class `cls` eligible under the config's class_id? ----
ZLY_CHIP_HD bool chip_eligible(int32_t cls, int32_t class_id) { return class_id == -1 || cls == class_id; }

// ---- step 1 ----
ZLY_CHIP_HD int32_t chip_stored(int32_t n_kept, int32_t cap) { return n_kept < 0 ? 0 : (n_kept > cap ? cap : n_kept); }

// ---- step 7: the chip slab ----
struct ChipLayout { uint64_t slab_bytes, pixels_off, chip_stride, chip_bytes; };
ZLY_CHIP_HD ChipLayout chip_layout(int32_t chip_w, int32_t chip_h, int32_t max_chips, int32_t layout_f32)
{
    ChipLayout l;
    const uint64_t rec_end = (uint64_t)ZLY_CHIP_HDR_BYTES + (uint64_t)max_chips * ZLY_CHIP_REC_BYTES;
    l.pixels_off = (rec_end + ZLY_CHIP_ALIGN - 1) / ZLY_CHIP_ALIGN * ZLY_CHIP_ALIGN;
    l.chip_bytes = (uint64_t)chip_w * (uint64_t)chip_h * (layout_f32 ? 12u : 3u);
    l.chip_stride = (l.chip_bytes + 15u) & ~(uint64_t)15u;
    l.slab_bytes = l.pixels_off + (uint64_t)max_chips * l.chip_stride;
    return l;
}
ZLY_CHIP_HD uint64_t chip_rec_off(int32_t j) { return (uint64_t)ZLY_CHIP_HDR_BYTES + (uint64_t)j * ZLY_CHIP_REC_BYTES; }

// ---- where frame pixel (x, y) keeps its samples: byte offsets from the buffer base.  Each is the pixel's OWN sample at its own position in the
//      frame, whatever rectangle it is read for.  o[0]: packed: the pixel's first byte (bytes 0..2 are read); 4:2:0: its Y; 4:2:2: its macropixel
//      (4 bytes).  o[1], o[2]: NV12: its U and V (adjacent bytes of plane 1); I420: its U in plane 1, its V in plane 2.  Returns the number of
//      offsets filled in; nbytes[k] = bytes read at o[k], plane[k] = the plane it lies in.
ZLY_CHIP_HD int chip_pixel_samples(const ChipFrame& f, int32_t x, int32_t y, uint64_t o[3], int32_t nbytes[3], int32_t plane[3])
{
    if (f.fam == ZLY_CHIP_FAM_PACKED) {
        o[0] = f.off[0] + (uint64_t)y * (uint64_t)f.pitch[0] + (uint64_t)x * (uint64_t)f.bpp; nbytes[0] = 3; plane[0] = 0;
        return 1;
    }
    if (f.fam == ZLY_CHIP_FAM_Y422) {
        o[0] = f.off[0] + (uint64_t)y * (uint64_t)f.pitch[0] + (uint64_t)(x >> 1) * 4u; nbytes[0] = 4; plane[0] = 0;
        return 1;
    }
    o[0] = f.off[0] + (uint64_t)y * (uint64_t)f.pitch[0] + (uint64_t)x; nbytes[0] = 1; plane[0] = 0;
    if (f.fam == ZLY_CHIP_FAM_NV12) {
        o[1] = f.off[1] + (uint64_t)(y >> 1) * (uint64_t)f.pitch[1] + (uint64_t)(x & ~1); nbytes[1] = 2; plane[1] = 1;
        return 2;
    }
    o[1] = f.off[1] + (uint64_t)(y >> 1) * (uint64_t)f.pitch[1] + (uint64_t)(x >> 1); nbytes[1] = 1; plane[1] = 1;
    o[2] = f.off[2] + (uint64_t)(y >> 1) * (uint64_t)f.pitch[2] + (uint64_t)(x >> 1); nbytes[2] = 1; plane[2] = 2;
    return 3;
}

// ---- the bytes of plane p that hold the samples of frame columns [xa, xb) of frame row y (xa even): offset from the buffer base and count.
//      What the cut kernel stages into LDS; the union of chip_pixel_samples over the columns.  (w is even wherever a sample serves two columns,
//      so rounding xb up to even stays inside the row.)
ZLY_CHIP_HD uint64_t chip_row_bytes(const ChipFrame& f, int p, int32_t y, int32_t xa, int32_t xb, uint32_t* nbytes)
{
    if (p == 0) {
        const int32_t xe = f.fam == ZLY_CHIP_FAM_Y422 ? (xb + 1) & ~1 : xb;
        *nbytes = (uint32_t)(xe - xa) * (uint32_t)f.bpp;
        return f.off[0] + (uint64_t)y * (uint64_t)f.pitch[0] + (uint64_t)xa * (uint64_t)f.bpp;
    }
    if (f.fam == ZLY_CHIP_FAM_NV12) {
        *nbytes = (uint32_t)(((xb + 1) & ~1) - xa);
        return f.off[1] + (uint64_t)(y >> 1) * (uint64_t)f.pitch[1] + (uint64_t)xa;
    }
    *nbytes = (uint32_t)(((xb + 1) >> 1) - (xa >> 1));
    return f.off[p] + (uint64_t)(y >> 1) * (uint64_t)f.pitch[p] + (uint64_t)(xa >> 1);
}

}  // namespace zly
