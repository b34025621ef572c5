// change_device.h -- the arithmetic of the change map (include/zly.h "Change map"): which bytes of a frame a thread of the sums pass loads and the luma
// it makes of them, the cells, the ACTIVE and GLOBAL predicates and the window of a peak, as the two kernels (kernels_change.hip), the host twin
// (change_rules.h) and a stand-alone CPU program (tests/cpp/test_change_rules.cpp) all compile it.  Nothing here includes a HIP header: a plain C++
// compiler takes this file as it is.  Everything is integer arithmetic.
#pragma once
#include <stdint.h>
#include "chip_device.h"        // ChipFrame and the format families: the change map reads a frame through the record the chips read it through
#include "zoom_device.h"        // zoom_size: step 6 is zoom step 1

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ZLY_CHG_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define ZLY_CHG_HD inline
#endif
#if defined(__clang__)
#define ZLY_CHG_UNROLL _Pragma("unroll")
#else
#define ZLY_CHG_UNROLL
#endif

namespace zly {

// The sums kernel's shape constants (kernels_change.hip).  tests/test_gpu_change.py parses them from this file: widths and heights one below, at and
// one above each of them are where the kernel changes path.
#define ZLY_CHANGE_THREADS     256    // threads per workgroup: 4 granules across x 64 rows
#define ZLY_CHANGE_TILE_PX     64     // a workgroup sums a tile of 64 x 64 pixels: whole cells of every legal size
#define ZLY_CHANGE_GRANULE_PX  16     // a thread sums 16 pixels of one row: 16-byte loads in every format

#define ZLY_CHANGE_MAX_CELLS   8192   // one workgroup's grid in 32 KB of LDS
#define ZLY_CHANGE_MAX_PEAKS   15
#define ZLY_CHANGE_HDR_BYTES   32     // sizeof(zly_change_header)
#define ZLY_CHANGE_PEAK_BYTES  32     // sizeof(zly_change_peak)
#define ZLY_CHANGE_F_FIRST     1u     // ZLY_CHANGE_FIRST
#define ZLY_CHANGE_F_GLOBAL    2u     // ZLY_CHANGE_GLOBAL

// the properties of a ZLY_PIX_* value the luma needs (change_rules.h asserts them against include/zly.h's numbers)
ZLY_CHG_HD bool change_fmt_709(int32_t fmt) { return fmt == 3 || fmt == 4 || fmt == 12 || fmt == 13; }
ZLY_CHG_HD bool change_fmt_uyvy(int32_t fmt) { return fmt == 11 || fmt == 13; }
ZLY_CHG_HD bool change_fmt_rgb(int32_t fmt) { return fmt == 16 || fmt == 18; }

// ---- step 1 ----
ZLY_CHG_HD uint32_t change_luma(uint32_t b, uint32_t g, uint32_t r) { return (29u * b + 150u * g + 77u * r + 128u) >> 8; }
ZLY_CHG_HD int32_t change_clamp255(int32_t v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
// the luma of a YUV sample: include/zly.h's fixed-point conversion to B, G, R (limited range, 20 fractional bits, floor, clamp), then the above
ZLY_CHG_HD uint32_t change_luma_yuv(uint32_t y, uint32_t u8, uint32_t v8, bool b709)
{
    const int32_t CY = b709 ? 1220945 : 1220542, CVR = b709 ? 1879825 : 1673527, CVG = b709 ? -558796 : -852492;
    const int32_t CUG = b709 ? -223607 : -409993, CUB = b709 ? 2215014 : 2116026;
    const int32_t y16 = (int32_t)y - 16;
    const int32_t yy = (y16 > 0 ? y16 : 0) * CY;
    const int32_t u = (int32_t)u8 - 128, v = (int32_t)v8 - 128;
    const int32_t r = change_clamp255((yy + CVR * v + (1 << 19)) >> 20);
    const int32_t g = change_clamp255((yy + CVG * v + CUG * u + (1 << 19)) >> 20);
    const int32_t b = change_clamp255((yy + CUB * u + (1 << 19)) >> 20);
    return change_luma((uint32_t)b, (uint32_t)g, (uint32_t)r);
}

// ---- the sums pass: a GRANULE is the 16 pixels [x0, x0 + 16) of frame row y, x0 a multiple of 16 below W.  Its samples are fetched with up to four
//      loads of 16 bytes: load k reads o[k] .. o[k] + 16 of the buffer, of which the first need[k] hold samples of the granule's pixels; the rest is
//      row padding, the next row or another plane's bytes and never enters a sum.  A load that would leave the extent of the plane it lies in
//      (change_load_lo, change_load_hi) is made byte by byte, inside it (kernels_change.hip: chg_load16) -- the needed bytes always lie inside.
//      Load k's words are d[4k .. 4k + 3] of the 16 words the sums below take.
struct ChangeLoads {
    int32_t  n, npx;          // loads, and the granule's pixels inside the frame: min(16, W - x0)
    int32_t  planar;          // 0: every load lies in plane 0; 1: load k lies in plane k
    uint64_t o[4];
    uint32_t need[4];
};
ZLY_CHG_HD uint32_t change_need(uint32_t nb, uint32_t k) { return nb > 16u * k ? (nb - 16u * k < 16u ? nb - 16u * k : 16u) : 0u; }
ZLY_CHG_HD ChangeLoads change_granule_loads(const ChipFrame& f, int32_t x0, int32_t y)
{
    ChangeLoads L;
    const int32_t npx = f.W - x0 < ZLY_CHANGE_GRANULE_PX ? f.W - x0 : ZLY_CHANGE_GRANULE_PX;
    L.npx = npx;
    const uint64_t row0 = f.off[0] + (uint64_t)y * (uint64_t)f.pitch[0];
    if (f.fam == ZLY_CHIP_FAM_PACKED || f.fam == ZLY_CHIP_FAM_Y422) {
        // 4:2:2: W is even, so the granule ends with a whole macropixel
        const uint32_t bpp = f.fam == ZLY_CHIP_FAM_Y422 ? 2u : (uint32_t)f.bpp;
        const uint32_t nb = (uint32_t)npx * bpp;
        const uint64_t base = row0 + (uint64_t)x0 * bpp;
        L.n = (int32_t)((nb + 15u) >> 4); L.planar = 0;
        L.o[0] = base; L.o[1] = base + 16u; L.o[2] = base + 32u; L.o[3] = base + 48u;
        L.need[0] = change_need(nb, 0u); L.need[1] = change_need(nb, 1u); L.need[2] = change_need(nb, 2u); L.need[3] = change_need(nb, 3u);
        return L;
    }
    // 4:2:0: W and H are even
    const bool nv12 = f.fam == ZLY_CHIP_FAM_NV12;
    L.n = nv12 ? 2 : 3; L.planar = 1;
    L.o[0] = row0 + (uint64_t)x0; L.need[0] = (uint32_t)npx;
    L.o[1] = f.off[1] + (uint64_t)(y >> 1) * (uint64_t)f.pitch[1] + (uint64_t)(nv12 ? x0 : x0 >> 1);
    L.need[1] = nv12 ? (uint32_t)((npx + 1) & ~1) : (uint32_t)((npx + 1) >> 1);
    L.o[2] = nv12 ? 0u : f.off[2] + (uint64_t)(y >> 1) * (uint64_t)f.pitch[2] + (uint64_t)(x0 >> 1);
    L.need[2] = nv12 ? 0u : (uint32_t)((npx + 1) >> 1);
    L.o[3] = 0u; L.need[3] = 0u;
    return L;
}
// the extent [lo, hi) of the plane load k (a constant where it matters) of L lies in
ZLY_CHG_HD uint64_t change_load_lo(const ChipFrame& f, const ChangeLoads& L, int k) { return L.planar && k < 3 ? f.off[k] : f.off[0]; }
ZLY_CHG_HD uint64_t change_load_hi(const ChipFrame& f, const ChangeLoads& L, int k) { return L.planar && k < 3 ? f.off[k] + f.ext[k] : f.off[0] + f.ext[0]; }

// byte j (a constant once the loops below are unrolled) of the words d
ZLY_CHG_HD uint32_t change_byte(const uint32_t* d, int j) { return (d[j >> 2] >> (8 * (j & 3))) & 0xffu; }

// lo += the luma of the granule's pixels 0..7, hi += of its pixels 8..15, pixels at or beyond npx left out: a cell of 8 pixels takes one half, every
// larger cell both
template <int BPP>
ZLY_CHG_HD void change_sums_packed(const uint32_t* d, int32_t npx, bool rgb, uint32_t& lo, uint32_t& hi)
{
    ZLY_CHG_UNROLL
    for (int i = 0; i < ZLY_CHANGE_GRANULE_PX; ++i) {
        const uint32_t c0 = change_byte(d, i * BPP), c1 = change_byte(d, i * BPP + 1), c2 = change_byte(d, i * BPP + 2);
        const uint32_t Y = rgb ? change_luma(c2, c1, c0) : change_luma(c0, c1, c2);
        const uint32_t v = i < npx ? Y : 0u;
        if (i < 8) lo += v; else hi += v;
    }
}
ZLY_CHG_HD void change_sums_y422(const uint32_t* d, int32_t npx, bool uyvy, bool b709, uint32_t& lo, uint32_t& hi)
{
    ZLY_CHG_UNROLL
    for (int i = 0; i < ZLY_CHANGE_GRANULE_PX; ++i) {
        const int m = (i >> 1) * 4;                                       // the pixel's macropixel: YUY2 Y0 U Y1 V, UYVY U Y0 V Y1
        const uint32_t ya = change_byte(d, m + (i & 1) * 2), yb = change_byte(d, m + 1 + (i & 1) * 2);
        const uint32_t b0 = change_byte(d, m), b1 = change_byte(d, m + 1), b2 = change_byte(d, m + 2), b3 = change_byte(d, m + 3);
        const uint32_t Y = change_luma_yuv(uyvy ? yb : ya, uyvy ? b0 : b1, uyvy ? b2 : b3, b709);
        const uint32_t v = i < npx ? Y : 0u;
        if (i < 8) lo += v; else hi += v;
    }
}
ZLY_CHG_HD void change_sums_yuv420(const uint32_t* d, int32_t npx, bool nv12, bool b709, uint32_t& lo, uint32_t& hi)
{
    ZLY_CHG_UNROLL
    for (int i = 0; i < ZLY_CHANGE_GRANULE_PX; ++i) {
        const uint32_t y = change_byte(d, i);
        const uint32_t u = nv12 ? change_byte(d + 4, i & ~1) : change_byte(d + 4, i >> 1);
        const uint32_t v8 = nv12 ? change_byte(d + 4, (i & ~1) + 1) : change_byte(d + 8, i >> 1);
        const uint32_t Y = change_luma_yuv(y, u, v8, b709);
        const uint32_t v = i < npx ? Y : 0u;
        if (i < 8) lo += v; else hi += v;
    }
}
// the format is uniform per frame, hence per workgroup
ZLY_CHG_HD void change_granule_sums(const ChipFrame& f, const uint32_t* d, int32_t npx, uint32_t& lo, uint32_t& hi)
{
    if (f.fam == ZLY_CHIP_FAM_PACKED) {
        if (f.bpp == 4) change_sums_packed<4>(d, npx, change_fmt_rgb(f.fmt), lo, hi);
        else change_sums_packed<3>(d, npx, change_fmt_rgb(f.fmt), lo, hi);
    } else if (f.fam == ZLY_CHIP_FAM_Y422) change_sums_y422(d, npx, change_fmt_uyvy(f.fmt), change_fmt_709(f.fmt), lo, hi);
    else change_sums_yuv420(d, npx, f.fam == ZLY_CHIP_FAM_NV12, change_fmt_709(f.fmt), lo, hi);
}

// ---- step 2 ----
ZLY_CHG_HD bool change_cell_ok(int32_t C) { return C == 8 || C == 16 || C == 32 || C == 64; }
ZLY_CHG_HD int32_t change_cells_axis(int32_t E, int32_t C) { return (E + C - 1) / C; }
ZLY_CHG_HD uint32_t change_span(int32_t c, int32_t C, int32_t E) { const int32_t a = c * C, b = (c + 1) * C < E ? (c + 1) * C : E; return (uint32_t)(b - a); }
// ---- step 4: A <= 64 * 64 * 255 and threshold_q4 * npix <= 4080 * 4096: both sides fit 32 bits ----
ZLY_CHG_HD uint32_t change_absdiff(uint32_t a, uint32_t b) { return a > b ? a - b : b - a; }
ZLY_CHG_HD bool change_active(uint32_t A, uint32_t threshold_q4, uint32_t npix) { return 16u * A > threshold_q4 * npix; }
// ---- step 5 ----
ZLY_CHG_HD bool change_global(uint32_t n_active, uint32_t max_active_permille, uint32_t n_cells) { return n_active * 1000u > max_active_permille * n_cells; }
// ---- step 6: the centre pixel of cell column (row) c, and the origin of the window around it ----
ZLY_CHG_HD int32_t change_centre(int32_t c, int32_t C, int32_t E) { const int32_t p = c * C + C / 2; return p < E - 1 ? p : E - 1; }
ZLY_CHG_HD int32_t change_origin(int32_t pc, int32_t r, int32_t omax)
{
    int32_t o = pc - r / 2;
    o = o < 0 ? 0 : o;
    o = o > omax ? omax : o;
    return o & ~1;
}
ZLY_CHG_HD bool change_inside(int32_t px, int32_t py, int32_t x0, int32_t y0, int32_t rw, int32_t rh)
{
    return px >= x0 && px < x0 + rw && py >= y0 && py < y0 + rh;
}
// ---- step 7: the order of the live cells as one key: the largest A first, then the lowest index (A >= 1 for a live cell: 0 is "none") ----
ZLY_CHG_HD uint64_t change_key(uint32_t A, uint32_t index) { return ((uint64_t)A << 32) | (uint64_t)(0xffffffffu - index); }
ZLY_CHG_HD uint32_t change_key_index(uint64_t k) { return 0xffffffffu - (uint32_t)k; }
ZLY_CHG_HD uint32_t change_key_value(uint64_t k) { return (uint32_t)(k >> 32); }

// ---- step 8: the record of a stream: header, max_peaks peaks, the activity grid (room for ZLY_CHANGE_MAX_CELLS cells) ----
struct ChangeLayout { uint64_t rec_bytes, peaks_off, activity_off; };
ZLY_CHG_HD ChangeLayout change_layout(int32_t max_peaks)
{
    ChangeLayout l;
    l.peaks_off = ZLY_CHANGE_HDR_BYTES;
    l.activity_off = l.peaks_off + (uint64_t)max_peaks * ZLY_CHANGE_PEAK_BYTES;
    l.rec_bytes = l.activity_off + 4u * (uint64_t)ZLY_CHANGE_MAX_CELLS;
    return l;
}

// what the pick kernel needs of one frame of a call, and what a stream keeps between its frames (its grid of sums lies in an array of its own)
struct ChangeItem   { int32_t W, H, stream, pad_; };
struct ChangeStream { int32_t W, H, C, have_prev; uint32_t step; uint32_t pad_[3]; };

}  // namespace zly
