// letterbox_device.h -- the pixel fetch of the letterbox resize mode (ZLY_FLAG_LETTERBOX, include/zly.h) for the front kernels, and the geometry the
// decode needs to map boxes back.
//
// A model pixel (x, y) of a letterbox engine is either padding -- the packed word of three 114 bytes -- or the bilinear blend of four source pixels
// of the request frame, in include/zly.h's integer arithmetic (16.16 coordinates, 8-bit weights, int32).  Either way it is the same packed
// B | G<<8 | R<<16 word the stretch fetch yields, so everything behind the fetch (/255, BGR->RGB, bf16 rounding) is the stretch path's.
// Everything that is uniform per frame (content size, padding, the two steps) is computed once per workgroup from the frame descriptor: the
// descriptor comes from a scalar load, so those values and the three divides stay out of the per-pixel code.
// Split into an issue half (the loads) and a blend half, as yuv_device.h is, so that a kernel can have its loads in flight before it blends.
#pragma once
#include "zly_internal.h"
#include "yuv_device.h"

namespace zly {

#define ZLY_LB_PAD_WORD 0x00727272u          // 114, 114, 114

// include/zly.h "Geometry".  Requests are at most ZLY_LETTERBOX_MAX_DIM on a side in this mode and so is the model (engine.cpp checks both), which keeps
// the products below 2^30: 32-bit divides on the device.
struct LbGeom { int nw, nh, pad_x, pad_y; };
__device__ __forceinline__ LbGeom lb_geometry(int w, int h, int tw, int th)
{
    LbGeom g;
    if ((unsigned)tw * (unsigned)h <= (unsigned)th * (unsigned)w) {
        g.nw = tw;
        g.nh = max(1, (int)((2u * (unsigned)h * (unsigned)tw + (unsigned)w) / (2u * (unsigned)w)));
    } else {
        g.nh = th;
        g.nw = max(1, (int)((2u * (unsigned)w * (unsigned)th + (unsigned)h) / (2u * (unsigned)h)));
    }
    g.pad_x = (tw - g.nw) >> 1;
    g.pad_y = (th - g.nh) >> 1;
    return g;
}

// one frame's resize, uniform across its workgroups
struct LbFrame {
    int nw, nh, pad_x, pad_y;
    int step_x, step_y;                      // 16.16 source pixels per content pixel
    int w, h;
};
__device__ __forceinline__ LbFrame lb_frame(int w, int h, int tw, int th)
{
    const LbGeom g = lb_geometry(w, h, tw, th);
    LbFrame f;
    f.nw = g.nw; f.nh = g.nh; f.pad_x = g.pad_x; f.pad_y = g.pad_y; f.w = w; f.h = h;
    f.step_x = (int)((((unsigned)w << 16) + ((unsigned)g.nw >> 1)) / (unsigned)g.nw);
    f.step_y = (int)((((unsigned)h << 16) + ((unsigned)g.nh >> 1)) / (unsigned)g.nh);
    return f;
}

// include/zly.h "Sampling", one axis: content index d -> first tap i0 and the weight a (0..255) of the second
__device__ __forceinline__ void lb_coord(int d, int step, int S, int& i0, int& a)
{
    int s = d * step + (step >> 1) - 32768;
    s = min(max(s, 0), (S - 1) << 16);
    i0 = s >> 16;
    a = (s >> 8) & 255;
}

// The loads of one model pixel.  m = LB_PAD: padding, nothing was loaded; else m = ax | ay << 16 and t[] holds the taps:
//   BGR, RGB: t[0], t[1] = 8 bytes from (xl, y0): B G R B' | G' R' . .   t[2], t[3] = the same from (xl, y1)
//   BGRA, RGBA: t[0], t[1] = 8 bytes from (xl, y0): B G R X | B' G' R' X' -- the two dwords ARE the two taps --   t[2], t[3] = the same from (xl, y1)
//   YUV: t[0..3] = the four taps p00, p01, p10, p11 as Y | U << 8 | V << 16
//   packed 4:2:2: t[0..3] = the MACROPIXELS of the four taps (xl and xl + 1 share one when xl is even and straddle two when it is odd: a dword load per
//   tap either way, each inside its row), and bit LB_Y422_ODD of m = xl's parity, from which lb_blend makes the taps' byte selectors
// The second column is always xl + 1: where the reference's x1 = min(x0 + 1, w - 1) is x0 itself (the last column), its weight ax is 0, so the fetch
// steps one column back (xl = w - 2) and gives the SECOND tap the whole weight (ax = 256) -- the same products.  One (unaligned) 8-byte load per row
// then covers both taps of a packed frame.  The R-first formats (RGB, RGBA) are loaded like their B-first twins; lb_blend exchanges the lanes.
#define LB_PAD (-1)
#define LB_Y422_ODD 30
struct LbTaps { unsigned int t[4]; int m; };

__device__ __forceinline__ bool lb_is_pad(const LbFrame& f, int ix, int iy)
{
    return (unsigned)(ix - f.pad_x) >= (unsigned)f.nw || (unsigned)(iy - f.pad_y) >= (unsigned)f.nh;
}

template <bool YUV, bool PK = false, bool Y2 = false, class PL>
__device__ __forceinline__ void lb_issue(const PL& pl, int fmt, const LbFrame& f, int ix, int iy, LbTaps& o)
{
    o.m = LB_PAD;
    o.t[0] = o.t[1] = o.t[2] = o.t[3] = 0u;
    if (lb_is_pad(f, ix, iy)) return;
    int x0, ax, y0, ay;
    lb_coord(ix - f.pad_x, f.step_x, f.w, x0, ax);
    lb_coord(iy - f.pad_y, f.step_y, f.h, y0, ay);
    const int y1 = min(y0 + 1, f.h - 1);
    const int xl = min(x0, max(f.w - 2, 0));
    if (x0 > xl) ax = 256;
    o.m = ax | (ay << 16);
    if constexpr (Y2) {
        if (pix_is_y422(fmt)) {                         // uniform per frame; 4:2:2 frames are at least 2 wide: xl + 1 is a column
            o.m |= (xl & 1) << LB_Y422_ODD;
            y422_issue(pl, xl, y0, o.t[0]); y422_issue(pl, xl + 1, y0, o.t[1]);
            y422_issue(pl, xl, y1, o.t[2]); y422_issue(pl, xl + 1, y1, o.t[3]);
            return;
        }
    }
    if (YUV && pix_yuv_frame<PK>(fmt)) {                // uniform per frame; YUV frames are at least 2 x 2
        unsigned int y, uv;
        yuv_issue(pl, fmt, xl, y0, y, uv);         o.t[0] = y | (uv << 8);
        yuv_issue(pl, fmt, xl + 1, y0, y, uv); o.t[1] = y | (uv << 8);
        yuv_issue(pl, fmt, xl, y1, y, uv);         o.t[2] = y | (uv << 8);
        yuv_issue(pl, fmt, xl + 1, y1, y, uv); o.t[3] = y | (uv << 8);
        return;
    }
    // 32-bit byte offsets from the frame's (uniform) base: a frame of this mode is at most ZLY_LETTERBOX_MAX_DIM on a side, 3 * 2^28 bytes -- 4 * 2^28 = 2^30
    // with four bytes per pixel, still below 2^31 (a view's plane extends over less than 2^31); the bound of the 8-byte loads is the end of the plane
    // (planes_device.h)
    const uint8_t* src = pl.f;
    unsigned int frame_bytes, off0, off1;
    if constexpr (PK) {
        const unsigned int bpp = pix_bpp(fmt);
        frame_bytes = pl.bgr_end32(bpp); off0 = pl.bgr_off32(xl, y0, bpp); off1 = pl.bgr_off32(xl, y1, bpp);
    } else {
        frame_bytes = pl.bgr_end32(); off0 = pl.bgr_off32(xl, y0); off1 = pl.bgr_off32(xl, y1);
    }
    typedef unsigned int u32x2 __attribute__((ext_vector_type(2), aligned(1)));
    if (off1 + 8 <= frame_bytes) {                      // off0 <= off1
        const u32x2 r0 = *reinterpret_cast<const u32x2*>(src + off0);        // (amdhsa: unaligned global access is enabled)
        const u32x2 r1 = *reinterpret_cast<const u32x2*>(src + off1);
        o.t[0] = r0[0]; o.t[1] = r0[1]; o.t[2] = r1[0]; o.t[3] = r1[1];
    } else if (PK && pix_bpp(fmt) == 4u) {
        // the last pixel of a one-column BGRA / RGBA frame: two dword loads, the second column clamped into the row (w == 1: its weight is 0)
        const unsigned int dx = f.w > 1 ? 4u : 0u;
        __builtin_memcpy(&o.t[0], src + off0, 4); __builtin_memcpy(&o.t[1], src + off0 + dx, 4);
        __builtin_memcpy(&o.t[2], src + off1, 4); __builtin_memcpy(&o.t[3], src + off1 + dx, 4);
    } else {
        // the last pixels of a frame: an 8-byte load would read past it.  Byte loads, the second column clamped into the row (w == 1: its weight is 0)
        const int dx = f.w > 1 ? 3 : 0;
        const uint8_t* q0 = src + off0;
        const uint8_t* q1 = src + off1;
        o.t[0] = (unsigned)q0[0] | ((unsigned)q0[1] << 8) | ((unsigned)q0[2] << 16) | ((unsigned)q0[dx] << 24);
        o.t[1] = (unsigned)q0[dx + 1] | ((unsigned)q0[dx + 2] << 8);
        o.t[2] = (unsigned)q1[0] | ((unsigned)q1[1] << 8) | ((unsigned)q1[2] << 16) | ((unsigned)q1[dx] << 24);
        o.t[3] = (unsigned)q1[dx + 1] | ((unsigned)q1[dx + 2] << 8);
    }
}

// taps -> B | G << 8 | R << 16 (include/zly.h "Sampling": the four products per channel, + 32768, >> 16)
template <bool YUV, bool PK = false, bool Y2 = false>
__device__ __forceinline__ unsigned int lb_blend(const LbTaps& o, int fmt)
{
    if (o.m == LB_PAD) return ZLY_LB_PAD_WORD;
    const int ax = o.m & 0xffff, ay = Y2 ? (o.m >> 16) & 0x1ff : o.m >> 16;
    const int w00 = __mul24(256 - ax, 256 - ay), w01 = __mul24(ax, 256 - ay), w10 = __mul24(256 - ax, ay), w11 = __mul24(ax, ay);
    unsigned int p00, p01, p10, p11;                     // B | G << 8 | R << 16 (| junk << 24)
    if (Y2 && pix_is_y422(fmt)) {
        const int odd = (o.m >> LB_Y422_ODD) & 1;
        const unsigned int s0 = y422_sel(fmt, odd), s1 = y422_sel(fmt, odd ^ 1);        // columns xl and xl + 1
        p00 = y422_bgr_word(o.t[0], s0, fmt); p01 = y422_bgr_word(o.t[1], s1, fmt);
        p10 = y422_bgr_word(o.t[2], s0, fmt); p11 = y422_bgr_word(o.t[3], s1, fmt);
    } else
    if (YUV && pix_yuv_frame<PK>(fmt)) {
        p00 = yuv_bgr_word(o.t[0] & 0xffu, o.t[0] >> 8, fmt); p01 = yuv_bgr_word(o.t[1] & 0xffu, o.t[1] >> 8, fmt);
        p10 = yuv_bgr_word(o.t[2] & 0xffu, o.t[2] >> 8, fmt); p11 = yuv_bgr_word(o.t[3] & 0xffu, o.t[3] >> 8, fmt);
    } else if (PK && pix_bpp(fmt) == 4u) {              // BGRA / RGBA: a dword per tap
        p00 = o.t[0]; p01 = o.t[1]; p10 = o.t[2]; p11 = o.t[3];
    } else {
        p00 = o.t[0]; p01 = __builtin_amdgcn_alignbyte(o.t[1], o.t[0], 3);
        p10 = o.t[2]; p11 = __builtin_amdgcn_alignbyte(o.t[3], o.t[2], 3);
    }
    unsigned int px = 0u;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int sh = 8 * c;
        const int v = (__mul24((int)((p00 >> sh) & 0xffu), w00) + __mul24((int)((p01 >> sh) & 0xffu), w01) +
                       __mul24((int)((p10 >> sh) & 0xffu), w10) + __mul24((int)((p11 >> sh) & 0xffu), w11) + 32768) >> 16;
        px |= (unsigned int)v << sh;
    }
    // the blend is the same arithmetic on each byte lane, so an R-first frame is blended as it lies and lanes 0 and 2 of the RESULT are exchanged: one
    // permute per pixel instead of one per tap (the pad word is grey on all three lanes and needs none)
    if (PK && pix_is_rgb_order(fmt)) px = pix_swap_rb(px);
    return px;
}

}  // namespace zly
