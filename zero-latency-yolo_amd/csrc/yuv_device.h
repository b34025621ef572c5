// yuv_device.h -- the pixel fetch of YUV 4:2:0 frames (ZLY_PIX_NV12_* / ZLY_PIX_I420_*, include/zly.h) and of packed 4:2:2 frames (ZLY_PIX_YUY2_* /
// ZLY_PIX_UYVY_*) for the front kernels.
//
// A YUV frame's source pixel (sx, sy) -- picked by the unchanged nearest-neighbour map -- becomes the same packed B | G<<8 | R<<16 word the
// BGR fetch yields, so everything behind the fetch (/255, BGR->RGB, bf16 rounding) is the BGR path's: a YUV frame gives exactly what its
// integer BGR conversion gives as a BGR frame.  The conversion is include/zly.h's fixed-point formula (limited range, 20 fractional bits):
// int32 only, the three products on the 24-bit multiplier (the front kernels are VALU-bound), arithmetic shifts (floor), clamp to [0, 255].
// Split into an issue half (the byte loads) and a convert half, so that a kernel can have all its loads in flight before it converts.
#pragma once
#include "zly_internal.h"
#include "planes_device.h"

namespace zly {

// The formats a format-aware front kernel meets (include/zly.h): BGR, the four YUV 4:2:0 layouts, and the packed family RGB / BGRA / RGBA, whose
// fetch is the BGR fetch with the frame's own pixel size and, for the two R-first layouts, bytes 0 and 2 of the fetched word exchanged.  All of
// them are uniform per frame, hence per wave.
// The front kernels come in three format levels: BGR only (YUV = false), BGR + YUV (YUV = true: the kernels as they were before the packed family
// existed -- a batch without a packed frame runs them, and they compile to the same code as ever), and every format (YUV = true, PK = true:
// kernels_pix.hip, kernels_pix_view.hip).  Only a PK instantiation ever meets a packed frame, so only there "is YUV" differs from "is not BGR".
__device__ __forceinline__ bool pix_is_yuv(int fmt) { return fmt >= ZLY_PIX_NV12_BT601 && fmt <= ZLY_PIX_I420_BT709; }
__device__ __forceinline__ bool pix_not_bgr(int fmt) { return fmt != ZLY_PIX_BGR; }          // the frame needs a format-aware fetch (the host's flag says the same of the batch)
template <bool PK> __device__ __forceinline__ bool pix_yuv_frame(int fmt) { if constexpr (PK) return pix_is_yuv(fmt); else return pix_not_bgr(fmt); }
__device__ __forceinline__ unsigned int pix_bpp(int fmt) { return fmt == ZLY_PIX_BGRA || fmt == ZLY_PIX_RGBA ? 4u : 3u; }        // bytes per pixel of a packed format
__device__ __forceinline__ bool pix_is_rgb_order(int fmt) { return fmt == ZLY_PIX_RGB || fmt == ZLY_PIX_RGBA; }
// R | G<<8 | B<<16 | X<<24  ->  B | G<<8 | R<<16 | 0: one v_perm_b32 (selector bytes, low to high: source byte 2, 1, 0, constant 0)
#define ZLY_PERM_SWAP_RB 0x0c000102u
#define ZLY_PERM_KEEP_BGR 0x0c020100u        // the same word with byte 3 cleared: the B-first formats' selector where one permute serves every packed format
__device__ __forceinline__ unsigned int pix_swap_rb(unsigned int v) { return __builtin_amdgcn_perm(0u, v, ZLY_PERM_SWAP_RB); }
// a packed pixel's offset in plane 0 and that plane's end (planes_device.h): with the frame's own pixel size in an instantiation that serves the packed
// family (PK), with the literal 3 in every other
template <bool PK, class PL> __device__ __forceinline__ auto pix_off(const PL& pl, int fmt, int x, int y)
{
    if constexpr (PK) return pl.bgr_off(x, y, pix_bpp(fmt)); else return pl.bgr_off(x, y);
}
template <bool PK, class PL> __device__ __forceinline__ auto pix_end(const PL& pl, int fmt)
{
    if constexpr (PK) return pl.bgr_end(pix_bpp(fmt)); else return pl.bgr_end();
}

// loads of one pixel of the YUV frame whose planes pl lays out (planes_device.h: a tight frame or a frame view): y = Y byte, uv = U | V << 8
template <class PL>
__device__ __forceinline__ void yuv_issue(const PL& pl, int fmt, int sx, int sy, unsigned int& y, unsigned int& uv)
{
    y = *pl.luma(sx, sy);
    if (fmt == ZLY_PIX_NV12_BT601 || fmt == ZLY_PIX_NV12_BT709) {
        unsigned short p;
        __builtin_memcpy(&p, pl.nv12(sx, sy), 2);                                   // interleaved U, V: one 2-byte load (inside the row: it needs no guard)
        uv = p;
    } else {
        uv = (unsigned int)*pl.cu(sx, sy) | ((unsigned int)*pl.cv(sx, sy) << 8);
    }
}

// ---- packed 4:2:2 (YUY2: Y0 U Y1 V, UYVY: U Y0 V Y1; only the ZLY_FRONT_YUV422 instantiations, kernels_y422.hip / kernels_y422_view.hip, meet one) ----
// The issue half is ONE (unaligned) 4-byte load of the pixel's macropixel, which lies wholly inside its row: no end-of-plane guard.  The convert half
// picks Y, U, V out of it with one v_perm_b32 -- selector bytes, low to high: the pixel's Y, U, V, constant 0; wave-uniform per frame but for the
// Y index, which follows the column's parity -- and hands the same (y, u | v << 8) pair to yuv_bgr_word.
__device__ __forceinline__ bool pix_is_y422(int fmt) { return fmt >= ZLY_PIX_YUY2_BT601 && fmt <= ZLY_PIX_UYVY_BT709; }
__device__ __forceinline__ bool pix_is_uyvy(int fmt) { return fmt == ZLY_PIX_UYVY_BT601 || fmt == ZLY_PIX_UYVY_BT709; }
#define ZLY_PERM_YUY2 0x0c030100u        // Y0 U V 0 of the word Y0 | U<<8 | Y1<<16 | V<<24; + 2: Y1 in place of Y0
#define ZLY_PERM_UYVY 0x0c020001u        // Y0 U V 0 of the word U | Y0<<8 | V<<16 | Y1<<24; + 2: Y1 in place of Y0
// the selector of column sx of a frame of format fmt
__device__ __forceinline__ unsigned int y422_sel(int fmt, int sx) { return (pix_is_uyvy(fmt) ? ZLY_PERM_UYVY : ZLY_PERM_YUY2) + (((unsigned int)sx & 1u) << 1); }
// the load of one pixel: m = its macropixel
template <class PL>
__device__ __forceinline__ void y422_issue(const PL& pl, int sx, int sy, unsigned int& m)
{
    __builtin_memcpy(&m, pl.y422(sx, sy), 4);          // (amdhsa: unaligned global access is enabled)
}
// macropixel, selector -> Y | U << 8 | V << 16
__device__ __forceinline__ unsigned int y422_yuv_word(unsigned int m, unsigned int sel) { return __builtin_amdgcn_perm(0u, m, sel); }
// the 4:2:0 format whose matrix a 4:2:2 format shares: the 601 / 709 choice of yuv_bgr_word
__device__ __forceinline__ int y422_matrix(int fmt) { return fmt >= ZLY_PIX_YUY2_BT709 ? ZLY_PIX_NV12_BT709 : ZLY_PIX_NV12_BT601; }

// Y, U | V << 8 -> B | G << 8 | R << 16
__device__ __forceinline__ unsigned int yuv_bgr_word(unsigned int y, unsigned int uv, int fmt)
{
    const bool b709 = fmt == ZLY_PIX_NV12_BT709 || fmt == ZLY_PIX_I420_BT709;
    const int CY = b709 ? 1220945 : 1220542, CVR = b709 ? 1879825 : 1673527, CVG = b709 ? -558796 : -852492;
    const int CUG = b709 ? -223607 : -409993, CUB = b709 ? 2215014 : 2116026;
    const int yy = __mul24(max((int)y - 16, 0), CY);
    const int u = (int)(uv & 0xffu) - 128, v = (int)(uv >> 8) - 128;
    const int r = min(max((yy + __mul24(CVR, v) + (1 << 19)) >> 20, 0), 255);
    const int g = min(max((yy + __mul24(CVG, v) + __mul24(CUG, u) + (1 << 19)) >> 20, 0), 255);
    const int b = min(max((yy + __mul24(CUB, u) + (1 << 19)) >> 20, 0), 255);
    return (unsigned int)b | ((unsigned int)g << 8) | ((unsigned int)r << 16);
}

// macropixel, selector -> B | G << 8 | R << 16
__device__ __forceinline__ unsigned int y422_bgr_word(unsigned int m, unsigned int sel, int fmt)
{
    const unsigned int yuv = y422_yuv_word(m, sel);
    return yuv_bgr_word(yuv & 0xffu, yuv >> 8, y422_matrix(fmt));
}

}  // namespace zly
