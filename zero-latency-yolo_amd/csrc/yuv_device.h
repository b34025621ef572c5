// yuv_device.h -- the pixel fetch of YUV 4:2:0 frames (ZLY_PIX_NV12_* / ZLY_PIX_I420_*, include/zly.h) for the front kernels.
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

__device__ __forceinline__ bool pix_is_yuv(int fmt) { return fmt != ZLY_PIX_BGR; }

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

}  // namespace zly
