// planes_device.h -- where a frame's samples lie, for the front kernels' fetches (the BGR fetch, yuv_device.h, letterbox_device.h).
//
// A fetch asks a "plane layout" value for the address of a sample instead of deriving it from w, h itself.  There are two layouts:
//   Planes<false>  include/zly.h's tight frame: no row pitch, the chroma planes right behind the Y plane.  Every address follows from w, h by the
//                  expressions the fetches used to spell out, so the kernels of tight frames compile as they did.
//   Planes<true>   a frame view (zly_frame_view): plane bases and row pitches come from the frame's ViewRec (zly_internal.h), which lies behind the call's
//                  descriptors and is read with two scalar loads per workgroup.  A valid view's planes extend over less than 2^31 bytes, so a sample's
//                  offset from its (uniform, 64-bit) plane base is a 32-bit value: no 64-bit multiply per pixel.
// A packed frame's pixel size (3 bytes for BGR / RGB, 4 for BGRA / RGBA) is an ARGUMENT of the bgr_* members, defaulted to the literal 3: the front kernels'
// instantiations that never meet a 4-byte pixel do not name it and compile to the `* 3` they always were; those that serve the packed family (PK) pass
// pix_bpp(fmt) (yuv_device.h).
// Wide loads (the 4-byte stretch fetch, the 8-byte letterbox taps, the 12-byte quads) are guarded by bgr_end(), the END OF PLANE 0: (h-1)*pitch + bpp*w for a
// view, w*h*bpp for a tight frame.  Inside it they may read row padding or a neighbouring column of the surface -- bytes of the caller's validated buffer --
// which the fetches mask or shift out as they always did with the next pixel's bytes.  The 2-byte NV12 pair and all byte loads lie inside a row.
#pragma once
#include "zly_internal.h"

namespace zly {

template <bool VIEW> struct Planes;

template <> struct Planes<false> {
    const uint8_t* f; int w, h;
    __device__ __forceinline__ size_t bgr_off(int x, int y) const { return ((size_t)y * w + x) * 3; }
    __device__ __forceinline__ size_t bgr_end() const { return (size_t)w * h * 3; }
    __device__ __forceinline__ size_t bgr_off(int x, int y, unsigned int bpp) const { return ((size_t)y * w + x) * bpp; }
    __device__ __forceinline__ size_t bgr_end(unsigned int bpp) const { return (size_t)w * h * bpp; }
    // the letterbox taps' 32-bit forms (requests of that mode are at most ZLY_LETTERBOX_MAX_DIM on a side: at most 4 * 2^28 = 2^30 bytes)
    __device__ __forceinline__ unsigned int bgr_off32(int x, int y) const { return ((unsigned)y * (unsigned)w + (unsigned)x) * 3u; }
    __device__ __forceinline__ unsigned int bgr_end32() const { return (unsigned)w * (unsigned)h * 3u; }
    __device__ __forceinline__ unsigned int bgr_off32(int x, int y, unsigned int bpp) const { return ((unsigned)y * (unsigned)w + (unsigned)x) * bpp; }
    __device__ __forceinline__ unsigned int bgr_end32(unsigned int bpp) const { return (unsigned)w * (unsigned)h * bpp; }
    __device__ __forceinline__ const uint8_t* luma(int x, int y) const { return f + ((size_t)y * w + x); }
    __device__ __forceinline__ size_t ci(int x, int y) const { return (size_t)(y >> 1) * (size_t)(w >> 1) + (size_t)(x >> 1); }     // one chroma sample per 2x2 block
    __device__ __forceinline__ const uint8_t* nv12(int x, int y) const { return f + (size_t)w * h + 2 * ci(x, y); }                 // interleaved U, V
    __device__ __forceinline__ const uint8_t* cu(int x, int y) const { return f + (size_t)w * h + ci(x, y); }
    __device__ __forceinline__ const uint8_t* cv(int x, int y) const { return f + (size_t)w * h + ((size_t)(w >> 1) * (size_t)(h >> 1) + ci(x, y)); }
    __device__ __forceinline__ const uint8_t* y422(int x, int y) const { return f + ((size_t)y * w + (size_t)(x & ~1)) * 2; }        // the 4-byte macropixel of a packed 4:2:2 pixel (w even)
};

template <> struct Planes<true> {
    const uint8_t* f; const uint8_t* p1; const uint8_t* p2;     // first sample of the region in plane 0 / 1 / 2
    unsigned int pitch0, pitch1, pitch2, end0;                  // end0: extent of plane 0 in bytes
    __device__ __forceinline__ unsigned int bgr_off(int x, int y, unsigned int bpp = 3u) const { return (unsigned)y * pitch0 + (unsigned)x * bpp; }
    __device__ __forceinline__ unsigned int bgr_end(unsigned int = 3u) const { return end0; }
    __device__ __forceinline__ unsigned int bgr_off32(int x, int y, unsigned int bpp = 3u) const { return bgr_off(x, y, bpp); }
    __device__ __forceinline__ unsigned int bgr_end32(unsigned int = 3u) const { return end0; }
    __device__ __forceinline__ const uint8_t* luma(int x, int y) const { return f + ((unsigned)y * pitch0 + (unsigned)x); }
    __device__ __forceinline__ const uint8_t* nv12(int x, int y) const { return p1 + ((unsigned)(y >> 1) * pitch1 + ((unsigned)x & ~1u)); }
    __device__ __forceinline__ const uint8_t* cu(int x, int y) const { return p1 + ((unsigned)(y >> 1) * pitch1 + (unsigned)(x >> 1)); }
    __device__ __forceinline__ const uint8_t* cv(int x, int y) const { return p2 + ((unsigned)(y >> 1) * pitch2 + (unsigned)(x >> 1)); }
    __device__ __forceinline__ const uint8_t* y422(int x, int y) const { return f + ((unsigned)y * pitch0 + (((unsigned)x & ~1u) << 1)); }
};

// The layout of frame fi of a call of n frames.  src: the frame's first sample in the source buffer (base + its descriptor's offset).
// fmt: the frame's format.  PK: the instantiation serves the packed RGB / BGRA / RGBA family (otherwise "not BGR" means YUV: one byte per pixel in plane 0).
// Y2: it serves packed 4:2:2 as well (two bytes per pixel).
template <bool VIEW, bool PK = false, bool Y2 = false>
__device__ __forceinline__ Planes<VIEW> frame_planes(const uint8_t* base, const uint8_t* src, const FrameDesc* desc, int n, int fi, const FrameDesc& d, int fmt)
{
    Planes<VIEW> pl;
    if constexpr (VIEW) {
        typedef unsigned int vu32x4 __attribute__((ext_vector_type(4)));
        const vu32x4* q = reinterpret_cast<const vu32x4*>(reinterpret_cast<const ViewRec*>(desc + n) + fi);
        const vu32x4 a = q[0], b = q[1];
        pl.f = src;
        pl.p1 = base + ((unsigned long long)a[0] | ((unsigned long long)a[1] << 32));
        pl.p2 = base + ((unsigned long long)a[2] | ((unsigned long long)a[3] << 32));
        pl.pitch0 = b[0]; pl.pitch1 = b[1]; pl.pitch2 = b[2];
        if constexpr (Y2)
            pl.end0 = (unsigned)(d.h - 1) * pl.pitch0 + (unsigned)d.w * (fmt >= ZLY_PIX_YUY2_BT601 && fmt <= ZLY_PIX_UYVY_BT709 ? 2u :
                                                                         fmt >= ZLY_PIX_NV12_BT601 && fmt <= ZLY_PIX_I420_BT709 ? 1u : fmt == ZLY_PIX_BGRA || fmt == ZLY_PIX_RGBA ? 4u : 3u);
        else
        pl.end0 = (unsigned)(d.h - 1) * pl.pitch0 + (unsigned)d.w * (!PK ? (fmt == ZLY_PIX_BGR ? 3u : 1u) :
                                                                             fmt >= ZLY_PIX_NV12_BT601 && fmt <= ZLY_PIX_I420_BT709 ? 1u : fmt == ZLY_PIX_BGRA || fmt == ZLY_PIX_RGBA ? 4u : 3u);
    } else {
        pl.f = src; pl.w = d.w; pl.h = d.h;
    }
    return pl;
}

}  // namespace zly
