// area_device.h -- the per-axis footprint arithmetic of the area-average resize filter (ZLY_FLAG_AREA, include/zly.h "Area resize"), for the
// pre-pass kernel (kernels_area.hip) and, compiled by a host compiler, for its check without a GPU (tests/cpp/test_area_footprint.cpp).
//
// One axis with source length S and content length D, in units of 1/D of a source pixel: content index d covers [lo, hi) = [d*S, (d+1)*S), source
// index i covers [i*D, (i+1)*D), and the weight of i in d is the length of their overlap.  Everything is an int32: S, D <= ZLY_AREA_MAX_DIM = 2^14,
// so no product exceeds 2^28.  Nothing here includes a HIP header: a plain C++ compiler takes this file as it is.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ZLY_AREA_HD __host__ __device__ inline
#else
#define ZLY_AREA_HD inline
#endif

namespace zly {

// The kernel's shape constants (kernels_area.hip).  tests/test_gpu_area.py parses them from this file: request widths and heights one below, at and
// one above each of them are where the kernel changes path.
#define ZLY_AREA_THREADS    256     // threads per workgroup = most content columns a workgroup owns
#define ZLY_AREA_CHUNK_PX   1020    // source pixels of a row staged into LDS at once (even; 4 bytes each plus 15 of alignment slack = 256 lanes x 16 bytes)
#define ZLY_AREA_BAND_ROWS  16      // model rows per workgroup at large batch ...
#define ZLY_AREA_BAND_SMALL 4       // ... and where the launch would otherwise not fill the chip (small batches)

// the footprint of content index d: source indices i0 .. i1, both inclusive
struct AreaSpan { int lo, hi, i0, i1; };
ZLY_AREA_HD AreaSpan area_span(int S, int D, int d)
{
    AreaSpan a;
    a.lo = d * S;
    a.hi = a.lo + S;
    a.i0 = a.lo / D;
    a.i1 = (a.hi - 1) / D;
    return a;
}

// w(d, i) for i in [i0, i1]: D for interior indices, 1 .. D at the two ends; the weights of one d sum to S
ZLY_AREA_HD int area_weight(const AreaSpan& a, int D, int i)
{
    const int b = i * D, e = b + D;
    return (a.hi < e ? a.hi : e) - (a.lo > b ? a.lo : b);
}

}  // namespace zly
