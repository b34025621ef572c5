// zoom_device.h -- the arithmetic of the zoom regions' plan (include/zly.h "Zoom regions", steps 1-6) and the record a frame's plan is made from, as
// the plan kernel (kernels_zoom.hip), the host twin (zoom_rules.h) and a stand-alone CPU program (tests/cpp/test_zoom_plan.cpp) all compile it: every
// decision about one slot -- is it eligible, where does it stand in the order, is it covered, where does its region go -- is a function of this file,
// and the kernel and the twin differ only in how they walk the slots (ballots and readlane broadcasts there, a loop here).  Nothing here includes a
// HIP header: a plain C++ compiler takes this file as it is.  Every float operation below is one IEEE fp32 operation, in the order written: each
// function that has one turns FP contraction off in its own body (ZLY_ZOOM_NO_CONTRACT: a pragma covers only the text behind it, so one in the
// including file, behind the #include, would not reach these functions); a compiler without the pragma is given -ffp-contract=off (the Makefile).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ZLY_ZOOM_HD __host__ __device__ inline
#else
#define ZLY_ZOOM_HD inline
#endif
#if defined(__clang__)
#define ZLY_ZOOM_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define ZLY_ZOOM_NO_CONTRACT
#endif

namespace zly {

#define ZLY_ZOOM_MAX_REGIONS 15      // K <= 15: with the whole surface, at most 16 views per frame

// What the plan kernel needs of one frame of a call; the host fills it from the surface's (checked) view (zoom_rules.h: zoom_frame_of) and uploads
// it.  view_crop's plane offsets are linear in the origin: plane p of the region at (x0, y0) starts at
//     off[p] + (y0 >> ysh[p]) * pitch[p] + (x0 >> xsh[p]) * xstep[p]
// so the format table stays on the host.  72 bytes.
struct ZoomFrame {
    uint64_t off[3];          // the surface view's plane offsets (planes the format does not have: 0)
    int32_t  pitch[3];
    int32_t  W, H;            // the surface
    int32_t  stream;          // whose track table the plan is made from
    int32_t  fmt;             // ZLY_PIX_*: rides in the top byte of the descriptor's offset
    int32_t  planes;
    uint8_t  xstep[3], xsh[3], ysh[3];
    uint8_t  pad_[7];
};

ZLY_ZOOM_HD uint64_t zoom_plane_off(const ZoomFrame& f, int p, int32_t x0, int32_t y0)
{
    return f.off[p] + (uint64_t)(y0 >> f.ysh[p]) * (uint64_t)f.pitch[p] + (uint64_t)(x0 >> f.xsh[p]) * (uint64_t)f.xstep[p];
}

// step 1: the region's size on a W x H surface and the largest origin
struct ZoomSize { int32_t rw, rh, xmax, ymax; };
ZLY_ZOOM_HD ZoomSize zoom_size(int32_t region_w, int32_t region_h, int32_t W, int32_t H)
{
    ZoomSize z;
    z.rw = region_w < (W & ~1) ? region_w : (W & ~1);
    z.rh = region_h < (H & ~1) ? region_h : (H & ~1);
    z.xmax = (W - z.rw) & ~1;
    z.ymax = (H - z.rh) & ~1;
    return z;
}

// step 6, one axis: the centred window
ZLY_ZOOM_HD int32_t zoom_fallback_origin(int32_t E, int32_t r) { return ((E - r) / 2) & ~1; }

// step 2.  F: the table's frame_no
ZLY_ZOOM_HD bool zoom_eligible(bool live, int32_t cls, uint32_t F, uint32_t last_seen, float w, float h, int32_t W, int32_t H, const ZoomSize& z,
                               int32_t max_age, int32_t class_id)
{
    ZLY_ZOOM_NO_CONTRACT
    if (!live) return false;
    if (class_id != -1 && cls != class_id) return false;
    if (F - last_seen > (uint32_t)max_age) return false;
    return w * (float)W <= (float)z.rw && h * (float)H <= (float)z.rh;
}

// step 3, one axis: the prediction to the coming frame
ZLY_ZOOM_HD float zoom_predict(float x, float v, uint32_t F, uint32_t last_seen)
{
    ZLY_ZOOM_NO_CONTRACT
    const float dtf = (float)(F + 1u - last_seen);
    const float d = v * dtf;
    return x + d;
}

// step 4: the area as a key whose unsigned order is the order of the fp32 values, -0 and +0 tying.  (A NaN area -- w or h infinite against a zero --
// is outside the rule; the key still gives it one place, the same everywhere.)
ZLY_ZOOM_HD uint32_t zoom_area_key(float w, float h)
{
    ZLY_ZOOM_NO_CONTRACT
    float a = w * h;
    if (a == 0.0f) a = 0.0f;
    uint32_t u;
    __builtin_memcpy(&u, &a, 4);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// step 4: does slot a come before slot b?  A strict total order
ZLY_ZOOM_HD bool zoom_before(uint32_t age_a, uint32_t key_a, int slot_a, uint32_t age_b, uint32_t key_b, int slot_b)
{
    if (age_a != age_b) return age_a < age_b;
    if (key_a != key_b) return key_a < key_b;
    return slot_a < slot_b;
}

// step 5, one axis: is the predicted extent [p - s/2, p + s/2] inside the region [o, o + r) of an extent of E pixels?
ZLY_ZOOM_HD bool zoom_covered_axis(float p, float s, int32_t o, int32_t r, int32_t E)
{
    ZLY_ZOOM_NO_CONTRACT
    const float half = s * 0.5f;
    const float lo = p - half, hi = p + half;
    const float a = (float)o / (float)E, b = (float)(o + r) / (float)E;
    return lo >= a && hi <= b;
}

// step 5, one axis: the origin of the region around the prediction p (a NaN goes to 0)
ZLY_ZOOM_HD int32_t zoom_origin(float p, int32_t E, int32_t r, int32_t omax)
{
    ZLY_ZOOM_NO_CONTRACT
    const float pc = p > 0.0f ? (p < 1.0f ? p : 1.0f) : 0.0f;
    const int32_t c = (int32_t)(pc * (float)E);
    int32_t o = c - r / 2;
    o = o < 0 ? 0 : o;
    o = o > omax ? omax : o;
    return o & ~1;
}

}  // namespace zly
