// camera_device.h -- the arithmetic of the camera motion estimate (include/zly.h "Camera motion"): the window, the order of the candidates, the
// sub-cell fit, the shift, the LOST predicate, the record's layout and the shift of step A, as the kernels (kernels_camera.hip), the host twin
// (camera_rules.h) and a stand-alone CPU program (tests/cpp/test_camera_rules.cpp) all compile it.  Nothing here includes a HIP header: a plain C++
// compiler takes this file as it is.  Everything is integer arithmetic except camera_norm, whose two fp32 operations are kept apart.
#pragma once
#include <stdint.h>
#include "change_device.h"      // the grid is the change map's: change_cells_axis, change_absdiff, ZLY_CHANGE_MAX_CELLS

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ZLY_CAM_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define ZLY_CAM_HD inline
#endif

namespace zly {

#define ZLY_CAMERA_THREADS   256    // threads per workgroup of the search and pick kernels
#define ZLY_CAMERA_R_MAX     8      // ZLY_CAMERA_MAX_RADIUS
#define ZLY_CAMERA_SIDE_MAX  17     // 2 * R_MAX + 1 candidates per axis
#define ZLY_CAMERA_HDR       96     // ZLY_CAMERA_HDR_BYTES
#define ZLY_CAMERA_F_FIRST   1u
#define ZLY_CAMERA_F_LOST    2u
#define ZLY_CAMERA_F_CLIPPED 4u

ZLY_CAM_HD bool camera_radius_ok(int32_t R) { return R >= 1 && R <= ZLY_CAMERA_R_MAX; }
// step 1: the grid holds a window at every candidate
ZLY_CAM_HD bool camera_grid_ok(int32_t gw, int32_t gh, int32_t R) { return gw >= 2 * R + 1 && gh >= 2 * R + 1; }
ZLY_CAM_HD int32_t camera_abs(int32_t v) { return v < 0 ? -v : v; }

// ---- step 4: the order of the candidates.  A candidate is its SAD and its RANK, (|dx| + |dy|, dy, dx) as one integer; less(a, b): a comes first ----
ZLY_CAM_HD uint32_t camera_rank(int32_t dx, int32_t dy, int32_t R)
{
    return ((uint32_t)(camera_abs(dx) + camera_abs(dy)) << 16) | ((uint32_t)(dy + R) << 8) | (uint32_t)(dx + R);
}
ZLY_CAM_HD int32_t camera_rank_dx(uint32_t rank, int32_t R) { return (int32_t)(rank & 0xffu) - R; }
ZLY_CAM_HD int32_t camera_rank_dy(uint32_t rank, int32_t R) { return (int32_t)((rank >> 8) & 0xffu) - R; }
ZLY_CAM_HD bool camera_less(uint64_t sad_a, uint32_t rank_a, uint64_t sad_b, uint32_t rank_b) { return sad_a < sad_b || (sad_a == sad_b && rank_a < rank_b); }
// the table's entry of (dx, dy)
ZLY_CAM_HD int32_t camera_entry(int32_t dx, int32_t dy, int32_t R) { return (dy + R) * (2 * R + 1) + (dx + R); }

// ---- step 5: the sub-cell part of one axis, sixteenths of a cell.  d: the best displacement on the axis; s0 the minimum, sm and sp the SADs at
//      d - 1 and d + 1 (not read where |d| = R: pass anything) ----
ZLY_CAM_HD int32_t camera_fit(int32_t d, int32_t R, uint64_t s0, uint64_t sm, uint64_t sp)
{
    if (camera_abs(d) == R) return 0;
    const uint64_t hi = sm > sp ? sm : sp;
    if (s0 == 0u || hi == s0) return 0;
    const uint64_t num = 16u * (sm > sp ? sm - sp : sp - sm), den = 2u * (hi - s0);     // hi > s0: s0 is the minimum
    const uint64_t q = num / den;
    const int32_t f = q < 8u ? (int32_t)q : 8;
    return sm >= sp ? f : -f;
}
// ---- step 6 ----
ZLY_CAM_HD int32_t camera_shift_q4(int32_t d, int32_t f, int32_t C) { return (16 * d + f) * C; }
// ---- step 7: SAD <= 255 * npix and npix <= 8192 * 4096: both sides fit 64 bits ----
ZLY_CAM_HD uint64_t camera_npix(int32_t gw, int32_t gh, int32_t R, int32_t C) { return (uint64_t)(gw - 2 * R) * (uint64_t)(gh - 2 * R) * (uint64_t)(C * C); }
ZLY_CAM_HD bool camera_lost(uint64_t sad_min, uint32_t max_residual_q4, uint64_t npix) { return 16u * sad_min > (uint64_t)max_residual_q4 * npix; }

// ---- step A: the shift as a fraction of the extent E (W or H): one conversion rounded to nearest even, one division.  Units that compile this
//      switch contraction off; there is nothing to contract in it, and the kernel's unit says so all the same ----
ZLY_CAM_HD float camera_norm(int64_t pend_q4, int32_t E)
{
    const float p = (float)pend_q4, d = (float)(16 * E);
    return p / d;
}

// ---- step 9: the record of a stream: header, then the SAD table (room for 17 x 17 entries) ----
struct CameraLayout { uint64_t rec_bytes, sad_off, sad_room; };
ZLY_CAM_HD CameraLayout camera_layout()
{
    CameraLayout l;
    l.sad_off = ZLY_CAMERA_HDR;
    l.sad_room = (uint64_t)ZLY_CAMERA_SIDE_MAX * ZLY_CAMERA_SIDE_MAX;
    l.rec_bytes = l.sad_off + 8u * l.sad_room;
    return l;
}

// what the kernels need of one frame of a call, and what a stream keeps between its frames beside its record (the pending shift and the two
// counters live in the record itself) and its grid of sums (an array of its own)
struct CameraItem   { int32_t W, H, stream, pad_; };
struct CameraStream { int32_t W, H, C, have_prev; uint32_t step; uint32_t pad_[3]; };
ZLY_CAM_HD bool camera_first(const CameraStream& st, int32_t W, int32_t H, int32_t C) { return !st.have_prev || st.W != W || st.H != H || st.C != C; }

}  // namespace zly
