// surface_device.h -- what the patch and move kernels of the resident surfaces (kernels_surface.hip; include/zly.h "Resident surfaces") and the host that
// feeds them (surface_rules.h) agree on: the shape constants, the band records, and the kernels' index arithmetic -- which bytes of a row a lane owns and
// how wide its stores are -- so that a host compiler can walk a band table exactly as the kernel does (tests/cpp/test_surface_rules.cpp, test_surface_moves.cpp).  Nothing
// here includes a HIP header: a plain C++ compiler takes this file as it is.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ZLY_SURFACE_HD __host__ __device__ inline
#else
#define ZLY_SURFACE_HD inline
#endif

namespace zly {

// The kernel's shape constants.  tests/test_gpu_surface.py parses them from this file: rectangle heights one below, at and one above a band's rows are
// where a job gets another band.
#define ZLY_SURFACE_THREADS     256      // threads per workgroup: 256 lanes x 16 bytes = 4 KiB per pass over a band
#define ZLY_SURFACE_BAND_BYTES  16384    // most bytes of a band of more than one row: a band is max(1, ZLY_SURFACE_BAND_BYTES / row_bytes) whole rows

// One band: `rows` rows of `row_bytes` bytes, tight at src_off in the staging buffer (row r at src_off + r * row_bytes), to dst_off + r * pitch in the
// store.  A JOB -- one plane of one rectangle -- is the same record before it is cut into bands.  32 bytes, 16-byte aligned on the device: two loads.
struct SurfaceJob {
    uint64_t src_off;       // from the staging buffer's base
    uint64_t dst_off;       // from the store's base
    uint32_t row_bytes;     // 1 .. 2^31 - 1
    uint32_t rows;          // >= 1
    uint32_t pitch;         // bytes from one destination row to the next (the surface's tight row of this plane)
    uint32_t pad_;
};

// A row of n bytes whose first byte goes to byte offset drow of the (16-byte aligned) store is cut at the DESTINATION's 16-byte granules.
// The most granules such a row touches: ceil((15 + n) / 16).
ZLY_SURFACE_HD uint32_t surface_row_granules(uint32_t n) { return (n + 30u) >> 4; }

// Granule g of the row holds the row's bytes [lo, hi): [16g - lead, 16g - lead + 16) with lead = drow & 15, clipped to [0, n).  False: the row ends
// before this granule.  hi - lo == 16 exactly when nothing was clipped, and then drow + lo is a multiple of 16.
ZLY_SURFACE_HD bool surface_granule(uint64_t drow, uint32_t n, uint32_t g, uint32_t* lo, uint32_t* hi)
{
    const int64_t lead = (int64_t)(drow & 15u);
    int64_t a = 16 * (int64_t)g - lead, b = a + 16;
    if (a < 0) a = 0;
    if (b > (int64_t)n) b = (int64_t)n;
    if (a >= b) return false;
    *lo = (uint32_t)a; *hi = (uint32_t)b;
    return true;
}

// A clipped granule (k = 1 .. 15 bytes at destination address low bits `addr`) goes out in the widest naturally aligned stores that stay inside it:
// the width of the next one, 8, 4, 2 or 1.
ZLY_SURFACE_HD uint32_t surface_edge_width(uint32_t addr, uint32_t k)
{
    uint32_t wd = addr & (0u - addr);       // the largest power of two that divides the address (0: a multiple of 2^32)
    if (wd == 0u || wd > 8u) wd = 8u;
    while (wd > k) wd >>= 1;
    return wd;
}

// ---- moves (zly_surface_move; kernels_surface.hip: surface_move_kernel) ----
// One band of a move: `rows` rows of `row_bytes` bytes from src_off + r * src_pitch in the STORE to dst_off + r * dst_pitch.  The destination is the
// store, or -- ZLY_SURFACE_MOVE_TO_BOUNCE set in dst_off -- the bounce buffer: a store has at most 2^56 bytes (ZLY_SURFACE_STORE_MAX), so bit 63 of
// an offset is free.  A move's JOB -- one plane of one move -- is the same record before it is cut into bands.  32 bytes, as SurfaceJob.
#define ZLY_SURFACE_MOVE_TO_BOUNCE (1ull << 63)
struct SurfaceMoveBand {
    uint64_t src_off;       // from the store's base
    uint64_t dst_off;       // from the store's base, or | ZLY_SURFACE_MOVE_TO_BOUNCE: from the bounce buffer's
    uint32_t row_bytes;     // 1 .. 2^31 - 1
    uint32_t rows;          // >= 1
    uint32_t src_pitch;     // bytes from one source row to the next
    uint32_t dst_pitch;     // ... and from one destination row to the next (the bounce buffer's rows are tight: row_bytes)
};

ZLY_SURFACE_HD bool surface_move_to_bounce(const SurfaceMoveBand& b) { return (b.dst_off & ZLY_SURFACE_MOVE_TO_BOUNCE) != 0; }
ZLY_SURFACE_HD uint64_t surface_move_dst(const SurfaceMoveBand& b) { return b.dst_off & ~ZLY_SURFACE_MOVE_TO_BOUNCE; }

// Item i of a band of `rows` rows of G granules each (i < rows * G) is granule *g of row *r.  A band of more than one row holds at most
// ZLY_SURFACE_BAND_BYTES bytes, hence at most 2 * ZLY_SURFACE_BAND_BYTES items: the division is one of 32 bits.  A band of one row may be very long.
ZLY_SURFACE_HD void surface_band_item(uint32_t rows, uint32_t G, uint64_t i, uint32_t* r, uint32_t* g)
{
    if (rows == 1u) { *r = 0u; *g = (uint32_t)i; }
    else { *r = (uint32_t)i / G; *g = (uint32_t)i - *r * G; }
}

// Where item (r, g) of a move's band reads and writes: bytes [lo, hi) of row r, from *src (an offset into the store) to *dst (an offset into the
// band's destination buffer).  False: the row ends before this granule.  The cut is surface_granule's, at the DESTINATION's granules.
ZLY_SURFACE_HD bool surface_move_item(const SurfaceMoveBand& b, uint32_t r, uint32_t g, uint64_t* src, uint64_t* dst, uint32_t* k)
{
    const uint64_t drow = surface_move_dst(b) + (uint64_t)r * b.dst_pitch;
    uint32_t lo, hi;
    if (!surface_granule(drow, b.row_bytes, g, &lo, &hi)) return false;
    *src = b.src_off + (uint64_t)r * b.src_pitch + lo;
    *dst = drow + lo;
    *k = hi - lo;
    return true;
}

}  // namespace zly
