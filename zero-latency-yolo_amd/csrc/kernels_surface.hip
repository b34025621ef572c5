// kernels_surface.hip -- the kernels of the resident surfaces (include/zly.h "Resident surfaces").  The patch kernel: ONE launch writes every rectangle
// of a zly_surface_update call from the staging buffer into the store.  The move kernel (at the end of the file): the copies inside the store of a
// zly_surface_move call.
//
// The host (surface_rules.h) turns (rectangle, plane) pairs into jobs and cuts the jobs into bands of whole rows (surface_device.h); the band table
// lies in the staging buffer behind the pixels, so one copy brings both.  A workgroup takes bands in a grid-stride loop: a 33 MB keyframe is two
// thousand bands, a 1 x 1 cursor rectangle is one, and both fill the chip by the same rule.
//
// A row of a band is n = row_bytes bytes from src (tight: the row starts at ANY byte) to dst (any byte as well: BGR at x0 has byte offset 3 * x0).
// The row is cut at the DESTINATION's 16-byte granules: granule g holds row bytes [16g - lead, 16g - lead + 16) with lead = dst & 15, clipped to
// [0, n).  A lane owns one granule of one row:
//   * a whole granule is one 16-byte load and one 16-byte store.  The store is aligned by construction.  The load is not: it names the 16 source
//     bytes of that granule at whatever address they have.  Global loads on gfx950 take any byte address (the unaligned access mode ROCm runs in);
//     a lane's 16 bytes straddle a 64-byte line for (src - dst) mod 16 != 0, and the 64 lanes of a wave still read one contiguous 1 KiB: nothing is
//     fetched twice from HBM.  The alternative -- aligned loads and a byte shuffle through v_alignbyte -- would read up to 15 bytes on either side of
//     the row and need the staging rows padded, which the tight staging copy (copy_view_tight) does not do.
//   * a clipped granule -- the row's head and tail, 1..15 bytes -- goes out in naturally aligned 8, 4, 2 and 1-byte stores.
// THE HARD REQUIREMENT: no byte outside [dst, dst + n) is written, not even with its own value.  Two disjoint rectangles of one launch may share a
// granule, and a read-modify-write of the neighbour's bytes would race with the neighbour's lane.  Loads never leave [src, src + n) either.
// No LDS, no atomics, no cross-lane traffic.
#include "zly_internal.h"
#include "surface_device.h"

namespace zly {

typedef unsigned int sf_u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int sf_u32x2 __attribute__((ext_vector_type(2)));

// k = 1 .. 15 bytes from sp to dp in the widest naturally aligned stores that stay inside [dp, dp + k)
__device__ __forceinline__ void surface_copy_edge(uint8_t* dp, const uint8_t* sp, unsigned int k)
{
    while (k) {
        const unsigned int wd = surface_edge_width((unsigned int)(uintptr_t)dp, k);
        if (wd == 8u)      { sf_u32x2 v; __builtin_memcpy(&v, sp, 8); *reinterpret_cast<sf_u32x2*>(dp) = v; }
        else if (wd == 4u) { unsigned int v; __builtin_memcpy(&v, sp, 4); *reinterpret_cast<unsigned int*>(dp) = v; }
        else if (wd == 2u) { unsigned short v; __builtin_memcpy(&v, sp, 2); *reinterpret_cast<unsigned short*>(dp) = v; }
        else               { *dp = *sp; }
        dp += wd; sp += wd; k -= wd;
    }
}

__global__ void __launch_bounds__(ZLY_SURFACE_THREADS)
surface_patch_kernel(const uint8_t* __restrict__ stage, const SurfaceJob* __restrict__ bands, int n_bands, uint8_t* __restrict__ store)
{
    for (int b = (int)blockIdx.x; b < n_bands; b += (int)gridDim.x) {
        const SurfaceJob j = bands[b];                          // uniform: scalar loads
        const unsigned int n = j.row_bytes;
        const unsigned int G = surface_row_granules(n);
        const unsigned long long items = (unsigned long long)j.rows * G;
        for (unsigned long long i = threadIdx.x; i < items; i += ZLY_SURFACE_THREADS) {
            unsigned int r, g;
            if (j.rows == 1u) { r = 0u; g = (unsigned int)i; }  // a band of one (possibly very long) row
            else { r = (unsigned int)i / G; g = (unsigned int)i - r * G; }      // otherwise items <= 2 * ZLY_SURFACE_BAND_BYTES: 32 bits
            const unsigned long long drow = j.dst_off + (unsigned long long)r * j.pitch;
            unsigned int lo, hi;
            if (!surface_granule(drow, n, g, &lo, &hi)) continue;              // the row ends before this granule
            const uint8_t* sp = stage + j.src_off + (unsigned long long)r * n + lo;
            uint8_t* dp = store + drow + lo;
            if (hi - lo == 16u) {                               // unclipped: drow + lo is a multiple of 16, and the store's base is 16-byte aligned
                sf_u32x4 v;
                __builtin_memcpy(&v, sp, 16);
                *reinterpret_cast<sf_u32x4*>(dp) = v;
            } else {
                surface_copy_edge(dp, sp, hi - lo);
            }
        }
    }
}

hipError_t launch_surface_patch(const uint8_t* stage, const SurfaceJob* bands, int n_bands, uint8_t* store, int num_cus, hipStream_t s)
{
    if (n_bands < 1) return hipSuccess;
    // up to eight workgroups (32 waves) per compute unit are resident: more bands than that are taken by the grid-stride loop
    const int most = 8 * (num_cus > 0 ? num_cus : 256);
    const dim3 grid((unsigned)(n_bands < most ? n_bands : most));
    hipLaunchKernelGGL(surface_patch_kernel, grid, dim3(ZLY_SURFACE_THREADS), 0, s, stage, bands, n_bands, store);
    return hipGetLastError();
}

// The move kernel (zly_surface_move): the patch kernel's scheme with a pitched source that lies in the STORE itself.  A band (surface_device.h:
// SurfaceMoveBand) goes store -> store, or store -> bounce buffer for a move whose source and destination intersect; the bounce buffer comes back
// through surface_patch_kernel in a launch of its own.  The host (surface_rules.h: surface_plan_moves) puts into one launch only bands of which none
// reads or writes a byte that another one writes, so the order in which workgroups run does not matter -- which is why store and bounce carry no
// __restrict__: a band's source and another band's destination may be neighbours in one granule, never the same byte.
// Rows are cut at the DESTINATION's granules, loads are at any byte address, and no access leaves its row: a source row's neighbours in the store
// are another rectangle's pixels, possibly being written by this very launch.
__global__ void __launch_bounds__(ZLY_SURFACE_THREADS)
surface_move_kernel(const SurfaceMoveBand* __restrict__ bands, int n_bands, uint8_t* store, uint8_t* bounce)
{
    for (int b = (int)blockIdx.x; b < n_bands; b += (int)gridDim.x) {
        const SurfaceMoveBand j = bands[b];                     // uniform: scalar loads
        const unsigned int G = surface_row_granules(j.row_bytes);
        const unsigned long long items = (unsigned long long)j.rows * G;
        uint8_t* const dbase = surface_move_to_bounce(j) ? bounce : store;
        for (unsigned long long i = threadIdx.x; i < items; i += ZLY_SURFACE_THREADS) {
            unsigned int r, g, k;
            surface_band_item(j.rows, G, i, &r, &g);
            uint64_t so, dof;
            if (!surface_move_item(j, r, g, &so, &dof, &k)) continue;           // the row ends before this granule
            const uint8_t* sp = store + so;
            uint8_t* dp = dbase + dof;
            if (k == 16u) {                                     // unclipped: dof is a multiple of 16, and both bases are 16-byte aligned
                sf_u32x4 v;
                __builtin_memcpy(&v, sp, 16);
                *reinterpret_cast<sf_u32x4*>(dp) = v;
            } else {
                surface_copy_edge(dp, sp, k);
            }
        }
    }
}

hipError_t launch_surface_move(const SurfaceMoveBand* bands, int n_bands, uint8_t* store, uint8_t* bounce, int num_cus, hipStream_t s)
{
    if (n_bands < 1) return hipSuccess;
    const int most = 8 * (num_cus > 0 ? num_cus : 256);         // as launch_surface_patch
    const dim3 grid((unsigned)(n_bands < most ? n_bands : most));
    hipLaunchKernelGGL(surface_move_kernel, grid, dim3(ZLY_SURFACE_THREADS), 0, s, bands, n_bands, store, bounce);
    return hipGetLastError();
}

}  // namespace zly
