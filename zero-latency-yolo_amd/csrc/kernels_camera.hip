// kernels_camera.hip -- the camera motion estimate (include/zly.h "Camera motion"; the arithmetic: camera_device.h) on gfx950: a block-matching search
// over the coarse grids of luma sums of two consecutive frames of a stream, and the shift of the stream's tracks by the result.  The grid itself is
// the change map's: a camera call launches change_sums_kernel (kernels_change.hip) as it is, into the camera's own scratch grids.
//
// camera_search_kernel: grid = (2R + 1 values of dy) x (frame); a workgroup of 256 threads computes the 2R + 1 entries SAD(-R .. R, dy) of the stream's
//   table.  A thread strides over the window's cells -- at most 8192 / 256 = 32 of them, each |S - S_prev| <= 64 * 64 * 255: a u32 per thread and
//   candidate holds the sum -- and keeps one accumulator per dx; a cell's S is loaded once and the 2R + 1 values of S_prev beside each other.  The
//   accumulators are added up across the wavefront with shuffles in 64 bits, across the four wavefronts through LDS, and one lane per dx stores its
//   entry.  No atomics and no zeroing pass: every entry is stored once, by one lane, as one sum of fixed operands -- integer addition commutes, so the
//   result does not depend on any order.  Both grids are at most 32 KB and sit in L2.  On a FIRST frame the kernel returns at once.
// camera_pick_kernel: one workgroup of 256 threads per frame, a launch of its own -- the stream order between the two launches is the only thing
//   that guarantees that every search workgroup has finished reading the previous grid before it is overwritten.  The ordered argmin over the at
//   most 289 entries (camera_less: SAD, then |dx| + |dy|, dy, dx) by a butterfly per wavefront and four slots of LDS; thread 0 makes the fit, the
//   flags, the record and the pending shift; then every thread copies S over the stream's previous grid, 16 bytes at a time.
// camera_apply_kernel: one wavefront per stream, lane t = slot t of the stream's track table; step A.
// camera_reset_kernel: a thread per stream.
// Stores are per-lane vector stores in plain C++.
#include "zly_internal.h"
#include "camera_device.h"

#pragma clang fp contract(off)

namespace zly {

static_assert(sizeof(zly_camera_header) == ZLY_CAMERA_HDR, "record size");
static_assert(ZLY_CAMERA_THREADS == 256 && ZLY_CAMERA_THREADS % 64 == 0, "four wavefronts");
static_assert(ZLY_CAMERA_SIDE_MAX <= ZLY_CAMERA_THREADS, "one lane per dx stores");
static_assert((uint64_t)(ZLY_CHANGE_MAX_CELLS / ZLY_CAMERA_THREADS) * 64u * 64u * 255u <= 0xffffffffull, "a thread's accumulator is a u32");
static_assert(ZLY_CHANGE_MAX_CELLS % 4 == 0, "the grids are copied 16 bytes at a time");

typedef unsigned int cam_u32x4 __attribute__((ext_vector_type(4)));

struct CameraArgs {
    const CameraItem* items; const uint32_t* sums; CameraStream* state; uint32_t* prev; uint8_t* recs;
    unsigned long long rec_bytes, sad_off;
    int C, R, max_residual_q4;
};

// the frame's grid, or false for a frame the host refuses: nothing is derived from such a frame
__device__ __forceinline__ bool camera_geometry(const CameraItem& it, int C, int R, int& gw, int& gh)
{
    gw = change_cells_axis(it.W, C); gh = change_cells_axis(it.H, C);
    return it.stream >= 0 && it.W >= 1 && it.H >= 1 && gw * gh <= ZLY_CHANGE_MAX_CELLS && camera_grid_ok(gw, gh, R);
}

__global__ __launch_bounds__(ZLY_CAMERA_THREADS) void camera_search_kernel(CameraArgs A)
{
    __shared__ unsigned long long part[ZLY_CAMERA_THREADS / 64][ZLY_CAMERA_SIDE_MAX];
    const int t = (int)threadIdx.x, f = (int)blockIdx.y, R = A.R, side = 2 * R + 1, dy = (int)blockIdx.x - R;
    const CameraItem it = A.items[f];
    int gw, gh;
    if (!camera_geometry(it, A.C, R, gw, gh)) return;               // uniform
    if (camera_first(A.state[it.stream], it.W, it.H, A.C)) return;  // uniform: no search, the table is left as it is
    const uint32_t* const S = A.sums + (size_t)f * ZLY_CHANGE_MAX_CELLS;
    const uint32_t* const prev = A.prev + (size_t)it.stream * ZLY_CHANGE_MAX_CELLS;
    const int ww = gw - 2 * R, nwin = ww * (gh - 2 * R);
    uint32_t acc[ZLY_CAMERA_SIDE_MAX];
#pragma unroll
    for (int k = 0; k < ZLY_CAMERA_SIDE_MAX; ++k) acc[k] = 0u;
    for (int i = t; i < nwin; i += ZLY_CAMERA_THREADS) {
        const int cx = R + i % ww, cy = R + i / ww;
        const uint32_t s = S[cy * gw + cx];
        // candidate k is dx = k - R: S_prev(cx - dx, cy - dy) = p[-k], columns cx - R .. cx + R of row cy - dy, all inside the grid
        const uint32_t* const p = prev + (cy - dy) * gw + cx + R;
#pragma unroll
        for (int k = 0; k < ZLY_CAMERA_SIDE_MAX; ++k)
            if (k < side) acc[k] += change_absdiff(s, p[-k]);
    }
#pragma unroll
    for (int k = 0; k < ZLY_CAMERA_SIDE_MAX; ++k) {
        unsigned long long v = acc[k];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
        if ((t & 63) == 0) part[t >> 6][k] = v;
    }
    __syncthreads();
    if (t < side) {
        unsigned long long v = part[0][t];
#pragma unroll
        for (int w = 1; w < ZLY_CAMERA_THREADS / 64; ++w) v += part[w][t];
        unsigned long long* const tab = reinterpret_cast<unsigned long long*>(A.recs + (size_t)it.stream * A.rec_bytes + A.sad_off);
        tab[(dy + R) * side + t] = v;
    }
}

__global__ __launch_bounds__(ZLY_CAMERA_THREADS) void camera_pick_kernel(CameraArgs A)
{
    __shared__ unsigned long long wsad[ZLY_CAMERA_THREADS / 64];
    __shared__ uint32_t wrank[ZLY_CAMERA_THREADS / 64];
    const int t = (int)threadIdx.x, f = (int)blockIdx.x, R = A.R, C = A.C, side = 2 * R + 1;
    const CameraItem it = A.items[f];
    int gw, gh;
    if (!camera_geometry(it, C, R, gw, gh)) return;                 // uniform
    CameraStream* const st = A.state + it.stream;
    const CameraStream old = *st;
    const bool first = camera_first(old, it.W, it.H, C);
    uint8_t* const rec = A.recs + (size_t)it.stream * A.rec_bytes;
    const unsigned long long* const tab = reinterpret_cast<const unsigned long long*>(rec + A.sad_off);

    // step 4: a lane without an entry holds the largest key there is
    unsigned long long best = ~0ull;
    uint32_t rank = ~0u;
    if (!first) {                                                    // uniform
        for (int i = t; i < side * side; i += ZLY_CAMERA_THREADS) {
            const unsigned long long s = tab[i];
            const uint32_t rk = camera_rank(i % side - R, i / side - R, R);
            if (camera_less(s, rk, best, rank)) { best = s; rank = rk; }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const unsigned long long os = __shfl_xor(best, off);
            const uint32_t ork = __shfl_xor(rank, off);
            if (camera_less(os, ork, best, rank)) { best = os; rank = ork; }
        }
        if ((t & 63) == 0) { wsad[t >> 6] = best; wrank[t >> 6] = rank; }
    }
    __syncthreads();                                                 // every thread has read *st; the wavefronts' choices are in LDS

    if (t == 0) {
        const zly_camera_header was = *reinterpret_cast<const zly_camera_header*>(rec);
        zly_camera_header h;
        h.flags = 0u; h.step = old.step + 1u; h.gw = gw; h.gh = gh;
        h.dx = h.dy = h.fx = h.fy = 0; h.sx_q4 = h.sy_q4 = 0;
        h.n_lost = was.n_lost; h.n_applied = was.n_applied;
        h.sad_min = h.sad_zero = 0u;
        h.pend_x_q4 = was.pend_x_q4; h.pend_y_q4 = was.pend_y_q4;
        h.pad[0] = h.pad[1] = h.pad[2] = h.pad[3] = 0u;
        if (first) {
            h.flags = ZLY_CAMERA_F_FIRST;
            h.pend_x_q4 = h.pend_y_q4 = 0;
        } else {
            best = wsad[0]; rank = wrank[0];
#pragma unroll
            for (int w = 1; w < ZLY_CAMERA_THREADS / 64; ++w)
                if (camera_less(wsad[w], wrank[w], best, rank)) { best = wsad[w]; rank = wrank[w]; }
            const int dx = camera_rank_dx(rank, R), dy = camera_rank_dy(rank, R);
            const bool clip_x = camera_abs(dx) == R, clip_y = camera_abs(dy) == R;
            // steps 5 and 6: the neighbours are read only where they lie in the table
            h.dx = dx; h.dy = dy;
            h.fx = camera_fit(dx, R, best, clip_x ? 0u : tab[camera_entry(dx - 1, dy, R)], clip_x ? 0u : tab[camera_entry(dx + 1, dy, R)]);
            h.fy = camera_fit(dy, R, best, clip_y ? 0u : tab[camera_entry(dx, dy - 1, R)], clip_y ? 0u : tab[camera_entry(dx, dy + 1, R)]);
            h.sx_q4 = camera_shift_q4(dx, h.fx, C); h.sy_q4 = camera_shift_q4(dy, h.fy, C);
            h.sad_min = best; h.sad_zero = tab[camera_entry(0, 0, R)];
            // steps 7 and 8
            const bool lost = camera_lost(best, (uint32_t)A.max_residual_q4, camera_npix(gw, gh, R, C));
            h.flags = (lost ? ZLY_CAMERA_F_LOST : 0u) | (clip_x || clip_y ? ZLY_CAMERA_F_CLIPPED : 0u);
            if (lost) h.n_lost += 1u;
            else { h.pend_x_q4 += h.sx_q4; h.pend_y_q4 += h.sy_q4; }
        }
        *reinterpret_cast<zly_camera_header*>(rec) = h;
        CameraStream ns;
        ns.W = it.W; ns.H = it.H; ns.C = C; ns.have_prev = 1; ns.step = old.step + 1u; ns.pad_[0] = ns.pad_[1] = ns.pad_[2] = 0u;
        *st = ns;
    }

    // the stored grid becomes S: whole groups of four cells, the last of which may reach beyond gw * gh but never beyond the grid's room --
    // cells there belong to no geometry the stream has
    const cam_u32x4* const src = reinterpret_cast<const cam_u32x4*>(A.sums + (size_t)f * ZLY_CHANGE_MAX_CELLS);
    cam_u32x4* const dst = reinterpret_cast<cam_u32x4*>(A.prev + (size_t)it.stream * ZLY_CHANGE_MAX_CELLS);
    const int n4 = (gw * gh + 3) / 4;
    for (int i = t; i < n4; i += ZLY_CAMERA_THREADS) dst[i] = src[i];
}

// streams: the call's n stream indices (device).  Lane t is slot t.
__global__ __launch_bounds__(64) void camera_apply_kernel(const int* streams, const CameraStream* state, uint8_t* recs, unsigned long long rec_bytes,
                                                          TrackStream* tracks, int max_tracks)
{
    const int t = (int)threadIdx.x, s = streams[blockIdx.x];
    const CameraStream st = state[s];
    if (st.W < 1 || st.H < 1) return;                                // uniform: a stream without a geometry is skipped whole
    zly_camera_header* const h = reinterpret_cast<zly_camera_header*>(recs + (size_t)s * rec_bytes);
    const long long px = h->pend_x_q4, py = h->pend_y_q4;
    const float nx = camera_norm(px, st.W), ny = camera_norm(py, st.H);
    TrackStream* const ts = tracks + s;
    if (t < max_tracks && ts->live[t]) {
        ts->x[t] = ts->x[t] + nx;
        ts->y[t] = ts->y[t] + ny;
    }
    if (t == 0) {                                                    // behind this wavefront's loads of the pending shift, in program order
        h->pend_x_q4 = 0; h->pend_y_q4 = 0;
        h->n_applied = h->n_applied + 1u;
    }
}

__global__ void camera_reset_kernel(CameraStream* state, uint8_t* recs, unsigned long long rec_bytes, int first, int count)
{
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= count) return;
    CameraStream z;
    z.W = z.H = z.C = z.have_prev = 0; z.step = 0u; z.pad_[0] = z.pad_[1] = z.pad_[2] = 0u;
    state[first + i] = z;
    zly_camera_header* const h = reinterpret_cast<zly_camera_header*>(recs + (size_t)(first + i) * rec_bytes);
    h->pend_x_q4 = 0; h->pend_y_q4 = 0;
}

hipError_t launch_camera(const CameraItem* items, int n, const uint32_t* sums, CameraStream* state, uint32_t* prev, void* recs, const zly_camera_config& cfg, hipStream_t s)
{
    if (!items || !sums || !state || !prev || !recs || n < 1 || !change_cell_ok(cfg.cell) || !camera_radius_ok(cfg.radius) || cfg.max_residual_q4 < 0 ||
        cfg.max_residual_q4 > 4080)
        return hipErrorInvalidValue;
    const CameraLayout l = camera_layout();
    CameraArgs a;
    a.items = items; a.sums = sums; a.state = state; a.prev = prev; a.recs = (uint8_t*)recs;
    a.rec_bytes = l.rec_bytes; a.sad_off = l.sad_off;
    a.C = cfg.cell; a.R = cfg.radius; a.max_residual_q4 = cfg.max_residual_q4;
    hipLaunchKernelGGL(camera_search_kernel, dim3((unsigned)(2 * cfg.radius + 1), (unsigned)n), dim3(ZLY_CAMERA_THREADS), 0, s, a);
    if (const hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(camera_pick_kernel, dim3((unsigned)n), dim3(ZLY_CAMERA_THREADS), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_camera_apply(const int* streams, int n, const CameraStream* state, void* recs, TrackStream* tracks, int max_tracks, hipStream_t s)
{
    if (!streams || !state || !recs || !tracks || n < 1 || max_tracks < 1 || max_tracks > ZLY_TRACK_MAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL(camera_apply_kernel, dim3((unsigned)n), dim3(64), 0, s, streams, state, (uint8_t*)recs, (unsigned long long)camera_layout().rec_bytes, tracks,
                       max_tracks);
    return hipGetLastError();
}

hipError_t launch_camera_reset(CameraStream* state, void* recs, int first, int count, hipStream_t s)
{
    if (!state || !recs || first < 0 || count < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(camera_reset_kernel, dim3((unsigned)((count + 63) / 64)), dim3(64), 0, s, state, (uint8_t*)recs, (unsigned long long)camera_layout().rec_bytes,
                       first, count);
    return hipGetLastError();
}

}  // namespace zly
