// kernels_change.hip -- the change map (include/zly.h "Change map"; the arithmetic: change_device.h) on gfx950: a grid of luma sums per frame, and what
// changed against the stream's previous grid.
//
// change_sums_kernel: the bandwidth pass.  grid = (tile column) x (tile row) x (frame); a workgroup of 256 threads sums one tile of 64 x 64 pixels --
//   whole cells of every legal size, so every cell is stored once, by one workgroup, and nothing is accumulated in memory.  Thread t takes the granule
//   g = t & 3 of row t >> 2: 16 pixels of one row, fetched with up to four 16-byte loads (a 4-byte format: 64 contiguous bytes per thread, 256 per
//   row of the tile, the rows of a wavefront 16 pitches apart) straight into registers; the loads start at the granule's first byte whatever its
//   alignment (global memory takes unaligned vector loads), so a thread's bytes are whole pixels and need no staging.  A load that would leave its
//   plane's extent is made byte by byte inside it.  One 1920 x 1080 surface is 510 workgroups, 2040 wavefronts, each with all its loads in flight at once.
//   Reduction: the granule's two halves of 8 pixels; a butterfly over the 8 rows of a wavefront that share a cell row of every size; 8 x 8 block
//   sums in LDS; one thread per cell of the tile adds its blocks and stores the cell.
// change_pick_kernel: one workgroup of 256 threads per frame.  It computes A = |S - S_prev| into LDS (a cell that is not ACTIVE is kept as 0: a live
//   cell has A >= 1), writes the activity grid, stores S as the stream's grid, decides FIRST and GLOBAL, applies the initial suppression and chooses
//   the peaks greedily: every thread scans its cells for the largest key (A, then the lowest index: change_key), a butterfly per wavefront and four
//   words of LDS make the workgroup's choice, and every thread clears the cells of the chosen window.  In a zoom call it reads the frame's plan as
//   zoom_plan_kernel left it -- the regions with slot >= 0 are the initial suppression -- and writes peak p into the p-th fallback region: the plan
//   record, FrameDesc::src_off, the ViewRec plane offsets and the merge table's x0, y0, with the plan kernel's arithmetic (zoom_plane_off, desc_pack).
// Stores are per-lane vector stores in plain C++.
#include "zly_internal.h"
#include "change_device.h"

namespace zly {

static_assert(sizeof(zly_change_header) == ZLY_CHANGE_HDR_BYTES && sizeof(zly_change_peak) == ZLY_CHANGE_PEAK_BYTES, "record sizes");
static_assert(ZLY_CHANGE_THREADS == (ZLY_CHANGE_TILE_PX / ZLY_CHANGE_GRANULE_PX) * ZLY_CHANGE_TILE_PX, "one thread per granule of the tile");
static_assert(ZLY_CHANGE_TILE_PX == 64 && ZLY_CHANGE_GRANULE_PX == 16, "the reduction below is written for 4 granules x 64 rows");

typedef unsigned int chg_u32x4 __attribute__((ext_vector_type(4)));

// 16 bytes at q (any alignment): one vector load where all of it lies inside [lo, hi), single bytes of the plane otherwise
__device__ __forceinline__ chg_u32x4 chg_load16(const uint8_t* q, const uint8_t* lo, const uint8_t* hi)
{
    chg_u32x4 v = {0u, 0u, 0u, 0u};
    if (q >= lo && q + 16 <= hi) {
        __builtin_memcpy(&v, q, 16);
        return v;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        unsigned int x = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const uint8_t* c = q + k * 4 + b;
            if (c >= lo && c < hi) x |= (unsigned int)*c << (8 * b);
        }
        v[k] = x;
    }
    return v;
}

// sums: [frame][ZLY_CHANGE_MAX_CELLS]
__global__ __launch_bounds__(ZLY_CHANGE_THREADS) void change_sums_kernel(const uint8_t* __restrict__ src, const ChipFrame* __restrict__ frames,
                                                                         uint32_t* __restrict__ sums, int C)
{
    __shared__ uint32_t blk[8][8];                                  // the tile's 8 x 8 blocks of 8 x 8 pixels
    const ChipFrame F = frames[blockIdx.z];
    const int tx0 = (int)blockIdx.x * ZLY_CHANGE_TILE_PX, ty0 = (int)blockIdx.y * ZLY_CHANGE_TILE_PX;
    if (tx0 >= F.W || ty0 >= F.H) return;                           // uniform: the grid is sized for the call's largest frame
    const int t = (int)threadIdx.x, g = t & 3, row = t >> 2;
    const int x0 = tx0 + g * ZLY_CHANGE_GRANULE_PX, y = ty0 + row;
    uint32_t lo = 0u, hi = 0u;
    if (x0 < F.W && y < F.H) {
        const ChangeLoads L = change_granule_loads(F, x0, y);
        uint32_t d[16];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            chg_u32x4 v = {0u, 0u, 0u, 0u};
            if (k < L.n) v = chg_load16(src + L.o[k], src + change_load_lo(F, L, k), src + change_load_hi(F, L, k));
            d[4 * k] = v[0]; d[4 * k + 1] = v[1]; d[4 * k + 2] = v[2]; d[4 * k + 3] = v[3];
        }
        change_granule_sums(F, d, L.npx, lo, hi);
    }
    // lane = (row & 15) * 4 + g: the lanes 4, 8 and 16 apart hold the other rows of this lane's group of 8
#pragma unroll
    for (int off = 4; off <= 16; off <<= 1) { lo += __shfl_xor(lo, off); hi += __shfl_xor(hi, off); }
    if ((row & 7) == 0) { blk[row >> 3][2 * g] = lo; blk[row >> 3][2 * g + 1] = hi; }
    __syncthreads();
    const int per = ZLY_CHANGE_TILE_PX / C, nb = C / 8;               // cells per axis of the tile, blocks per axis of a cell
    if (t < per * per) {
        const int cxl = t % per, cyl = t / per;
        const int gw = change_cells_axis(F.W, C), gh = change_cells_axis(F.H, C);
        const int cx = tx0 / C + cxl, cy = ty0 / C + cyl;
        if (cx < gw && cy < gh) {
            uint32_t s = 0u;
            for (int j = 0; j < nb; ++j)
                for (int i = 0; i < nb; ++i) s += blk[cyl * nb + j][cxl * nb + i];
            sums[(size_t)blockIdx.z * ZLY_CHANGE_MAX_CELLS + (size_t)cy * gw + cx] = s;
        }
    }
}

struct ChangePickArgs {
    const ChangeItem* items; const uint32_t* sums; ChangeStream* state; uint32_t* prev; uint8_t* recs;
    unsigned long long rec_bytes, peaks_off, activity_off;
    int C, threshold_q4, max_active_permille, max_peaks, window_w, window_h;
    // a zoom call (plan != null): the frame records the plan kernel was given and what it wrote and patched
    const ZoomFrame* zf; FrameDesc* desc; int n_views; int* tab; int n; zly_zoom_region* plan; int K;
};

__global__ __launch_bounds__(ZLY_CHANGE_THREADS) void change_pick_kernel(ChangePickArgs A)
{
    __shared__ uint32_t val[ZLY_CHANGE_MAX_CELLS];                  // A of the live cells, 0 elsewhere
    __shared__ unsigned long long wkey[ZLY_CHANGE_THREADS / 64];
    __shared__ int s_active;
    __shared__ zly_change_peak s_peaks[ZLY_CHANGE_MAX_PEAKS];
    __shared__ zly_zoom_region s_reg[ZLY_ZOOM_MAX_REGIONS];
    const int t = (int)threadIdx.x, f = (int)blockIdx.x;
    const ChangeItem it = A.items[f];
    const int W = it.W, H = it.H, C = A.C;
    const int gw = change_cells_axis(W, C), gh = change_cells_axis(H, C), nc = gw * gh;
    if (nc > ZLY_CHANGE_MAX_CELLS || it.stream < 0) return;          // the host refuses such a call: nothing below is derived from it
    ChangeStream* const st = A.state + it.stream;
    const ChangeStream old = *st;
    uint32_t* const prev = A.prev + (size_t)it.stream * ZLY_CHANGE_MAX_CELLS;
    const uint32_t* const S = A.sums + (size_t)f * ZLY_CHANGE_MAX_CELLS;
    uint8_t* const rec = A.recs + (size_t)it.stream * A.rec_bytes;
    uint32_t* const activity = reinterpret_cast<uint32_t*>(rec + A.activity_off);
    const bool first = !old.have_prev || old.W != W || old.H != H || old.C != C;
    const int K = A.plan ? A.K : 0;
    if (t == 0) s_active = 0;
    if (t < K) s_reg[t] = A.plan[(size_t)f * K + t];
    __syncthreads();

    // steps 3 and 4
    int mine = 0;
    for (int c = t; c < nc; c += ZLY_CHANGE_THREADS) {
        const uint32_t s = S[c];
        const uint32_t a = first ? 0u : change_absdiff(s, prev[c]);
        const bool act = !first && change_active(a, (uint32_t)A.threshold_q4, change_span(c % gw, C, W) * change_span(c / gw, C, H));
        val[c] = act ? a : 0u;
        activity[c] = a;
        prev[c] = s;
        mine += act ? 1 : 0;
    }
    if (mine) atomicAdd(&s_active, mine);                           // LDS
    __syncthreads();
    const int n_active = s_active;
    const bool global = change_global((uint32_t)n_active, (uint32_t)A.max_active_permille, (uint32_t)nc);
    const ZoomSize z = zoom_size(A.window_w, A.window_h, W, H);

    int n_peaks = 0;
    if (!first && !global && W >= 2 && H >= 2) {                     // uniform
        if (K > 0) {                                                 // the initial suppression: the plan's track regions
            for (int c = t; c < nc; c += ZLY_CHANGE_THREADS) {
                if (!val[c]) continue;
                const int px = change_centre(c % gw, C, W), py = change_centre(c / gw, C, H);
                bool in = false;
                for (int j = 0; j < K; ++j) in = in || (s_reg[j].slot >= 0 && change_inside(px, py, s_reg[j].x0, s_reg[j].y0, s_reg[j].w, s_reg[j].h));
                if (in) val[c] = 0u;
            }
            __syncthreads();
        }
        while (n_peaks < A.max_peaks) {
            unsigned long long best = 0ull;
            for (int c = t; c < nc; c += ZLY_CHANGE_THREADS) {
                const uint32_t v = val[c];
                if (v) { const unsigned long long k = change_key(v, (uint32_t)c); best = k > best ? k : best; }
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) { const unsigned long long o = __shfl_xor(best, off); best = o > best ? o : best; }
            if ((t & 63) == 0) wkey[t >> 6] = best;
            __syncthreads();
            best = wkey[0];
#pragma unroll
            for (int w = 1; w < ZLY_CHANGE_THREADS / 64; ++w) best = wkey[w] > best ? wkey[w] : best;
            if (change_key_value(best) == 0u) break;                 // uniform: no cell is live
            const int pi = (int)change_key_index(best), cx = pi % gw, cy = pi / gw;
            zly_change_peak p;
            p.x0 = change_origin(change_centre(cx, C, W), z.rw, z.xmax); p.y0 = change_origin(change_centre(cy, C, H), z.rh, z.ymax);
            p.w = z.rw; p.h = z.rh; p.cx = cx; p.cy = cy; p.activity = change_key_value(best); p.pad = 0u;
            if (t == 0) {
                s_peaks[n_peaks] = p;
                *reinterpret_cast<zly_change_peak*>(rec + A.peaks_off + (size_t)n_peaks * ZLY_CHANGE_PEAK_BYTES) = p;
            }
            for (int c = t; c < nc; c += ZLY_CHANGE_THREADS)
                if (c == pi || (val[c] && change_inside(change_centre(c % gw, C, W), change_centre(c / gw, C, H), p.x0, p.y0, p.w, p.h))) val[c] = 0u;
            ++n_peaks;
            __syncthreads();                                         // val and s_peaks are written, wkey is read
        }
    }
    __syncthreads();

    if (t == 0) {
        zly_change_header h;
        h.n_cells = nc; h.n_active = n_active; h.n_peaks = n_peaks;
        h.flags = (first ? ZLY_CHANGE_F_FIRST : 0u) | (global ? ZLY_CHANGE_F_GLOBAL : 0u);
        h.gw = gw; h.gh = gh; h.step = old.step + 1u; h.pad = 0u;
        *reinterpret_cast<zly_change_header*>(rec) = h;
        ChangeStream ns;
        ns.W = W; ns.H = H; ns.C = C; ns.have_prev = 1; ns.step = old.step + 1u; ns.pad_[0] = ns.pad_[1] = ns.pad_[2] = 0u;
        *st = ns;
    }

    // the fill: thread j owns region j, as in the plan kernel
    if (t < K && s_reg[t].slot == -1) {
        int rank = 0;
        for (int j = 0; j < t; ++j) rank += s_reg[j].slot == -1 ? 1 : 0;
        if (rank < n_peaks) {
            const ZoomFrame fr = A.zf[f];
            const int rx0 = s_peaks[rank].x0, ry0 = s_peaks[rank].y0;
            zly_zoom_region o = s_reg[t];
            o.x0 = rx0; o.y0 = ry0; o.slot = -2; o.track_id = 0u;
            A.plan[(size_t)f * K + t] = o;
            const int b = f * (1 + K) + 1 + t;                       // the region's batch item
            if (A.desc) {
                A.desc[b].src_off = desc_pack(zoom_plane_off(fr, 0, rx0, ry0), fr.fmt);
                ViewRec* vr = reinterpret_cast<ViewRec*>(A.desc + A.n_views) + b;
                if (fr.planes > 1) vr->off1 = zoom_plane_off(fr, 1, rx0, ry0);
                if (fr.planes > 2) vr->off2 = zoom_plane_off(fr, 2, rx0, ry0);
            }
            if (A.tab) {
                int* mrec = A.tab + (A.n + 1) + (size_t)b * ZLY_MERGE_TILE_INTS;
                mrec[1] = rx0; mrec[2] = ry0;
            }
        }
    }
}

hipError_t launch_change_sums(const uint8_t* src, const ChipFrame* frames, int n, int max_w, int max_h, int cell, uint32_t* sums, hipStream_t s)
{
    if (!src || !frames || !sums || n < 1 || max_w < 1 || max_h < 1 || max_w > ZLY_AREA_MAX_DIM || max_h > ZLY_AREA_MAX_DIM || !change_cell_ok(cell))
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)((max_w + ZLY_CHANGE_TILE_PX - 1) / ZLY_CHANGE_TILE_PX), (unsigned)((max_h + ZLY_CHANGE_TILE_PX - 1) / ZLY_CHANGE_TILE_PX), (unsigned)n);
    hipLaunchKernelGGL(change_sums_kernel, grid, dim3(ZLY_CHANGE_THREADS), 0, s, src, frames, sums, cell);
    return hipGetLastError();
}

hipError_t launch_change_pick(const ChangeItem* items, int n, const uint32_t* sums, ChangeStream* state, uint32_t* prev, void* recs, const zly_change_config& cfg,
                              const ZoomFrame* zf, FrameDesc* desc, int* tab, zly_zoom_region* plan, int K, hipStream_t s)
{
    if (!items || !sums || !state || !prev || !recs || n < 1 || !change_cell_ok(cfg.cell) || cfg.max_peaks < 1 || cfg.max_peaks > ZLY_CHANGE_MAX_PEAKS) return hipErrorInvalidValue;
    if (plan && (!zf || K < 1 || K > ZLY_ZOOM_MAX_REGIONS)) return hipErrorInvalidValue;
    const ChangeLayout l = change_layout(cfg.max_peaks);
    ChangePickArgs a;
    a.items = items; a.sums = sums; a.state = state; a.prev = prev; a.recs = (uint8_t*)recs;
    a.rec_bytes = l.rec_bytes; a.peaks_off = l.peaks_off; a.activity_off = l.activity_off;
    a.C = cfg.cell; a.threshold_q4 = cfg.threshold_q4; a.max_active_permille = cfg.max_active_permille; a.max_peaks = cfg.max_peaks;
    a.window_w = cfg.window_w; a.window_h = cfg.window_h;
    a.zf = zf; a.desc = desc; a.n_views = n * (1 + K); a.tab = tab; a.n = n; a.plan = plan; a.K = plan ? K : 0;
    hipLaunchKernelGGL(change_pick_kernel, dim3((unsigned)n), dim3(ZLY_CHANGE_THREADS), 0, s, a);
    return hipGetLastError();
}

}  // namespace zly
