// change_rules.h -- the host side of the change map (include/zly.h "Change map"): the config and call checks, and the HOST TWIN of the two kernels
// (kernels_change.hip) -- the same functions of change_device.h, walked granule by granule and cell by cell in loops.  Nothing here touches a device
// or the engine, as frame_rules.h does not: engine.cpp and a stand-alone test program (tests/cpp/test_change_rules.cpp) compile the same text.
#pragma once
#include <vector>
#include "chip_rules.h"
#include "zoom_rules.h"
#include "change_device.h"

namespace zly {

static_assert(sizeof(zly_change_header) == ZLY_CHANGE_HDR_BYTES && sizeof(zly_change_peak) == ZLY_CHANGE_PEAK_BYTES, "change_device.h's offsets are include/zly.h's records");
static_assert(ZLY_CHANGE_F_FIRST == ZLY_CHANGE_FIRST && ZLY_CHANGE_F_GLOBAL == ZLY_CHANGE_GLOBAL, "the flags");
static_assert(sizeof(ChangeItem) == 16 && sizeof(ChangeStream) == 32, "uploaded and kept as arrays");
static_assert(ZLY_PIX_NV12_BT709 == 3 && ZLY_PIX_I420_BT709 == 4 && ZLY_PIX_YUY2_BT709 == 12 && ZLY_PIX_UYVY_BT709 == 13 && ZLY_PIX_UYVY_BT601 == 11 &&
              ZLY_PIX_RGB == 16 && ZLY_PIX_RGBA == 18, "change_device.h's format predicates");

inline void change_default_config(int32_t model_w, int32_t model_h, zly_change_config* c)
{
    c->cell = 32;                                // chosen, not tuned
    c->threshold_q4 = 32;                        // two luma levels per pixel: chosen, not tuned
    c->max_active_permille = 250;                // chosen, not tuned
    c->max_peaks = 3;
    c->window_w = model_w & ~1; c->window_h = model_h & ~1;
}

inline int change_check_config(const zly_change_config* c, int32_t max_streams, std::string* err)
{
    if (!c) return refuse(err, ZLY_ERR_INVALID_ARGUMENT, "null change config");
    if (!change_cell_ok(c->cell)) return refuse(err, ZLY_ERR_INVALID_ARGUMENT, "cell must be 8, 16, 32 or 64");
    if (c->threshold_q4 < 0 || c->threshold_q4 > 4080) return refuse(err, ZLY_ERR_INVALID_ARGUMENT, "threshold_q4 must lie in 0..4080");
    if (c->max_active_permille < 0 || c->max_active_permille > 1000) return refuse(err, ZLY_ERR_INVALID_ARGUMENT, "max_active_permille must lie in 0..1000");
    if (c->max_peaks < 1 || c->max_peaks > ZLY_CHANGE_MAX_PEAKS) return refuse(err, ZLY_ERR_INVALID_ARGUMENT, "max_peaks must lie in 1..15");
    if (c->window_w < 2 || c->window_h < 2 || c->window_w > ZLY_ZOOM_MAX_REGION_DIM || c->window_h > ZLY_ZOOM_MAX_REGION_DIM || ((c->window_w | c->window_h) & 1))
        return refuse(err, ZLY_ERR_INVALID_ARGUMENT, "a window's width and height must be even and lie in 2..16384");
    if (max_streams < 1) return refuse(err, ZLY_ERR_INVALID_ARGUMENT, "max_streams must be >= 1");
    return ZLY_OK;
}

// the arguments of a call that need no engine state
inline int change_check_call(int32_t n, int32_t max_batch, const void* frames, const int32_t* streams, std::string* err)
{
    if (n < 1 || n > max_batch) return refuse(err, ZLY_ERR_INVALID_ARGUMENT, "batch size out of range");
    if (!frames) return refuse(err, ZLY_ERR_INVALID_ARGUMENT, "null views");
    if (!streams) return refuse(err, ZLY_ERR_INVALID_ARGUMENT, "null streams");
    return ZLY_OK;
}

inline int change_check_streams(int32_t n, const int32_t* streams, int32_t max_streams, std::string* err)
{
    for (int i = 0; i < n; ++i) {
        if (streams[i] < 0 || streams[i] >= max_streams)
            return refuse(err, ZLY_ERR_INVALID_ARGUMENT, "stream " + std::to_string(streams[i]) + " out of range (the change map has " + std::to_string(max_streams) + ")");
        for (int k = 0; k < i; ++k)
            if (streams[k] == streams[i]) return refuse(err, ZLY_ERR_INVALID_ARGUMENT, "stream " + std::to_string(streams[i]) + " occurs twice in a change call");
    }
    return ZLY_OK;
}

// the size of a (valid) view's grid
inline int change_check_size(int32_t W, int32_t H, int32_t C, std::string* err)
{
    if (W < 1 || H < 1 || W > ZLY_AREA_MAX_DIM || H > ZLY_AREA_MAX_DIM)
        return refuse(err, ZLY_ERR_INVALID_INPUT, "a change map is made of frames of at most " + std::to_string(ZLY_AREA_MAX_DIM) + " pixels on a side, got " +
                                                  std::to_string(W) + " x " + std::to_string(H));
    const int64_t cells = (int64_t)change_cells_axis(W, C) * change_cells_axis(H, C);
    if (cells > ZLY_CHANGE_MAX_CELLS)
        return refuse(err, ZLY_ERR_INVALID_INPUT, std::to_string(W) + " x " + std::to_string(H) + " at cell " + std::to_string(C) + " is " + std::to_string(cells) +
                                                  " cells, above ZLY_CHANGE_MAX_CELLS");
    return ZLY_OK;
}

// ---- the host twin of change_sums_kernel: S[gw*gh] of the frame f of the buffer `base`, granule by granule through change_granule_loads.  A load is
//      made as the kernel makes it: whole where it lies inside its plane's extent, otherwise only its bytes inside.  *outside counts the NEEDED bytes
//      that lie outside their plane's extent (they would be missing from a sum): the rule says 0.
inline void change_sums_host(const uint8_t* base, const ChipFrame& f, int32_t C, uint32_t* S, uint64_t* outside)
{
    const int32_t gw = change_cells_axis(f.W, C), gh = change_cells_axis(f.H, C);
    for (int32_t c = 0; c < gw * gh; ++c) S[c] = 0u;
    for (int32_t y = 0; y < f.H; ++y)
        for (int32_t x0 = 0; x0 < f.W; x0 += ZLY_CHANGE_GRANULE_PX) {
            const ChangeLoads L = change_granule_loads(f, x0, y);
            uint32_t d[16] = {};
            for (int k = 0; k < L.n; ++k)
                for (uint32_t b = 0; b < 16u; ++b) {
                    const uint64_t a = L.o[k] + b;
                    const bool in = a >= change_load_lo(f, L, k) && a < change_load_hi(f, L, k);
                    if (!in && b < L.need[k] && outside) ++*outside;
                    if (in) d[4 * k + (b >> 2)] |= (uint32_t)base[a] << (8 * (b & 3u));
                }
            uint32_t lo = 0u, hi = 0u;
            change_granule_sums(f, d, L.npx, lo, hi);
            const int32_t cy = y / C;
            if (C == 8) { S[cy * gw + x0 / 8] += lo; if (x0 + 8 < f.W) S[cy * gw + x0 / 8 + 1] += hi; }
            else S[cy * gw + x0 / C] += lo + hi;
        }
}

// a stream's state as the pick kernel keeps it
struct ChangeStateHost {
    ChangeStream st{};
    std::vector<uint32_t> prev;
};

// ---- the host twin of change_pick_kernel for one frame: S -> header, peaks[0 .. n_peaks), activity[0 .. gw*gh); the state advances.  init: n_init
//      rectangles of the initial suppression (x0, y0, w, h of zly_zoom_region records with slot >= 0; others are skipped) ----
inline void change_pick_host(ChangeStateHost& s, const uint32_t* S, int32_t W, int32_t H, const zly_change_config& c, const zly_zoom_region* init, int n_init,
                             zly_change_header* hd, zly_change_peak* peaks, uint32_t* activity)
{
    const int32_t C = c.cell, gw = change_cells_axis(W, C), gh = change_cells_axis(H, C), nc = gw * gh;
    const bool first = !s.st.have_prev || s.st.W != W || s.st.H != H || s.st.C != C;
    std::vector<uint32_t> val((size_t)nc, 0u);
    uint32_t n_active = 0;
    s.prev.resize((size_t)ZLY_CHANGE_MAX_CELLS, 0u);
    for (int32_t i = 0; i < nc; ++i) {
        const uint32_t A = first ? 0u : change_absdiff(S[i], s.prev[(size_t)i]);
        const bool act = !first && change_active(A, (uint32_t)c.threshold_q4, change_span(i % gw, C, W) * change_span(i / gw, C, H));
        val[(size_t)i] = act ? A : 0u;
        activity[i] = A;
        s.prev[(size_t)i] = S[i];
        n_active += act ? 1u : 0u;
    }
    const bool global = change_global(n_active, (uint32_t)c.max_active_permille, (uint32_t)nc);
    const ZoomSize z = zoom_size(c.window_w, c.window_h, W, H);
    int n_peaks = 0;
    if (!first && !global && W >= 2 && H >= 2) {
        for (int32_t i = 0; i < nc; ++i) {
            const int32_t px = change_centre(i % gw, C, W), py = change_centre(i / gw, C, H);
            for (int j = 0; j < n_init; ++j)
                if (init[j].slot >= 0 && change_inside(px, py, init[j].x0, init[j].y0, init[j].w, init[j].h)) val[(size_t)i] = 0u;
        }
        while (n_peaks < c.max_peaks) {
            uint64_t best = 0;
            for (int32_t i = 0; i < nc; ++i)
                if (val[(size_t)i]) { const uint64_t k = change_key(val[(size_t)i], (uint32_t)i); best = k > best ? k : best; }
            if (change_key_value(best) == 0u) break;
            const int32_t pi = (int32_t)change_key_index(best), cx = pi % gw, cy = pi / gw;
            zly_change_peak p;
            p.x0 = change_origin(change_centre(cx, C, W), z.rw, z.xmax); p.y0 = change_origin(change_centre(cy, C, H), z.rh, z.ymax);
            p.w = z.rw; p.h = z.rh; p.cx = cx; p.cy = cy; p.activity = change_key_value(best); p.pad = 0u;
            peaks[n_peaks++] = p;
            for (int32_t i = 0; i < nc; ++i)
                if (i == pi || change_inside(change_centre(i % gw, C, W), change_centre(i / gw, C, H), p.x0, p.y0, p.w, p.h)) val[(size_t)i] = 0u;
        }
    }
    s.st.W = W; s.st.H = H; s.st.C = C; s.st.have_prev = 1; s.st.step += 1u;
    hd->n_cells = nc; hd->n_active = (int32_t)n_active; hd->n_peaks = n_peaks;
    hd->flags = (first ? ZLY_CHANGE_FIRST : 0u) | (global ? ZLY_CHANGE_GLOBAL : 0u);
    hd->gw = gw; hd->gh = gh; hd->step = s.st.step; hd->pad = 0u;
}

// ---- the fill of a zoom call: peak p goes to the p-th fallback region (slot == -1) of the K regions, in region order ----
inline void change_fill_host(zly_zoom_region* plan, int K, const zly_change_peak* peaks, int n_peaks)
{
    int p = 0;
    for (int j = 0; j < K && p < n_peaks; ++j) {
        if (plan[j].slot != -1) continue;
        plan[j].x0 = peaks[p].x0; plan[j].y0 = peaks[p].y0; plan[j].slot = -2; plan[j].track_id = 0u;
        ++p;
    }
}

}  // namespace zly
