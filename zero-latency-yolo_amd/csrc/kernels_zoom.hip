// kernels_zoom.hip -- the plan of a frame's zoom regions on gfx950 (the rule: include/zly.h, "Zoom regions"; its arithmetic: zoom_device.h).
//
// One workgroup of ONE wavefront per frame of a call, lane t = slot t of the frame's stream -- the tracker's layout.  It reads the stream's track
// table where the tracker left it (it is launched behind the previous call's tracking), and
//   1. every lane decides its slot's eligibility, age, area key and prediction;
//   2. every eligible lane counts the eligible slots that come before its own (a ballot walk with readlane broadcasts): its place in the order;
//   3. the greedy choice walks the places in turn: the slot of place r is broadcast, lane j < chosen tests it against region j (the regions chosen
//      so far live one per lane), a ballot says whether any covers it, and an uncovered slot's region goes to lane `chosen`;
//   4. lanes chosen .. K - 1 take the fallback; lane j < K then stores region j: the plan record and, in a frame call, what depends on the origin in
//      the frame's descriptor (FrameDesc::src_off), its view record (ViewRec::off1 / off2) and its tile of the merge table (x0, y0).  Everything else
//      in those three tables the host has uploaded, with every region at its fallback origin.
// Stores are per-lane vector stores in plain C++.  FP contraction is OFF for this file, as for kernels_track.hip, and the pragma stands IN FRONT of
// zoom_device.h, whose functions hold all the float arithmetic (they also turn it off in their own bodies): the prediction is a rounded product,
// then a rounded sum -- never an fma.
#include "zly_internal.h"

#pragma clang fp contract(off)

#include "zoom_device.h"

namespace zly {

__device__ __forceinline__ float zm_rl_f(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }
__device__ __forceinline__ int zm_rl_i(int v, int l) { return __builtin_amdgcn_readlane(v, l); }

// desc: the call's n_views descriptors with its n_views view records behind them, frame i's views at i * (1 + K) (null: plan only);
// tab: the call's merge table of n groups of 1 + K members each (null: plan only); plan: n * K records
__global__ __launch_bounds__(64) void zoom_plan_kernel(const TrackStream* __restrict__ states, const TrackMotion* __restrict__ motion,
                                                       const ZoomFrame* __restrict__ frames, FrameDesc* __restrict__ desc, int n_views, int* __restrict__ tab, int n,
                                                       zly_zoom_region* __restrict__ plan, int K, int T, int region_w, int region_h, int max_age, int class_id)
{
    const int lane = threadIdx.x;
    const int i = blockIdx.x;
    const ZoomFrame fr = frames[i];
    const TrackStream* st = states + fr.stream;
    const int W = fr.W, H = fr.H;
    const ZoomSize z = zoom_size(region_w, region_h, W, H);

    // 1. this lane's slot
    const uint32_t F = st->frame_no;
    const bool live = lane < T && st->live[lane] != 0u;
    const float sx = st->x[lane], sy = st->y[lane], sw = st->w[lane], sh = st->h[lane];
    const int scls = st->cls[lane];
    const uint32_t sid = st->id[lane], seen = st->last_seen[lane];
    float vx = 0.f, vy = 0.f;
    if (motion) { vx = motion[fr.stream].vx[lane]; vy = motion[fr.stream].vy[lane]; }
    const bool elig = zoom_eligible(live, scls, F, seen, sw, sh, W, H, z, max_age, class_id);
    const uint32_t age = F - seen, key = zoom_area_key(sw, sh);
    const float px = zoom_predict(sx, vx, F, seen), py = zoom_predict(sy, vy, F, seen);

    // 2. its place among the eligible slots
    const unsigned long long E = __ballot(elig);
    int place = 0;
    for (unsigned long long m = E; m; m &= m - 1ull) {
        const int t = __builtin_ctzll(m);
        const uint32_t a = (uint32_t)zm_rl_i((int)age, t), k = (uint32_t)zm_rl_i((int)key, t);
        place += zoom_before(a, k, t, age, key, lane) ? 1 : 0;
    }

    // 3. the greedy choice: lane j holds region j
    const int n_elig = __popcll(E);
    int chosen = 0;
    int rx0 = 0, ry0 = 0, rslot = -1;
    uint32_t rid = 0u;
    for (int r = 0; r < n_elig && chosen < K; ++r) {
        const int t = __builtin_ctzll(__ballot(elig && place == r));            // exactly one lane: the order is total
        const float cpx = zm_rl_f(px, t), cpy = zm_rl_f(py, t), cw = zm_rl_f(sw, t), ch = zm_rl_f(sh, t);
        const uint32_t cid = (uint32_t)zm_rl_i((int)sid, t);
        const bool cov = lane < chosen && zoom_covered_axis(cpx, cw, rx0, z.rw, W) && zoom_covered_axis(cpy, ch, ry0, z.rh, H);
        if (__ballot(cov) != 0ull) continue;
        const int nx = zoom_origin(cpx, W, z.rw, z.xmax), ny = zoom_origin(cpy, H, z.rh, z.ymax);
        if (lane == chosen) { rx0 = nx; ry0 = ny; rslot = t; rid = cid; }
        ++chosen;
    }

    // 4. fallbacks, then the stores of region `lane`
    if (lane >= chosen) { rx0 = zoom_fallback_origin(W, z.rw); ry0 = zoom_fallback_origin(H, z.rh); rslot = -1; rid = 0u; }
    if (lane < K) {
        zly_zoom_region o;
        o.x0 = rx0; o.y0 = ry0; o.w = z.rw; o.h = z.rh; o.slot = rslot; o.track_id = rid;
        plan[(size_t)i * K + lane] = o;
        const int b = i * (1 + K) + 1 + lane;                                    // the region's batch item
        if (desc) {
            desc[b].src_off = desc_pack(zoom_plane_off(fr, 0, rx0, ry0), fr.fmt);
            ViewRec* vr = reinterpret_cast<ViewRec*>(desc + n_views) + b;
            if (fr.planes > 1) vr->off1 = zoom_plane_off(fr, 1, rx0, ry0);
            if (fr.planes > 2) vr->off2 = zoom_plane_off(fr, 2, rx0, ry0);
        }
        if (tab) {
            int* mrec = tab + (n + 1) + (size_t)b * ZLY_MERGE_TILE_INTS;
            mrec[1] = rx0; mrec[2] = ry0;
        }
    }
}

hipError_t launch_zoom_plan(const TrackStream* states, const TrackMotion* motion, const ZoomFrame* frames, int n, FrameDesc* desc, int* tab, zly_zoom_region* plan,
                            int K, int max_tracks, int region_w, int region_h, int max_age, int class_id, hipStream_t s)
{
    if (!states || !frames || !plan || n < 1 || K < 1 || K > ZLY_ZOOM_MAX_REGIONS || max_tracks < 1 || max_tracks > ZLY_TRACK_MAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL(zoom_plan_kernel, dim3(n), dim3(64), 0, s, states, motion, frames, desc, n * (1 + K), tab, n, plan, K, max_tracks, region_w, region_h, max_age,
                       class_id);
    return hipGetLastError();
}

}  // namespace zly
