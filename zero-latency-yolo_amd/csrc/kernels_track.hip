// kernels_track.hip -- frame-to-frame association of a stream's detections on gfx950 (the rule and the step: include/zly.h, "Tracking").
//
// One workgroup of ONE wavefront per distinct stream of a call.  It loads the stream's track table (lane t = slot t), walks the stream's
// frames of the call in index order -- the sequential part: frame k's table is frame k-1's result -- and stores the table once.
// Per frame, with K <= 64 stored detections (lane d = detection d) and T <= 64 slots:
//   1. the K x T matrix of candidate IoUs (0 = no candidate) goes to LDS, lane t computing column t against the broadcast detection;
//   2. greedy matching as rounds of mutually-best pairs: every free slot finds its best free detection (IoU desc, d asc), every free
//      detection its best free slot (IoU desc, t asc); a pair that is both is the first of the specification's total order among the pairs that
//      touch its detection or its slot, so the sequential greedy loop accepts it -- and the overall best remaining pair always is one, so every
//      round accepts at least one pair.  Scenes of objects that do not overlap each other finish in one round;
//   3. expiry, then births: free slots in ascending order first, then evictions by (last_seen, slot), ranked with readlane broadcasts.
// track_motion_kernel is the same walk with the opt-in constant-velocity model (zly_track_motion_enable): lane t predicts its slot's box to the
// frame before step 1, the candidates are taken against the prediction, and an accepted pair updates the slot's vx, vy and hits beside its box.
// FP contraction is OFF for this file: the IoU is the same sequence of IEEE fp32 operations as iou_cxcywh in kernels_post.hip, and the motion
// model's products, quotients and sums are rounded one by one.
#include "zly_internal.h"

#pragma clang fp contract(off)

namespace zly {

#define TRK_PITCH 65              // row pitch of the IoU matrix in LDS: a lane that walks ITS row (detection lanes) hits 64 different banks

__device__ __forceinline__ float trk_rl_f(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }
__device__ __forceinline__ int trk_rl_i(int v, int l) { return __builtin_amdgcn_readlane(v, l); }

// LDS hand-over inside the one wave
__device__ __forceinline__ void trk_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// calculateIoU exactly as iou_cxcywh (kernels_post.hip): a = the detection, b = the slot
__device__ __forceinline__ float trk_iou(float ax, float ay, float aw, float ah, float bx, float by, float bw, float bh)
{
    const float ax0 = ax - aw / 2, ay0 = ay - ah / 2, ax1 = ax + aw / 2, ay1 = ay + ah / 2;
    const float bx0 = bx - bw / 2, by0 = by - bh / 2, bx1 = bx + bw / 2, by1 = by + bh / 2;
    const float lo_x = (ax0 < bx0) ? bx0 : ax0, hi_x = (bx1 < ax1) ? bx1 : ax1;
    const float lo_y = (ay0 < by0) ? by0 : ay0, hi_y = (by1 < ay1) ? by1 : ay1;
    const float dx = hi_x - lo_x, dy = hi_y - lo_y;
    const float ox = (0.0f < dx) ? dx : 0.0f;
    const float oy = (0.0f < dy) ? dy : 0.0f;
    const float inter = ox * oy;
    const float area_a = aw * ah, area_b = bw * bh;
    const float uni = area_a + area_b - inter;
    return (uni > 0) ? inter / uni : 0.0f;
}

// the j-th id after n0 in the sequence n0, n0 + 1, ..., 0xFFFFFFFF, 1, 2, ... (0 is never an id); j <= 64
__device__ __forceinline__ uint32_t trk_id_after(uint32_t n0, int j)
{
    const unsigned long long r = (unsigned long long)n0 + (unsigned long long)j;
    return r > 0xFFFFFFFFull ? (uint32_t)(r - 0xFFFFFFFFull) : (uint32_t)r;
}

// A frame as the walk needs it: the header's count and detection `lane`.  The detections are requested without waiting for the count (the slab holds cap
// records whatever n_kept says; those at or beyond it are masked afterwards), so that a frame costs one global round trip, and the walk requests
// frame k + 1 before it works on frame k: the serial case is a chain of round trips otherwise (measured: 1.5 us per frame with next to nothing to match).
struct TrkFrame { int n_kept; float x, y, w, h; int cls; };
__device__ __forceinline__ TrkFrame trk_load(const unsigned char* __restrict__ slabs, size_t slab_bytes, int f, int lane, int cap)
{
    const unsigned char* slab = slabs + (size_t)f * slab_bytes;
    const zly_det* dets = reinterpret_cast<const zly_det*>(slab + sizeof(zly_slab_header));
    TrkFrame r;
    r.n_kept = reinterpret_cast<const zly_slab_header*>(slab)->n_kept;
    r.x = r.y = r.w = r.h = 0.f; r.cls = -1;
    if (lane < cap) { r.x = dets[lane].x; r.y = dets[lane].y; r.w = dets[lane].w; r.h = dets[lane].h; r.cls = dets[lane].class_id; }
    return r;
}

__global__ __launch_bounds__(64) void track_kernel(TrackStream* __restrict__ states, const int* __restrict__ grp, unsigned char* __restrict__ slabs,
                                                   int cap, int T, float match_iou, uint32_t max_lost)
{
    __shared__ float M[64 * TRK_PITCH];     // candidate IoU of (detection d, slot t) at d * TRK_PITCH + t; 0 = not a candidate
    __shared__ int order[64];               // birth j takes slot order[j]: free slots ascending, then eviction candidates by (last_seen, slot)
    __shared__ int born[64];                // slot -> the detection born into it in this frame, -1 = none

    const int lane = threadIdx.x;
    const unsigned long long below = (1ull << lane) - 1ull;
    const int n_seg = grp[0];
    const int seg = blockIdx.x;
    const int f_begin = grp[1 + seg], f_end = grp[2 + seg];
    TrackStream* st = states + grp[2 + n_seg + seg];
    const int* frames = grp + 2 + 2 * n_seg;
    const size_t slab_bytes = sizeof(zly_slab_header) + (size_t)cap * sizeof(zly_det);

    uint32_t frame_no = st->frame_no, next_id = st->next_id, evictions = st->evictions;
    const bool is_slot = lane < T;
    bool live = is_slot && st->live[lane] != 0u;
    float sx = st->x[lane], sy = st->y[lane], sw = st->w[lane], sh = st->h[lane];
    int scls = st->cls[lane];
    uint32_t sid = st->id[lane], seen = st->last_seen[lane];
    order[lane] = lane;                                 // every entry a slot index from the start

    // the stream's frames in chunks of 64: lane j holds the index of the chunk's j-th frame
    for (int base = f_begin; base < f_end; base += 64) {
        const int cnt = min(64, f_end - base);
        const int my_frame = lane < cnt ? frames[base + lane] : 0;
        TrkFrame nxt = trk_load(slabs, slab_bytes, trk_rl_i(my_frame, 0), lane, cap);
        for (int j = 0; j < cnt; ++j) {
            const TrkFrame cur = nxt;
            zly_det* dets = reinterpret_cast<zly_det*>(slabs + (size_t)trk_rl_i(my_frame, j) * slab_bytes + sizeof(zly_slab_header));
            if (j + 1 < cnt) nxt = trk_load(slabs, slab_bytes, trk_rl_i(my_frame, j + 1), lane, cap);
            int K = cur.n_kept;
            K = K < 0 ? 0 : (K > cap ? cap : K);
            K = __builtin_amdgcn_readfirstlane(K);
            frame_no += 1u;
            const bool is_det = lane < K;
            const float dx = is_det ? cur.x : 0.f, dy = is_det ? cur.y : 0.f, dw = is_det ? cur.w : 0.f, dh = is_det ? cur.h : 0.f;
            const int dcls = is_det ? cur.cls : -1;

            // 1. candidate matrix, column `lane`
            for (int d = 0; d < K; ++d) {
                const float bx = trk_rl_f(dx, d), by = trk_rl_f(dy, d), bw = trk_rl_f(dw, d), bh = trk_rl_f(dh, d);
                const int bc = trk_rl_i(dcls, d);
                float v = 0.f;
                if (live && bc == scls) {
                    v = trk_iou(bx, by, bw, bh, sx, sy, sw, sh);
                    if (!(v > match_iou)) v = 0.f;
                }
                M[d * TRK_PITCH + lane] = v;
            }
            born[lane] = -1;
            trk_wave_sync();

            // 2. greedy matching in rounds of mutually-best pairs
            unsigned long long freeD = K >= 64 ? ~0ull : ((1ull << K) - 1ull);          // detections not accepted yet
            unsigned long long freeT = __ballot(live);                                   // live slots not accepted yet
            uint32_t det_id = 0u;
            while (freeD != 0ull && freeT != 0ull) {
                unsigned long long ks = 0ull, kd = 0ull;                                  // (IoU bits << 6) | (63 - index): the maximum is the best, the lower index on equal IoU
                if ((freeT >> lane) & 1ull)
                    for (unsigned long long m = freeD; m; m &= m - 1ull) {
                        const int d = __builtin_ctzll(m);
                        const float v = M[d * TRK_PITCH + lane];
                        const unsigned long long key = v > 0.f ? (((unsigned long long)__float_as_uint(v) << 6) | (unsigned long long)(63 - d)) : 0ull;
                        ks = key > ks ? key : ks;
                    }
                if ((freeD >> lane) & 1ull)
                    for (unsigned long long m = freeT; m; m &= m - 1ull) {
                        const int t = __builtin_ctzll(m);
                        const float v = M[lane * TRK_PITCH + t];
                        const unsigned long long key = v > 0.f ? (((unsigned long long)__float_as_uint(v) << 6) | (unsigned long long)(63 - t)) : 0ull;
                        kd = key > kd ? key : kd;
                    }
                const bool has_s = ks != 0ull, has_d = kd != 0ull;
                if (__ballot(has_s) == 0ull) break;                                       // no candidate pair is left
                const int bd = 63 - (int)(ks & 63ull);                                    // this slot's best detection
                const int bt = 63 - (int)(kd & 63ull);                                    // this detection's best slot
                const int slot_of_bd = __shfl(has_d ? bt : -1, bd);
                const int det_of_bt = __shfl(has_s ? bd : -1, bt);
                const bool acc_s = has_s && slot_of_bd == lane;
                const bool acc_d = has_d && det_of_bt == lane;
                const float nx = __shfl(dx, bd), ny = __shfl(dy, bd), nw = __shfl(dw, bd), nh = __shfl(dh, bd);
                const uint32_t id_of_bt = (uint32_t)__shfl((int)sid, bt);
                if (acc_s) { sx = nx; sy = ny; sw = nw; sh = nh; seen = frame_no; }
                if (acc_d) det_id = id_of_bt;
                freeT &= ~__ballot(acc_s);
                freeD &= ~__ballot(acc_d);
            }

            // 3. expiry of the live slots that were not matched
            if (live && ((freeT >> lane) & 1ull) && frame_no - seen > max_lost) live = false;

            // 4. births, in ascending detection index
            const int n_born = __popcll(freeD);
            if (n_born > 0) {
                const unsigned long long F = __ballot(is_slot && !live);
                const int n_free = __popcll(F);
                const bool evictable = live && ((freeT >> lane) & 1ull);                  // live, not matched in this frame (and, being ranked before any birth, not born in it)
                int pos = -1;
                if (is_slot && !live) pos = __popcll(F & below);
                if (n_born > n_free) {                                                    // wave-uniform
                    const unsigned long long E = __ballot(evictable);
                    int rank = 0;
                    for (unsigned long long m = E; m; m &= m - 1ull) {
                        const int t = __builtin_ctzll(m);
                        const uint32_t ls = (uint32_t)trk_rl_i((int)seen, t);
                        rank += (ls < seen || (ls == seen && t < lane)) ? 1 : 0;
                    }
                    if (evictable) pos = n_free + rank;
                    evictions += (uint32_t)(n_born - n_free);
                }
                if (pos >= 0) order[pos] = lane;
                trk_wave_sync();
                const int j = __popcll(freeD & below);                                    // this detection's birth index
                if ((freeD >> lane) & 1ull) {
                    born[order[j]] = lane;
                    det_id = trk_id_after(next_id, j);
                }
                trk_wave_sync();
                const int b = born[lane];
                const int bsrc = b < 0 ? 0 : b;
                const float nx = __shfl(dx, bsrc), ny = __shfl(dy, bsrc), nw = __shfl(dw, bsrc), nh = __shfl(dh, bsrc);
                const int ncls = __shfl(dcls, bsrc);
                const uint32_t nid = (uint32_t)__shfl((int)det_id, bsrc);
                if (is_slot && b >= 0) { live = true; sx = nx; sy = ny; sw = nw; sh = nh; scls = ncls; sid = nid; seen = frame_no; }
                next_id = trk_id_after(next_id, n_born);
            }
            if (lane < K) dets[lane].track_id = det_id;
            trk_wave_sync();                                                              // the next frame rewrites M, born and order
        }
    }

    st->live[lane] = live ? 1u : 0u;
    st->x[lane] = sx; st->y[lane] = sy; st->w[lane] = sw; st->h[lane] = sh;
    st->cls[lane] = scls; st->id[lane] = sid; st->last_seen[lane] = seen;
    if (lane == 0) { st->frame_no = frame_no; st->next_id = next_id; st->evictions = evictions; }
}

// track_kernel with the constant-velocity motion model (include/zly.h, steps P, 2', 4'), for an engine that has called zly_track_motion_enable;
// motion[i] belongs to states[i].  The walk is track_kernel's, line for line -- a copy, not a shared body: sharing one through a template changed
// track_kernel's own assembly, and an engine without the model must run exactly what it ran before.  What differs is marked "motion:".
__global__ __launch_bounds__(64) void track_motion_kernel(TrackStream* __restrict__ states, TrackMotion* __restrict__ motion, const int* __restrict__ grp,
                                                          unsigned char* __restrict__ slabs, int cap, int T, float match_iou, uint32_t max_lost, float beta,
                                                          float v_max)
{
    __shared__ float M[64 * TRK_PITCH];
    __shared__ int order[64];
    __shared__ int born[64];

    const int lane = threadIdx.x;
    const unsigned long long below = (1ull << lane) - 1ull;
    const int n_seg = grp[0];
    const int seg = blockIdx.x;
    const int f_begin = grp[1 + seg], f_end = grp[2 + seg];
    TrackStream* st = states + grp[2 + n_seg + seg];
    TrackMotion* mo = motion + grp[2 + n_seg + seg];
    const int* frames = grp + 2 + 2 * n_seg;
    const size_t slab_bytes = sizeof(zly_slab_header) + (size_t)cap * sizeof(zly_det);

    uint32_t frame_no = st->frame_no, next_id = st->next_id, evictions = st->evictions;
    const bool is_slot = lane < T;
    bool live = is_slot && st->live[lane] != 0u;
    float sx = st->x[lane], sy = st->y[lane], sw = st->w[lane], sh = st->h[lane];
    int scls = st->cls[lane];
    uint32_t sid = st->id[lane], seen = st->last_seen[lane];
    float mvx = mo->vx[lane], mvy = mo->vy[lane];                                       // motion: the slot's velocity per frame and its hit count
    uint32_t mhits = mo->hits[lane];
    order[lane] = lane;

    for (int base = f_begin; base < f_end; base += 64) {
        const int cnt = min(64, f_end - base);
        const int my_frame = lane < cnt ? frames[base + lane] : 0;
        TrkFrame nxt = trk_load(slabs, slab_bytes, trk_rl_i(my_frame, 0), lane, cap);
        for (int j = 0; j < cnt; ++j) {
            const TrkFrame cur = nxt;
            zly_det* dets = reinterpret_cast<zly_det*>(slabs + (size_t)trk_rl_i(my_frame, j) * slab_bytes + sizeof(zly_slab_header));
            if (j + 1 < cnt) nxt = trk_load(slabs, slab_bytes, trk_rl_i(my_frame, j + 1), lane, cap);
            int K = cur.n_kept;
            K = K < 0 ? 0 : (K > cap ? cap : K);
            K = __builtin_amdgcn_readfirstlane(K);
            frame_no += 1u;
            const bool is_det = lane < K;
            const float dx = is_det ? cur.x : 0.f, dy = is_det ? cur.y : 0.f, dw = is_det ? cur.w : 0.f, dh = is_det ? cur.h : 0.f;
            const int dcls = is_det ? cur.cls : -1;

            // motion: P. this slot's box predicted to the frame, once: the product is rounded, then the sum (dt >= 1 for a live slot)
            const float dtf = (float)(frame_no - seen);
            const float px = sx + mvx * dtf, py = sy + mvy * dtf;

            // 1. candidate matrix, column `lane`; motion: against the predicted box
            for (int d = 0; d < K; ++d) {
                const float bx = trk_rl_f(dx, d), by = trk_rl_f(dy, d), bw = trk_rl_f(dw, d), bh = trk_rl_f(dh, d);
                const int bc = trk_rl_i(dcls, d);
                float v = 0.f;
                if (live && bc == scls) {
                    v = trk_iou(bx, by, bw, bh, px, py, sw, sh);
                    if (!(v > match_iou)) v = 0.f;
                }
                M[d * TRK_PITCH + lane] = v;
            }
            born[lane] = -1;
            trk_wave_sync();

            // 2. greedy matching in rounds of mutually-best pairs
            unsigned long long freeD = K >= 64 ? ~0ull : ((1ull << K) - 1ull);
            unsigned long long freeT = __ballot(live);
            uint32_t det_id = 0u;
            while (freeD != 0ull && freeT != 0ull) {
                unsigned long long ks = 0ull, kd = 0ull;
                if ((freeT >> lane) & 1ull)
                    for (unsigned long long m = freeD; m; m &= m - 1ull) {
                        const int d = __builtin_ctzll(m);
                        const float v = M[d * TRK_PITCH + lane];
                        const unsigned long long key = v > 0.f ? (((unsigned long long)__float_as_uint(v) << 6) | (unsigned long long)(63 - d)) : 0ull;
                        ks = key > ks ? key : ks;
                    }
                if ((freeD >> lane) & 1ull)
                    for (unsigned long long m = freeT; m; m &= m - 1ull) {
                        const int t = __builtin_ctzll(m);
                        const float v = M[lane * TRK_PITCH + t];
                        const unsigned long long key = v > 0.f ? (((unsigned long long)__float_as_uint(v) << 6) | (unsigned long long)(63 - t)) : 0ull;
                        kd = key > kd ? key : kd;
                    }
                const bool has_s = ks != 0ull, has_d = kd != 0ull;
                if (__ballot(has_s) == 0ull) break;
                const int bd = 63 - (int)(ks & 63ull);
                const int bt = 63 - (int)(kd & 63ull);
                const int slot_of_bd = __shfl(has_d ? bt : -1, bd);
                const int det_of_bt = __shfl(has_s ? bd : -1, bt);
                const bool acc_s = has_s && slot_of_bd == lane;
                const bool acc_d = has_d && det_of_bt == lane;
                const float nx = __shfl(dx, bd), ny = __shfl(dy, bd), nw = __shfl(dw, bd), nh = __shfl(dh, bd);
                const uint32_t id_of_bt = (uint32_t)__shfl((int)sid, bt);
                if (acc_s) {
                    // motion: 4'. the velocity takes the residual against the prediction, per frame of the gap; the first match takes all of it
                    const float rx = nx - px, ry = ny - py;
                    const float g = mhits == 1u ? 1.0f : beta;
                    const float ux = mvx + g * (rx / dtf), uy = mvy + g * (ry / dtf);
                    mvx = ux < -v_max ? -v_max : (ux > v_max ? v_max : ux);
                    mvy = uy < -v_max ? -v_max : (uy > v_max ? v_max : uy);
                    mhits = mhits == 0xFFFFFFFFu ? mhits : mhits + 1u;
                    sx = nx; sy = ny; sw = nw; sh = nh; seen = frame_no;
                }
                if (acc_d) det_id = id_of_bt;
                freeT &= ~__ballot(acc_s);
                freeD &= ~__ballot(acc_d);
            }

            // 3. expiry of the live slots that were not matched
            if (live && ((freeT >> lane) & 1ull) && frame_no - seen > max_lost) live = false;

            // 4. births, in ascending detection index
            const int n_born = __popcll(freeD);
            if (n_born > 0) {
                const unsigned long long F = __ballot(is_slot && !live);
                const int n_free = __popcll(F);
                const bool evictable = live && ((freeT >> lane) & 1ull);
                int pos = -1;
                if (is_slot && !live) pos = __popcll(F & below);
                if (n_born > n_free) {
                    const unsigned long long E = __ballot(evictable);
                    int rank = 0;
                    for (unsigned long long m = E; m; m &= m - 1ull) {
                        const int t = __builtin_ctzll(m);
                        const uint32_t ls = (uint32_t)trk_rl_i((int)seen, t);
                        rank += (ls < seen || (ls == seen && t < lane)) ? 1 : 0;
                    }
                    if (evictable) pos = n_free + rank;
                    evictions += (uint32_t)(n_born - n_free);
                }
                if (pos >= 0) order[pos] = lane;
                trk_wave_sync();
                const int j = __popcll(freeD & below);
                if ((freeD >> lane) & 1ull) {
                    born[order[j]] = lane;
                    det_id = trk_id_after(next_id, j);
                }
                trk_wave_sync();
                const int b = born[lane];
                const int bsrc = b < 0 ? 0 : b;
                const float nx = __shfl(dx, bsrc), ny = __shfl(dy, bsrc), nw = __shfl(dw, bsrc), nh = __shfl(dh, bsrc);
                const int ncls = __shfl(dcls, bsrc);
                const uint32_t nid = (uint32_t)__shfl((int)det_id, bsrc);
                if (is_slot && b >= 0) {
                    live = true; sx = nx; sy = ny; sw = nw; sh = nh; scls = ncls; sid = nid; seen = frame_no;
                    mvx = 0.f; mvy = 0.f; mhits = 1u;                                     // motion: a birth starts at rest
                }
                next_id = trk_id_after(next_id, n_born);
            }
            if (lane < K) dets[lane].track_id = det_id;
            trk_wave_sync();
        }
    }

    st->live[lane] = live ? 1u : 0u;
    st->x[lane] = sx; st->y[lane] = sy; st->w[lane] = sw; st->h[lane] = sh;
    st->cls[lane] = scls; st->id[lane] = sid; st->last_seen[lane] = seen;
    if (lane == 0) { st->frame_no = frame_no; st->next_id = next_id; st->evictions = evictions; }
    mo->vx[lane] = mvx; mo->vy[lane] = mvy; mo->hits[lane] = mhits;
}

__global__ __launch_bounds__(64) void track_reset_kernel(TrackStream* __restrict__ states, uint32_t first_id)
{
    TrackStream* st = states + blockIdx.x;
    const int lane = threadIdx.x;
    st->live[lane] = 0u;
    st->x[lane] = 0.f; st->y[lane] = 0.f; st->w[lane] = 0.f; st->h[lane] = 0.f;
    st->cls[lane] = 0; st->id[lane] = 0u; st->last_seen[lane] = 0u;
    if (lane == 0) {
        st->frame_no = 0u; st->evictions = 0u; st->pad_ = 0u;
        if (first_id != 0u) st->next_id = first_id;
    }
}

__global__ __launch_bounds__(64) void track_motion_reset_kernel(TrackMotion* __restrict__ motion)
{
    TrackMotion* mo = motion + blockIdx.x;
    const int lane = threadIdx.x;
    mo->vx[lane] = 0.f; mo->vy[lane] = 0.f; mo->hits[lane] = 0u;
}

hipError_t launch_track(TrackStream* states, const int* grp, int n_seg, void* slabs, int cap, int max_tracks, float match_iou, uint32_t max_lost, hipStream_t s)
{
    if (n_seg < 1 || cap < 1 || cap > max_tracks || max_tracks > ZLY_TRACK_MAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL(track_kernel, dim3(n_seg), dim3(64), 0, s, states, grp, (unsigned char*)slabs, cap, max_tracks, match_iou, max_lost);
    return hipGetLastError();
}

hipError_t launch_track_reset(TrackStream* states, int first, int count, uint32_t first_id, hipStream_t s)
{
    if (first < 0 || count < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(track_reset_kernel, dim3(count), dim3(64), 0, s, states + first, first_id);
    return hipGetLastError();
}

hipError_t launch_track_motion(TrackStream* states, TrackMotion* motion, const int* grp, int n_seg, void* slabs, int cap, int max_tracks, float match_iou,
                               uint32_t max_lost, float beta, float v_max, hipStream_t s)
{
    if (!motion || n_seg < 1 || cap < 1 || cap > max_tracks || max_tracks > ZLY_TRACK_MAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL(track_motion_kernel, dim3(n_seg), dim3(64), 0, s, states, motion, grp, (unsigned char*)slabs, cap, max_tracks, match_iou, max_lost, beta, v_max);
    return hipGetLastError();
}

hipError_t launch_track_motion_reset(TrackMotion* motion, int first, int count, hipStream_t s)
{
    if (!motion || first < 0 || count < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(track_motion_reset_kernel, dim3(count), dim3(64), 0, s, motion + first);
    return hipGetLastError();
}

}  // namespace zly
