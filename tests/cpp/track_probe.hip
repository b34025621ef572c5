// track_probe.hip -- TEST INFRASTRUCTURE (never part of libzly.so): single launches of the SHIPPED zoom_plan_kernel, track_kernel and
// track_motion_kernel on track tables, frame records, descriptor blocks, merge tables and slabs the caller wrote byte for byte.  Linked against the
// very kernels_zoom.o and kernels_track.o that go into libzly.so (Makefile: $(OUT)/libtrack_probe.so, -Wl,-Bsymbolic so that its calls bind to its
// own copy when libzly.so lives in the same process); tests/test_gpu_track_tables.py loads it with ctypes.
//
// Every entry uploads, launches ONCE, synchronises and copies back, and returns the first HIP error code (0 = hipSuccess) -- or -1, having launched
// nothing, for arguments the kernels must not see.  Every device buffer is allocated with `guard` more bytes of the fill byte behind its payload, and
// the host arrays the results come back in are payload + guard long: the guard comes back too.
#include "zly_internal.h"
#include "zoom_rules.h"
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <vector>

using namespace zly;

#define PROBE_TRY(x) do { hipError_t r_ = (x); if (r_ != hipSuccess && rc == hipSuccess) rc = r_; } while (0)

namespace {

// one device buffer of `bytes` payload + `guard` bytes of fill behind it
struct Guarded {
    unsigned char* d = nullptr;
    size_t bytes = 0, guard = 0;
    hipError_t make(size_t b, size_t g, int fill, hipStream_t s)
    {
        bytes = b; guard = g;
        hipError_t rc = hipMalloc((void**)&d, b + g);
        if (rc == hipSuccess) rc = hipMemsetAsync(d, fill & 0xff, b + g, s);
        return rc;
    }
    hipError_t upload(const void* src, hipStream_t s) { return hipMemcpyAsync(d, src, bytes, hipMemcpyHostToDevice, s); }
    hipError_t download(void* dst) { return hipMemcpy(dst, d, bytes + guard, hipMemcpyDeviceToHost); }       // payload and guard
    hipError_t release() { hipError_t rc = d ? hipFree(d) : hipSuccess; d = nullptr; return rc; }
};

}  // namespace

// sizeof / offsetof of every record the tests write or read, and the three limits: the Python side asserts its numpy dtypes against these.
// Writes TRACK_PROBE_LAYOUT_INTS ints; returns that count (or -1 for a null pointer)
#define TRACK_PROBE_LAYOUT_INTS 40
extern "C" int track_probe_layout(int* out)
{
    if (!out) return -1;
    int k = 0;
    out[k++] = (int)sizeof(TrackStream);
    out[k++] = (int)offsetof(TrackStream, frame_no); out[k++] = (int)offsetof(TrackStream, next_id); out[k++] = (int)offsetof(TrackStream, evictions);
    out[k++] = (int)offsetof(TrackStream, live); out[k++] = (int)offsetof(TrackStream, x); out[k++] = (int)offsetof(TrackStream, y);
    out[k++] = (int)offsetof(TrackStream, w); out[k++] = (int)offsetof(TrackStream, h); out[k++] = (int)offsetof(TrackStream, cls);
    out[k++] = (int)offsetof(TrackStream, id); out[k++] = (int)offsetof(TrackStream, last_seen);                                       // 12
    out[k++] = (int)sizeof(TrackMotion);
    out[k++] = (int)offsetof(TrackMotion, vx); out[k++] = (int)offsetof(TrackMotion, vy); out[k++] = (int)offsetof(TrackMotion, hits);  // 16
    out[k++] = (int)sizeof(ZoomFrame);
    out[k++] = (int)offsetof(ZoomFrame, off); out[k++] = (int)offsetof(ZoomFrame, pitch); out[k++] = (int)offsetof(ZoomFrame, W);
    out[k++] = (int)offsetof(ZoomFrame, H); out[k++] = (int)offsetof(ZoomFrame, stream); out[k++] = (int)offsetof(ZoomFrame, fmt);
    out[k++] = (int)offsetof(ZoomFrame, planes); out[k++] = (int)offsetof(ZoomFrame, xstep); out[k++] = (int)offsetof(ZoomFrame, xsh);
    out[k++] = (int)offsetof(ZoomFrame, ysh);                                                                                          // 27
    out[k++] = (int)sizeof(zly_zoom_region);
    out[k++] = (int)offsetof(zly_zoom_region, slot); out[k++] = (int)offsetof(zly_zoom_region, track_id);                              // 30
    out[k++] = (int)sizeof(FrameDesc);
    out[k++] = (int)offsetof(FrameDesc, src_off); out[k++] = (int)offsetof(FrameDesc, w); out[k++] = (int)offsetof(FrameDesc, h);       // 34
    out[k++] = (int)sizeof(ViewRec);
    out[k++] = (int)offsetof(ViewRec, off1); out[k++] = (int)offsetof(ViewRec, off2);                                                  // 37
    out[k++] = ZLY_MERGE_TILE_INTS; out[k++] = ZLY_TRACK_MAX; out[k++] = ZLY_ZOOM_MAX_REGIONS;                                         // 40
    static_assert(TRACK_PROBE_LAYOUT_INTS == 40, "the list above");
    return k;
}

// One launch of zoom_plan_kernel (through launch_zoom_plan, nothing else) on n frames.
//   states: n_streams TrackStream records; motion: n_streams TrackMotion records or null (the kernel is then given null: vx = vy = 0);
//   views, streams: the n frames' surfaces and their stream indices; each ZoomFrame is made by zoom_frame_of (csrc/zoom_rules.h), as the engine makes it;
//   desc_io: null (the kernel is given null), or the descriptor block as the kernel expects it -- n * (1 + K) FrameDesc, then as many ViewRec --
//            + guard bytes: uploaded, and read back with its guard;
//   tab_io: null, or the merge table -- n + 1 offsets, then n * (1 + K) members of ZLY_MERGE_TILE_INTS ints -- + guard bytes: likewise;
//   plan_out: n * K zly_zoom_region + guard bytes; the device buffer holds the fill byte before the launch;
//   states_out, motion_out, frames_out (each may be null): the tables and the n ZoomFrame records as they are AFTER the launch, + guard bytes each.
extern "C" int track_probe_zoom(const void* states, int n_streams, const void* motion, const zly_frame_view* views, const int32_t* streams, int n, int K, int T,
                                int region_w, int region_h, int max_age, int class_id, void* desc_io, void* tab_io, void* plan_out, void* states_out,
                                void* motion_out, void* frames_out, int fill, int guard)
{
    if (!states || !views || !streams || !plan_out) return -1;
    if (n < 1 || n > 4096 || n_streams < 1 || K < 1 || K > ZLY_ZOOM_MAX_REGIONS || T < 1 || T > ZLY_TRACK_MAX || guard < 0 || guard > (1 << 20)) return -1;
    zly_zoom_config cfg{};
    cfg.regions = K; cfg.region_w = region_w; cfg.region_h = region_h; cfg.max_age = max_age; cfg.class_id = class_id;
    if (zoom_check_config(&cfg, nullptr) != ZLY_OK) return -1;
    std::vector<ZoomFrame> zf((size_t)n);
    for (int i = 0; i < n; ++i) {
        size_t need = 0;
        if (streams[i] < 0 || streams[i] >= n_streams) return -1;
        if (zoom_check_surface(&views[i], nullptr) != ZLY_OK || !view_valid(&views[i], &need)) return -1;
        for (int p = 0; p < 3; ++p) if (views[i].off[p] >> ZLY_DESC_FMT_SHIFT) return -1;          // the format rides in the top byte
        zf[(size_t)i] = zoom_frame_of(&views[i], streams[i]);
    }
    const size_t nb = (size_t)n * (size_t)(1 + K);
    const size_t desc_bytes = nb * (sizeof(FrameDesc) + sizeof(ViewRec));
    const size_t tab_bytes = ((size_t)n + 1 + nb * ZLY_MERGE_TILE_INTS) * sizeof(int);
    const size_t g = (size_t)guard;

    hipError_t rc = hipSuccess;
    hipStream_t s = nullptr;
    Guarded d_states, d_motion, d_frames, d_desc, d_tab, d_plan;
    PROBE_TRY(hipStreamCreate(&s));
    if (rc == hipSuccess) {
        PROBE_TRY(d_states.make((size_t)n_streams * sizeof(TrackStream), g, fill, s));
        if (motion) PROBE_TRY(d_motion.make((size_t)n_streams * sizeof(TrackMotion), g, fill, s));
        PROBE_TRY(d_frames.make((size_t)n * sizeof(ZoomFrame), g, fill, s));
        if (desc_io) PROBE_TRY(d_desc.make(desc_bytes, g, fill, s));
        if (tab_io) PROBE_TRY(d_tab.make(tab_bytes, g, fill, s));
        PROBE_TRY(d_plan.make((size_t)n * K * sizeof(zly_zoom_region), g, fill, s));
    }
    if (rc == hipSuccess) {
        PROBE_TRY(d_states.upload(states, s));
        if (motion) PROBE_TRY(d_motion.upload(motion, s));
        PROBE_TRY(d_frames.upload(zf.data(), s));
        if (desc_io) PROBE_TRY(d_desc.upload(desc_io, s));
        if (tab_io) PROBE_TRY(d_tab.upload(tab_io, s));
    }
    if (rc == hipSuccess)
        PROBE_TRY(launch_zoom_plan(reinterpret_cast<const TrackStream*>(d_states.d), reinterpret_cast<const TrackMotion*>(d_motion.d),
                                   reinterpret_cast<const ZoomFrame*>(d_frames.d), n, reinterpret_cast<FrameDesc*>(d_desc.d), reinterpret_cast<int*>(d_tab.d),
                                   reinterpret_cast<zly_zoom_region*>(d_plan.d), K, T, region_w, region_h, max_age, class_id, s));
    if (rc == hipSuccess) PROBE_TRY(hipStreamSynchronize(s));
    if (rc == hipSuccess) {
        PROBE_TRY(d_plan.download(plan_out));
        if (desc_io) PROBE_TRY(d_desc.download(desc_io));
        if (tab_io) PROBE_TRY(d_tab.download(tab_io));
        if (states_out) PROBE_TRY(d_states.download(states_out));
        if (motion_out && motion) PROBE_TRY(d_motion.download(motion_out));
        if (frames_out) PROBE_TRY(d_frames.download(frames_out));
    }
    if (s) PROBE_TRY(hipStreamDestroy(s));
    PROBE_TRY(d_states.release()); PROBE_TRY(d_motion.release()); PROBE_TRY(d_frames.release());
    PROBE_TRY(d_desc.release()); PROBE_TRY(d_tab.release()); PROBE_TRY(d_plan.release());
    return (int)rc;
}

// One launch of track_kernel (motion_io null: launch_track) or track_motion_kernel (launch_track_motion) on the call described by grp.
//   states_io: n_streams TrackStream + guard bytes, in and out; motion_io: null, or n_streams TrackMotion + guard bytes, in and out;
//   grp: the call's table as zly_internal.h describes it, grp_ints long -- checked here entry by entry, since the kernels index with it;
//   slabs_io: n_slabs slabs of 16 + 40 * cap bytes + guard bytes, in and out.
extern "C" int track_probe_track(void* states_io, int n_streams, void* motion_io, const int* grp, int grp_ints, void* slabs_io, int n_slabs, int cap, int T,
                                 float match_iou, uint32_t max_lost, float beta, float v_max, int fill, int guard)
{
    if (!states_io || !grp || !slabs_io) return -1;
    if (n_streams < 1 || n_slabs < 1 || cap < 1 || cap > ZLY_TRACK_MAX || T < 1 || T > ZLY_TRACK_MAX || cap > T || guard < 0 || guard > (1 << 20)) return -1;
    if (grp_ints < 4) return -1;
    const int S = grp[0];
    if (S < 1 || S > n_streams || (long long)2 + 2 * (long long)S > grp_ints) return -1;
    const int n_frames = grp[1 + S];
    if (grp[1] != 0 || n_frames < 1 || (long long)2 + 2 * (long long)S + n_frames != grp_ints) return -1;
    std::vector<char> stream_used((size_t)n_streams, 0), slab_used((size_t)n_slabs, 0);
    for (int k = 0; k < S; ++k) {
        if (grp[1 + k] >= grp[2 + k]) return -1;                                         // every segment has a frame; offsets ascend
        const int st = grp[2 + S + k];
        if (st < 0 || st >= n_streams || stream_used[(size_t)st]) return -1;             // one workgroup per stream
        stream_used[(size_t)st] = 1;
    }
    for (int j = 0; j < n_frames; ++j) {
        const int f = grp[2 + 2 * S + j];
        if (f < 0 || f >= n_slabs || slab_used[(size_t)f]) return -1;
        slab_used[(size_t)f] = 1;
    }
    const size_t slab_bytes = sizeof(zly_slab_header) + (size_t)cap * sizeof(zly_det);
    const size_t g = (size_t)guard;

    hipError_t rc = hipSuccess;
    hipStream_t s = nullptr;
    Guarded d_states, d_motion, d_grp, d_slabs;
    PROBE_TRY(hipStreamCreate(&s));
    if (rc == hipSuccess) {
        PROBE_TRY(d_states.make((size_t)n_streams * sizeof(TrackStream), g, fill, s));
        if (motion_io) PROBE_TRY(d_motion.make((size_t)n_streams * sizeof(TrackMotion), g, fill, s));
        PROBE_TRY(d_grp.make((size_t)grp_ints * sizeof(int), g, fill, s));
        PROBE_TRY(d_slabs.make((size_t)n_slabs * slab_bytes, g, fill, s));
    }
    if (rc == hipSuccess) {
        PROBE_TRY(d_states.upload(states_io, s));
        if (motion_io) PROBE_TRY(d_motion.upload(motion_io, s));
        PROBE_TRY(d_grp.upload(grp, s));
        PROBE_TRY(d_slabs.upload(slabs_io, s));
    }
    if (rc == hipSuccess) {
        if (motion_io)
            PROBE_TRY(launch_track_motion(reinterpret_cast<TrackStream*>(d_states.d), reinterpret_cast<TrackMotion*>(d_motion.d),
                                          reinterpret_cast<const int*>(d_grp.d), S, d_slabs.d, cap, T, match_iou, max_lost, beta, v_max, s));
        else
            PROBE_TRY(launch_track(reinterpret_cast<TrackStream*>(d_states.d), reinterpret_cast<const int*>(d_grp.d), S, d_slabs.d, cap, T, match_iou, max_lost, s));
    }
    if (rc == hipSuccess) PROBE_TRY(hipStreamSynchronize(s));
    if (rc == hipSuccess) {
        PROBE_TRY(d_states.download(states_io));
        if (motion_io) PROBE_TRY(d_motion.download(motion_io));
        PROBE_TRY(d_slabs.download(slabs_io));
    }
    if (s) PROBE_TRY(hipStreamDestroy(s));
    PROBE_TRY(d_states.release()); PROBE_TRY(d_motion.release()); PROBE_TRY(d_grp.release()); PROBE_TRY(d_slabs.release());
    return (int)rc;
}
