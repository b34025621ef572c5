// engine.cpp -- the detect engine behind the C ABI of include/zly.h: model plan, HBM layout,
// stream/graph orchestration.  Compiled with hipcc; the kernels live in kernels_*.hip.
//
// Path (reference OnnxInferenceEngine::runInference, src/inference/onnx_engine.cpp:518-646):
//   preprocess -> YOLOv8 forward (57 convs as 54 MFMA launches, SPPF pools, 2 upsamples) -> fused Detect
//   tail (6 final 1x1 convs + DFL + sigmoid + decode/threshold) -> class-aware NMS -> result slab per frame.
//
// HBM layout: every activation is NHWC, batch-major, in the engine dtype (bf16 or fp32).  Concat
// and C2f's split never move data: producers write into channel slices of the consumer's concat
// buffer (ConvArgs::out_cs/out_co) and consumers read channel slices (in_cs/in_co).
#include "zly_internal.h"
#include "frame_rules.h"
#include "surface_rules.h"
#include "zoom_rules.h"
#include "chip_rules.h"
#include "change_rules.h"
#include "camera_rules.h"
#include "upload_ring.h"
#include "weights.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <limits>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>
#include <string.h>
#include <stdio.h>
#include <stdlib.h>

namespace zly {

static thread_local std::string g_last_error;

static int fail(int code, const std::string& msg) { g_last_error = msg; return code; }

#define HIP_TRY(expr, code)                                                                        \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess)                                                                      \
            return fail((code), std::string(#expr) + ": " + hipGetErrorString(_e));                \
    } while (0)

struct View { int buf; int co; int C; };

struct Buffer {
    std::string name;
    int H = 0, W = 0, C = 0;
    bool f32 = false;          // always fp32 (final Detect logits) regardless of engine dtype
    void* ptr = nullptr;
    size_t elems_per_frame() const { return (size_t)H * W * C; }
};

enum OpKind { OP_PREPROCESS = 0, OP_CONV = 1, OP_SPPF = 2, OP_HEAD = 4, OP_NMS = 6 };

struct Op {
    int kind = 0;
    std::string name;
    int lane = 0;                      // 0 = main stream; 1, 2 = Detect-branch streams that run beside the neck
    int level = 0;                     // OP_HEAD: the Detect level the tail op stands for
    // conv (OP_SPPF: `in` = the hidden-width slice of the block's concat buffer that the pools read)
    View in{-1, 0, 0}, out{-1, 0, 0}, res{-1, 0, 0};
    View in2{-1, 0, 0};                // 1x1 convs: second (full-size) source of a fused Upsample+Concat input; `in` is then half-size
    int ks = 1, stride = 1, act = 0, out_f32 = 0;
    int cout = 0, cout_pad = 0, nk = 0, K = 0;
    size_t w_off = 0, b_off = 0;       // offsets into the device weight blob
    std::vector<std::string> taps;     // conv names whose outputs this op produces (for zly_debug_tap)
    std::vector<int> tap_co;           // channel offset of each tap inside `out`
    std::vector<int> tap_c;
    size_t wsk_w = 0;                  // the 80 -> 80 class-branch convs: weights once more, tiled with cin_store = 80 for conv3x3_wsk_kernel (K packed across taps); 0 = none
    int pair = -1;                     // index of the PairGroup this conv is a member of (its first or second conv), -1 = none
    int c2f = -1;                      // index of the C2fGroup that covers this conv, -1 = none
    double flops = 0, bytes = 0;
    double wbytes = 0;                 // weight + bias bytes of this op (part of `bytes`)
    double cin_frac = 1.0;             // real / stored input channels (the 3-of-8 channel image, the 80-of-96 channel class branch)
};

// fused bottleneck pair (kernels_pair.hip): a bottleneck's two 3x3 convs as one launch at the first one; the second is a no-op when the pair kernel ran
struct PairGroup {
    int first = -1, second = -1;       // member ops
    int c = 0, res = 0;                // width; 1 = shortcut
    View out{-1, 0, 0};                // the second conv's output
    size_t wA = 0, bA = 0, wB = 0, bB = 0;     // the pair kernel's operands (for c = 16 its own weight tiling: one tap per 16x16x16 MFMA k-step)
};

// fused C2f block (kernels_pair.hip: c2f_kernel) around one bottleneck: launched at `leader` (cv1, or the second bottleneck's first conv for the back
// half of a two-bottleneck C2f); the other members launch nothing when it is active
struct C2fGroup {
    struct Member { int op, vis; };    // vis: the op's output with the fused kernel: 0 = in HBM, 1 = only with ZLY_FLAG_DUMP_LOGITS, 2 = stays in LDS
    int leader = -1;
    std::vector<Member> members;       // the leader included
    int mode = 0, c = 0, res = 0, cat = -1;    // mode bit 0 = cv1 in front, bit 1 = cv2 behind; width; shortcut; the block's concat buffer
    int pair = -1;                     // the PairGroup of the bottleneck it wraps (its weights and channel offsets inside cat)
    View x{-1, 0, 0}, x2{-1, 0, 0}, out{-1, 0, 0};
    View mid{-1, 0, 0};                // c = 64: the 64-channel kernel can dump the bottleneck's intermediate map (debug taps)
    size_t w1 = 0, b1 = 0, w2 = 0, b2 = 0;
    int nk1 = 0, nk2 = 0, cout2 = 0;
    int vis_of(int op) const { for (const Member& m : members) if (m.op == op) return m.vis; return 0; }
};

// fused Detect tail (kernels_head.hip): the final 1x1 convs + DFL + sigmoid + decode of all three levels.  One record per engine; the three
// tail ops (one per level) only say which level a launch stands for.
struct DetectTail {
    HeadArgs args{};                   // the launch template: the weight / activation pointers are set once the blob and the buffers are on the device
    int op[3] = {-1, -1, -1};          // the tail op of each level
    int box[3] = {-1, -1, -1}, cls[3] = {-1, -1, -1}, logits[3] = {-1, -1, -1};     // buffers the tail reads / (ZLY_FLAG_DUMP_LOGITS) writes per level
    int stem[3] = {-1, -1, -1};        // the level's Detect stem buffer: what the tail reads instead of box[] where it computes cv2.L.1 itself (Launch::box_mode)
    size_t wb[3] = {}, bb[3] = {}, wc[3] = {}, bc[3] = {};                          // final 1x1 weights / biases in the weight blob
};

// The model plan: everything build_plan derives from the model file, the config and the switches, with no device call.  Weights are offsets into
// `blob` and tensors are indices into `bufs`; upload_plan allocates, uploads and turns them into pointers.
struct Plan {
    int nc = 0, N = 0;                 // classes, anchors of all levels
    std::vector<Buffer> bufs;
    std::vector<Op> ops;               // in launch order
    std::vector<PairGroup> pairs;
    std::vector<C2fGroup> c2fs;
    DetectTail tail;
    int in_buf = -1;
    std::map<std::string, std::pair<int, int>> tap_index;   // conv name -> (op index, tap slot)
    std::map<std::string, std::pair<int, int>> tap_final;   // final Detect convs -> (logits buffer, channel offset)
    bool stem_fused = false;          // bf16 + 16-channel stem: preprocess and model.0 are one kernel on the detect paths
    bool stem1 = false;               // ... and model.1 (32 channels) as well: the stem map stays in LDS (kernels_stem.hip: stem_model1_kernel)
    size_t stem_w = 0, stem_b = 0, m1_w = 0, m1_b = 0, stem_w0p = 0;     // the front kernels' weight tilings in the blob
    int stem_out = -1, m1_out = -1;   // the buffers of model.0 / model.1
    int sppf_cv1 = -1, sppf_pool = -1, sppf_cv2 = -1;     // op indices of the SPPF block (model.9): one launch where kernels_sppf.hip covers the shape
    int det_stem[3] = {-1, -1, -1}, det_a[3] = {-1, -1, -1}, det_b[3] = {-1, -1, -1};   // op indices of the Detect convs (stem, box .1, class .1) per level
    bool det_merge_ok = false;        // all three levels suit the shared kernel shape of the merged Detect launches (latency path)
    int join_at = -1;                 // the op in front of which the side streams are joined (the P5 Detect stem)
    std::vector<uint8_t> blob;        // host image of the device weight blob: built outside the exclusive gate, released after upload
};

// What one op launches at one batch size: a record of the launch table (resolve_launches)
enum LaunchKind { LK_NONE, LK_PREPROCESS, LK_STEM, LK_STEM1, LK_CONV, LK_CONV_WSK, LK_MULTI, LK_C2F, LK_PAIR, LK_WS_PAIR, LK_SPPF_FUSED, LK_SPPF_POOL, LK_HEAD, LK_NMS };
struct Launch {
    int kind = LK_NONE;                // LK_NONE: the op's work is done inside the launch of op `covered_by`
    int covered_by = -1;               // index of the op whose launch does this op's work (the op itself when it launches)
    bool hbm = true;                   // the op's output reaches HBM (false: it stays in LDS inside a fused kernel; zly_debug_tap)
    ConvPlan conv{};                   // conv ops: the per-conv launch (conv_plan), also when a fusion covers the op (zly_forward runs model.0 / model.1 on it)
    WskPlan wsk{};                     // LK_CONV_WSK
    C2fPlan c2f{};                     // LK_C2F
    PairPlan pair{};                   // LK_PAIR
    WsPairPlan ws_pair{};              // LK_WS_PAIR
    int multi_ct = 0;                  // LK_MULTI: 3 = the three Detect stems, 2 = the six Detect branch convs
    int only_level = -1;               // LK_HEAD: -1 = all three levels, else that level only
    int box_mode[3] = {0, 0, 0};       // LK_HEAD: per level, HeadLevel::box_mode -- the tail computes the box branch's second conv itself, at surviving anchors (tail_box_mode)
    bool pool16 = false;               // LK_SPPF_POOL: sppf_pool16_kernel (else sppf_pool_kernel)
    bool lb = false;                   // LK_HEAD of a letterbox engine (ZLY_FLAG_LETTERBOX): the Detect tail's LB instantiation (kernels_lb.hip).  Set on the front launches too, where it
                                       // only names the kernel for zly_profile_ops: which front kernel runs is zly_engine::front
};

struct Ingest;        // pipelined host-to-host path (zly_submit / zly_wait), below

// Tracking (zly_track_enable; include/zly.h "Tracking"): the streams' track tables in HBM, and the ring (upload_ring.h) through which a call's grouping
// of its frames by stream reaches track_kernel.
struct Track {
    zly_track_config cfg{};
    TrackStream* d_state = nullptr;   // [max_streams]
    TrackMotion* d_motion = nullptr;  // [max_streams], allocated by zly_track_motion_enable (under mu): from then on every launch is track_motion_kernel
    zly_track_motion_config mcfg{};
    UploadRing ring;                  // an entry: 2 + 3 * max_batch int32 (zly_internal.h: launch_track)
    std::vector<int> seg_of;          // [max_streams] scratch of the grouping: a stream's segment in the current call, -1 = none yet
};

// Merging the slabs of a surface's tiles (zly_merge_slabs; include/zly.h "Tiles"): created by an engine's first merge.  The tile table of a call reaches
// merge_kernel through a ring (upload_ring.h); d_out is the engine-owned output buffer (max_batch slabs), allocated with the ring.
struct Merge {
    UploadRing ring;                  // an entry: max_batch + 1 offsets + ZLY_MERGE_TILE_INTS * max_batch int32 (zly_internal.h: launch_merge)
    unsigned char* d_out = nullptr;   // [max_batch][slab_bytes]
};

// Resident surfaces (zly_surfaces_enable; include/zly.h "Resident surfaces"): the store in HBM and what the host knows of its slots.  The job table of
// an update rides in the engine's staging buffer behind the pixels (surface_rules.h: SurfacePlan), so there is no ring: staging is reused call to call.
struct Surfaces {
    SurfaceStore store;
    std::vector<SurfaceSlot> slots;   // [max_surfaces]
    uint8_t* d_store = nullptr;       // [max_surfaces][stride]
    hipEvent_t ev_patch = nullptr;    // behind the most recent patch kernel (on the engine's stream): a detect call on a foreign stream waits for it
    bool patched = false;
    // behind the most recent zly_detect_surfaces call, on the stream its last kernel ran on: the next patch kernel waits for it, so that it never
    // overwrites a slot that a call still queued on a caller's stream reads.  Before it is recorded again the engine's stream is made to wait for
    // the previous recording: the engine's stream collects every reader, whichever streams they ran on.
    hipEvent_t ev_read = nullptr;
    bool read_pending = false;
    SurfacePlan plan;                 // scratch of the current update
    // moves (zly_surface_moves_enable): the bounce buffer through which a move that overlaps itself goes, and the scratch of the current call
    uint8_t* d_bounce = nullptr;
    size_t bounce_bytes = 0;
    SurfaceMovePlan mplan;
};

// Zoom regions (zly_zoom_enable; include/zly.h "Zoom regions"): the ring (upload_ring.h) through which a call's frame records reach zoom_plan_kernel,
// and the plans the kernel writes.
struct Zoom {
    zly_zoom_config cfg{};
    UploadRing ring;                  // an entry: max_batch ZoomFrame
    int last_frames = -1;             // the entry of the most recent frame call (-1: none yet), last_n its frames
    int last_n = 0;
    zly_zoom_region* d_plan = nullptr;    // [max_batch] of the most recent frame call (n * K <= max_batch), then [max_batch * K] of zly_zoom_plan
};

// Chips (zly_chips_enable; include/zly.h "Chips"): the ring (upload_ring.h) through which a call's frame records reach the two chip kernels, and the
// engine-owned chip slabs.
struct Chips {
    zly_chip_config cfg{};
    ChipLayout lay{};
    UploadRing ring;                  // an entry: max_batch ChipFrame
    unsigned char* d_out = nullptr;   // [max_batch][lay.slab_bytes]
};

// Change map (zly_change_enable; include/zly.h "Change map"): the streams' states, grids and records in HBM, the scratch grids of a call, and the ring
// (upload_ring.h) through which a call's frame records and items reach the two kernels.  zly_change_reset marks an entry too, without filling it.
struct Change {
    zly_change_config cfg{};
    ChangeLayout lay{};
    int max_streams = 0;
    bool zoom_on = false;             // zly_zoom_use_change
    UploadRing ring;                  // an entry: max_batch ChipFrame, then (at items_off) max_batch ChangeItem
    size_t items_off = 0;
    ChangeItem* items(unsigned char* entry) const { return reinterpret_cast<ChangeItem*>(entry + items_off); }
    uint32_t* d_sums = nullptr;       // [max_batch][ZLY_CHANGE_MAX_CELLS]: the scratch grids
    ChangeStream* d_state = nullptr;  // [max_streams]
    uint32_t* d_prev = nullptr;       // [max_streams][ZLY_CHANGE_MAX_CELLS]
    unsigned char* d_recs = nullptr;  // [max_streams][lay.rec_bytes]
};

// Camera motion (zly_camera_enable; include/zly.h "Camera motion"): the streams' states, grids and records in HBM, the scratch grids of a call, and the
// ring (upload_ring.h) through which a call's frame records and items -- or an apply's stream indices -- reach the kernels.  zly_camera_reset marks an
// entry too, without filling it.
struct Camera {
    zly_camera_config cfg{};
    CameraLayout lay{};
    int max_streams = 0;
    UploadRing ring;                  // an entry: max_batch ChipFrame, then (at items_off) max_batch CameraItem; an apply's: max_streams int32
    size_t items_off = 0;
    CameraItem* items(unsigned char* entry) const { return reinterpret_cast<CameraItem*>(entry + items_off); }
    uint32_t* d_sums = nullptr;       // [max_batch][ZLY_CHANGE_MAX_CELLS]: the scratch grids
    CameraStream* d_state = nullptr;  // [max_streams]
    uint32_t* d_prev = nullptr;       // [max_streams][ZLY_CHANGE_MAX_CELLS]
    unsigned char* d_recs = nullptr;  // [max_streams][lay.rec_bytes]
};

}  // namespace zly

using namespace zly;

static hipError_t first_error(std::initializer_list<hipError_t> rs) { for (hipError_t r : rs) if (r != hipSuccess) return r; return hipSuccess; }

// One release function per feature state, for the failure path of its *_enable (which ignores the error) and for destroy_engine: frees whatever the state
// owns so far (hipFree takes a null pointer) and the state itself; returns the first HIP error met.
static hipError_t track_free(Track* tk) { const hipError_t r = first_error({hipFree(tk->d_state), hipFree(tk->d_motion), tk->ring.destroy()}); delete tk; return r; }
static hipError_t merge_free(Merge* mg) { const hipError_t r = first_error({mg->ring.destroy(), hipFree(mg->d_out)}); delete mg; return r; }
static hipError_t surfaces_free(Surfaces* sf)
{
    const hipError_t r = first_error({hipFree(sf->d_store), hipFree(sf->d_bounce), sf->ev_patch ? hipEventDestroy(sf->ev_patch) : hipSuccess,
                                      sf->ev_read ? hipEventDestroy(sf->ev_read) : hipSuccess});
    delete sf;
    return r;
}
static hipError_t zoom_free(Zoom* zm) { const hipError_t r = first_error({zm->ring.destroy(), hipFree(zm->d_plan)}); delete zm; return r; }
static hipError_t chips_free(Chips* cp) { const hipError_t r = first_error({cp->ring.destroy(), hipFree(cp->d_out)}); delete cp; return r; }
static hipError_t change_free(Change* ch)
{
    const hipError_t r = first_error({ch->ring.destroy(), hipFree(ch->d_sums), hipFree(ch->d_state), hipFree(ch->d_prev), hipFree(ch->d_recs)});
    delete ch;
    return r;
}
static hipError_t camera_free(Camera* cm)
{
    const hipError_t r = first_error({cm->ring.destroy(), hipFree(cm->d_sums), hipFree(cm->d_state), hipFree(cm->d_prev), hipFree(cm->d_recs)});
    delete cm;
    return r;
}

struct zly_engine : Plan {
    zly_config cfg;
    std::string weights_path;
    int dev = 0;
    int dtype = ZLY_DTYPE_BF16;
    size_t esz = 2;
    ModelFile model;

    void* d_weights = nullptr;
    float* d_head = nullptr;          // [max_batch][4+nc][N]
    Cand* d_cand = nullptr;           // [max_batch][N]
    Cand* d_scratch = nullptr;        // [max_batch][N]  (NMS spill when a frame has > 1024 candidates)
    int* d_count = nullptr;           // [max_batch]
    // ZLY_FLAG_ASYNC_NMS: second candidate buffer + a stream of its own for NMS, so that NMS of call k (64 workgroups,
    // latency-bound) runs beside the first kernels of call k+1 instead of idling the chip at the end of every step
    Cand* d_cand_alt = nullptr;
    int* d_count_alt = nullptr;
    Cand* cur_cand = nullptr;         // buffers the Detect tail / NMS of the current call use
    int* cur_count = nullptr;
    hipStream_t nms_stream = nullptr;
    hipEvent_t ev_head = nullptr, ev_nms[2] = {nullptr, nullptr};
    int parity = 0;
    bool nms_recorded[2] = {false, false};
    int last_async = -1;              // parity of the last deferred NMS, -1 = none outstanding
    unsigned char* d_slabs = nullptr; // [max_batch][slab_bytes]
    FrameDesc* d_desc = nullptr;      // [max_batch]
    // per-call descriptor ring (pinned; the slot discipline of upload_ring.h over the one device copy d_desc): a call whose frame sizes differ from
    // the previous call's writes the next ring entry and uploads it in stream order, so no call ever waits for the device -- a mixed-client stream
    // (800x600 next to 416x416) used to cost a hipDeviceSynchronize
    FrameDesc* h_desc = nullptr;      // pinned [SlotRing::DEPTH][max_batch]
    SlotRing desc_ring;               // an entry's event: behind the upload that read it
    std::vector<FrameDesc> desc_cache;
    // a call on frame views (zly_*_view) uploads n ViewRec behind its n descriptors (zly_internal.h); a ring entry and d_desc hold both
    static constexpr size_t DESC_SLOT = sizeof(FrameDesc) + sizeof(ViewRec);      // bytes per frame
    std::vector<ViewRec> view_cache;
    int last_desc_n = 0;              // frames of the upload d_desc holds
    bool desc_cache_view = false;     // what d_desc holds came from a view call: a plain call and a view call never reuse each other's upload
    // ZLY_FLAG_AREA: the pre-pass's output, max_batch model-sized tight BGR frames, and the constant descriptor table the front kernel reads it with
    // (frame f at f * model_w * model_h * 3, model_w x model_h, BGR; uploaded once).  Calls on an engine are stream-ordered: no ring.
    uint8_t* d_area = nullptr;
    FrameDesc* d_area_desc = nullptr;
    bool area_view = false;           // the current call's request frames are frame views (set by run_path, with `front`)
    uint8_t* d_stage = nullptr;       // frame staging (host path)
    uint8_t* h_stage = nullptr;       // pinned
    size_t stage_bytes = 0;
    unsigned char* h_slabs = nullptr; // pinned
    float* d_scratch_f32 = nullptr;   // stage-level entry points
    size_t scratch_f32_elems = 0;

    StemArgs stem{};                  // stem_fused / stem1 (Plan): the front kernels' launch templates
    Stem1Args stem1a{};
    bool ingest_active = false;       // set while the pipelined host path (zly_submit) enqueues: see run_path
    bool last_front = false;          // the most recent call launched the front kernel (zly_forward does not: model.0 is then in HBM)
    FrontVariant front;               // which instantiation of the front kernel the current call launches (front_variants.h; set by run_path)
    hipStream_t stream = nullptr;
    hipStream_t side[2] = {nullptr, nullptr};     // P3 / P4 Detect branches (forked from and joined to the main stream)
    hipEvent_t ev_fork[2] = {nullptr, nullptr}, ev_join[2] = {nullptr, nullptr};
    std::map<int, hipGraphExec_t> graphs;   // (batch size, fused front, candidate-buffer parity) -> captured forward+decode
    std::map<int, int> graph_failures;      // failed captures per key (a second failure leaves the shape on eager launches)
    std::map<int, std::vector<Launch>> launches;             // batch size -> what every op launches (resolve_launches)
    int last_n = 0;

    // production phase timing: every SAMPLE_EVERY-th call of a detect path is bracketed by four timing events
    static constexpr int SAMPLE_EVERY = 16;
    hipEvent_t ev_t[4] = {nullptr, nullptr, nullptr, nullptr};
    bool t_pending = false;
    int t_frames = 0;
    unsigned sample_ctr = 0;

    // completion of the last two zly_detect_device calls (recorded behind each call's NMS, on whichever stream it ran): zly_join orders
    // a foreign stream behind them -- the RCCL gather of a step's slabs when the step ran on the engine's own stream (several engines
    // per GPU) or with deferred NMS
    hipEvent_t ev_call[2] = {nullptr, nullptr};
    uint64_t call_seq = 0;
    int cu_part_n = 1;                // ZLY_CU_PART: number of CU partitions (1 = whole chip)
    uint32_t cu_mask[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    std::atomic<Ingest*> ingest{nullptr};   // created by the first zly_submit (under mu), read lock-free afterwards
    std::atomic<Track*> track{nullptr};     // created by zly_track_enable (under mu), read lock-free afterwards
    Merge* merge = nullptr;                 // created by the first zly_merge_slabs / zly_detect_tiled (under mu)
    Surfaces* surf = nullptr;               // created by zly_surfaces_enable (under mu)
    Zoom* zoom = nullptr;                   // created by zly_zoom_enable (under mu)
    Chips* chips = nullptr;                 // created by zly_chips_enable (under mu)
    Change* change = nullptr;               // created by zly_change_enable (under mu)
    Camera* camera = nullptr;               // created by zly_camera_enable (under mu)
    hipStream_t last_ns = nullptr;          // the stream the most recent zly_detect_device* call's NMS ran on, and whether that was the engine's NMS stream
    bool last_deferred = false;

    Switches sw;                      // tuning / test switches of the environment, read ONCE at zly_create (read_switches; the list: zly_internal.h)

    std::mutex mu;                    // serialises every call that touches engine / device state
    mutable std::mutex stats_mu;      // guards `stats` only, never held across a device call: zly_get_stats cannot wait on a batch
    zly_stats stats{};
};

namespace zly {

static size_t slab_bytes_of(const zly_engine* e) { return sizeof(zly_slab_header) + (size_t)e->cfg.max_dets * sizeof(zly_det); }

template <typename F> static void with_stats(zly_engine* e, F&& f) { std::lock_guard<std::mutex> lk(e->stats_mu); f(e->stats); }

// The environment's tuning / test switches (zly_internal.h: Switches is the list).  The ONLY place that reads the environment: zly_create calls it
// once, before the plan is built, and everything that plans or launches gets the record -- an engine never looks at the environment again.
static void read_switches(Switches* sw)
{
    auto on = [](const char* name) { return getenv(name) != nullptr; };
    auto num = [](const char* name, auto* out) { if (const char* v = getenv(name)) *out = (std::remove_pointer_t<decltype(out)>)atoll(v); };
    *sw = Switches();
    if (const char* cp = getenv("ZLY_CU_PART")) {
        int pi = 0, pn = 1;
        if (sscanf(cp, "%d/%d", &pi, &pn) == 2 && pn >= 1 && pn <= 8 && pi >= 0 && pi < pn) { sw->cu_part_i = pi; sw->cu_part_n = pn; sw->num_cus = 256 / pn; }
    }
    sw->no_lanes = on("ZLY_NO_LANES") || on("ZLY_CU_PART");           // a CU partition runs one chain
    sw->no_c2f = on("ZLY_NO_C2F");
    sw->no_det_merge = on("ZLY_NO_DET_MERGE");
    sw->no_tail_split = on("ZLY_NO_TAIL_SPLIT");
    num("ZLY_TAIL_BOX", &sw->tail_box);
    if (const char* v = getenv("ZLY_TAIL_BOX_MIN_CONF")) sw->tail_box_min_conf = (float)atof(v);
    sw->sppf_fused = on("ZLY_SPPF_FUSED");
    sw->pool_six_pass = on("ZLY_SPPF_POOL_LDS");
    sw->no_wsk = on("ZLY_NO_WSK");
    sw->nms_general = on("ZLY_NMS_GENERAL");
    sw->no_cout_pad = on("ZLY_NO_COUT_PAD");
    sw->no_cin_pad = on("ZLY_NO_CIN_PAD");
    sw->no_stem1 = on("ZLY_NO_STEM1");
    num("ZLY_STEM1_NW", &sw->stem1_nw);
    num("ZLY_STEM1_VAR", &sw->stem1_var);
    num("ZLY_STEM1_GRID", &sw->stem1_grid);
    num("ZLY_STEM1_TW", &sw->stem1_tw);
    num("ZLY_STEM1_TH", &sw->stem1_th);
    sw->stem1_keep_tiles = on("ZLY_STEM1_TW") || on("ZLY_STEM1_TH") || on("ZLY_STEM1_BIG_TILES");
    num("ZLY_PAIR_MIN_TILES", &sw->pair_min_tiles);
    num("ZLY_PAIR_WIDTHS", &sw->pair_widths);
    auto num_nonempty = [&](const char* name, int* out) { const char* v = getenv(name); if (v && *v) *out = atoi(v); };
    num_nonempty("ZLY_STAGE_SLOTS", &sw->stage_slots);
    num_nonempty("ZLY_STAGE_MB", &sw->stage_mb);
    num_nonempty("ZLY_INFLIGHT", &sw->inflight);
    { int d = 0; num_nonempty("ZLY_D2H_STREAM", &d); sw->d2h_stream = d != 0; }
    num("ZLY_PROFILE_INNER", &sw->profile_inner);
    if (sw->profile_inner < 1) sw->profile_inner = 1;
#ifdef ZLY_DIAG
    if (const char* v = getenv("ZLY_ABLATE_SKIP")) sw->ablate = std::string(",") + v + ",";       // result-changing: compiled into libzly_diag.so only (tools/ablate_launches.sh)
#endif
    sw->no_stream = on("ZLY_NO_STREAM");
    sw->stream_ct2 = on("ZLY_STREAM_CT2");
    num("ZLY_STREAM_MAX_NK", &sw->stream_max_nk);
    num("ZLY_STREAM_MIN_GROUPS", &sw->stream_min_groups);
    num("ZLY_STREAM_WGS", &sw->stream_wgs);
    num("ZLY_WS1", &sw->ws1_mode);
    sw->ws1_no_dual = on("ZLY_WS1_NO_DUAL");
    num("ZLY_WS1_MIN_PX", &sw->ws1_min_px);
    sw->ws1_max_bytes = on("ZLY_WS1_MAX_BYTES");
    sw->no_ws = on("ZLY_NO_WS");
    sw->no_ws_s2 = on("ZLY_NO_WS_S2");
    sw->no_ws_s2_c32 = on("ZLY_NO_WS_S2_C32");
    sw->ws_rowt = on("ZLY_WS_ROWT");
    num("ZLY_WS_TPW1_MAXCT", &sw->ws_tpw1_maxct);
    num("ZLY_WS_MIN_TILES", &sw->ws_min_tiles);
    num("ZLY_WS_MAX_BYTES", &sw->ws_max_bytes);
    num("ZLY_WS_PAIR", &sw->ws_pair);
    num("ZLY_WS_PAIR_GRID", &sw->ws_pair_grid);
    num("ZLY_WS_PAIR_MAX_TILES", &sw->ws_pair_max_tiles);
    sw->no_wres = on("ZLY_NO_WRES");
    num("ZLY_WRES_MAXCHUNKS", &sw->wres_maxchunks);
    sw->lds_s2_pt1 = on("ZLY_LDS_S2_PT1");
    num("ZLY_LDS_MIN_TILES", &sw->lds_min_tiles);
    num("ZLY_LDS_WGS_PER_CU", &sw->lds_wgs_per_cu);
    num("ZLY_DIRECT_PT4_MIN", &sw->direct_pt4_min);
    num("ZLY_DIRECT_PT2_MIN", &sw->direct_pt2_min);
    num("ZLY_DIRECT_KSPLIT_NK", &sw->direct_ksplit_nk);
    num("ZLY_C2F32_NW", &sw->c2f32_nw);
    num("ZLY_C2F_LDS_KB", &sw->c2f_lds_kb);
    if (const char* ft = getenv("ZLY_C2F_TILE")) { int th = 0, tw = 0; if (sscanf(ft, "%d,%d", &th, &tw) == 2) { sw->c2f_tile_th = th; sw->c2f_tile_tw = tw; } }
    sw->c2f64 = on("ZLY_C2F64");
}

// ------------------------------------------------------------------------------------------------
// plan
// ------------------------------------------------------------------------------------------------
struct PlanBuilder {
    Plan* p;
    const ModelFile& model;
    const zly_config& cfg;
    const int dtype;
    const Switches& sw;
    const size_t esz;
    const int kstep;
    std::string err;

    bool bf16() const { return dtype == ZLY_DTYPE_BF16; }
    bool fail(const std::string& msg) { err = msg; return false; }
    int add_buffer(const std::string& name, int H, int W, int C, bool f32 = false) {
        Buffer b;
        b.name = name; b.H = H; b.W = W; b.C = C; b.f32 = f32;
        p->bufs.push_back(b);
        return (int)p->bufs.size() - 1;
    }
    int add_op(const Op& op) { p->ops.push_back(op); return (int)p->ops.size() - 1; }
    size_t append(const void* d, size_t bytes) {
        std::vector<uint8_t>& blob = p->blob;
        size_t off = (blob.size() + 255) / 256 * 256;
        blob.resize(off + bytes);
        memcpy(blob.data() + off, d, bytes);
        return off;
    }
    const ConvRec* find(const std::string& name) {
        const ConvRec* r = model.find(name);
        if (!r) err = "conv missing from model file: " + name;
        return r;
    }
    // one conv's weights in a tiling of their own (the tilings of the fused kernels), appended to the blob
    void pack(const ConvRec* r, int cin_store, int ks, bool pair_rows, int epl, const int* tap_slot, size_t* w_off, size_t* b_off, int* nk, int* cout_pad) {
        std::vector<uint8_t> w;
        std::vector<float> b;
        int cout = 0;
        repack_conv({r}, cin_store, ks, bf16(), &w, &b, &cout, cout_pad, nk, pair_rows, epl, tap_slot);
        *w_off = append(w.data(), w.size());
        if (b_off) *b_off = append(b.data(), b.size() * sizeof(float));
    }
    // the conv op of `names` (several convs of one input = one launch); returns its op index, -1 on error
    int conv(const std::vector<std::string>& names, View in, View out, View res = View{-1, 0, 0}, bool out_f32 = false, View in2 = View{-1, 0, 0}, int lane = 0) {
        std::vector<const ConvRec*> srcs;
        for (const std::string& n : names) {
            const ConvRec* r = find(n);
            if (!r) return -1;
            srcs.push_back(r);
        }
        auto bad = [&](const char* what) { err = what + names[0]; return -1; };
        const ConvRec* r0 = srcs[0];
        for (const ConvRec* r : srcs)
            if (r->cin != r0->cin || r->k != r0->k || r->stride != r0->stride || r->act != r0->act) return bad("cannot fuse ");
        const Buffer& ib = p->bufs[(size_t)in.buf];
        const Buffer& ob = p->bufs[(size_t)out.buf];
        const int epl = bf16() ? 8 : 4;
        const int cin_total = in.C + (in2.buf >= 0 ? in2.C : 0);
        if (cin_total < r0->cin || in.C % epl != 0 || in.co % epl != 0 || ib.C % epl != 0 || in.co + in.C > ib.C) return bad("bad input view for ");
        if (in2.buf >= 0) {
            const Buffer& i2 = p->bufs[(size_t)in2.buf];
            if (r0->k != 1 || in.C % kstep != 0 || in2.C % epl != 0 || in2.co % epl != 0 || i2.C % epl != 0 || in2.co + in2.C > i2.C ||
                i2.H != ob.H || i2.W != ob.W || ib.H * 2 != ob.H || ib.W * 2 != ob.W) return bad("bad upsample+concat input for ");
        }
        Op op;
        op.kind = OP_CONV;
        op.lane = lane;
        op.name = names[0];
        for (size_t i = 1; i < names.size(); ++i) op.name += "+" + names[i];
        if (op.name.size() > 47) op.name.resize(47);
        op.in = in; op.out = out; op.res = res; op.in2 = in2;
        op.ks = r0->k; op.stride = r0->stride; op.act = r0->act; op.out_f32 = out_f32 ? 1 : 0;
        std::vector<uint8_t> w;
        std::vector<float> b;
        repack_conv(srcs, cin_total, kstep, bf16(), &w, &b, &op.cout, &op.cout_pad, &op.nk, true);
        // 5 channel tiles (the 80-channel Detect class branch) suit no kernel's channel blocking: CT = 5 needs more registers than
        // two waves per SIMD leave.  One whole zero tile is appended instead (6 tiles = 2 blocks of CT = 3); its outputs are never
        // stored (channel >= Cout) -- 20 % more MFMAs on these layers, but the LDS-tiled kernel instead of the direct one.
        if (bf16() && op.ks == 3 && op.cout_pad == 80 && cin_total % 32 == 0 && !sw.no_cout_pad) {
            w.resize(w.size() + (size_t)op.nk * 1024, 0);
            b.resize(b.size() + 16, 0.0f);
            op.cout_pad = 96;
        }
        if (out.C != op.cout || out.co % 4 != 0 || ob.C % 4 != 0 || out.co + out.C > ob.C) return bad("bad output view for ");
        if (out_f32 != ob.f32) return bad("output dtype mismatch for ");
        const int Ho = ob.H, Wo = ob.W;
        const int Hin = in2.buf >= 0 ? ib.H * 2 : ib.H, Win = in2.buf >= 0 ? ib.W * 2 : ib.W;
        if (Ho != (Hin + 2 * (op.ks / 2) - op.ks) / op.stride + 1 || Wo != (Win + 2 * (op.ks / 2) - op.ks) / op.stride + 1) return bad("spatial mismatch for ");
        op.K = op.ks * op.ks * cin_total;
        op.w_off = append(w.data(), w.size());
        op.b_off = append(b.data(), b.size() * sizeof(float));
        int co = 0;
        double macs = 0;
        for (size_t i = 0; i < srcs.size(); ++i) {
            op.taps.push_back(names[i]); op.tap_co.push_back(co); op.tap_c.push_back(srcs[i]->cout);
            co += srcs[i]->cout;
            macs += (double)Ho * Wo * srcs[i]->cout * srcs[i]->cin * op.ks * op.ks;
        }
        op.flops = 2.0 * macs;
        const double osz = out_f32 ? 4.0 : (double)esz;
        op.cin_frac = (double)r0->cin / cin_total;
        op.wbytes = (double)op.cout * r0->cin * op.ks * op.ks * esz + (double)op.cout * 4.0;
        op.bytes = ((double)ib.H * ib.W * in.C + (in2.buf >= 0 ? (double)Ho * Wo * in2.C : 0.0)) * esz * op.cin_frac + (double)Ho * Wo * op.cout * osz +
                   op.wbytes + (res.buf >= 0 ? (double)Ho * Wo * op.cout * esz : 0.0);
        const int idx = add_op(op);
        for (size_t i = 0; i < names.size(); ++i) p->tap_index[names[i]] = std::make_pair(idx, (int)i);
        return idx;
    }
    // Ops a and b are a bottleneck's 3x3 pair: when the fused kernel covers this width, a PairGroup holds the pair kernel's operands
    // (for c = 16 its own weight tiling: one tap per 16x16x16 MFMA k-step).
    bool mark_pair(const std::string& m, int a, int b, int c, bool shortcut) {
        if (!bf16() || (c != 16 && c != 32 && c != 64)) return true;
        Op& A = p->ops[(size_t)a];
        Op& B = p->ops[(size_t)b];
        if (A.ks != 3 || B.ks != 3 || A.stride != 1 || B.stride != 1 || !A.act || !B.act || A.cout != c || B.cout != c) return true;
        if (A.in.co % 8 || B.out.co % 8 || p->bufs[(size_t)A.in.buf].C % 8 || p->bufs[(size_t)B.out.buf].C % 8) return true;
        PairGroup g;
        g.first = a; g.second = b; g.c = c; g.res = shortcut ? 1 : 0;
        g.out = B.out;
        g.wA = A.w_off; g.bA = A.b_off; g.wB = B.w_off; g.bB = B.b_off;
        if (c == 16) {
            const char* names[2] = {".cv1", ".cv2"};
            size_t* wo[2] = {&g.wA, &g.wB};
            size_t* bo[2] = {&g.bA, &g.bB};
            for (int k = 0; k < 2; ++k) {
                const ConvRec* r = find(m + names[k]);
                if (!r) return false;
                int cout_pad = 0, nk = 0;
                pack(r, c, 16, false, 4, nullptr, wo[k], bo[k], &nk, &cout_pad);
                if (nk != 9 || cout_pad != 16) return fail("internal: pair weight tiling for " + m);
            }
        }
        A.pair = B.pair = (int)p->pairs.size();
        p->pairs.push_back(g);
        return true;
    }
    // C2f(c1 -> c2, n bottlenecks): cv1 writes [0,2c) of the concat buffer, bottleneck i reads
    // [(1+i)c,(2+i)c) and writes [(2+i)c,(3+i)c), cv2 reads all (2+n)c channels.
    bool c2f(const std::string& pfx, View in, View out, int n, bool shortcut, int H, int W, View in2 = View{-1, 0, 0}) {
        const int c = out.C / 2;
        const int cat = add_buffer(pfx + ".cat", H, W, (2 + n) * c);
        const int cv1 = conv({pfx + ".cv1"}, in, View{cat, 0, 2 * c}, View{-1, 0, 0}, false, in2);
        if (cv1 < 0) return false;
        for (int i = 0; i < n; ++i) {
            const View src{cat, (1 + i) * c, c};
            const std::string m = pfx + ".m." + std::to_string(i);
            const int tmp = add_buffer(m + ".tmp", H, W, c);
            const int a = conv({m + ".cv1"}, src, View{tmp, 0, c});
            const int b = a < 0 ? -1 : conv({m + ".cv2"}, View{tmp, 0, c}, View{cat, (2 + i) * c, c}, shortcut ? src : View{-1, 0, 0});
            if (b < 0 || !mark_pair(m, a, b, c, shortcut)) return false;
        }
        const int cv2 = conv({pfx + ".cv2"}, View{cat, 0, (2 + n) * c}, out);
        return cv2 >= 0 && mark_c2f(pfx, cv1, cv2, cat, c, n, shortcut, in, in2, out);
    }
    // Ops [cv1, cv2] are a C2f block: its fused kernel's launch groups (n = 1: the whole block; n = 2: front half = cv1 + first bottleneck,
    // back half = second bottleneck + cv2).  Weight tilings are shared with the per-conv kernels where the layout is the same (C = 32); the
    // 16-channel block gets its own cv1 (rows in channel order) and cv2 (k-steps of 16) tilings.
    bool mark_c2f(const std::string& pfx, int cv1, int cv2, int cat, int c, int n, bool shortcut, View in, View in2, View out) {
        if (!bf16() || (c != 16 && c != 32 && c != 64) || (n != 1 && n != 2) || (cfg.flags & ZLY_FLAG_NO_FUSION)) return true;
        const Op& o1 = p->ops[(size_t)cv1];
        const Op& o2 = p->ops[(size_t)cv2];
        const int cin = in.C + (in2.buf >= 0 ? in2.C : 0);
        if (cin % 32 != 0 || o2.cout != 2 * c || o1.cout != 2 * c || !o1.act || !o2.act) return true;
        for (int i = 0; i < n; ++i) if (p->ops[(size_t)cv1 + 1 + 2 * (size_t)i].pair < 0) return true;       // mark_pair declined
        C2fGroup g;
        g.c = c; g.res = shortcut ? 1 : 0; g.cat = cat;
        g.x = in; g.x2 = in2; g.out = out;
        g.w1 = o1.w_off; g.b1 = o1.b_off; g.nk1 = o1.nk; g.w2 = o2.w_off; g.b2 = o2.b_off; g.nk2 = o2.nk; g.cout2 = o2.cout;
        if (c == 16) {
            int cout_pad = 0;
            pack(model.find(pfx + ".cv1"), cin, 32, false, 0, nullptr, &g.w1, &g.b1, &g.nk1, &cout_pad);
            pack(model.find(pfx + ".cv2"), (2 + n) * c, 16, true, 4, nullptr, &g.w2, &g.b2, &g.nk2, &cout_pad);
        }
        if (g.nk2 != (c == 64 ? 2 : 1) * (2 + n)) return true;            // cv2's k-steps: one per source map (c = 16 / 32), two per map of 64 channels
        // one group, led by its first member, around the bottleneck whose first conv is op a
        auto group = [&](int mode, int a, std::initializer_list<C2fGroup::Member> members) {
            g.mode = mode; g.pair = p->ops[(size_t)a].pair; g.leader = members.begin()->op; g.members = members;
            if (c == 64) g.mid = p->ops[(size_t)a].out;
            for (const C2fGroup::Member& m : members) p->ops[(size_t)m.op].c2f = (int)p->c2fs.size();
            p->c2fs.push_back(g);
        };
        const int mid_vis = c == 64 ? 1 : 2;
        if (n == 1) group(3, cv1 + 1, {{cv1, 1}, {cv1 + 1, mid_vis}, {cv1 + 2, 1}, {cv2, 0}});
        else {
            group(1, cv1 + 1, {{cv1, 0}, {cv1 + 1, mid_vis}, {cv1 + 2, 0}});
            group(2, cv1 + 3, {{cv1 + 3, mid_vis}, {cv1 + 4, 1}, {cv2, 0}});
        }
        return true;
    }
    // One Detect level right behind the C2f that feeds it: the two branches' first 3x3 convs read the same tensor and are one launch, then each
    // branch's second conv, then the level's tail op.  P3 and P4 only depend on model.15 / model.18: on side streams (lanes 1, 2) they run, inside
    // the captured graph, BESIDE the rest of the neck (model.16-21) instead of after it.  These launches are latency/issue-bound and leave most
    // of the chip idle, so the overlap is nearly free.
    bool detect_level(int l, View feat, int c2, int c3, const Op& tail_total) {
        const std::string L = std::to_string(l);
        const int lane = l == 0 ? 1 : (l == 1 ? 2 : 0);
        DetectTail& t = p->tail;
        HeadLevel& hl = t.args.lv[l];
        // the class branch's 80 channels are stored as 96 (16 zero channels, never written) so that its second 3x3 conv has
        // Cin % 32 == 0 and takes the LDS-tiled kernel; the padded k-steps carry zero weights
        const int c3s = (bf16() && c3 % 32 != 0 && c2 % 32 == 0 && !sw.no_cin_pad) ? (c3 + 31) / 32 * 32 : c3;
        const int hd1 = add_buffer("detect." + L + ".stem", hl.H, hl.W, c2 + c3s);
        t.stem[l] = hd1;
        t.box[l] = add_buffer("detect." + L + ".box2", hl.H, hl.W, c2);
        t.cls[l] = add_buffer("detect." + L + ".cls2", hl.H, hl.W, c3);
        t.logits[l] = add_buffer("detect." + L + ".logits", hl.H, hl.W, hl.logits_cs, true);
        const View none{-1, 0, 0};
        const int s = p->det_stem[l] = conv({"model.22.cv2." + L + ".0", "model.22.cv3." + L + ".0"}, feat, View{hd1, 0, c2 + c3}, none, false, none, lane);
        const int a = p->det_a[l] = s < 0 ? -1 : conv({"model.22.cv2." + L + ".1"}, View{hd1, 0, c2}, View{t.box[l], 0, c2}, none, false, none, lane);
        const int b = p->det_b[l] = a < 0 ? -1 : conv({"model.22.cv3." + L + ".1"}, View{hd1, c2, c3s}, View{t.cls[l], 0, c3}, none, false, none, lane);
        if (b < 0) return false;
        if (l == 2) p->join_at = s;
        if (bf16() && c3 == 80 && c3s >= 80) {
            // the same conv for conv3x3_wsk_kernel: k = tap * 80 + c without channel padding (23 k-steps instead of 27), plain tile rows, no zero output tile
            const ConvRec* r = model.find("model.22.cv3." + L + ".1");
            size_t w_off = 0;
            int cout_pad = 0, nk = 0;
            pack(r, 80, kstep, false, 0, nullptr, &w_off, nullptr, &nk, &cout_pad);
            if (nk == 23 && cout_pad == 80 && r->k == 3 && r->stride == 1) p->ops[(size_t)b].wsk_w = w_off;
        }
        // the final 1x1 convs run inside the fused tail: weights only
        const ConvRec* rb = find("model.22.cv2." + L + ".2");
        const ConvRec* rc = rb ? find("model.22.cv3." + L + ".2") : nullptr;
        if (!rc) return false;
        int cout_pad = 0;
        pack(rb, c2, kstep, false, 0, nullptr, &t.wb[l], &t.bb[l], &hl.nkb, &cout_pad);
        pack(rc, c3, kstep, false, 0, nullptr, &t.wc[l], &t.bc[l], &hl.nkc, &cout_pad);
        // the fused tail holds a branch's fragments in HEAD_KMAX k-steps of registers (launch_head_fused refuses more): refuse the model here, at load
        if (hl.nkb > HEAD_KMAX || hl.nkc > HEAD_KMAX)
            return fail("Detect branch too wide for the fused tail: " + std::to_string(c2) + " / " + std::to_string(c3) + " channels = " + std::to_string(hl.nkb) + " / " +
                        std::to_string(hl.nkc) + " k-steps, at most " + std::to_string(HEAD_KMAX) + (bf16() ? " in bf16" : " in fp32"));
        p->tap_final["model.22.cv2." + L + ".2"] = std::make_pair(t.logits[l], 0);
        p->tap_final["model.22.cv3." + L + ".2"] = std::make_pair(t.logits[l], 64);
        // the merged launches of the latency path: all three levels must suit the shared kernel shape
        const Op& S = p->ops[(size_t)s];
        const Op& A = p->ops[(size_t)a];
        const Op& Bc = p->ops[(size_t)b];
        p->det_merge_ok = p->det_merge_ok && S.ks == 3 && A.ks == 3 && Bc.ks == 3 && S.stride == 1 && S.in.C % 32 == 0 && A.in.C % 32 == 0 && Bc.in.C % 32 == 0 &&
                          S.cout_pad % 48 == 0 && A.cout_pad % 32 == 0 && Bc.cout_pad % 32 == 0 && S.in2.buf < 0 && S.res.buf < 0 && A.res.buf < 0 && Bc.res.buf < 0;
        // Three tail ops, one per level.  From batch 16 up each is its own launch right behind its level's branch convs (P3 and
        // P4 on the side streams, i.e. beside the neck) and only the small P5 launch is left at the end of the step; below
        // that the first two are skipped and the last one covers all levels in a single launch (fewest launches).
        Op op;
        op.kind = OP_HEAD; op.lane = lane; op.level = l;
        op.name = std::string("detect.tail.P") + std::to_string(3 + l) + (l == 2 ? " (all levels below batch 16)" : "");
        const double share = (double)hl.hw / (double)p->N;
        op.flops = tail_total.flops * share; op.bytes = tail_total.bytes * share; op.wbytes = tail_total.wbytes * share;
        t.op[l] = add_op(op);
        return true;
    }
};

// The plan is made in two halves: build_plan -- the op list and every weight repack into a host image of the device blob -- needs no
// device call and runs before zly_create takes the process-wide exclusive gate; upload_plan (hipMalloc / hipMemcpy, pointers into the blob) runs
// under it.  A hot reload builds its new engines beside running ones: their enqueue sections now stall for the allocations only, not for the repack.
// The ops are emitted in launch order: the main chain, each Detect level behind the C2f that feeds it, NMS last.
static int build_plan(const ModelFile& m, const zly_config& cfg, int dtype, const Switches& sw, Plan* plan, std::string* err)
{
    const size_t esz = dtype == ZLY_DTYPE_BF16 ? 2 : 4;
    PlanBuilder pb{plan, m, cfg, dtype, sw, esz, conv_kstep(dtype), std::string()};
    Plan* const p = plan;
    const int W = cfg.model_w, H = cfg.model_h;
    const int* ch = m.ch;
    const int* nb = m.n_c2f;
    auto refuse = [&](const std::string& msg) { *err = msg; return (int)ZLY_ERR_MODEL_LOAD; };
    if (m.reg_max != 16) return refuse("only reg_max = 16 is supported");
    for (int i = 0; i < 5; ++i)
        if (ch[i] % 16 != 0) return refuse("channel widths must be multiples of 16");
    const int c2 = std::max(16, std::max(ch[2] / 4, 4 * m.reg_max));
    const int c3 = std::max(ch[2], std::min(m.nc, 100));
    if (m.nc > 80) return refuse("nc > 80 is not supported by the fused Detect kernel");
    // the class branch's stored width is c3 itself: for 65 <= nc <= 79 (YOLOv8n) its pixel rows would not be whole 16-channel
    // tiles, and no conv epilogue nor the Detect tail's 16-byte fragment loads is written for that
    if (c3 % 16 != 0) return refuse("Detect class-branch width max(ch[2], nc) = " + std::to_string(c3) + " is not a multiple of 16 (nc = " + std::to_string(m.nc) + ")");
    const int H2 = H / 2, W2 = W / 2, H4 = H / 4, W4 = W / 4, H8 = H / 8, W8 = W / 8, H16 = H / 16, W16 = W / 16, H32 = H / 32, W32 = W / 32;
    p->nc = m.nc;

    p->in_buf = pb.add_buffer("images", H, W, 8);
    const int a0 = p->stem_out = pb.add_buffer("model.0", H2, W2, ch[0]);
    const int a1 = p->m1_out = pb.add_buffer("model.1", H4, W4, ch[1]);
    const int a2 = pb.add_buffer("model.2", H4, W4, ch[1]);
    const int a3 = pb.add_buffer("model.3", H8, W8, ch[2]);
    const int cat14 = pb.add_buffer("cat14[up(12),4]", H8, W8, ch[3] + ch[2]);
    const int a5 = pb.add_buffer("model.5", H16, W16, ch[3]);
    const int cat11 = pb.add_buffer("cat11[up(9),6]", H16, W16, ch[4] + ch[3]);
    const int a7 = pb.add_buffer("model.7", H32, W32, ch[4]);
    const int a8 = pb.add_buffer("model.8", H32, W32, ch[4]);
    const int spp = pb.add_buffer("model.9.cat", H32, W32, 2 * ch[4]);
    const int cat20 = pb.add_buffer("cat20[19,9]", H32, W32, ch[3] + ch[4]);
    const int cat17 = pb.add_buffer("cat17[16,12]", H16, W16, ch[2] + ch[3]);
    const int a15 = pb.add_buffer("model.15", H8, W8, ch[2]);
    const int a18 = pb.add_buffer("model.18", H16, W16, ch[3]);
    const int a21 = pb.add_buffer("model.21", H32, W32, ch[4]);

    // The Detect tail's geometry and its three-level accounting, of which each tail op reports its level's share: they need only c2, c3, nc and the map sizes
    const int fh[3] = {H8, H16, H32}, fw[3] = {W8, W16, W32};
    HeadArgs& head = p->tail.args;
    Op tail_total;
    p->N = fh[0] * fw[0] + fh[1] * fw[1] + fh[2] * fw[2];
    int anchor_off = 0, block0 = 0;
    for (int l = 0; l < 3; ++l) {
        HeadLevel& hl = head.lv[l];
        hl.box_cs = c2; hl.cls_cs = c3; hl.box_cin = c2; hl.cls_cin = c3;
        hl.H = fh[l]; hl.W = fw[l]; hl.hw = fh[l] * fw[l]; hl.stride_px = 8 << l; hl.anchor_off = anchor_off; hl.block0 = block0;
        hl.logits_cs = 64 + (m.nc + 3) / 4 * 4;
        block0 += (hl.hw + HEAD_GROUP - 1) / HEAD_GROUP;
        anchor_off += hl.hw;
        const double macs = (double)hl.hw * (c2 * 64.0 + (double)c3 * m.nc);
        tail_total.flops += 2.0 * macs;
        // algorithmic bytes: both branch activations in, the weights, and -- only when the engine materialises it -- the fp32 head tensor out
        tail_total.bytes += (double)hl.hw * ((c2 + c3) * (double)esz + ((cfg.flags & ZLY_FLAG_NO_HEAD_TENSOR) ? 0.0 : (4 + m.nc) * 4.0)) + (c2 * 64.0 + (double)c3 * m.nc) * esz;
        tail_total.wbytes += (c2 * 64.0 + (double)c3 * m.nc) * esz;
    }
    head.nc = m.nc; head.N_total = p->N; head.total_blocks = block0; head.only_level = -1;
    p->det_merge_ok = pb.bf16();

    Op pre; pre.kind = OP_PREPROCESS; pre.name = "preprocess";
    pre.bytes = (double)W * H * 3 + (double)W * H * 3 * esz;          // algorithmic: u8 frame in, the 3-channel tensor out (stored as 8 channels)
    pb.add_op(pre);

    bool ok = true;
    ok = ok && pb.conv({"model.0"}, View{p->in_buf, 0, 8}, View{a0, 0, ch[0]}) >= 0;
    p->stem_fused = pb.bf16() && (ch[0] == 16 || ch[0] == 32);          // YOLOv8n / YOLOv8-s stems: preprocess + model.0 in one kernel
    if (ok && p->stem_fused) {
        int nk = 0, cout_pad = 0;
        pb.pack(m.find("model.0"), 4, pb.kstep, ch[0] == 32, 0, nullptr, &p->stem_w, &p->stem_b, &nk, &cout_pad);
        ok = nk == 2;
    }
    ok = ok && pb.conv({"model.1"}, View{a0, 0, ch[0]}, View{a1, 0, ch[1]}) >= 0;
    p->stem1 = p->stem_fused && ch[0] == 16 && ch[1] == 32 && !(cfg.flags & ZLY_FLAG_NO_FUSION) && !sw.no_stem1 && ok;
    if (p->stem1) {
        // model.1 in the fused kernel's tiling: one 16x16x16 MFMA per tap (k = ci), pair-permuted rows, bias in channel order
        const ConvRec* r = m.find("model.1");
        int cout_pad = 0, nk = 0;
        pb.pack(r, ch[0], 16, true, 4, nullptr, &p->m1_w, &p->m1_b, &nk, &cout_pad);
        if (nk != 9 || cout_pad != 32 || r->k != 3 || r->stride != 2) p->stem1 = false;
    }
    if (p->stem1) {
        // the stem's weights once more in the tap order of the fused kernel's conflict-free fragment reads (kernels_stem.hip: STEM1_TAP_SLOT)
        int cout_pad = 0, nk0 = 0;
        pb.pack(m.find("model.0"), 4, pb.kstep, false, 0, stem1_tap_slot(), &p->stem_w0p, nullptr, &nk0, &cout_pad);
        if (nk0 != 2 || cout_pad != 16) p->stem1 = false;
    }
    ok = ok && pb.c2f("model.2", View{a1, 0, ch[1]}, View{a2, 0, ch[1]}, nb[0], true, H4, W4);
    ok = ok && pb.conv({"model.3"}, View{a2, 0, ch[1]}, View{a3, 0, ch[2]}) >= 0;
    ok = ok && pb.c2f("model.4", View{a3, 0, ch[2]}, View{cat14, ch[3], ch[2]}, nb[1], true, H8, W8);          // P3 -> cat14
    ok = ok && pb.conv({"model.5"}, View{cat14, ch[3], ch[2]}, View{a5, 0, ch[3]}) >= 0;
    ok = ok && pb.c2f("model.6", View{a5, 0, ch[3]}, View{cat11, ch[4], ch[3]}, nb[2], true, H16, W16);        // P4 -> cat11
    ok = ok && pb.conv({"model.7"}, View{cat11, ch[4], ch[3]}, View{a7, 0, ch[4]}) >= 0;
    ok = ok && pb.c2f("model.8", View{a7, 0, ch[4]}, View{a8, 0, ch[4]}, nb[3], true, H32, W32);
    // SPPF
    ok = ok && (p->sppf_cv1 = pb.conv({"model.9.cv1"}, View{a8, 0, ch[4]}, View{spp, 0, ch[4] / 2})) >= 0;
    if (ok) {
        Op pool; pool.kind = OP_SPPF; pool.name = "model.9.pool"; pool.in = View{spp, 0, ch[4] / 2};
        pool.bytes = (double)H32 * W32 * (ch[4] / 2) * 4 * esz;
        p->sppf_pool = pb.add_op(pool);
    }
    ok = ok && (p->sppf_cv2 = pb.conv({"model.9.cv2"}, View{spp, 0, 2 * ch[4]}, View{cat20, ch[3], ch[4]})) >= 0;               // P5 -> cat20
    // neck, top-down.  Upsample(x2, nearest) + Concat are fused into the consumer: model.12.cv1 / model.15.cv1 read
    // their first channels from the half-size tensor at (y>>1, x>>1) and the rest from the skip tensor.
    ok = ok && pb.c2f("model.12", View{cat20, ch[3], ch[4]}, View{cat17, ch[2], ch[3]}, nb[4], false, H16, W16, View{cat11, ch[4], ch[3]});
    ok = ok && pb.c2f("model.15", View{cat17, ch[2], ch[3]}, View{a15, 0, ch[2]}, nb[5], false, H8, W8, View{cat14, ch[3], ch[2]});
    ok = ok && pb.detect_level(0, View{a15, 0, ch[2]}, c2, c3, tail_total);
    // neck, bottom-up
    ok = ok && pb.conv({"model.16"}, View{a15, 0, ch[2]}, View{cat17, 0, ch[2]}) >= 0;
    ok = ok && pb.c2f("model.18", View{cat17, 0, ch[2] + ch[3]}, View{a18, 0, ch[3]}, nb[6], false, H16, W16);
    ok = ok && pb.detect_level(1, View{a18, 0, ch[3]}, c2, c3, tail_total);
    ok = ok && pb.conv({"model.19"}, View{a18, 0, ch[3]}, View{cat20, 0, ch[3]}) >= 0;
    ok = ok && pb.c2f("model.21", View{cat20, 0, ch[3] + ch[4]}, View{a21, 0, ch[4]}, nb[7], false, H32, W32);
    ok = ok && pb.detect_level(2, View{a21, 0, ch[4]}, c2, c3, tail_total);
    if (!ok) return refuse(pb.err);
    Op nm; nm.kind = OP_NMS; nm.name = "nms"; pb.add_op(nm);
    return ZLY_OK;
}

// the device half: allocates the buffers, uploads the weight blob and turns the plan's offsets and buffer indices into the pointers of the launch templates
static int upload_plan(zly_engine* e, std::string* err)
{
    const int W = e->cfg.model_w, H = e->cfg.model_h;
    const int B = e->cfg.max_batch;
    for (Buffer& b : e->bufs) {
        if (b.elems_per_frame() * (size_t)B >= (1ull << 31)) { *err = "activation buffer " + b.name + " exceeds 2^31 elements: lower max_batch"; return ZLY_ERR_INVALID_ARGUMENT; }
        const size_t bytes = b.elems_per_frame() * (b.f32 ? 4 : e->esz) * (size_t)B;
        if (hipMalloc(&b.ptr, bytes) != hipSuccess) { *err = "hipMalloc failed for " + b.name; return ZLY_ERR_SYSTEM; }
        hipMemset(b.ptr, 0, bytes);
    }
    if (hipMalloc(&e->d_weights, e->blob.size()) != hipSuccess) { *err = "hipMalloc failed for weights"; return ZLY_ERR_SYSTEM; }
    if (hipMemcpy(e->d_weights, e->blob.data(), e->blob.size(), hipMemcpyHostToDevice) != hipSuccess) { *err = "weight upload failed"; return ZLY_ERR_SYSTEM; }
    e->blob = std::vector<uint8_t>();                    // the host image of the weight blob is on the device now
    const char* wb = (const char*)e->d_weights;
    if (e->stem_fused) {
        const Buffer& ob = e->bufs[(size_t)e->stem_out];
        StemArgs& st = e->stem;
        st.wgt = wb + e->stem_w; st.bias = (const float*)(wb + e->stem_b);
        st.out = ob.ptr; st.out_cs = ob.C; st.out_co = 0;
        st.tw = W; st.th = H; st.Ho = ob.H; st.Wo = ob.W; st.Cout = ob.C; st.tiles_x = stem_tiles_x(ob.W);
    }
    if (e->stem1) {
        const Buffer& ob = e->bufs[(size_t)e->m1_out];
        Stem1Args& s1 = e->stem1a;
        s1.st = e->stem;
        s1.w1 = wb + e->m1_w; s1.b1 = (const float*)(wb + e->m1_b);
        s1.out1 = ob.ptr; s1.out1_cs = ob.C; s1.out1_co = 0;
        s1.H1 = ob.H; s1.W1 = ob.W;
        stem1_plan(ob.H, ob.W, e->sw, &s1.TH, &s1.TW);
        s1.tiles_x = (ob.W + s1.TW - 1) / s1.TW; s1.tiles_y = (ob.H + s1.TH - 1) / s1.TH;
        s1.dump = (e->cfg.flags & ZLY_FLAG_DUMP_LOGITS) ? 1 : 0;
        s1.wgt0p = wb + e->stem_w0p;
        s1.nw = e->sw.stem1_nw; s1.var = e->sw.stem1_var; s1.pgrid = e->sw.stem1_grid;
        s1.small_tiles = e->sw.stem1_keep_tiles ? 0 : 1;
    }
    DetectTail& t = e->tail;
    for (int l = 0; l < 3; ++l) {
        HeadLevel& hl = t.args.lv[l];
        hl.box_in = e->bufs[(size_t)t.box[l]].ptr;
        hl.cls_in = e->bufs[(size_t)t.cls[l]].ptr;
        hl.wb = wb + t.wb[l]; hl.bb = (const float*)(wb + t.bb[l]);
        hl.wc = wb + t.wc[l]; hl.bc = (const float*)(wb + t.bc[l]);
        hl.logits = (e->cfg.flags & ZLY_FLAG_DUMP_LOGITS) ? (float*)e->bufs[(size_t)t.logits[l]].ptr : nullptr;
        // cv2.L.1's operands for the launches in which the tail computes it (Launch::box_mode): the dense op's own tiles
        const Op& a1 = e->ops[(size_t)e->det_a[l]];
        hl.box_mode = 0;
        hl.w1 = wb + a1.w_off; hl.b1 = (const float*)(wb + a1.b_off);
        hl.box2 = (e->cfg.flags & ZLY_FLAG_DUMP_LOGITS) ? e->bufs[(size_t)t.box[l]].ptr : nullptr;
    }
    return ZLY_OK;
}

// ------------------------------------------------------------------------------------------------
// execution
// ------------------------------------------------------------------------------------------------
// Detect branches on side streams (and per-level tail launches): measured at batch 1 the cross-stream edges cost more
// than the overlap buys (0.27 -> 0.34 ms/frame); from batch 16 up the branches are long enough to pay
static bool lanes_active(const zly_engine* e, int n)
{
    if (e->cfg.flags & ZLY_FLAG_SINGLE_CHAIN) return false;
    return n >= 16 && !e->sw.no_lanes;                               // ZLY_NO_LANES / ZLY_CU_PART: tuning aid; a CU partition runs one chain
}

// launch arguments of a conv op at batch n
static ConvArgs make_conv_args(zly_engine* e, const Op& op, int n)
{
    const Buffer& ib = e->bufs[(size_t)op.in.buf];
    const Buffer& ob = e->bufs[(size_t)op.out.buf];
    ConvArgs a;
    a.in = ib.ptr; a.in_cs = ib.C; a.in_co = op.in.co;
    a.H = ib.H; a.W = ib.W; a.Cin = op.in.C;
    a.wgt = (const char*)e->d_weights + op.w_off;
    a.bias = (const float*)((const char*)e->d_weights + op.b_off);
    a.out = ob.ptr; a.out_cs = ob.C; a.out_co = op.out.co;
    a.Ho = ob.H; a.Wo = ob.W; a.Cout = op.cout; a.cout_pad = op.cout_pad;
    if (op.res.buf >= 0) { const Buffer& rb = e->bufs[(size_t)op.res.buf]; a.res = rb.ptr; a.res_cs = rb.C; a.res_co = op.res.co; }
    else { a.res = nullptr; a.res_cs = 0; a.res_co = 0; }
    a.stride = op.stride; a.pad = op.ks / 2;
    a.K = op.K; a.nk = op.nk; a.M = n * ob.H * ob.W; a.act = op.act; a.out_f32 = op.out_f32;
    a.in2 = nullptr; a.in2_cs = 0; a.in2_co = 0; a.split_c = 0;
    a.inv_wo = 0.f; a.inv_ho = 0.f;                                   // filled where the split-K kernel is launched
    if (op.in2.buf >= 0) {
        const Buffer& i2 = e->bufs[(size_t)op.in2.buf];
        a.in2 = i2.ptr; a.in2_cs = i2.C; a.in2_co = op.in2.co; a.split_c = op.in.C;
        a.H = ob.H; a.W = ob.W; a.Cin = op.in.C + op.in2.C;        // logical (full-size, concatenated) input
    }
    return a;
}

// ... and of an 80 -> 80 class-branch conv as the K-packed kernel sees it: 80 of the 96 stored input channels, weights tiled with cin_store = 80
static ConvArgs make_wsk_args(zly_engine* e, const Op& op, int n)
{
    ConvArgs k = make_conv_args(e, op, n);
    k.Cin = 80; k.K = 9 * 80; k.nk = 23; k.cout_pad = 80;
    k.wgt = (const char*)e->d_weights + op.wsk_w;
    return k;
}

// the fused SPPF kernel's arguments at batch n: model.9.cv1's input and weights, cv2's weights and output, the block's concat buffer
static SppfArgs make_sppf_args(const zly_engine* e, int n)
{
    const Op& op = e->ops[(size_t)e->sppf_cv1];
    const Op& o2 = e->ops[(size_t)e->sppf_cv2];
    const Buffer& ib = e->bufs[(size_t)op.in.buf];
    const Buffer& cb = e->bufs[(size_t)op.out.buf];     // the block's concat buffer [y | p1 | p2 | p3]
    const Buffer& ob2 = e->bufs[(size_t)o2.out.buf];
    const char* wb = (const char*)e->d_weights;
    SppfArgs sa{};
    sa.x = ib.ptr; sa.x_cs = ib.C; sa.x_co = op.in.co; sa.Cin = op.in.C;
    sa.w1 = wb + op.w_off; sa.b1 = (const float*)(wb + op.b_off);
    sa.w2 = wb + o2.w_off; sa.b2 = (const float*)(wb + o2.b_off);
    sa.out = ob2.ptr; sa.out_cs = ob2.C; sa.out_co = o2.out.co; sa.Cout = o2.cout;
    sa.cat = cb.ptr; sa.cat_cs = cb.C;
    sa.H = cb.H; sa.W = cb.W; sa.n = n; sa.c = op.cout; sa.split = sppf_split(o2.cout, n, e->sw);
    sa.dump = (e->cfg.flags & ZLY_FLAG_DUMP_LOGITS) ? 1 : 0;
    return sa;
}

// the fused bottleneck pair's arguments at batch n, on the tiling of plan pl
static PairArgs make_pair_args(const zly_engine* e, const PairGroup& g, const PairPlan& pl, int n)
{
    const Op& A = e->ops[(size_t)g.first];
    const Buffer& ib = e->bufs[(size_t)A.in.buf];
    const Buffer& ob = e->bufs[(size_t)g.out.buf];
    const char* wb = (const char*)e->d_weights;
    PairArgs pa;
    pa.in = ib.ptr; pa.in_cs = ib.C; pa.in_co = A.in.co;
    pa.out = ob.ptr; pa.out_cs = ob.C; pa.out_co = g.out.co;
    pa.wA = wb + g.wA; pa.bA = (const float*)(wb + g.bA);
    pa.wB = wb + g.wB; pa.bB = (const float*)(wb + g.bB);
    pa.H = ib.H; pa.W = ib.W; pa.n = n;
    pa.TH = pl.th; pa.TW = pl.tw; pa.tiles_x = pl.tiles_x; pa.tiles_y = pl.tiles_y; pa.total_tiles = pl.total_tiles;
    pa.res = g.res;
    return pa;
}

// the fused C2f kernel's arguments at batch n, on the tiling of plan pl: the block's input(s), concat buffer and output, cv1 / cv2 and the bottleneck's pair
static C2fArgs make_c2f_args(const zly_engine* e, const C2fGroup& g, const C2fPlan& pl, int n)
{
    const PairGroup& pg = e->pairs[(size_t)g.pair];
    const Buffer& cb = e->bufs[(size_t)g.cat];
    const Buffer& xb = e->bufs[(size_t)g.x.buf];
    const Buffer& ob = e->bufs[(size_t)g.out.buf];
    const char* wb = (const char*)e->d_weights;
    C2fArgs ca{};
    ca.x = xb.ptr; ca.x_cs = xb.C; ca.x_co = g.x.co;
    if (g.x2.buf >= 0) {
        const Buffer& x2 = e->bufs[(size_t)g.x2.buf];
        ca.x2 = x2.ptr; ca.x2_cs = x2.C; ca.x2_co = g.x2.co; ca.split_c = g.x.C;
    }
    ca.w1 = wb + g.w1; ca.b1 = (const float*)(wb + g.b1); ca.nk1 = g.nk1;
    ca.cat = cb.ptr; ca.cat_cs = cb.C; ca.pair_in_co = e->ops[(size_t)pg.first].in.co; ca.pair_out_co = pg.out.co;
    ca.wA = wb + pg.wA; ca.bA = (const float*)(wb + pg.bA); ca.wB = wb + pg.wB; ca.bB = (const float*)(wb + pg.bB);
    ca.res = g.res;
    ca.w2 = wb + g.w2; ca.b2 = (const float*)(wb + g.b2); ca.nk2 = g.nk2; ca.Cout2 = g.cout2;
    ca.out = ob.ptr; ca.out_cs = ob.C; ca.out_co = g.out.co;
    ca.H = cb.H; ca.W = cb.W; ca.n = n;
    ca.TH = pl.th; ca.TW = pl.tw; ca.tiles_x = pl.tiles_x; ca.tiles_y = pl.tiles_y; ca.total_tiles = pl.total_tiles;
    ca.dump = (e->cfg.flags & ZLY_FLAG_DUMP_LOGITS) ? 1 : 0;
    if (g.c == 64 && g.mid.buf >= 0) { const Buffer& mb = e->bufs[(size_t)g.mid.buf]; ca.mid = mb.ptr; ca.mid_cs = mb.C; }
    return ca;
}

// What every op launches at batch n, in op order: built once per batch size (under e->mu; run_path builds it before it captures that size) and
// read by run_op, zly_op_kernel_name, zly_launch_info_at, zly_profile_ops and zly_debug_tap, so that what they report is what runs.
// It describes the detect paths, whose front kernel covers ops[0..2] (preprocess, model.0, model.1) where the stem is fused; zly_forward,
// which has no frames, runs model.0 and model.1 as generic convs (run_ops).  Where fusions could claim the same op, the first of these takes it:
// the front kernel, the fused C2f block (over the bottleneck pair inside it), the fused SPPF, the merged Detect convs, the bottleneck pair, the
// K-packed class-branch conv, the generic conv.
static const std::vector<Launch>& resolve_launches(zly_engine* e, int n)
{
    auto it = e->launches.find(n);
    if (it != e->launches.end()) return it->second;
    const bool bf16 = e->dtype == ZLY_DTYPE_BF16, fusion = bf16 && !(e->cfg.flags & ZLY_FLAG_NO_FUSION), dump = (e->cfg.flags & ZLY_FLAG_DUMP_LOGITS) != 0;
    const int nops = (int)e->ops.size();
    // the fused C2f kernel for group g (ZLY_NO_C2F: tuning / tests)
    auto c2f_of = [&](const C2fGroup& g, C2fPlan* pl) {
        if (!fusion || e->sw.no_c2f) return false;
        const Buffer& b = e->bufs[(size_t)g.cat];
        return c2f_plan(g.c, g.mode, g.nk1, g.nk2, g.cout2, n, b.H, b.W, e->sw, pl);
    };
    // the fused bottleneck pair at its first conv, op a.  Only degenerate launches (a handful of tiles) stay on the per-conv kernels: at batch 1
    // (91 / 234 tiles) one fused launch beats two per-conv launches, 4370 -> 4475 fps.  Width 64 is built and tested, but no faster than two launches.
    auto pair_of = [&](int a, PairPlan* pl) {
        const Op& A = e->ops[(size_t)a];
        if (A.pair < 0 || !fusion) return false;
        const PairGroup& g = e->pairs[(size_t)A.pair];
        if (g.first != a || !(e->sw.pair_widths & g.c)) return false;
        const Buffer& b = e->bufs[(size_t)A.in.buf];
        return pair_plan(g.c, n, b.H, b.W, e->sw, pl) && pl->total_tiles >= e->sw.pair_min_tiles;
    };
    // a 64-channel bottleneck's pair as one weight-stationary launch at its first conv, op a (conv3x3_ws_pair_kernel): where the old LDS-weight pair
    // kernel is not asked for (width 64 in ZLY_PAIR_WIDTHS keeps that meaning) and both convs would on their own be the weight-stationary kernel
    auto ws_pair_of = [&](int a, WsPairPlan* pl) {
        const Op& A = e->ops[(size_t)a];
        if (A.pair < 0 || !fusion) return false;
        const PairGroup& g = e->pairs[(size_t)A.pair];
        if (g.first != a || g.c != 64 || (e->sw.pair_widths & 64)) return false;
        const ConvArgs ca = make_conv_args(e, A, n), cb = make_conv_args(e, e->ops[(size_t)g.second], n);
        ConvPlan pa{}, pb{};
        conv_plan(e->dtype, 3, ca, e->sw, &pa);
        conv_plan(e->dtype, 3, cb, e->sw, &pb);
        return conv_ws_pair_plan(ca, cb, pa, pb, e->sw, pl);
    };
    // SPPF as one launch at model.9.cv1 (opt-in, ZLY_SPPF_FUSED=1); the pool and cv2 then launch nothing
    bool sppf = fusion && e->sw.sppf_fused && e->sppf_cv1 >= 0;
    if (sppf) {
        const Op& a = e->ops[(size_t)e->sppf_cv1];
        const Op& b = e->ops[(size_t)e->sppf_cv2];
        sppf = a.act && b.act && a.res.buf < 0 && b.res.buf < 0 && a.in2.buf < 0 && b.in.C == 4 * a.cout && a.cout_pad == a.cout && b.cout_pad == b.cout &&
               sppf_fused_ok(make_sppf_args(e, n));
    }
    // the Detect convs as two launches on the latency path (conv_igemm_multi_kernel): batch <= 4, no side streams in use.  The launch of the
    // three stems is booked on the P5 stem, that of the six branch convs on P5's box-branch conv.
    const bool merge = bf16 && e->det_merge_ok && n <= 4 && !lanes_active(e, n) && !e->sw.no_det_merge;
    auto merged_at = [&](int i) {
        for (int l = 0; l < 3; ++l) {
            if (i == e->det_stem[l]) return e->det_stem[2];
            if (i == e->det_a[l] || i == e->det_b[l]) return e->det_a[2];
        }
        return -1;
    };
    // the Detect tail: one launch per level behind its branch convs when the side streams are in use (+0.3 % at batch 64), else one launch of
    // all levels at the last tail op
    const bool tail_split = lanes_active(e, n) && !e->sw.no_tail_split;
    const int tail = e->tail.op[2];
    // The box branch's second conv (cv2.L.1, 64 -> 64) inside the tail, at surviving anchors only (kernels_head.hip: tail_box_conv): per level, where the
    // tail can reproduce the bits of the dense launch -- i.e. where that launch would be one of the two kernels whose k-step order it carries.
    // conv3x3_ws_kernel (TPW = 1 and 2 alike) walks the k-steps in storage order, conv3x3_lds_kernel chunk by chunk; the row-tile form (ZLY_WS_ROWT) has a
    // third order, the direct kernel and the merged latency-path launch stay dense.  Automatic mode: only where the tail's early-out is live, and from
    // the confidence threshold up at which it measured no slower than the dense launch.
    auto tail_box_mode = [&](int l) {
        const int ai = e->det_a[l];
        if (!bf16 || !fusion || e->sw.tail_box == 0 || ai < 0 || merge) return 0;
        if (e->sw.tail_box != 2 && (dump || !(e->cfg.flags & ZLY_FLAG_NO_HEAD_TENSOR) || e->cfg.conf_thr < e->sw.tail_box_min_conf)) return 0;
        const Op& op = e->ops[(size_t)ai];
        const Buffer& sb = e->bufs[(size_t)e->tail.stem[l]];
        if (op.ks != 3 || op.stride != 1 || !op.act || op.in.C != 64 || op.cout != 64 || op.cout_pad != 64 || op.nk != 18 || op.res.buf >= 0 || op.in.co != 0 || op.pair >= 0 || op.c2f >= 0) return 0;
        if ((size_t)n * sb.H * sb.W * sb.C * 2 >= ((size_t)1 << 31)) return 0;          // the tail's pixel fragments are buffer loads with 32-bit offsets
        ConvPlan cp{};
        conv_plan(e->dtype, op.ks, make_conv_args(e, op, n), e->sw, &cp);
        if (cp.ksplit > 1) return 0;
        if (cp.kind == CONV_WS && !cp.rowt) return 1;
        if (cp.kind == CONV_LDS) return 2;
        return 0;
    };
    const int box_mode[3] = {tail_box_mode(0), tail_box_mode(1), tail_box_mode(2)};
    auto box_level = [&](int i) { for (int l = 0; l < 3; ++l) if (i == e->det_a[l] && box_mode[l]) return l; return -1; };

    const bool lb = (e->cfg.flags & ZLY_FLAG_LETTERBOX) != 0;
    std::vector<Launch> t((size_t)nops);
    for (int i = 0; i < nops; ++i) {
        const Op& op = e->ops[(size_t)i];
        Launch& L = t[(size_t)i];
        L.covered_by = i;
        L.lb = lb && (op.kind == OP_PREPROCESS || op.kind == OP_HEAD || (i == 1 && e->stem_fused));
        auto covered = [&](int by) { L.kind = LK_NONE; L.covered_by = by; };
        switch (op.kind) {
        case OP_PREPROCESS:
            if (e->stem_fused) covered(1);
            else L.kind = LK_PREPROCESS;
            break;
        case OP_SPPF: {
            const Buffer& b = e->bufs[(size_t)op.in.buf];
            if (sppf) covered(e->sppf_cv1);
            else { L.kind = LK_SPPF_POOL; L.pool16 = sppf_pool16_ok(e->dtype, b.C, op.in.C, n, b.H, b.W, e->sw.pool_six_pass ? 1 : 0); }
            break;
        }
        case OP_HEAD:
            if (tail_split || op.level == 2) { L.kind = LK_HEAD; L.only_level = tail_split ? op.level : -1; for (int l = 0; l < 3; ++l) L.box_mode[l] = box_mode[l]; }
            else covered(tail);
            break;
        case OP_NMS:
            L.kind = LK_NMS;
            break;
        case OP_CONV: {
            conv_plan(e->dtype, op.ks, make_conv_args(e, op, n), e->sw, &L.conv);
            C2fPlan cp{};
            PairPlan pp{};
            WsPairPlan wp{};
            if (i == 1 && e->stem_fused) {
                L.kind = e->stem1 ? LK_STEM1 : LK_STEM;
                L.hbm = !e->stem1 || dump;                                  // stem_model1_kernel keeps the stem map in LDS
            } else if (i == 2 && e->stem1) {
                covered(1);
            } else if (op.c2f >= 0 && c2f_of(e->c2fs[(size_t)op.c2f], &cp)) {
                const C2fGroup& g = e->c2fs[(size_t)op.c2f];
                if (g.leader == i) { L.kind = LK_C2F; L.c2f = cp; }
                else covered(g.leader);
                L.hbm = g.vis_of(i) == 0 || (g.vis_of(i) == 1 && dump);
            } else if (sppf && i == e->sppf_cv1) {
                L.kind = LK_SPPF_FUSED;
                L.hbm = dump;
            } else if (sppf && i == e->sppf_cv2) {
                covered(e->sppf_cv1);
            } else if (box_level(i) >= 0) {
                covered(tail_split ? e->tail.op[box_level(i)] : tail);
                L.hbm = dump;                                               // computed where a wave survives the tail's early-out; with the dump flag at every anchor, and written out
            } else if (merge && merged_at(i) >= 0) {
                if (merged_at(i) == i) { L.kind = LK_MULTI; L.multi_ct = i == e->det_stem[2] ? 3 : 2; }
                else covered(merged_at(i));
            } else if (pair_of(i, &pp)) {
                L.kind = LK_PAIR; L.pair = pp;
                L.hbm = false;                                              // the intermediate map stays in LDS
            } else if (op.pair >= 0 && e->pairs[(size_t)op.pair].second == i && pair_of(e->pairs[(size_t)op.pair].first, &pp)) {
                covered(e->pairs[(size_t)op.pair].first);
            } else if (ws_pair_of(i, &wp)) {
                L.kind = LK_WS_PAIR; L.ws_pair = wp;
                L.hbm = dump;                                               // the intermediate map stays in LDS; with the dump flag the kernel writes it out as well
            } else if (op.pair >= 0 && e->pairs[(size_t)op.pair].second == i && ws_pair_of(e->pairs[(size_t)op.pair].first, &wp)) {
                covered(e->pairs[(size_t)op.pair].first);
            } else if (op.wsk_w && !e->sw.no_wsk && bf16 && conv_wsk_ok(make_wsk_args(e, op, n), e->sw, &L.wsk)) {
                L.kind = LK_CONV_WSK;
            } else {
                L.kind = LK_CONV;
            }
            break;
        }
        }
    }
    return e->launches.emplace(n, std::move(t)).first->second;
}

// channel ranges an op reads / writes, as (buffer, first channel, channels, pixels per frame, scale) records
struct IoView { int buf, co, C; double px, scale; };
static void op_reads(const zly_engine* e, const Op& op, std::vector<IoView>* out)
{
    if (op.kind == OP_CONV) {
        const Buffer& ib = e->bufs[(size_t)op.in.buf];
        out->push_back({op.in.buf, op.in.co, op.in.C, (double)ib.H * ib.W, op.cin_frac});
        if (op.in2.buf >= 0) { const Buffer& b2 = e->bufs[(size_t)op.in2.buf]; out->push_back({op.in2.buf, op.in2.co, op.in2.C, (double)b2.H * b2.W, op.cin_frac}); }
        if (op.res.buf >= 0) { const Buffer& rb = e->bufs[(size_t)op.res.buf]; out->push_back({op.res.buf, op.res.co, op.res.C > 0 ? op.res.C : op.cout, (double)rb.H * rb.W, 1.0}); }
    } else if (op.kind == OP_SPPF) {
        const Buffer& b = e->bufs[(size_t)op.in.buf];
        out->push_back({op.in.buf, op.in.co, op.in.C, (double)b.H * b.W, 1.0});
    } else if (op.kind == OP_HEAD) {                      // a tail op stands for its own level; one launch for all levels = a group of the three
        const int box = e->tail.box[op.level], cls = e->tail.cls[op.level];
        const Buffer& bb = e->bufs[(size_t)box];
        const Buffer& cb = e->bufs[(size_t)cls];
        out->push_back({box, 0, bb.C, (double)bb.H * bb.W, 1.0});
        out->push_back({cls, 0, cb.C, (double)cb.H * cb.W, 1.0});
    }
}
static void op_writes(const zly_engine* e, const Op& op, std::vector<IoView>* out)
{
    if (op.kind == OP_CONV) {
        const Buffer& ob = e->bufs[(size_t)op.out.buf];
        out->push_back({op.out.buf, op.out.co, op.cout, (double)ob.H * ob.W, 1.0});
    } else if (op.kind == OP_SPPF) {
        const Buffer& b = e->bufs[(size_t)op.in.buf];
        out->push_back({op.in.buf, op.in.co + op.in.C, 3 * op.in.C, (double)b.H * b.W, 1.0});
    } else if (op.kind == OP_PREPROCESS) {
        const Buffer& b = e->bufs[(size_t)e->in_buf];
        out->push_back({e->in_buf, 0, 8, (double)b.H * b.W, 3.0 / 8.0});
    }
}

// What the front kernel of a call reads.  A plain engine: the call's frames and descriptors, as they are.  An area engine (ZLY_FLAG_AREA): the pre-pass
// (kernels_area.hip) runs here, on the call's stream ahead of the front kernel, and the front kernel reads its output -- model-sized tight BGR frames,
// for which the engine's BGR variant (e->front: run_path, area_front) is the identity map -- through the constant table.  The Detect tail keeps reading
// d_desc: boxes are mapped from the request's sizes.
static hipError_t front_source(zly_engine* e, int n, const uint8_t** src, const FrameDesc** desc, hipStream_t s)
{
    if (!(e->cfg.flags & ZLY_FLAG_AREA)) return hipSuccess;
    const hipError_t r = launch_area(*src, e->d_desc, n, e->area_view, e->d_area, e->cfg.model_w, e->cfg.model_h, (e->cfg.flags & ZLY_FLAG_LETTERBOX) != 0,
                                     e->sw.num_cus, s);
    *src = e->d_area; *desc = e->d_area_desc;
    return r;
}

// launches what the launch table says op i launches at batch n (nothing for LK_NONE)
static hipError_t run_op(zly_engine* e, size_t i, const Launch& L, int n, const uint8_t* d_src, void* d_slabs_out, uint32_t tag0, hipStream_t s)
{
    const Op& op = e->ops[i];
    const FrameDesc* desc = e->d_desc;
    if (L.kind == LK_PREPROCESS || L.kind == LK_STEM || L.kind == LK_STEM1) {
        const hipError_t r = front_source(e, n, &d_src, &desc, s);
        if (r != hipSuccess) return r;
    }
    switch (L.kind) {
    case LK_NONE:
        return hipSuccess;
    case LK_PREPROCESS:
        return launch_preprocess(e->dtype, d_src, desc, n, e->bufs[(size_t)e->in_buf].ptr, nullptr, e->cfg.model_w, e->cfg.model_h, s, e->front);
    case LK_STEM: {
        StemArgs st = e->stem;
        st.src = d_src; st.desc = desc;
        return launch_stem_fused(st, n, s, e->front);
    }
    case LK_STEM1: {
        Stem1Args st = e->stem1a;
        st.st.src = d_src; st.st.desc = desc;
        return launch_stem_model1(st, n, s, e->front);
    }
    case LK_CONV:
        return launch_conv(make_conv_args(e, op, n), L.conv, s);
    case LK_CONV_WSK:
        return launch_conv_wsk(make_wsk_args(e, op, n), L.wsk, s);
    case LK_MULTI: {
        ConvArgsMulti m{};
        for (int l = 0; l < 3; ++l) {
            if (L.multi_ct == 3) m.a[m.n++] = make_conv_args(e, e->ops[(size_t)e->det_stem[l]], n);
            else { m.a[m.n++] = make_conv_args(e, e->ops[(size_t)e->det_a[l]], n); m.a[m.n++] = make_conv_args(e, e->ops[(size_t)e->det_b[l]], n); }
        }
        return launch_conv_multi(m, L.multi_ct, s);
    }
    case LK_C2F: {
        const C2fGroup& g = e->c2fs[(size_t)op.c2f];
        return launch_c2f(g.c, g.mode, make_c2f_args(e, g, L.c2f, n), L.c2f, s);
    }
    case LK_PAIR: {
        const PairGroup& g = e->pairs[(size_t)op.pair];
        return launch_pair(g.c, make_pair_args(e, g, L.pair, n), L.pair, s);
    }
    case LK_WS_PAIR: {
        const PairGroup& g = e->pairs[(size_t)op.pair];
        return launch_conv_ws_pair(make_conv_args(e, op, n), make_conv_args(e, e->ops[(size_t)g.second], n), L.ws_pair, (e->cfg.flags & ZLY_FLAG_DUMP_LOGITS) != 0, s);
    }
    case LK_SPPF_FUSED:
        return launch_sppf_fused(make_sppf_args(e, n), s);
    case LK_SPPF_POOL: {
        const Buffer& b = e->bufs[(size_t)op.in.buf];
        return launch_sppf_pool(e->dtype, b.ptr, b.C, op.in.C, n, b.H, b.W, s, e->sw.pool_six_pass ? 1 : 0);
    }
    case LK_HEAD: {
        HeadArgs h = e->tail.args;
        h.only_level = L.only_level;
        for (int l = 0; l < 3; ++l) {
            if (!L.box_mode[l]) continue;
            const Buffer& sb = e->bufs[(size_t)e->tail.stem[l]];
            h.lv[l].box_mode = L.box_mode[l]; h.lv[l].box_in = sb.ptr; h.lv[l].box_cs = sb.C;     // cv2.L.1's input: the stem buffer's box half (channels [0, 64))
        }
        if (L.lb) { h.lb_tw = e->cfg.model_w; h.lb_th = e->cfg.model_h; }      // boxes are mapped out of the letterbox (the geometry comes from d_desc at run time: no graph key)
        h.head = (e->cfg.flags & ZLY_FLAG_NO_HEAD_TENSOR) ? nullptr : e->d_head; h.desc = e->d_desc; h.conf_thr = e->cfg.conf_thr; h.cand = e->cur_cand; h.cand_count = e->cur_count;
        return launch_head_fused(e->dtype, h, n, s);
    }
    case LK_NMS:
        return launch_nms(e->cur_cand, e->cur_count, e->N, n, e->cfg.iou_thr, e->nc, e->d_scratch,
                          d_slabs_out ? d_slabs_out : e->d_slabs, e->cfg.max_dets, tag0, s, e->sw.nms_general ? 1 : 0);
    }
    return hipErrorInvalidValue;
}

// ops [first, last) of the launch table `tab` -- the graph-capturable middle of the path is [1, ops.size()-1).  Side-lane ops are
// launched on the engine's side streams behind a fork event; the Detect tail (OP_HEAD) joins them.
static hipError_t run_ops(zly_engine* e, const std::vector<Launch>& tab, size_t first, size_t last, int n, hipStream_t s)
{
    bool forked[3] = {false, false, false};
    hipError_t r = hipSuccess;
    auto join_all = [&]() {
        for (int l = 1; l <= 2 && r == hipSuccess; ++l) {
            if (!forked[l]) continue;
            r = hipEventRecord(e->ev_join[l - 1], e->side[l - 1]);
            if (r == hipSuccess) r = hipStreamWaitEvent(s, e->ev_join[l - 1], 0);
            forked[l] = false;
        }
    };
    for (size_t i = first; i < last && r == hipSuccess; ++i) {
        const Op& op = e->ops[i];
        hipStream_t st = s;
        // measured: at batch 1 the cross-stream edges cost more than the overlap buys (0.27 -> 0.34 ms/frame);
        // from batch 16 up the Detect branches are long enough to pay (1.42 -> 1.38 ms per 64 frames)
        if (op.lane > 0 && lanes_active(e, n)) {
            st = e->side[op.lane - 1];
            if (!forked[op.lane]) {
                r = hipEventRecord(e->ev_fork[op.lane - 1], s);
                if (r == hipSuccess) r = hipStreamWaitEvent(st, e->ev_fork[op.lane - 1], 0);
                forked[op.lane] = true;
                if (r != hipSuccess) break;
            }
        }
        if (op.kind == OP_NMS) { join_all(); if (r != hipSuccess) break; }       // the tail launches only append candidates: no join needed before them
        // the side streams are joined in front of the P5 branch rather than at the very end: they have long finished by then, and
        // the hand-over (~10 us on the main stream) then overlaps nothing less than at the step boundary (+0.7 %)
        if ((int)i == e->join_at) { join_all(); if (r != hipSuccess) break; }
        // ZLY_ABLATE_SKIP=<op name>[,<op name>...]: the named launches are left out (results are garbage): measures what a launch costs the
        // step when several engines' chains overlap, which its isolated duration does not tell (tools/ablate_launches.sh)
#ifdef ZLY_DIAG         // diagnostic build only (libzly_diag.so): a shipped engine cannot be told to skip launches
        if (!e->sw.ablate.empty() && e->sw.ablate.find("," + op.name + ",") != std::string::npos) continue;
#endif
        // zly_forward has no frames: the convs the front kernel covers on the detect paths (model.0, model.1) run as generic convs
        const int by = tab[(size_t)tab[i].covered_by].kind;
        if (op.kind == OP_CONV && (by == LK_STEM || by == LK_STEM1)) { Launch g = tab[i]; g.kind = LK_CONV; r = run_op(e, i, g, n, nullptr, nullptr, 0, st); }
        else r = run_op(e, i, tab[i], n, nullptr, nullptr, 0, st);
    }
    if (r == hipSuccess) join_all();
    return r;
}

// every stream that may hold an outstanding deferred NMS is joined into `s`
// lag = 0: all of them; lag = 1: all but the most recent call's (so that the caller can consume call k-1's slabs on
// `s` right after enqueuing call k without putting NMS(k) in front of call k+1).  NMS launches are serialised on one
// stream, so waiting for a call's event covers every earlier call.
static int join_nms(zly_engine* e, hipStream_t s, int lag = 0)
{
    if (e->last_async < 0) return ZLY_OK;                // nothing outstanding
    const int p = lag == 0 ? e->last_async : e->last_async ^ 1;
    if (e->nms_recorded[p]) HIP_TRY(hipStreamWaitEvent(s, e->ev_nms[p], 0), ZLY_ERR_INFERENCE);
    return ZLY_OK;
}

// The process-wide enqueue gate.  Enqueue sections of different engines (launches, async copies, event records: ~0.03-0.1 ms of host
// work per batch) hold it SHARED and run concurrently -- with ZLY_NUM_DEVICES x ZLY_ENGINES_PER_GPU dispatcher threads a single mutex
// here serialised sixteen threads at the same order of time a GPU needs per batch.  What must be alone in the process holds it
// EXCLUSIVE: stream capture (a HIP call from another engine's thread while a capture was open -- a launch, an async copy, an event
// wait -- failed both sides with "operation failed due to a previous error during capture", thread-local and relaxed modes alike) and
// device allocation / release (zly_create, zly_destroy, the staging ring: hot reload builds engines beside running ones).  Captures
// happen at zly_create (batch 1 and max_batch) and otherwise only on the first call of a new batch size on the synchronous entry points.
// Writers are preferred: a waiting capture is not starved by a steady stream of enqueues.
class EnqueueGate {
    std::mutex m_;
    std::condition_variable cv_;
    int readers_ = 0, writers_waiting_ = 0;
    bool writer_ = false;
public:
    void lock_shared() { std::unique_lock<std::mutex> lk(m_); cv_.wait(lk, [&] { return !writer_ && writers_waiting_ == 0; }); ++readers_; }
    void unlock_shared() { std::lock_guard<std::mutex> lk(m_); if (--readers_ == 0) cv_.notify_all(); }
    void lock() { std::unique_lock<std::mutex> lk(m_); ++writers_waiting_; cv_.wait(lk, [&] { return !writer_ && readers_ == 0; }); --writers_waiting_; writer_ = true; }
    void unlock() { std::lock_guard<std::mutex> lk(m_); writer_ = false; cv_.notify_all(); }
};
static EnqueueGate g_gate;
struct SharedGate {
    bool held = true;
    SharedGate() { g_gate.lock_shared(); }
    ~SharedGate() { if (held) g_gate.unlock_shared(); }
    void release() { if (held) { g_gate.unlock_shared(); held = false; } }
    SharedGate(const SharedGate&) = delete; SharedGate& operator=(const SharedGate&) = delete;
};
struct ExclusiveGate {
    ExclusiveGate() { g_gate.lock(); }
    ~ExclusiveGate() { g_gate.unlock(); }
    ExclusiveGate(const ExclusiveGate&) = delete; ExclusiveGate& operator=(const ExclusiveGate&) = delete;
};

// phase timing of the last sampled call, if its events have completed: added to the stats, never waited for
static void harvest_timing(zly_engine* e)
{
    if (!e->t_pending || hipEventQuery(e->ev_t[3]) != hipSuccess) return;
    float pre = 0.f, fwd = 0.f, post = 0.f;
    if (hipEventElapsedTime(&pre, e->ev_t[0], e->ev_t[1]) == hipSuccess && hipEventElapsedTime(&fwd, e->ev_t[1], e->ev_t[2]) == hipSuccess &&
        hipEventElapsedTime(&post, e->ev_t[2], e->ev_t[3]) == hipSuccess) {
        const int nf = e->t_frames;
        with_stats(e, [&](zly_stats& st) {
            st.sampled_frames += (uint64_t)nf;
            st.sampled_preprocess_ms += pre; st.sampled_forward_ms += fwd; st.sampled_postprocess_ms += post > 0.f ? post : 0.f;
        });
    }
    e->t_pending = false;
}

// the front-kernel variant of a call on this engine: the batch's format level (the highest front_level of its frames), tight frames or frame views
static FrontVariant front_of(const zly_engine* e, int level, bool view = false) { return FrontVariant(level, (e->cfg.flags & ZLY_FLAG_LETTERBOX) != 0, view); }

// An area engine's front kernel reads the pre-pass's output whatever the call's frames are (front_source): the variant of model-sized tight BGR frames.
// What the request frames are -- their formats ride in d_desc -- is the pre-pass's business; it only needs to know whether view records lie behind them.
static FrontVariant area_front(zly_engine* e, FrontVariant variant)
{
    if (!(e->cfg.flags & ZLY_FLAG_AREA)) return variant;
    e->area_view = variant.view;
    return front_of(e, ZLY_FRONT_BGR);
}

// nms_stream_out: the stream the call's NMS (its last kernel) was launched on -- `s`, or the engine's NMS stream when deferred
// variant: the call's front-kernel variant (front_of: the batch's format level -- d_desc says which format each frame has --, and whether the frames are views, d_desc then holding their ViewRec too)
static int run_path(zly_engine* e, int n, const uint8_t* d_src, void* d_slabs_out, uint32_t tag0, hipStream_t s, bool with_pre, bool defer_nms,
                    hipStream_t* nms_stream_out, FrontVariant variant)
{
    e->front = area_front(e, variant);
    const size_t nops = e->ops.size();
    harvest_timing(e);
    const bool sample = with_pre && !e->t_pending && (e->sample_ctr++ % zly_engine::SAMPLE_EVERY) == 0;
    with_stats(e, [&](zly_stats& st) { st.batches++; });
    // like the Detect side streams: below batch 16 the cross-stream edges (event record + two stream waits per call) cost
    // more than the overlap buys -- measured 0.236 -> 0.290 ms per frame at batch 1 -- so small batches stay in stream order
    defer_nms = defer_nms && e->nms_stream != nullptr && n >= 16;
    int par = 0;
    if (defer_nms) {
        // this call's Detect tail fills candidate buffer `par`; the NMS that last read it (two calls back) must be done
        par = e->parity;
        if (e->nms_recorded[par]) HIP_TRY(hipStreamWaitEvent(s, e->ev_nms[par], 0), ZLY_ERR_INFERENCE);
    } else if (e->last_async >= 0) {
        int rcj = join_nms(e, s);                       // a synchronous-path call after deferred ones: plain stream order again
        if (rcj != ZLY_OK) return rcj;
        e->last_async = -1;
    }
    e->cur_cand = par ? e->d_cand_alt : e->d_cand;
    e->cur_count = par ? e->d_count_alt : e->d_count;
    // The front kernel -- preprocess, or on the bf16 engine preprocess + model.0 [+ model.1] as ONE kernel (kernels_stem.hip) -- is the
    // launch of ops[0] or ops[1]; the middle starts at the first op it does not cover.  zly_forward (caller-supplied fp32 images) launches
    // no front kernel and starts at model.0.
    const std::vector<Launch>& tab = resolve_launches(e, n);
    const size_t front = (size_t)tab[0].covered_by;
    size_t first = 1;
    if (sample) HIP_TRY(hipEventRecord(e->ev_t[0], s), ZLY_ERR_INFERENCE);
    if (with_pre) {
#ifdef ZLY_DIAG
        if (tab[front].kind == LK_STEM1 && e->sw.ablate.find(",stem,") != std::string::npos) { /* ZLY_ABLATE_SKIP=stem (libzly_diag.so only) */ } else
#endif
        HIP_TRY(run_op(e, front, tab[front], n, d_src, nullptr, 0, s), ZLY_ERR_INFERENCE);
        for (first = front + 1; tab[first].covered_by == (int)front; ++first) {}
    }
    e->last_front = with_pre;
    const bool fused = with_pre && front > 0;
    if (sample) HIP_TRY(hipEventRecord(e->ev_t[1], s), ZLY_ERR_INFERENCE);
    // Graph replay.  Graphs are captured at zly_create for batch 1 and max_batch (warm_batch) and, on the synchronous entry points, on the
    // first call of any other batch size.  The pipelined host path (dispatcher threads, several per process) never captures: it replays
    // what exists -- a lone frame and a full batch, its two steady states -- and launches other partial batches eagerly with cached
    // kernel shapes: no capture storm over the 62 partial sizes, no capture while other engines run.
    // No "YUV in batch" or "views" bit: the front kernel (preprocess / fused stem, the only kernel that reads pixels and hence the only one with a YUV
    // instantiation) is launched above, outside the captured range [first, nops - 1), so one graph serves BGR, YUV and mixed batches alike.
    const int key = (n * 2 + (fused ? 1 : 0)) * 2 + par;     // the captured Detect tail holds the candidate buffer's address
    auto git = e->graphs.find(key);
    if (e->cfg.use_graph && git == e->graphs.end() && !e->ingest_active) {
        // Capture on the engine's own stream, then replay on whichever stream the caller uses.  The caller holds the enqueue gate shared;
        // a capture needs it exclusively (see EnqueueGate).  e->mu is held throughout, so nothing else touches this engine meanwhile.
        hipGraph_t g = nullptr;
        hipGraphExec_t ge = nullptr;
        HIP_TRY(hipStreamSynchronize(s), ZLY_ERR_INFERENCE);
        g_gate.unlock_shared();
        {
            ExclusiveGate x;
            hipError_t r = hipStreamBeginCapture(e->stream, hipStreamCaptureModeRelaxed);
            if (r == hipSuccess) {
                r = run_ops(e, tab, first, nops - 1, n, e->stream);
                hipError_t r2 = hipStreamEndCapture(e->stream, &g);
                if (r == hipSuccess) r = r2;
            }
            if (r == hipSuccess) r = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
            if (g) hipGraphDestroy(g);
            if (r != hipSuccess) { (void)hipGetLastError(); ge = nullptr; }
        }
        g_gate.lock_shared();
        // a failed capture is retried once (on the next call of this shape) before the shape is left on eager launches for good
        if (ge || ++e->graph_failures[key] >= 2) git = e->graphs.emplace(key, ge).first;
    }
    if (e->cfg.use_graph && git != e->graphs.end() && git->second) {
        HIP_TRY(hipGraphLaunch(git->second, s), ZLY_ERR_INFERENCE);
        with_stats(e, [](zly_stats& st) { st.graph_replays++; });
    } else {
        HIP_TRY(run_ops(e, tab, first, nops - 1, n, s), ZLY_ERR_INFERENCE);
        with_stats(e, [](zly_stats& st) { st.eager_batches++; });
    }
    if (sample) HIP_TRY(hipEventRecord(e->ev_t[2], s), ZLY_ERR_INFERENCE);
    hipStream_t ns = s;
    if (defer_nms) {
        ns = e->nms_stream;
        HIP_TRY(hipEventRecord(e->ev_head, s), ZLY_ERR_INFERENCE);
        HIP_TRY(hipStreamWaitEvent(e->nms_stream, e->ev_head, 0), ZLY_ERR_INFERENCE);
        HIP_TRY(run_op(e, nops - 1, tab[nops - 1], n, nullptr, d_slabs_out, tag0, e->nms_stream), ZLY_ERR_INFERENCE);
        HIP_TRY(hipEventRecord(e->ev_nms[par], e->nms_stream), ZLY_ERR_INFERENCE);
        e->nms_recorded[par] = true; e->last_async = par; e->parity = par ^ 1;
    } else {
        HIP_TRY(run_op(e, nops - 1, tab[nops - 1], n, nullptr, d_slabs_out, tag0, s), ZLY_ERR_INFERENCE);
    }
    if (sample) {
        HIP_TRY(hipEventRecord(e->ev_t[3], ns), ZLY_ERR_INFERENCE);
        e->t_pending = true; e->t_frames = n;
    }
    if (nms_stream_out) *nms_stream_out = ns;
    e->last_n = n;
    return ZLY_OK;
}

// fmt: per-frame ZLY_PIX_* (null = all BGR), packed into the top byte of src_off (zly_internal.h)
// views: per-frame ViewRec of a call on frame views (null = tight frames), uploaded behind the n descriptors
static int set_desc(zly_engine* e, int n, const int32_t* w, const int32_t* h, const size_t* offs, hipStream_t s, const int32_t* fmt = nullptr,
                    const ViewRec* views = nullptr)
{
    // what the device holds is reused only by a call of the same kind: a plain call's upload has no view records, and a view call's records
    // belong to its own pitches and plane offsets even where src_off, w, h agree
    bool same = (int)e->desc_cache.size() >= n && e->desc_cache_view == (views != nullptr);
    for (int i = 0; i < n && same; ++i)
        same = e->desc_cache[(size_t)i].w == w[i] && e->desc_cache[(size_t)i].h == h[i] && e->desc_cache[(size_t)i].src_off == desc_pack(offs[i], fmt ? fmt[i] : ZLY_PIX_BGR);
    if (same && views) same = (int)e->view_cache.size() >= n && memcmp(e->view_cache.data(), views, sizeof(ViewRec) * (size_t)n) == 0;
    // the view records lie at desc + n: a view call of another batch size finds them elsewhere
    if (same && views) same = e->last_desc_n == n;
    if (same) return ZLY_OK;
    // frame sizes / offsets changed: next entry of the pinned ring, uploaded in stream order.  Calls on one engine are
    // stream-ordered by contract (they share every activation buffer), so the upload cannot overtake a kernel of the
    // previous call that still reads d_desc; the ring entry itself is only reused once ITS upload has completed.
    int r = 0;
    HIP_TRY(e->desc_ring.claim(&r), ZLY_ERR_INFERENCE);
    FrameDesc* hd = reinterpret_cast<FrameDesc*>(reinterpret_cast<unsigned char*>(e->h_desc) + (size_t)r * (size_t)e->cfg.max_batch * zly_engine::DESC_SLOT);
    if ((int)e->desc_cache.size() < n) e->desc_cache.resize((size_t)n);
    for (int i = 0; i < n; ++i) {
        FrameDesc d; d.src_off = desc_pack(offs[i], fmt ? fmt[i] : ZLY_PIX_BGR); d.w = w[i]; d.h = h[i];
        hd[i] = d;
        e->desc_cache[(size_t)i] = d;
    }
    for (size_t i = (size_t)n; i < e->desc_cache.size(); ++i) e->desc_cache[i].w = -1;
    size_t bytes = sizeof(FrameDesc) * (size_t)n;
    if (views) {
        memcpy(hd + n, views, sizeof(ViewRec) * (size_t)n);
        e->view_cache.assign(views, views + n);
        bytes += sizeof(ViewRec) * (size_t)n;
    }
    e->desc_cache_view = views != nullptr;
    e->last_desc_n = n;
    HIP_TRY(hipMemcpyAsync(e->d_desc, hd, bytes, hipMemcpyHostToDevice, s), ZLY_ERR_INFERENCE);
    HIP_TRY(e->desc_ring.mark(r, s), ZLY_ERR_INFERENCE);
    return ZLY_OK;
}

// Track, in place, the frames of `slabs` (n slabs of this engine's size) whose entry of streams[] is not -1: group them by stream, upload the
// grouping, launch track_kernel on `s` -- the stream the slabs' NMS ran on, or one already ordered behind it.  Under e->mu, enqueue gate held;
// streams[] is validated by the caller.  A call without a tracked frame launches nothing (*launched = false).
static int track_enqueue(zly_engine* e, Track* tk, int n, const int32_t* streams, void* slabs, hipStream_t s, bool* launched)
{
    *launched = false;
    int n_tracked = 0, n_seg = 0;
    for (int i = 0; i < n; ++i) if (streams[i] >= 0) ++n_tracked;
    if (n_tracked == 0) return ZLY_OK;
    // an engine with camera motion: behind the most recent zly_camera_apply_tracks, which marks an entry of this ring, on whichever stream it ran
    if (e->camera) HIP_TRY(tk->ring.wait_last(s), ZLY_ERR_INFERENCE);
    int r = 0;
    HIP_TRY(tk->ring.claim(&r), ZLY_ERR_INFERENCE);
    int* g = tk->ring.host<int>(r);
    // segments in the order of their stream's first occurrence; frames of a segment in index order
    std::vector<int>& seg_of = tk->seg_of;
    int* count = g + 1;                                                              // first: frames per segment, at [1 + seg + 1]
    for (int i = 0; i < n; ++i) {
        if (streams[i] < 0) continue;
        int& sg = seg_of[(size_t)streams[i]];
        if (sg < 0) { sg = n_seg++; count[sg + 1] = 0; }
        count[sg + 1]++;
    }
    int* seg_stream = g + 2 + n_seg;
    int* frames = g + 2 + 2 * n_seg;
    g[0] = n_seg;
    g[1] = 0;
    for (int sg = 0; sg < n_seg; ++sg) g[2 + sg] += g[1 + sg];                       // inclusive scan: g[1 + sg] = offset of segment sg, g[1 + n_seg] = n_tracked
    std::vector<int> fill((size_t)n_seg);
    for (int sg = 0; sg < n_seg; ++sg) fill[(size_t)sg] = g[1 + sg];
    for (int i = 0; i < n; ++i) {
        if (streams[i] < 0) continue;
        const int sg = seg_of[(size_t)streams[i]];
        seg_stream[sg] = streams[i];
        frames[fill[(size_t)sg]++] = i;
    }
    for (int i = 0; i < n; ++i) if (streams[i] >= 0) seg_of[(size_t)streams[i]] = -1;
    const int* dg = tk->ring.dev<int>(r);
    HIP_TRY(tk->ring.upload(r, sizeof(int) * (size_t)(2 + 2 * n_seg + n_tracked), s), ZLY_ERR_INFERENCE);
    if (tk->d_motion)
        HIP_TRY(launch_track_motion(tk->d_state, tk->d_motion, dg, n_seg, slabs, e->cfg.max_dets, tk->cfg.max_tracks, tk->cfg.match_iou, (uint32_t)tk->cfg.max_lost,
                                    tk->mcfg.beta, tk->mcfg.v_max, s), ZLY_ERR_INFERENCE);
    else
        HIP_TRY(launch_track(tk->d_state, dg, n_seg, slabs, e->cfg.max_dets, tk->cfg.max_tracks, tk->cfg.match_iou, (uint32_t)tk->cfg.max_lost, s), ZLY_ERR_INFERENCE);
    HIP_TRY(tk->ring.mark(r, s), ZLY_ERR_INFERENCE);
    *launched = true;
    return ZLY_OK;
}

// every tracked launch made so far has completed (under e->mu: none can be enqueued meanwhile)
static int track_drain(Track* tk)
{
    HIP_TRY(tk->ring.drain(), ZLY_ERR_INFERENCE);
    return ZLY_OK;
}

// Where work on the slabs of the most recent zly_detect_device* call goes (tracking, a merge, chips): behind that call's NMS, on whichever stream it
// ran.  s: the caller's choice on entry.  It becomes the engine's NMS stream when the NMS was deferred; otherwise it stays, and waits for the call's
// completion event where it is not the stream the call itself was given.  Before any such call: s as it is.
static int stream_after_detect(zly_engine* e, hipStream_t& s)
{
    if (e->call_seq == 0) return ZLY_OK;
    if (e->last_deferred) s = e->last_ns;
    else if (s != e->last_ns) HIP_TRY(hipStreamWaitEvent(s, e->ev_call[(e->call_seq - 1) & 1], 0), ZLY_ERR_INFERENCE);
    return ZLY_OK;
}

// ... and once that work is enqueued on s, the call's completion events move behind it: zly_join, zly_read_slabs, a later call's NMS and whatever
// stream_after_detect orders next wait for both
static int detect_events_behind(zly_engine* e, hipStream_t s)
{
    if (e->call_seq == 0) return ZLY_OK;
    HIP_TRY(hipEventRecord(e->ev_call[(e->call_seq - 1) & 1], s), ZLY_ERR_INFERENCE);
    if (e->last_deferred && e->last_async >= 0) HIP_TRY(hipEventRecord(e->ev_nms[e->last_async], s), ZLY_ERR_INFERENCE);
    return ZLY_OK;
}

static int ensure_stage(zly_engine* e, size_t bytes)
{
    if (bytes <= e->stage_bytes) return ZLY_OK;
    HIP_TRY(hipStreamSynchronize(e->stream), ZLY_ERR_SYSTEM);
    if (e->d_stage) hipFree(e->d_stage);
    if (e->h_stage) hipHostFree(e->h_stage);
    e->d_stage = nullptr; e->h_stage = nullptr; e->stage_bytes = 0;
    const size_t cap = (bytes + (1u << 20) - 1) / (1u << 20) * (1u << 20);
    HIP_TRY(hipMalloc((void**)&e->d_stage, cap), ZLY_ERR_SYSTEM);
    HIP_TRY(hipHostMalloc((void**)&e->h_stage, cap, hipHostMallocDefault), ZLY_ERR_SYSTEM);
    e->stage_bytes = cap;
    return ZLY_OK;
}

static int ensure_scratch_f32(zly_engine* e, size_t elems)
{
    if (elems <= e->scratch_f32_elems) return ZLY_OK;
    HIP_TRY(hipStreamSynchronize(e->stream), ZLY_ERR_SYSTEM);
    if (e->d_scratch_f32) hipFree(e->d_scratch_f32);
    e->d_scratch_f32 = nullptr; e->scratch_f32_elems = 0;
    HIP_TRY(hipMalloc((void**)&e->d_scratch_f32, elems * sizeof(float)), ZLY_ERR_SYSTEM);
    e->scratch_f32_elems = elems;
    return ZLY_OK;
}

static uint64_t now_ms()
{
    return (uint64_t)std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::system_clock::now().time_since_epoch()).count();
}

static void ingest_destroy(zly_engine* e);

// what the VIEW instantiations of the front kernels read of a (checked) view
static ViewRec view_rec(const zly_frame_view* v)
{
    int64_t rows[3], rb[3];
    const int np = plane_shape(v->fmt, v->w, v->h, rows, rb);
    ViewRec r{};
    r.off1 = np > 1 ? v->off[1] : 0; r.off2 = np > 2 ? v->off[2] : 0;
    r.pitch0 = v->pitch[0]; r.pitch1 = np > 1 ? v->pitch[1] : 0; r.pitch2 = np > 2 ? v->pitch[2] : 0;
    return r;
}

// ------------------------------------------------------------------------------------------------
// the scaffold of a call: what the device entries and the read-backs of the C ABI share
// ------------------------------------------------------------------------------------------------

// An engine's feature state, or null with the error set: one message per feature, stated here once.  All but track_of under e->mu.
static const char* const NO_TRACK = "tracking is not enabled on this engine (zly_track_enable)";
static const char* const NO_MERGE = "this engine has not merged yet (zly_merge_slabs)";
static const char* const NO_STORE = "resident surfaces are not enabled on this engine (zly_surfaces_enable)";
static const char* const NO_ZOOM = "zoom regions are not enabled on this engine (zly_track_enable, then zly_zoom_enable)";
static const char* const NO_CHIPS = "chips are not enabled on this engine (zly_chips_enable)";
static const char* const NO_CHANGE = "the change map is not enabled on this engine (zly_change_enable)";
static const char* const NO_CAMERA = "camera motion is not enabled on this engine (zly_camera_enable)";
template <typename T> static T* enabled(T* state, const char* or_else)
{
    if (!state) fail(ZLY_ERR_INVALID_ARGUMENT, or_else);
    return state;
}
static Track* track_of(zly_engine* e) { return enabled(e->track.load(), NO_TRACK); }
static Surfaces* surfaces_of(zly_engine* e) { return enabled(e->surf, NO_STORE); }
static Zoom* zoom_of(zly_engine* e) { return enabled(e->zoom, NO_ZOOM); }
static Chips* chips_of(zly_engine* e) { return enabled(e->chips, NO_CHIPS); }
static Change* change_of(zly_engine* e) { return enabled(e->change, NO_CHANGE); }
static Camera* camera_of(zly_engine* e) { return enabled(e->camera, NO_CAMERA); }

// The stream a device entry enqueues on: the caller's, or the engine's own where the caller names none.  wait_for: an event the caller's stream has to
// wait for first (null = none); the engine's own stream lies behind it already.  Enqueue gate held.
static int wait_if_foreign(zly_engine* e, hipStream_t s, hipEvent_t wait_for)
{
    if (wait_for && s != e->stream) HIP_TRY(hipStreamWaitEvent(s, wait_for, 0), ZLY_ERR_INFERENCE);
    return ZLY_OK;
}
static int call_stream(zly_engine* e, void* stream, hipStream_t* s, hipEvent_t wait_for = nullptr)
{
    *s = stream ? (hipStream_t)stream : e->stream;
    return wait_if_foreign(e, *s, wait_for);
}

// Where a call's frames lie: views v[] of the device buffer [base, base + bytes), and the event a caller's stream waits for before it reads them
struct FrameSource {
    const void* base;
    size_t bytes;
    const zly_frame_view* v;
    hipEvent_t wait_for = nullptr;
};

// The frame table of a call -- what set_desc uploads and run_path's front kernel reads: per frame size, format, offset and (a call on frame views)
// the ViewRec, and the batch's format level.  Appended to view by view, or made of n tight frames; five allocations at the most, as many as the
// arrays it holds.
struct FrameTable {
    std::vector<int32_t> w, h, fmt;
    std::vector<size_t> off;
    std::vector<ViewRec> recs;        // a call on frame views; empty: tight frames
    bool views;
    int level = ZLY_FRONT_BGR;        // the highest front_level of the frames
    FrameTable(int n, bool of_views) : views(of_views)
    {
        w.reserve((size_t)n); h.reserve((size_t)n); fmt.reserve((size_t)n); off.reserve((size_t)n);
        if (views) recs.reserve((size_t)n);
    }
    // n tight w x h frames of one format, frame_bytes apart
    static FrameTable tight(int32_t fmt, int32_t w, int32_t h, size_t frame_bytes, int n)
    {
        FrameTable t(n, false);
        for (int i = 0; i < n; ++i) t.add(fmt, w, h, (size_t)i * frame_bytes);
        return t;
    }
    void add(int32_t f, int32_t fw, int32_t fh, size_t o)
    {
        w.push_back(fw); h.push_back(fh); fmt.push_back(f); off.push_back(o);
        level = std::max(level, front_level(f));
    }
    void add(const zly_frame_view& v) { add(v.fmt, v.w, v.h, (size_t)v.off[0]); recs.push_back(view_rec(&v)); }      // v: checked (check_view)
    int n() const { return (int)w.size(); }
    FrontVariant front(const zly_engine* e) const { return front_of(e, level, views); }
};
static int set_desc(zly_engine* e, const FrameTable& t, hipStream_t s)
{
    return set_desc(e, t.n(), t.w.data(), t.h.data(), t.off.data(), s, t.fmt.data(), t.views ? t.recs.data() : nullptr);
}

// The tail of every device detect entry, behind set_desc: the path on `s` with the engine's NMS mode, then the call's completion event behind its NMS,
// the call counted and remembered (last_ns, last_deferred: stream_after_detect).  record_call = false: a call that enqueues more behind its NMS and
// moves the completion events there itself (detect_events_behind) records none here.  Under e->mu, enqueue gate held.
static int detect_run(zly_engine* e, const FrameTable& t, const void* d_src, void* d_slabs, uint32_t frame_tag0, hipStream_t s, bool record_call = true)
{
    hipStream_t ns = s;
    const int rc = run_path(e, t.n(), (const uint8_t*)d_src, d_slabs, frame_tag0, s, true, (e->cfg.flags & ZLY_FLAG_ASYNC_NMS) != 0, &ns, t.front(e));
    if (rc != ZLY_OK) { with_stats(e, [](zly_stats& st) { st.inference_errors++; }); return rc; }
    if (record_call) HIP_TRY(hipEventRecord(e->ev_call[e->call_seq & 1], ns), ZLY_ERR_INFERENCE);
    e->call_seq++;
    e->last_ns = ns; e->last_deferred = ns != s;
    with_stats(e, [&](zly_stats& st) { st.inference_count += (uint64_t)t.n(); });
    return ZLY_OK;
}
static int detect_enqueue(zly_engine* e, const FrameTable& t, const void* d_src, void* d_slabs, uint32_t frame_tag0, hipStream_t s)
{
    if (int rc = set_desc(e, t, s)) return rc;
    return detect_run(e, t, d_src, d_slabs, frame_tag0, s);
}

// The resident store's side of the reader / writer protocol (Surfaces::ev_read, ev_patch), three halves.  Under e->mu.
// 1. The store has a reader now: a call that read its slots has been enqueued, and its last kernel went to `ran`.  The next writer goes behind it,
//    whichever stream that is.  Takes the enqueue gate itself.
static int surfaces_note_reader(zly_engine* e, Surfaces* sf, hipStream_t ran)
{
    SharedGate gl;
    if (sf->read_pending) HIP_TRY(hipStreamWaitEvent(e->stream, sf->ev_read, 0), ZLY_ERR_INFERENCE);
    HIP_TRY(hipEventRecord(sf->ev_read, ran), ZLY_ERR_INFERENCE);
    sf->read_pending = true;
    return ZLY_OK;
}
// 2. In front of a writer's kernels on the engine's stream: detect calls on other streams may still read the slots it writes.  Enqueue gate held.
static int surfaces_begin_write(zly_engine* e, Surfaces* sf)
{
    if (!sf->read_pending) return ZLY_OK;
    HIP_TRY(hipStreamWaitEvent(e->stream, sf->ev_read, 0), ZLY_ERR_INFERENCE);
    sf->read_pending = false;                                            // from here on the dependency is the engine stream's own order
    return ZLY_OK;
}
// 3. ... and behind them: a reader on a caller's stream waits for ev_patch (StoreFrames::read_by).  Enqueue gate held.
static int surfaces_end_write(zly_engine* e, Surfaces* sf)
{
    HIP_TRY(hipEventRecord(sf->ev_patch, e->stream), ZLY_ERR_INFERENCE);
    sf->patched = true;
    return ZLY_OK;
}

// Frames that come from the resident store: open() asks for the store, frames() resolves n slots (and regions of them) to views of it, and read_by
// hands them to the body of a call -- body(const FrameSource&, hipStream_t* ran), *ran the stream its last kernel went to -- and tells the store of its
// reader once the body has enqueued.  The store's base, size and patch event leave this object in no other way: a reader cannot forget the note.
class StoreFrames {
    zly_engine* e = nullptr;
    Surfaces* sf = nullptr;
    std::vector<zly_frame_view> views;
public:
    int open(zly_engine* engine) { e = engine; sf = surfaces_of(e); return sf ? ZLY_OK : ZLY_ERR_INVALID_ARGUMENT; }
    int frames(int n, const int32_t* surfaces, const zly_roi* rois = nullptr)
    {
        views.resize((size_t)n);
        return surface_detect_views(sf->store, sf->slots.data(), n, surfaces, rois, views.data(), &g_last_error);
    }
    template <typename Body> int read_by(Body&& body)
    {
        hipStream_t ran = nullptr;
        if (int rc = body(FrameSource{sf->d_store, sf->store.total, views.data(), sf->patched ? sf->ev_patch : nullptr}, &ran)) return rc;
        return surfaces_note_reader(e, sf, ran);
    }
};

// A read-back to host memory: the copies enqueued on the engine's stream behind whatever `behind` enqueues there first (a ring's wait_last, one ring
// event, join_nms; it is handed the engine's stream, the only one a read-back uses), then the stream synchronised.  The gate is held over the
// enqueue only: waiting for the device is not an enqueue section.  Under e->mu.
struct HostCopy { void* dst; const void* src; size_t bytes; };             // bytes = 0: no copy
template <typename Behind> static int read_back(zly_engine* e, Behind&& behind, std::initializer_list<HostCopy> copies)
{
    HIP_TRY(hipSetDevice(e->dev), ZLY_ERR_SYSTEM);
    {
        SharedGate gl;
        if (int rc = behind(e->stream)) return rc;
        for (const HostCopy& c : copies)
            if (c.bytes) HIP_TRY(hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDeviceToHost, e->stream), ZLY_ERR_INFERENCE);
    }
    HIP_TRY(hipStreamSynchronize(e->stream), ZLY_ERR_INFERENCE);
    return ZLY_OK;
}
static int behind_nothing(hipStream_t) { return ZLY_OK; }
static auto behind_ring(const SlotRing& ring)
{
    return [&ring](hipStream_t s) -> int { HIP_TRY(ring.wait_last(s), ZLY_ERR_INFERENCE); return ZLY_OK; };
}

// In front of a host-synchronous call's copy into pinned staging: room for `bytes` -- growth beyond what zly_create staged is an allocation, alone in
// the process --, then the engine's stream drained, because pinned staging is reused call to call.  Waiting for the device is not an enqueue section:
// no gate is held across it (other engines keep enqueuing).  Under e->mu, no gate held.
static int stage_for(zly_engine* e, size_t bytes)
{
    if (bytes > e->stage_bytes) {
        ExclusiveGate x;
        if (int rc = ensure_stage(e, bytes)) return rc;
    }
    HIP_TRY(hipStreamSynchronize(e->stream), ZLY_ERR_INFERENCE);
    return ZLY_OK;
}

// One result slab on the host to the caller's records: the first min(n_kept, max_dets, cap) detections, stamped ts; returns n_kept
static int unpack_slab(const unsigned char* slab, int cap, int max_dets, uint64_t ts, zly_det* out)
{
    const zly_slab_header* hd = reinterpret_cast<const zly_slab_header*>(slab);
    const zly_det* d = reinterpret_cast<const zly_det*>(hd + 1);
    const int m = std::min(std::min(hd->n_kept, max_dets), cap);
    for (int k = 0; k < m; ++k) { out[k] = d[k]; out[k].timestamp = ts; }
    return hd->n_kept;
}

// Returns the first HIP error met while draining / releasing (the engine is gone either way).
static hipError_t destroy_engine(zly_engine* e)
{
    if (!e) return hipSuccess;
    hipError_t first = hipSuccess;
    auto note = [&](hipError_t r) { if (r != hipSuccess && first == hipSuccess) first = r; };
    note(hipSetDevice(e->dev));
    ingest_destroy(e);                                   // joins the dispatcher / completion threads (they take the gate themselves)
    // drain this engine's streams with no gate held (up to a batch of device time: other engines keep enqueuing) ...
    if (e->stream) note(hipStreamSynchronize(e->stream));
    for (int i = 0; i < 2; ++i) if (e->side[i]) note(hipStreamSynchronize(e->side[i]));
    if (e->nms_stream) note(hipStreamSynchronize(e->nms_stream));
    // ... and release alone in the process: a hipFree / hipGraphExecDestroy from this thread while another engine (a hot reload builds the
    // new engines beside the running ones) has a capture open fails both sides
    ExclusiveGate x;
    for (auto& kv : e->graphs) if (kv.second) note(hipGraphExecDestroy(kv.second));
    for (Buffer& b : e->bufs) if (b.ptr) note(hipFree(b.ptr));
    void* dptrs[] = {e->d_weights, e->d_head, e->d_cand, e->d_cand_alt, e->d_count_alt, e->d_scratch, e->d_count, e->d_slabs, e->d_desc, e->d_stage, e->d_scratch_f32, e->d_area, e->d_area_desc};
    for (void* p : dptrs) if (p) note(hipFree(p));
    if (e->h_desc) note(hipHostFree(e->h_desc));
    if (e->h_stage) note(hipHostFree(e->h_stage));
    if (e->h_slabs) note(hipHostFree(e->h_slabs));
    if (Track* tk = e->track.load()) note(track_free(tk));
    if (e->merge) note(merge_free(e->merge));
    if (e->surf) note(surfaces_free(e->surf));
    if (e->zoom) note(zoom_free(e->zoom));
    if (e->chips) note(chips_free(e->chips));
    if (e->change) note(change_free(e->change));
    if (e->camera) note(camera_free(e->camera));
    for (int i = 0; i < 2; ++i) {
        if (e->ev_fork[i]) hipEventDestroy(e->ev_fork[i]);
        if (e->ev_join[i]) hipEventDestroy(e->ev_join[i]);
        if (e->side[i]) hipStreamDestroy(e->side[i]);
    }
    if (e->ev_head) hipEventDestroy(e->ev_head);
    for (int i = 0; i < 2; ++i) if (e->ev_nms[i]) hipEventDestroy(e->ev_nms[i]);
    note(e->desc_ring.destroy());
    for (int i = 0; i < 4; ++i) if (e->ev_t[i]) hipEventDestroy(e->ev_t[i]);
    for (int i = 0; i < 2; ++i) if (e->ev_call[i]) hipEventDestroy(e->ev_call[i]);
    if (e->nms_stream) hipStreamDestroy(e->nms_stream);
    if (e->stream) hipStreamDestroy(e->stream);
    delete e;
    return first;
}


// ------------------------------------------------------------------------------------------------
// pipelined host-to-host path: zly_submit / zly_poll / zly_wait  (include/zly.h)
//
//   submitting threads --memcpy--> pinned slot k+2      (host cores, in parallel)
//   copy stream        --H2D-----> d_stage of slot k+1  (PCIe, while ...)
//   engine stream      -- path --> slot k               (... the previous batch computes)
//   d2h stream         --D2H-----> pinned slabs of slot k-1, completion thread wakes the waiters
//
// A ring slot goes FREE -> OPEN (accepting frames) -> CLOSED (no more frames; copies may still be in progress) ->
// INFLIGHT (enqueued on the device) -> DONE (results in pinned host memory) -> FREE (every ticket consumed).  Slots are
// used in ring order, so batch b lives in slot b % S and a ticket is (batch << 16 | index in batch).
// ------------------------------------------------------------------------------------------------
enum { SLOT_FREE = 0, SLOT_OPEN, SLOT_CLOSED, SLOT_INFLIGHT, SLOT_DONE };

struct IngestSlot {
    uint8_t* h_stage = nullptr; uint8_t* d_stage = nullptr;
    unsigned char* h_slabs = nullptr; unsigned char* d_slabs = nullptr;
    hipEvent_t ev_h2d = nullptr, ev_done = nullptr, ev_out = nullptr;
    int state = SLOT_FREE;
    uint64_t batch = 0;
    int n_reserved = 0, n_committed = 0, n_consumed = 0;
    size_t bytes_used = 0;
    std::vector<int32_t> w, h, fmt;
    std::vector<int32_t> trk;            // the frames' stream indices (zly_submit_view_tracked), -1 = untracked
    int n_trk = 0;                       // frames of the batch with a stream
    std::vector<size_t> off;
    int level = 0;                       // the batch's format level (ZLY_FRONT_*): the highest of its frames', i.e. which front kernel serves it
    std::vector<uint8_t> consumed;
    int rc = ZLY_OK;
    std::string err;
    uint64_t ts_ms = 0;
};

struct Ingest {
    std::mutex mu;
    std::condition_variable cv_free;     // submitters waiting for a slot to open
    std::condition_variable cv_disp;     // dispatcher: frames arrived / copies finished / a batch completed
    std::condition_variable cv_comp;     // completion thread: a batch went in flight
    std::condition_variable cv_done;     // waiters: a batch completed
    std::vector<IngestSlot> slots;
    size_t slot_bytes = 0;
    int open = -1;                       // slot accepting frames, -1 = none
    uint64_t next_batch = 0;             // batch number the next opened slot gets (slot = batch % S)
    std::deque<int> closed, inflight;
    int depth = 2;                       // batches enqueued on the device at once
    bool stop = false;
    std::thread dispatcher, completer;
    hipStream_t copy_stream = nullptr, d2h_stream = nullptr;
    bool use_d2h_stream = false;
};

// One H2D and one D2H stream per device, shared by every engine of the process: each HIP stream beyond the hardware-queue limit (4 by default)
// shares a hardware queue with another stream and the two serialise -- an upload stream of engine B landing on the queue of engine A's
// compute stream stalled A for a whole 33 MB transfer.  Uploads of different engines share the PCIe link anyway.
static hipStream_t g_h2d_stream[16] = {}, g_d2h_stream[16] = {};

// under ing->mu: make the next ring slot the open one if it is free
static bool ingest_try_open(zly_engine* e, Ingest* g)
{
    IngestSlot& sl = g->slots[(size_t)(g->next_batch % g->slots.size())];
    if (sl.state != SLOT_FREE) return false;
    sl.state = SLOT_OPEN; sl.batch = g->next_batch++;
    sl.n_reserved = sl.n_committed = sl.n_consumed = 0; sl.bytes_used = 0; sl.level = 0; sl.n_trk = 0; sl.rc = ZLY_OK; sl.err.clear();
    std::fill(sl.consumed.begin(), sl.consumed.end(), (uint8_t)0);
    g->open = (int)(sl.batch % g->slots.size());
    (void)e;
    return true;
}

static void ingest_close_open(Ingest* g)
{
    if (g->open < 0) return;
    g->slots[(size_t)g->open].state = SLOT_CLOSED;
    g->closed.push_back(g->open);
    g->open = -1;
}

// enqueue one closed, fully copied batch: H2D on the copy stream, the path on the engine's stream, slabs back on the d2h stream
static void ingest_enqueue(zly_engine* e, Ingest* g, IngestSlot& sl)
{
    std::lock_guard<std::mutex> lk(e->mu);
    SharedGate gl;
    const int n = sl.n_reserved;
    hipStream_t out_stream = e->stream;
    auto body = [&]() -> int {
        HIP_TRY(hipSetDevice(e->dev), ZLY_ERR_SYSTEM);
        HIP_TRY(hipMemcpyAsync(sl.d_stage, sl.h_stage, sl.bytes_used, hipMemcpyHostToDevice, g->copy_stream), ZLY_ERR_INFERENCE);
        HIP_TRY(hipEventRecord(sl.ev_h2d, g->copy_stream), ZLY_ERR_INFERENCE);
        HIP_TRY(hipStreamWaitEvent(e->stream, sl.ev_h2d, 0), ZLY_ERR_INFERENCE);
        int rc = set_desc(e, n, sl.w.data(), sl.h.data(), sl.off.data(), e->stream, sl.fmt.data());
        if (rc != ZLY_OK) return rc;
        hipStream_t ns = e->stream;
        e->ingest_active = true;
        rc = run_path(e, n, sl.d_stage, sl.d_slabs, (uint32_t)(sl.batch << 16), e->stream, true, (e->cfg.flags & ZLY_FLAG_ASYNC_NMS) != 0, &ns, front_of(e, sl.level));
        e->ingest_active = false;
        if (rc != ZLY_OK) return rc;
        // the tracker, right behind the batch's NMS on the stream that ran it; the candidate-buffer event of a deferred NMS moves behind it, so that whatever
        // is ordered behind this batch's NMS (a later batch's NMS into these slabs, a join) is ordered behind its tracking too
        Track* tk = e->track.load();
        if (tk && sl.n_trk > 0) {
            bool launched = false;
            rc = track_enqueue(e, tk, n, sl.trk.data(), sl.d_slabs, ns, &launched);
            if (rc != ZLY_OK) return rc;
            if (launched && ns != e->stream && e->last_async >= 0) HIP_TRY(hipEventRecord(e->ev_nms[e->last_async], ns), ZLY_ERR_INFERENCE);
        }
        // the slabs (n x 2.6 KB) go back on the stream the NMS ran on, right behind it: a download stream of its own would be the fifth
        // stream of a three-engine process and share a hardware queue with a compute stream (ZLY_D2H_STREAM=1 restores it)
        out_stream = g->use_d2h_stream ? g->d2h_stream : ns;
        if (g->use_d2h_stream) {
            HIP_TRY(hipEventRecord(sl.ev_done, ns), ZLY_ERR_INFERENCE);
            HIP_TRY(hipStreamWaitEvent(g->d2h_stream, sl.ev_done, 0), ZLY_ERR_INFERENCE);
        }
        HIP_TRY(hipMemcpyAsync(sl.h_slabs, sl.d_slabs, slab_bytes_of(e) * (size_t)n, hipMemcpyDeviceToHost, out_stream), ZLY_ERR_INFERENCE);
        return ZLY_OK;
    };
    sl.rc = body();
    if (sl.rc != ZLY_OK) sl.err = g_last_error;
    hipEventRecord(sl.ev_out, out_stream);             // also on failure: the completion thread must never wait forever
}

static void ingest_dispatch_loop(zly_engine* e, Ingest* g)
{
    hipSetDevice(e->dev);
    std::unique_lock<std::mutex> lk(g->mu);
    while (true) {
        // work = a closed batch, or frames in the open batch while the device has room (no batching window: a lone frame goes at once)
        g->cv_disp.wait(lk, [&] {
            if (g->stop) return true;
            if ((int)g->inflight.size() >= g->depth) return false;
            if (!g->closed.empty()) return g->slots[(size_t)g->closed.front()].n_committed == g->slots[(size_t)g->closed.front()].n_reserved;
            return g->open >= 0 && g->slots[(size_t)g->open].n_reserved > 0;
        });
        if (g->stop) return;
        if (g->closed.empty()) {
            ingest_close_open(g);
            ingest_try_open(e, g);
            g->cv_free.notify_all();
            continue;                                  // re-evaluate: its copies may still be running
        }
        const int si = g->closed.front();
        g->closed.pop_front();
        IngestSlot& sl = g->slots[(size_t)si];
        lk.unlock();
        ingest_enqueue(e, g, sl);
        lk.lock();
        sl.state = SLOT_INFLIGHT;
        g->inflight.push_back(si);
        g->cv_comp.notify_one();
    }
}

static void ingest_complete_loop(zly_engine* e, Ingest* g)
{
    hipSetDevice(e->dev);
    std::unique_lock<std::mutex> lk(g->mu);
    while (true) {
        g->cv_comp.wait(lk, [&] { return g->stop || !g->inflight.empty(); });
        if (g->inflight.empty()) { if (g->stop) return; continue; }
        const int si = g->inflight.front();
        IngestSlot& sl = g->slots[(size_t)si];
        lk.unlock();
        const hipError_t r = hipEventSynchronize(sl.ev_out);
        const uint64_t ts = now_ms();                                       // onnx_engine.cpp:813-815
        lk.lock();
        if (r != hipSuccess && sl.rc == ZLY_OK) { sl.rc = ZLY_ERR_INFERENCE; sl.err = std::string("hipEventSynchronize: ") + hipGetErrorString(r); }
        sl.ts_ms = ts;
        sl.state = SLOT_DONE;
        g->inflight.pop_front();
        const int n = sl.n_reserved;
        const bool ok = sl.rc == ZLY_OK;
        with_stats(e, [&](zly_stats& st) { if (ok) st.inference_count += (uint64_t)n; else st.inference_errors += (uint64_t)n; });
        g->cv_done.notify_all();
        g->cv_disp.notify_one();
    }
}

static void ingest_free(zly_engine* e, Ingest* g);

// first zly_submit: allocate the ring and start the two engine-owned threads (under e->mu)
static int ingest_start(zly_engine* e)
{
    std::lock_guard<std::mutex> lk(e->mu);
    ExclusiveGate gl;                                  // allocations: alone in the process (another engine may otherwise have a capture open)
    if (e->ingest.load()) return ZLY_OK;
    HIP_TRY(hipSetDevice(e->dev), ZLY_ERR_SYSTEM);
    Ingest* g = new Ingest();
    // six slots (round 4; four before): two batches on the device, one filling, and three whose results wait for their consumer.  A host that delivers results
    // in submission order across several engines (the plugin) consumes an engine's finished batch only when the other engines' earlier frames are back as
    // well; with four slots that wait reached the submitters as back-pressure (plugin 78 - 91 k frames/s from run to run; six: 93 k beside the C ABI's 96 k)
    const int S = std::max(3, std::min(16, e->sw.stage_slots));
    const size_t frame = (size_t)e->cfg.model_w * e->cfg.model_h * 3;
    size_t bytes = (size_t)((double)e->cfg.max_batch * (double)frame * 1.25);
    if (bytes < (8u << 20)) bytes = 8u << 20;
    if (e->sw.stage_mb > 0) bytes = (size_t)e->sw.stage_mb << 20;
    g->slot_bytes = (bytes + 4095) / 4096 * 4096;
    g->depth = std::max(1, std::min(S - 2, e->sw.inflight));
    g->slots.resize((size_t)S);
    const int dv = e->dev & 15;
    g->use_d2h_stream = e->sw.d2h_stream;
    bool ok = (g_h2d_stream[dv] || hipStreamCreateWithFlags(&g_h2d_stream[dv], hipStreamNonBlocking) == hipSuccess) &&
              (!g->use_d2h_stream || g_d2h_stream[dv] || hipStreamCreateWithFlags(&g_d2h_stream[dv], hipStreamNonBlocking) == hipSuccess);
    g->copy_stream = g_h2d_stream[dv]; g->d2h_stream = g_d2h_stream[dv];
    const size_t sb = slab_bytes_of(e) * (size_t)e->cfg.max_batch;
    for (IngestSlot& sl : g->slots) {
        ok = ok && hipHostMalloc((void**)&sl.h_stage, g->slot_bytes, hipHostMallocDefault) == hipSuccess &&
             hipMalloc((void**)&sl.d_stage, g->slot_bytes) == hipSuccess &&
             hipHostMalloc((void**)&sl.h_slabs, sb, hipHostMallocDefault) == hipSuccess && hipMalloc((void**)&sl.d_slabs, sb) == hipSuccess &&
             hipEventCreateWithFlags(&sl.ev_h2d, hipEventDisableTiming) == hipSuccess &&
             hipEventCreateWithFlags(&sl.ev_done, hipEventDisableTiming) == hipSuccess &&
             hipEventCreateWithFlags(&sl.ev_out, hipEventDisableTiming) == hipSuccess;
        if (ok) hipMemset(sl.d_slabs, 0, sb);
        sl.w.resize((size_t)e->cfg.max_batch); sl.h.resize((size_t)e->cfg.max_batch); sl.fmt.resize((size_t)e->cfg.max_batch); sl.off.resize((size_t)e->cfg.max_batch);
        sl.trk.assign((size_t)e->cfg.max_batch, -1);
        sl.consumed.resize((size_t)e->cfg.max_batch);
    }
    if (!ok) { ingest_free(e, g); return fail(ZLY_ERR_SYSTEM, "allocation of the staging ring failed"); }
    g->dispatcher = std::thread(ingest_dispatch_loop, e, g);
    g->completer = std::thread(ingest_complete_loop, e, g);
    e->ingest.store(g);
    return ZLY_OK;
}

static void ingest_destroy(zly_engine* e)
{
    Ingest* g = e->ingest.load();
    if (!g) return;
    {
        std::lock_guard<std::mutex> lk(g->mu);
        g->stop = true;
    }
    g->cv_disp.notify_all(); g->cv_comp.notify_all(); g->cv_free.notify_all(); g->cv_done.notify_all();
    if (g->dispatcher.joinable()) g->dispatcher.join();
    if (g->completer.joinable()) g->completer.join();
    e->ingest.store(nullptr);
    if (g->copy_stream) hipStreamSynchronize(g->copy_stream);
    if (e->stream) hipStreamSynchronize(e->stream);
    if (e->nms_stream) hipStreamSynchronize(e->nms_stream);
    if (g->d2h_stream) hipStreamSynchronize(g->d2h_stream);
    ExclusiveGate x;                                   // releases: alone in the process
    ingest_free(e, g);
}

// caller holds the exclusive gate and has drained the streams
static void ingest_free(zly_engine* e, Ingest* g)
{
    (void)e;
    for (IngestSlot& sl : g->slots) {
        if (sl.h_stage) hipHostFree(sl.h_stage);
        if (sl.d_stage) hipFree(sl.d_stage);
        if (sl.h_slabs) hipHostFree(sl.h_slabs);
        if (sl.d_slabs) hipFree(sl.d_slabs);
        if (sl.ev_h2d) hipEventDestroy(sl.ev_h2d);
        if (sl.ev_done) hipEventDestroy(sl.ev_done);
        if (sl.ev_out) hipEventDestroy(sl.ev_out);
    }
    delete g;                                          // the copy streams are shared by the process and stay
}

// view: the request is a frame view of the buffer bgr[0 .. nbytes) (zly_submit_view): the region's rows are copied into a tight frame of the ring, and
// from there on the request is that frame
// track_stream: the frame's stream index (validated by the caller), -1 = untracked; it rides with the frame through the ring
static int ingest_submit(zly_engine* e, const uint8_t* bgr, size_t nbytes, int32_t w, int32_t h, uint64_t* ticket, bool nonblock = false,
                         int32_t fmt = ZLY_PIX_BGR, const zly_frame_view* view = nullptr, int32_t track_stream = -1)
{
    int rcv;
    if (view) {
        rcv = check_view(e->cfg.flags, bgr, nbytes, view, &g_last_error);
        if (rcv == ZLY_OK) { fmt = view->fmt; w = view->w; h = view->h; nbytes = zly_frame_bytes(fmt, w, h); }
    } else {
        rcv = check_frame(fmt, bgr, nbytes, w, h, &g_last_error);
        if (rcv == ZLY_OK) rcv = check_frame_mode(e->cfg.flags, w, h, &g_last_error);
    }
    if (rcv != ZLY_OK) {
        with_stats(e, [](zly_stats& st) { st.inference_errors++; });
        return rcv;
    }
    if (!e->ingest.load()) {
        int rc = ingest_start(e);
        if (rc != ZLY_OK) return rc;
    }
    Ingest* g = e->ingest.load();
    const size_t padded = (nbytes + 15) / 16 * 16;
    if (padded > g->slot_bytes)
        return fail(ZLY_ERR_INVALID_INPUT, "frame of " + std::to_string(nbytes) + " bytes does not fit a staging slot of " + std::to_string(g->slot_bytes) + " bytes (ZLY_STAGE_MB)");
    IngestSlot* sl = nullptr;
    int idx = 0;
    size_t off = 0;
    {
        std::unique_lock<std::mutex> lk(g->mu);
        while (true) {
            if (g->stop) return fail(ZLY_ERR_NOT_INITIALIZED, "Engine not running");
            if (g->open < 0 && !ingest_try_open(e, g)) {                                       // every ring slot is busy: back-pressure
                if (nonblock) return ZLY_PENDING;                                                // zly_submit_try: the caller offers the frame elsewhere
                g->cv_free.wait(lk);
                continue;
            }
            IngestSlot& o = g->slots[(size_t)g->open];
            if (o.n_reserved >= e->cfg.max_batch || o.bytes_used + padded > g->slot_bytes) {   // full: the dispatcher takes it from here
                ingest_close_open(g);
                g->cv_disp.notify_one();
                continue;
            }
            sl = &o;
            idx = o.n_reserved++;
            off = o.bytes_used;
            o.bytes_used += padded;
            o.w[(size_t)idx] = w; o.h[(size_t)idx] = h; o.fmt[(size_t)idx] = fmt; o.off[(size_t)idx] = off;
            o.trk[(size_t)idx] = track_stream;
            if (track_stream >= 0) o.n_trk++;
            o.level = std::max(o.level, front_level(fmt));
            *ticket = (o.batch << 16) | (uint64_t)idx;
            if (o.n_reserved == e->cfg.max_batch) ingest_close_open(g);
            break;
        }
    }
    if (view) copy_view_tight(sl->h_stage + off, bgr, view);
    else memcpy(sl->h_stage + off, bgr, nbytes);          // the one host copy of the request, on the caller's thread
    {
        std::lock_guard<std::mutex> lk(g->mu);
        sl->n_committed++;
    }
    g->cv_disp.notify_one();
    return ZLY_OK;
}

// under g->mu: the slot a ticket lives in, or null
static IngestSlot* ingest_slot_of(Ingest* g, uint64_t ticket, int* idx)
{
    const uint64_t batch = ticket >> 16;
    *idx = (int)(ticket & 0xffffu);
    IngestSlot& sl = g->slots[(size_t)(batch % g->slots.size())];
    if (sl.state == SLOT_FREE || sl.batch != batch || *idx >= sl.n_reserved || sl.consumed[(size_t)*idx]) return nullptr;   // consumed: 1 = done, 2 = claimed by a waiter
    return &sl;
}

static int ingest_poll(zly_engine* e, uint64_t ticket)
{
    Ingest* g = e->ingest.load();
    if (!g) return fail(ZLY_ERR_INVALID_ARGUMENT, "unknown ticket");
    std::lock_guard<std::mutex> lk(g->mu);
    int idx = 0;
    IngestSlot* sl = ingest_slot_of(g, ticket, &idx);
    if (!sl) return fail(ZLY_ERR_INVALID_ARGUMENT, "unknown or already consumed ticket");
    return sl->state == SLOT_DONE ? ZLY_OK : ZLY_PENDING;
}

static int ingest_wait(zly_engine* e, uint64_t ticket, zly_det* out, int32_t cap, int32_t* n_out)
{
    Ingest* g = e->ingest.load();
    if (!g) return fail(ZLY_ERR_INVALID_ARGUMENT, "unknown ticket");
    std::unique_lock<std::mutex> lk(g->mu);
    int idx = 0;
    IngestSlot* sl = ingest_slot_of(g, ticket, &idx);
    if (!sl) return fail(ZLY_ERR_INVALID_ARGUMENT, "unknown or already consumed ticket");
    // the ticket is CLAIMED before the wait: a second zly_wait on it (concurrent, or entered before this one finishes) fails instead of
    // consuming it twice -- two consumptions freed the ring slot while other tickets of the batch were still unread
    sl->consumed[(size_t)idx] = 2;
    g->cv_done.wait(lk, [&] { return g->stop || sl->state == SLOT_DONE; });
    if (sl->state != SLOT_DONE) { sl->consumed[(size_t)idx] = 0; return fail(ZLY_ERR_NOT_INITIALIZED, "Engine not running"); }
    const int rc = sl->rc;
    std::string err = sl->err;
    const uint64_t ts = sl->ts_ms;
    lk.unlock();
    int kept = 0;
    if (rc == ZLY_OK)                                      // the slot cannot be recycled before this ticket is consumed below
        kept = unpack_slab(sl->h_slabs + slab_bytes_of(e) * (size_t)idx, cap, e->cfg.max_dets, ts, out);
    lk.lock();
    sl->consumed[(size_t)idx] = 1;
    if (++sl->n_consumed == sl->n_reserved) {
        sl->state = SLOT_FREE;
        g->cv_free.notify_all();
        g->cv_disp.notify_one();
    }
    lk.unlock();
    if (rc != ZLY_OK) return fail(rc, err);
    *n_out = kept;
    return ZLY_OK;
}

}  // namespace zly

// ================================================================================================
// C ABI
// ================================================================================================
extern "C" {

const char* zly_last_error(void) { return g_last_error.c_str(); }
const char* zly_version(void) { return "zly-hip 0.2 (gfx950)"; }

void zly_default_config(zly_config* c)
{
    memset(c, 0, sizeof *c);
    c->weights_path = nullptr;
    c->model_w = 416; c->model_h = 416;          // configs/server.json:30-31
    c->conf_thr = 0.5f; c->iou_thr = 0.45f;      // configs/server.json:7-8
    c->max_batch = 1; c->max_dets = 64; c->device = 0;
    c->dtype = ZLY_DTYPE_BF16; c->warmup_runs = 3; c->use_graph = 1;
}

// One untimed pass of the device-resident path at batch n on constant-128 frames, through run_path exactly as zly_detect_device and the
// pipelined host path run it (deferred NMS: both candidate-buffer parities): captures the batch-n graph(s) and replays each once, so that
// neither the capture (stream sync + capture + instantiate) nor a graph's first launch falls into a production call -- at start-up or
// after a hot reload.  warmupModel analogue for the throughput path (onnx_engine.cpp:919-954 warms its single-frame path only).
static int warm_batch(zly_engine* e, int n)
{
    std::lock_guard<std::mutex> lk(e->mu);
    const size_t fb = (size_t)e->cfg.model_w * e->cfg.model_h * 3;
    const size_t total = fb * (size_t)n;
    if (total > e->stage_bytes) {
        ExclusiveGate x;
        int rc = ensure_stage(e, total);
        if (rc != ZLY_OK) return rc;
    }
    SharedGate gl;
    HIP_TRY(hipMemsetAsync(e->d_stage, 128, total, e->stream), ZLY_ERR_INFERENCE);
    std::vector<int32_t> ws((size_t)n, e->cfg.model_w), hs((size_t)n, e->cfg.model_h);
    std::vector<size_t> offs((size_t)n);
    for (int i = 0; i < n; ++i) offs[(size_t)i] = (size_t)i * fb;
    int rc = set_desc(e, n, ws.data(), hs.data(), offs.data(), e->stream);
    if (rc != ZLY_OK) return rc;
    const bool defer = (e->cfg.flags & ZLY_FLAG_ASYNC_NMS) != 0;
    for (int k = 0; k < (defer ? 4 : 2); ++k) {
        rc = run_path(e, n, e->d_stage, nullptr, 0, e->stream, true, defer, nullptr, front_of(e, ZLY_FRONT_BGR));
        if (rc != ZLY_OK) return rc;
    }
    gl.release();
    HIP_TRY(hipStreamSynchronize(e->stream), ZLY_ERR_INFERENCE);
    if (e->nms_stream) HIP_TRY(hipStreamSynchronize(e->nms_stream), ZLY_ERR_INFERENCE);
    return ZLY_OK;
}

int32_t zly_create(const zly_config* cfg, zly_engine** out)
{
    if (!cfg || !out) return fail(ZLY_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    if (cfg->model_w <= 0 || cfg->model_h <= 0 || cfg->model_w % 32 || cfg->model_h % 32)
        return fail(ZLY_ERR_INVALID_ARGUMENT, "model_w/model_h must be positive multiples of 32");
    if (cfg->max_batch < 1 || cfg->max_dets < 1) return fail(ZLY_ERR_INVALID_ARGUMENT, "max_batch/max_dets must be >= 1");
    if (cfg->max_batch > 65535) return fail(ZLY_ERR_INVALID_ARGUMENT, "max_batch must be <= 65535 (a ticket of the pipelined path carries the frame's index in 16 bits)");
    if (cfg->dtype != ZLY_DTYPE_BF16 && cfg->dtype != ZLY_DTYPE_FP32) return fail(ZLY_ERR_INVALID_ARGUMENT, "dtype must be ZLY_DTYPE_FP32 or ZLY_DTYPE_BF16");
    if ((cfg->flags & ZLY_FLAG_LETTERBOX) && (cfg->model_w > ZLY_LETTERBOX_MAX_DIM || cfg->model_h > ZLY_LETTERBOX_MAX_DIM))
        return fail(ZLY_ERR_INVALID_ARGUMENT, "ZLY_FLAG_LETTERBOX: model_w/model_h must be <= " + std::to_string(ZLY_LETTERBOX_MAX_DIM));
    if ((cfg->flags & ZLY_FLAG_AREA) && (cfg->model_w > ZLY_AREA_MAX_DIM || cfg->model_h > ZLY_AREA_MAX_DIM))
        return fail(ZLY_ERR_INVALID_ARGUMENT, "ZLY_FLAG_AREA: model_w/model_h must be <= " + std::to_string(ZLY_AREA_MAX_DIM));
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(ZLY_ERR_SYSTEM, "no HIP device available: this engine has no CPU fallback");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(ZLY_ERR_INVALID_ARGUMENT, "device ordinal out of range");

    zly_engine* e = new zly_engine();
    e->cfg = *cfg;
    e->weights_path = cfg->weights_path ? cfg->weights_path : "";
    e->cfg.weights_path = nullptr;
    e->dev = cfg->device;
    e->dtype = cfg->dtype;
    e->esz = cfg->dtype == ZLY_DTYPE_BF16 ? 2 : 4;
    read_switches(&e->sw);
    std::string err;
    int rc = load_zlyw(e->weights_path.c_str(), &e->model, &err);        // host only: file parse
    if (rc != ZLY_OK) { delete e; return fail(rc, err); }
    rc = build_plan(e->model, e->cfg, e->dtype, e->sw, e, &err);         // host only: op list + weight repack, outside the gate
    if (rc != ZLY_OK) { delete e; return fail(rc, err); }

    // Everything that allocates on / uploads to the device runs alone in the process (ExclusiveGate): a hot reload builds new engines beside
    // running ones, and a hipMalloc / hipMemcpy here while one of them had a stream capture open failed both sides.
    auto device_setup = [&]() -> int {
        HIP_TRY(hipSetDevice(cfg->device), ZLY_ERR_SYSTEM);
        HIP_TRY(conv_init(), ZLY_ERR_SYSTEM);
        HIP_TRY(pair_init(), ZLY_ERR_SYSTEM);
        HIP_TRY(stem1_init(), ZLY_ERR_SYSTEM);
        HIP_TRY(c2f_init(), ZLY_ERR_SYSTEM);
        HIP_TRY(sppf_init(), ZLY_ERR_SYSTEM);
        HIP_TRY(nms_init(), ZLY_ERR_SYSTEM);
        // ZLY_CU_PART="i/n": this engine's streams only use the i-th of n equal slices of the chip's compute units (spatial
        // partitioning: several engines run side by side, the launch-latency-bound small-map layers of one beside the
        // bandwidth-bound layers of another).  Experiment switch: see DESIGN.md section 5.
        e->cu_part_n = e->sw.cu_part_n;
        if (e->cu_part_n > 1)
            for (int b = e->sw.cu_part_i * e->sw.num_cus; b < (e->sw.cu_part_i + 1) * e->sw.num_cus; ++b) e->cu_mask[b / 32] |= 1u << (b % 32);
        auto make_stream = [&](hipStream_t* st) {
            if (e->cu_part_n > 1) return hipExtStreamCreateWithCUMask(st, 8, e->cu_mask) == hipSuccess;
            return hipStreamCreateWithFlags(st, hipStreamNonBlocking) == hipSuccess;
        };
        bool sok = make_stream(&e->stream);
        // side streams only when the Detect-branch lanes can be used: every stream beyond the hardware-queue limit shares a hardware queue
        // with another one, and two streams on one queue serialise -- several engines per GPU want few streams each
        const bool want_lanes = !(cfg->flags & ZLY_FLAG_SINGLE_CHAIN) && !e->sw.no_lanes;
        for (int i = 0; i < 2 && sok && want_lanes; ++i) {
            sok = make_stream(&e->side[i]) &&
                  hipEventCreateWithFlags(&e->ev_fork[i], hipEventDisableTiming) == hipSuccess &&
                  hipEventCreateWithFlags(&e->ev_join[i], hipEventDisableTiming) == hipSuccess;
        }
        if (!sok) return fail(ZLY_ERR_SYSTEM, "hipStreamCreate failed");
        int prc = upload_plan(e, &err);
        if (prc != ZLY_OK) return fail(prc, err);

        const size_t B = (size_t)cfg->max_batch, N = (size_t)e->N;
        bool ok = true;
        ok = ok && hipMalloc((void**)&e->d_head, ((cfg->flags & ZLY_FLAG_NO_HEAD_TENSOR) ? 1 : B) * (4 + (size_t)e->nc) * N * sizeof(float)) == hipSuccess;
        ok = ok && hipMalloc((void**)&e->d_cand, B * N * sizeof(Cand)) == hipSuccess;
        ok = ok && hipMalloc((void**)&e->d_scratch, B * N * sizeof(Cand)) == hipSuccess;
        ok = ok && hipMalloc((void**)&e->d_count, B * sizeof(int)) == hipSuccess;
        ok = ok && hipMalloc((void**)&e->d_slabs, B * slab_bytes_of(e)) == hipSuccess;
        ok = ok && hipMalloc((void**)&e->d_desc, B * zly_engine::DESC_SLOT) == hipSuccess;
        ok = ok && hipHostMalloc((void**)&e->h_desc, SlotRing::DEPTH * B * zly_engine::DESC_SLOT, hipHostMallocDefault) == hipSuccess;
        ok = ok && e->desc_ring.create() == hipSuccess;
        for (int i = 0; i < 4 && ok; ++i) ok = hipEventCreate(&e->ev_t[i]) == hipSuccess;
        for (int i = 0; i < 2 && ok; ++i) ok = hipEventCreateWithFlags(&e->ev_call[i], hipEventDisableTiming) == hipSuccess;
        ok = ok && hipHostMalloc((void**)&e->h_slabs, B * slab_bytes_of(e), hipHostMallocDefault) == hipSuccess;
        if (!ok) return fail(ZLY_ERR_SYSTEM, "device allocation failed");
        ok = hipMemset(e->d_slabs, 0, B * slab_bytes_of(e)) == hipSuccess && hipMemset(e->d_count, 0, B * sizeof(int)) == hipSuccess;
        e->cur_cand = e->d_cand; e->cur_count = e->d_count;
        if (ok && (cfg->flags & ZLY_FLAG_ASYNC_NMS)) {
            ok = hipMalloc((void**)&e->d_cand_alt, B * N * sizeof(Cand)) == hipSuccess && hipMalloc((void**)&e->d_count_alt, B * sizeof(int)) == hipSuccess &&
                 make_stream(&e->nms_stream) &&
                 hipEventCreateWithFlags(&e->ev_head, hipEventDisableTiming) == hipSuccess &&
                 hipEventCreateWithFlags(&e->ev_nms[0], hipEventDisableTiming) == hipSuccess &&
                 hipEventCreateWithFlags(&e->ev_nms[1], hipEventDisableTiming) == hipSuccess &&
                 hipMemset(e->d_count_alt, 0, B * sizeof(int)) == hipSuccess;
            if (!ok) return fail(ZLY_ERR_SYSTEM, "device allocation failed (deferred NMS)");
        }
        if (!ok) return fail(ZLY_ERR_SYSTEM, "device initialisation failed");
        if (cfg->flags & ZLY_FLAG_AREA) {
            const size_t afb = (size_t)cfg->model_w * cfg->model_h * 3;
            std::vector<FrameDesc> ad(B);
            for (size_t i = 0; i < B; ++i) { ad[i].src_off = desc_pack(i * afb, ZLY_PIX_BGR); ad[i].w = cfg->model_w; ad[i].h = cfg->model_h; }
            ok = hipMalloc((void**)&e->d_area, B * afb) == hipSuccess && hipMalloc((void**)&e->d_area_desc, B * sizeof(FrameDesc)) == hipSuccess &&
                 hipMemcpy(e->d_area_desc, ad.data(), B * sizeof(FrameDesc), hipMemcpyHostToDevice) == hipSuccess;
            if (!ok) return fail(ZLY_ERR_SYSTEM, "device allocation failed (area resize)");
        }
        // staging for one frame (zly_detect) -- or, with a warm-up, for max_batch model-sized frames (warm_batch; zly_detect_batch then never allocates)
        const size_t fb = (size_t)cfg->model_w * cfg->model_h * 3;
        return ensure_stage(e, cfg->warmup_runs > 0 ? fb * B : fb);
    };
    {
        ExclusiveGate x;
        rc = device_setup();
    }
    if (rc != ZLY_OK) { std::string m = g_last_error; destroy_engine(e); return fail(rc, m); }

    // warmupModel analogue (onnx_engine.cpp:919-954): constant-128 frames of model size through the single-frame path, then the
    // throughput path at max_batch.  Both go through the normal entry points' machinery (gate, capture, replay).
    if (cfg->warmup_runs > 0) {
        const size_t fb = (size_t)cfg->model_w * cfg->model_h * 3;
        std::vector<uint8_t> grey(fb, 128);
        std::vector<zly_det> dets((size_t)cfg->max_dets);
        for (int i = 0; i < cfg->warmup_runs && rc == ZLY_OK; ++i) {
            int32_t nd = 0;
            rc = zly_detect(e, grey.data(), fb, cfg->model_w, cfg->model_h, dets.data(), cfg->max_dets, &nd);
        }
        if (rc == ZLY_OK && cfg->max_batch > 1) rc = warm_batch(e, cfg->max_batch);
        if (rc != ZLY_OK) { std::string m = g_last_error; destroy_engine(e); return fail(rc, "warm-up failed: " + m); }
        with_stats(e, [](zly_stats& st) { st = zly_stats{}; });
        e->sample_ctr = 0; e->t_pending = false;
    }
    *out = e;
    return ZLY_OK;
}

int32_t zly_destroy(zly_engine* e)
{
    if (!e) return ZLY_OK;
    const hipError_t r = destroy_engine(e);
    if (r != hipSuccess) return fail(ZLY_ERR_SYSTEM, std::string("zly_destroy: ") + hipGetErrorString(r));
    return ZLY_OK;
}

// fmt: per-frame ZLY_PIX_* (null = all BGR)
// views: per-frame views of the buffers bgr[i][0 .. nbytes[i]) (zly_detect[_batch]_view; w, h, fmt are then the views'): the staging copy takes the
// regions' rows only, as tight frames, and everything behind it is the path of those frames
static int detect_host_locked(zly_engine* e, int32_t n, const uint8_t* const* bgr, const size_t* nbytes,
                              const int32_t* w, const int32_t* h, zly_det* out, int32_t cap, int32_t* n_out, const int32_t* fmt = nullptr,
                              const zly_frame_view* views = nullptr)
{
    HIP_TRY(hipSetDevice(e->dev), ZLY_ERR_SYSTEM);
    std::vector<size_t> offs((size_t)n);
    std::vector<int32_t> vw, vh, vf;
    if (views) { vw.resize((size_t)n); vh.resize((size_t)n); vf.resize((size_t)n); }
    size_t total = 0;
    int level = ZLY_FRONT_BGR;
    for (int i = 0; i < n; ++i) {
        int rcv;
        if (views) {
            rcv = check_view(e->cfg.flags, bgr[i], nbytes[i], &views[i], &g_last_error);
            vw[(size_t)i] = views[i].w; vh[(size_t)i] = views[i].h; vf[(size_t)i] = views[i].fmt;
        } else {
            rcv = check_frame(fmt ? fmt[i] : ZLY_PIX_BGR, bgr[i], nbytes[i], w[i], h[i], &g_last_error);
            if (rcv == ZLY_OK) rcv = check_frame_mode(e->cfg.flags, w[i], h[i], &g_last_error);
        }
        if (rcv != ZLY_OK) {
            with_stats(e, [](zly_stats& st) { st.inference_errors++; });
            return rcv;
        }
        const int32_t fi = views ? views[i].fmt : fmt ? fmt[i] : ZLY_PIX_BGR;
        level = std::max(level, front_level(fi));
        offs[(size_t)i] = total;
        total += ((views ? zly_frame_bytes(fi, views[i].w, views[i].h) : nbytes[i]) + 15) / 16 * 16;
    }
    if (views) { w = vw.data(); h = vh.data(); fmt = vf.data(); }
    int rc = stage_for(e, total);                                        // frames larger than the model input grow the staging
    if (rc != ZLY_OK) return rc;
    for (int i = 0; i < n; ++i) {                                        // the host copy is no enqueue section either: no gate yet
        if (views) copy_view_tight(e->h_stage + offs[(size_t)i], bgr[i], &views[i]);
        else memcpy(e->h_stage + offs[(size_t)i], bgr[i], nbytes[i]);
    }
    SharedGate gl;
    HIP_TRY(hipMemcpyAsync(e->d_stage, e->h_stage, total, hipMemcpyHostToDevice, e->stream), ZLY_ERR_INFERENCE);
    rc = set_desc(e, n, w, h, offs.data(), e->stream, fmt);
    if (rc != ZLY_OK) return rc;
    rc = run_path(e, n, e->d_stage, nullptr, 0, e->stream, true, false, nullptr, front_of(e, level));
    if (rc != ZLY_OK) { with_stats(e, [](zly_stats& st) { st.inference_errors++; }); return rc; }
    const size_t sb = slab_bytes_of(e);
    HIP_TRY(hipMemcpyAsync(e->h_slabs, e->d_slabs, sb * (size_t)n, hipMemcpyDeviceToHost, e->stream), ZLY_ERR_INFERENCE);
    gl.release();                                                        // waiting for the device is not an enqueue section
    HIP_TRY(hipStreamSynchronize(e->stream), ZLY_ERR_INFERENCE);
    const uint64_t ts = now_ms();                                        // onnx_engine.cpp:813-815
    for (int i = 0; i < n; ++i) n_out[i] = unpack_slab(e->h_slabs + sb * (size_t)i, cap, e->cfg.max_dets, ts, out + (size_t)i * cap);
    harvest_timing(e);                                                   // the stream is idle: a sampled call's events are complete
    with_stats(e, [&](zly_stats& st) { st.inference_count += (uint64_t)n; });
    return ZLY_OK;
}

// the host-only entry points: the rules are frame_rules.h's
size_t zly_frame_bytes(int32_t fmt, int32_t w, int32_t h) { return frame_bytes(fmt, w, h); }

size_t zly_view_bytes(const zly_frame_view* v) { return view_bytes(v); }

int32_t zly_view_tight(int32_t fmt, int32_t w, int32_t h, zly_frame_view* out)
{
    if (!out) return fail(ZLY_ERR_INVALID_ARGUMENT, "null output");
    return view_tight(fmt, w, h, out, &g_last_error);
}

int32_t zly_view_crop(const zly_frame_view* surface, int32_t x0, int32_t y0, int32_t w, int32_t h, zly_frame_view* out)
{
    if (!surface || !out) return fail(ZLY_ERR_INVALID_ARGUMENT, "null argument");
    return view_crop(surface, x0, y0, w, h, out, &g_last_error);
}

int32_t zly_letterbox_geometry(int32_t w, int32_t h, int32_t model_w, int32_t model_h, int32_t* nw, int32_t* nh, int32_t* pad_x, int32_t* pad_y)
{
    return letterbox_geometry(w, h, model_w, model_h, nw, nh, pad_x, pad_y, &g_last_error);      // null outputs are refused there, behind the sizes
}

int32_t zly_detect(zly_engine* e, const uint8_t* bgr, size_t nbytes, int32_t w, int32_t h, zly_det* out, int32_t cap, int32_t* n_out)
{
    return zly_detect_fmt(e, ZLY_PIX_BGR, bgr, nbytes, w, h, out, cap, n_out);
}

int32_t zly_detect_fmt(zly_engine* e, int32_t fmt, const uint8_t* bgr, size_t nbytes, int32_t w, int32_t h, zly_det* out, int32_t cap, int32_t* n_out)
{
    if (!e) return fail(ZLY_ERR_NOT_INITIALIZED, "Engine not running");
    if (!out || !n_out || cap < 0) return fail(ZLY_ERR_INVALID_ARGUMENT, "null output");
    std::lock_guard<std::mutex> lk(e->mu);
    const auto t0 = std::chrono::steady_clock::now();
    const uint8_t* ptrs[1] = {bgr};
    int rc = detect_host_locked(e, 1, ptrs, &nbytes, &w, &h, out, cap, n_out, &fmt);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    with_stats(e, [&](zly_stats& st) { st.last_detect_ms = ms; });
    return rc;
}

int32_t zly_detect_batch(zly_engine* e, int32_t n, const uint8_t* const* bgr, const size_t* nbytes,
                         const int32_t* w, const int32_t* h, zly_det* out, int32_t cap, int32_t* n_out)
{
    if (!e) return fail(ZLY_ERR_NOT_INITIALIZED, "Engine not running");
    if (!bgr || !nbytes || !w || !h || !out || !n_out || cap < 0) return fail(ZLY_ERR_INVALID_ARGUMENT, "null argument");
    if (n < 1 || n > e->cfg.max_batch) return fail(ZLY_ERR_INVALID_ARGUMENT, "batch size out of range");
    std::lock_guard<std::mutex> lk(e->mu);
    return detect_host_locked(e, n, bgr, nbytes, w, h, out, cap, n_out);
}

int32_t zly_detect_batch_fmt(zly_engine* e, int32_t n, const int32_t* fmt, const uint8_t* const* frames, const size_t* nbytes,
                             const int32_t* w, const int32_t* h, zly_det* out, int32_t cap, int32_t* n_out)
{
    if (!e) return fail(ZLY_ERR_NOT_INITIALIZED, "Engine not running");
    if (!fmt || !frames || !nbytes || !w || !h || !out || !n_out || cap < 0) return fail(ZLY_ERR_INVALID_ARGUMENT, "null argument");
    if (n < 1 || n > e->cfg.max_batch) return fail(ZLY_ERR_INVALID_ARGUMENT, "batch size out of range");
    std::lock_guard<std::mutex> lk(e->mu);
    return detect_host_locked(e, n, frames, nbytes, w, h, out, cap, n_out, fmt);
}

int32_t zly_detect_view(zly_engine* e, const uint8_t* base, size_t buf_bytes, const zly_frame_view* v, zly_det* out, int32_t cap, int32_t* n_out)
{
    if (!e) return fail(ZLY_ERR_NOT_INITIALIZED, "Engine not running");
    if (!v || !out || !n_out || cap < 0) return fail(ZLY_ERR_INVALID_ARGUMENT, "null argument");
    std::lock_guard<std::mutex> lk(e->mu);
    const auto t0 = std::chrono::steady_clock::now();
    const uint8_t* ptrs[1] = {base};
    int rc = detect_host_locked(e, 1, ptrs, &buf_bytes, nullptr, nullptr, out, cap, n_out, nullptr, v);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    with_stats(e, [&](zly_stats& st) { st.last_detect_ms = ms; });
    return rc;
}

int32_t zly_detect_batch_view(zly_engine* e, int32_t n, const uint8_t* const* base, const size_t* buf_bytes, const zly_frame_view* v,
                              zly_det* out, int32_t cap, int32_t* n_out)
{
    if (!e) return fail(ZLY_ERR_NOT_INITIALIZED, "Engine not running");
    if (!base || !buf_bytes || !v || !out || !n_out || cap < 0) return fail(ZLY_ERR_INVALID_ARGUMENT, "null argument");
    if (n < 1 || n > e->cfg.max_batch) return fail(ZLY_ERR_INVALID_ARGUMENT, "batch size out of range");
    std::lock_guard<std::mutex> lk(e->mu);
    return detect_host_locked(e, n, base, buf_bytes, nullptr, nullptr, out, cap, n_out, nullptr, v);
}

int32_t zly_submit_view(zly_engine* e, const uint8_t* base, size_t buf_bytes, const zly_frame_view* v, uint64_t* ticket)
{
    if (!e) return fail(ZLY_ERR_NOT_INITIALIZED, "Engine not running");
    if (!ticket || !v) return fail(ZLY_ERR_INVALID_ARGUMENT, "null argument");
    return ingest_submit(e, base, buf_bytes, 0, 0, ticket, false, ZLY_PIX_BGR, v);
}

int32_t zly_submit_try_view(zly_engine* e, const uint8_t* base, size_t buf_bytes, const zly_frame_view* v, uint64_t* ticket)
{
    if (!e) return fail(ZLY_ERR_NOT_INITIALIZED, "Engine not running");
    if (!ticket || !v) return fail(ZLY_ERR_INVALID_ARGUMENT, "null argument");
    return ingest_submit(e, base, buf_bytes, 0, 0, ticket, true, ZLY_PIX_BGR, v);
}

int32_t zly_submit(zly_engine* e, const uint8_t* bgr, size_t nbytes, int32_t w, int32_t h, uint64_t* ticket)
{
    return zly_submit_fmt(e, ZLY_PIX_BGR, bgr, nbytes, w, h, ticket);
}

int32_t zly_submit_try(zly_engine* e, const uint8_t* bgr, size_t nbytes, int32_t w, int32_t h, uint64_t* ticket)
{
    return zly_submit_try_fmt(e, ZLY_PIX_BGR, bgr, nbytes, w, h, ticket);
}

int32_t zly_submit_fmt(zly_engine* e, int32_t fmt, const uint8_t* frame, size_t nbytes, int32_t w, int32_t h, uint64_t* ticket)
{
    if (!e) return fail(ZLY_ERR_NOT_INITIALIZED, "Engine not running");
    if (!ticket) return fail(ZLY_ERR_INVALID_ARGUMENT, "null ticket");
    return ingest_submit(e, frame, nbytes, w, h, ticket, false, fmt);
}

int32_t zly_submit_try_fmt(zly_engine* e, int32_t fmt, const uint8_t* frame, size_t nbytes, int32_t w, int32_t h, uint64_t* ticket)
{
    if (!e) return fail(ZLY_ERR_NOT_INITIALIZED, "Engine not running");
    if (!ticket) return fail(ZLY_ERR_INVALID_ARGUMENT, "null ticket");
    return ingest_submit(e, frame, nbytes, w, h, ticket, true, fmt);
}

int32_t zly_poll(zly_engine* e, uint64_t ticket)
{
    if (!e) return fail(ZLY_ERR_NOT_INITIALIZED, "Engine not running");
    return ingest_poll(e, ticket);
}

int32_t zly_wait(zly_engine* e, uint64_t ticket, zly_det* out, int32_t cap, int32_t* n_out)
{
    if (!e) return fail(ZLY_ERR_NOT_INITIALIZED, "Engine not running");
    if (!out || !n_out || cap < 0) return fail(ZLY_ERR_INVALID_ARGUMENT, "null output");
    return ingest_wait(e, ticket, out, cap, n_out);
}

int32_t zly_detect_device(zly_engine* e, int32_t n, const void* d_frames, int32_t w, int32_t h, void* d_slabs, uint32_t frame_tag0, void* stream)
{
    return zly_detect_device_fmt(e, ZLY_PIX_BGR, n, d_frames, w, h, d_slabs, frame_tag0, stream);
}

int32_t zly_detect_device_fmt(zly_engine* e, int32_t fmt, int32_t n, const void* d_frames, int32_t w, int32_t h, void* d_slabs, uint32_t frame_tag0, void* stream)
{
    if (!e) return fail(ZLY_ERR_NOT_INITIALIZED, "Engine not running");
    if (!pix_format(fmt)) return fail(ZLY_ERR_INVALID_ARGUMENT, "unknown pixel format " + std::to_string(fmt));
    const size_t fb = zly_frame_bytes(fmt, w, h);
    if (!d_frames || w <= 0 || h <= 0 || fb == 0) return fail(ZLY_ERR_INVALID_INPUT, "bad frame pointer or size");
    if (n < 1 || n > e->cfg.max_batch) return fail(ZLY_ERR_INVALID_ARGUMENT, "batch size out of range");
    if (int rcm = check_frame_mode(e->cfg.flags, w, h, &g_last_error)) return rcm;
    std::lock_guard<std::mutex> lk(e->mu);
    SharedGate gl;
    HIP_TRY(hipSetDevice(e->dev), ZLY_ERR_SYSTEM);
    hipStream_t s = nullptr;
    if (int rc = call_stream(e, stream, &s)) return rc;
    return detect_enqueue(e, FrameTable::tight(fmt, w, h, fb, n), d_frames, d_slabs, frame_tag0, s);
}

// The body of zly_detect_device_view, shared with zly_detect_surfaces and zly_detect_delta: the n (1..max_batch) views of the source.  Under e->mu;
// takes the enqueue gate itself.  *ran_on (if asked for): the stream the call's last kernel went to.
static int detect_device_view_locked(zly_engine* e, int32_t n, const FrameSource& f, void* d_slabs, uint32_t frame_tag0, void* stream, hipStream_t* ran_on = nullptr)
{
    FrameTable t(n, true);
    for (int i = 0; i < n; ++i) {
        if (int rcv = check_view(e->cfg.flags, f.base, f.bytes, &f.v[i], &g_last_error)) return rcv;
        t.add(f.v[i]);
    }
    SharedGate gl;
    HIP_TRY(hipSetDevice(e->dev), ZLY_ERR_SYSTEM);
    hipStream_t s = nullptr;
    if (int rc = call_stream(e, stream, &s, f.wait_for)) return rc;
    if (int rc = detect_enqueue(e, t, f.base, d_slabs, frame_tag0, s)) return rc;
    if (ran_on) *ran_on = e->last_ns;
    return ZLY_OK;
}

int32_t zly_detect_device_view(zly_engine* e, int32_t n, const void* d_base, size_t buf_bytes, const zly_frame_view* v, void* d_slabs, uint32_t frame_tag0, void* stream)
{
    if (!e) return fail(ZLY_ERR_NOT_INITIALIZED, "Engine not running");
    if (!v) return fail(ZLY_ERR_INVALID_ARGUMENT, "null views");
    if (n < 1 || n > e->cfg.max_batch) return fail(ZLY_ERR_INVALID_ARGUMENT, "batch size out of range");
    std::lock_guard<std::mutex> lk(e->mu);
    return detect_device_view_locked(e, n, FrameSource{d_base, buf_bytes, v}, d_slabs, frame_tag0, stream);
}

int32_t zly_join(zly_engine* e, void* stream, int32_t lag)
{
    if (!e) return fail(ZLY_ERR_NOT_INITIALIZED, "Engine not running");
    // completion events are kept for the last two calls only: a larger lag could not be ordered and used to return ZLY_OK without ordering anything
    if (lag < 0 || lag > 1) return fail(ZLY_ERR_INVALID_ARGUMENT, "lag must be 0 or 1");
    std::lock_guard<std::mutex> lk(e->mu);
    SharedGate gl;
    HIP_TRY(hipSetDevice(e->dev), ZLY_ERR_SYSTEM);
    hipStream_t s = nullptr;
    if (int rc = call_stream(e, stream, &s)) return rc;
    // every call but the last `lag`: calls are stream-ordered among themselves, so waiting for call (last - lag) covers all earlier ones
    if (e->call_seq > (uint64_t)lag)
        HIP_TRY(hipStreamWaitEvent(s, e->ev_call[(e->call_seq - 1 - (uint64_t)lag) & 1], 0), ZLY_ERR_INFERENCE);
    return join_nms(e, s, lag);
}

size_t zly_slab_bytes(const zly_engine* e) { return e ? slab_bytes_of(e) : 0; }

int32_t zly_sync(zly_engine* e)
{
    if (!e) return fail(ZLY_ERR_NOT_INITIALIZED, "Engine not running");
    std::lock_guard<std::mutex> lk(e->mu);
    HIP_TRY(hipSetDevice(e->dev), ZLY_ERR_SYSTEM);
    HIP_TRY(hipStreamSynchronize(e->stream), ZLY_ERR_INFERENCE);
    if (e->nms_stream) HIP_TRY(hipStreamSynchronize(e->nms_stream), ZLY_ERR_INFERENCE);
    harvest_timing(e);
    return ZLY_OK;
}

int32_t zly_read_slabs(zly_engine* e, int32_t n, void* host_slabs)
{
    if (!e) return fail(ZLY_ERR_NOT_INITIALIZED, "Engine not running");
    if (!host_slabs || n < 1 || n > e->cfg.max_batch) return fail(ZLY_ERR_INVALID_ARGUMENT, "bad argument");
    std::lock_guard<std::mutex> lk(e->mu);
    return read_back(e, [&](hipStream_t s) { return join_nms(e, s); }, {{host_slabs, e->d_slabs, slab_bytes_of(e) * (size_t)n}});
}

// --- tracking --------------------------------------------------------------------------------------
void zly_default_track_config(zly_track_config* c)
{
    if (!c) return;
    c->max_streams = 64;
    c->max_tracks = 64;
    c->match_iou = 0.3f;          // reference src/game/kalman_tracker.h:173
    c->max_lost = 6;              // the adapter's 100 ms at the reference's 60 FPS target
}

int32_t zly_track_enable(zly_engine* e, const zly_track_config* c)
{
    if (!e) return fail(ZLY_ERR_NOT_INITIALIZED, "Engine not running");
    if (!c) return fail(ZLY_ERR_INVALID_ARGUMENT, "null track config");
    if (c->max_streams < 1) return fail(ZLY_ERR_INVALID_ARGUMENT, "max_streams must be >= 1");
    if (c->max_tracks < e->cfg.max_dets || c->max_tracks > ZLY_TRACK_MAX)
        return fail(ZLY_ERR_INVALID_ARGUMENT, "max_tracks must lie in [max_dets, 64] (max_dets = " + std::to_string(e->cfg.max_dets) + ")");
    if (!(c->match_iou >= 0.0f && c->match_iou < 1.0f)) return fail(ZLY_ERR_INVALID_ARGUMENT, "match_iou must lie in [0, 1)");
    if (c->max_lost < 0) return fail(ZLY_ERR_INVALID_ARGUMENT, "max_lost must be >= 0");
    std::lock_guard<std::mutex> lk(e->mu);
    if (e->track.load()) return fail(ZLY_ERR_INVALID_ARGUMENT, "tracking is already enabled on this engine");
    ExclusiveGate gl;                                  // allocations: alone in the process
    HIP_TRY(hipSetDevice(e->dev), ZLY_ERR_SYSTEM);
    Track* tk = new Track();
    tk->cfg = *c;
    tk->seg_of.assign((size_t)c->max_streams, -1);
    const bool ok = hipMalloc((void**)&tk->d_state, sizeof(TrackStream) * (size_t)c->max_streams) == hipSuccess &&
                    tk->ring.create(sizeof(int) * (2 + 3 * (size_t)e->cfg.max_batch)) == hipSuccess &&
                    launch_track_reset(tk->d_state, 0, c->max_streams, 1u, e->stream) == hipSuccess && hipStreamSynchronize(e->stream) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        (void)track_free(tk);
        return fail(ZLY_ERR_SYSTEM, "allocation of the track tables failed");
    }
    e->track.store(tk);
    return ZLY_OK;
}

int32_t zly_track_reset(zly_engine* e, int32_t stream, uint32_t first_id)
{
    if (!e) return fail(ZLY_ERR_NOT_INITIALIZED, "Engine not running");
    Track* tk = track_of(e);
    if (!tk) return ZLY_ERR_INVALID_ARGUMENT;
    if (stream < -1 || stream >= tk->cfg.max_streams) return fail(ZLY_ERR_INVALID_ARGUMENT, "stream " + std::to_string(stream) + " out of range");
    std::lock_guard<std::mutex> lk(e->mu);
    HIP_TRY(hipSetDevice(e->dev), ZLY_ERR_SYSTEM);
    if (int rc = track_drain(tk)) return rc;
    {
        SharedGate gl;
        HIP_TRY(launch_track_reset(tk->d_state, stream < 0 ? 0 : stream, stream < 0 ? tk->cfg.max_streams : 1, first_id, e->stream), ZLY_ERR_INFERENCE);
        if (tk->d_motion) HIP_TRY(launch_track_motion_reset(tk->d_motion, stream < 0 ? 0 : stream, stream < 0 ? tk->cfg.max_streams : 1, e->stream), ZLY_ERR_INFERENCE);
    }
    HIP_TRY(hipStreamSynchronize(e->stream), ZLY_ERR_INFERENCE);
    return ZLY_OK;
}

void zly_default_track_motion_config(zly_track_motion_config* c)
{
    if (!c) return;
    c->beta = 0.5f;               // chosen, not tuned
    c->v_max = 0.25f;
}

int32_t zly_track_motion_enable(zly_engine* e, const zly_track_motion_config* c)
{
    if (!e) return fail(ZLY_ERR_NOT_INITIALIZED, "Engine not running");
    if (!c) return fail(ZLY_ERR_INVALID_ARGUMENT, "null track motion config");
    if (!(c->beta > 0.0f && c->beta <= 1.0f)) return fail(ZLY_ERR_INVALID_ARGUMENT, "beta must lie in (0, 1]");
    if (!(c->v_max >= 0.0f && c->v_max <= std::numeric_limits<float>::max())) return fail(ZLY_ERR_INVALID_ARGUMENT, "v_max must be >= 0 and finite");
    Track* tk = track_of(e);
    if (!tk) return ZLY_ERR_INVALID_ARGUMENT;
    std::lock_guard<std::mutex> lk(e->mu);
    if (tk->d_motion) return fail(ZLY_ERR_INVALID_ARGUMENT, "the motion model is already enabled on this engine");
    ExclusiveGate gl;                                  // an allocation: alone in the process
    HIP_TRY(hipSetDevice(e->dev), ZLY_ERR_SYSTEM);
    if (int rc = track_drain(tk)) return rc;
    TrackMotion* m = nullptr;
    bool ok = hipMalloc((void**)&m, sizeof(TrackMotion) * (size_t)tk->cfg.max_streams) == hipSuccess;
    // every stream starts over, as after zly_track_reset(e, -1, 0): a table matched without the model has no velocities to go on with
    ok = ok && launch_track_reset(tk->d_state, 0, tk->cfg.max_streams, 0u, e->stream) == hipSuccess &&
         launch_track_motion_reset(m, 0, tk->cfg.max_streams, e->stream) == hipSuccess && hipStreamSynchronize(e->stream) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        if (m) hipFree(m);
        return fail(ZLY_ERR_SYSTEM, "allocation of the motion state failed");
    }
    tk->mcfg = *c;
    tk->d_motion = m;
    return ZLY_OK;
}

int32_t zly_track_read(zly_engine* e, int32_t stream, zly_track* out, int32_t cap, int32_t* n_out)
{
    if (!e) return fail(ZLY_ERR_NOT_INITIALIZED, "Engine not running");
    Track* tk = track_of(e);
    if (!tk) return ZLY_ERR_INVALID_ARGUMENT;
    if (!n_out || cap < 0 || (cap > 0 && !out)) return fail(ZLY_ERR_INVALID_ARGUMENT, "null output");
    if (stream < 0 || stream >= tk->cfg.max_streams) return fail(ZLY_ERR_INVALID_ARGUMENT, "stream " + std::to_string(stream) + " out of range");
    std::lock_guard<std::mutex> lk(e->mu);
    if (int rc = track_drain(tk)) return rc;
    std::vector<unsigned char> host(sizeof(TrackStream)), hostm(sizeof(TrackMotion), 0);
    if (int rc = read_back(e, behind_nothing, {{host.data(), tk->d_state + stream, sizeof(TrackStream)},
                                               {hostm.data(), tk->d_motion ? tk->d_motion + stream : nullptr, tk->d_motion ? sizeof(TrackMotion) : 0}})) return rc;
    const TrackStream* ts = reinterpret_cast<const TrackStream*>(host.data());
    const TrackMotion* tm = reinterpret_cast<const TrackMotion*>(hostm.data());      // all zero on an engine without the model
    int32_t n = 0;
    for (int t = 0; t < tk->cfg.max_tracks; ++t) {
        if (!ts->live[t]) continue;
        if (n < cap) {
            zly_track& o = out[n];
            o.x = ts->x[t]; o.y = ts->y[t]; o.w = ts->w[t]; o.h = ts->h[t];
            o.vx = tm->vx[t]; o.vy = tm->vy[t];
            o.class_id = ts->cls[t]; o.id = ts->id[t]; o.hits = tm->hits[t]; o.last_seen = ts->last_seen[t];
        }
        ++n;
    }
    *n_out = n;
    return ZLY_OK;
}

int32_t zly_track_state_at(zly_engine* e, int32_t stream, zly_track_state* out)
{
    if (!e) return fail(ZLY_ERR_NOT_INITIALIZED, "Engine not running");
    Track* tk = track_of(e);
    if (!tk) return ZLY_ERR_INVALID_ARGUMENT;
    if (!out) return fail(ZLY_ERR_INVALID_ARGUMENT, "null output");
    if (stream < 0 || stream >= tk->cfg.max_streams) return fail(ZLY_ERR_INVALID_ARGUMENT, "stream " + std::to_string(stream) + " out of range");
    std::lock_guard<std::mutex> lk(e->mu);
    if (int rc = track_drain(tk)) return rc;
    std::vector<unsigned char> host(sizeof(TrackStream));
    if (int rc = read_back(e, behind_nothing, {{host.data(), tk->d_state + stream, sizeof(TrackStream)}})) return rc;
    const TrackStream* ts = reinterpret_cast<const TrackStream*>(host.data());
    out->frame_no = ts->frame_no; out->next_id = ts->next_id; out->evictions = ts->evictions;
    out->n_live = 0;
    for (int t = 0; t < tk->cfg.max_tracks; ++t) out->n_live += ts->live[t] ? 1 : 0;
    return ZLY_OK;
}

int32_t zly_track_slabs(zly_engine* e, int32_t n, const int32_t* streams, void* d_slabs, void* stream)
{
    if (!e) return fail(ZLY_ERR_NOT_INITIALIZED, "Engine not running");
    Track* tk = track_of(e);
    if (!tk) return ZLY_ERR_INVALID_ARGUMENT;
    if (n < 1 || n > e->cfg.max_batch) return fail(ZLY_ERR_INVALID_ARGUMENT, "batch size out of range");
    if (!streams) return fail(ZLY_ERR_INVALID_ARGUMENT, "null streams");
    for (int i = 0; i < n; ++i)
        if (streams[i] < -1 || streams[i] >= tk->cfg.max_streams) return fail(ZLY_ERR_INVALID_ARGUMENT, "stream " + std::to_string(streams[i]) + " out of range");
    std::lock_guard<std::mutex> lk(e->mu);
    SharedGate gl;
    HIP_TRY(hipSetDevice(e->dev), ZLY_ERR_SYSTEM);
    hipStream_t s = nullptr;
    if (int rc = call_stream(e, stream, &s)) return rc;
    if (int rc = stream_after_detect(e, s)) return rc;
    bool launched = false;
    int rc = track_enqueue(e, tk, n, streams, d_slabs ? d_slabs : e->d_slabs, s, &launched);
    if (rc != ZLY_OK) return rc;
    return launched ? detect_events_behind(e, s) : ZLY_OK;
}

static int submit_tracked(zly_engine* e, const uint8_t* base, size_t buf_bytes, const zly_frame_view* v, int32_t stream, uint64_t* ticket, bool nonblock)
{
    if (!e) return fail(ZLY_ERR_NOT_INITIALIZED, "Engine not running");
    Track* tk = track_of(e);
    if (!tk) return ZLY_ERR_INVALID_ARGUMENT;
    if (!v) return fail(ZLY_ERR_INVALID_ARGUMENT, "null view");
    if (!ticket) return fail(ZLY_ERR_INVALID_ARGUMENT, "null ticket");
    if (stream < -1 || stream >= tk->cfg.max_streams) return fail(ZLY_ERR_INVALID_ARGUMENT, "stream " + std::to_string(stream) + " out of range");
    return ingest_submit(e, base, buf_bytes, 0, 0, ticket, nonblock, ZLY_PIX_BGR, v, stream);
}

int32_t zly_submit_view_tracked(zly_engine* e, const uint8_t* base, size_t buf_bytes, const zly_frame_view* v, int32_t stream, uint64_t* ticket)
{
    return submit_tracked(e, base, buf_bytes, v, stream, ticket, false);
}

int32_t zly_submit_try_view_tracked(zly_engine* e, const uint8_t* base, size_t buf_bytes, const zly_frame_view* v, int32_t stream, uint64_t* ticket)
{
    return submit_tracked(e, base, buf_bytes, v, stream, ticket, true);
}

// --- tiles -----------------------------------------------------------------------------------------
void zly_default_merge_config(zly_merge_config* c)
{
    if (!c) return;
    c->metric = ZLY_MERGE_IOS;    // chosen, not tuned
    c->thr = 0.5f;
}

int32_t zly_tile_grid(int32_t W, int32_t H, int32_t tile_w, int32_t tile_h, int32_t overlap_x, int32_t overlap_y, int32_t even, zly_tile* out,
                      int32_t cap, int32_t* n_out)
{
    if (!n_out || cap < 0 || (cap > 0 && !out)) return fail(ZLY_ERR_INVALID_ARGUMENT, "zly_tile_grid: null output");
    return tile_grid(W, H, tile_w, tile_h, overlap_x, overlap_y, even, out, cap, n_out, &g_last_error);
}

// the argument checks of a merge (include/zly.h lists them); *max_slots = the largest tiles x cap of a group
static int merge_check(const zly_engine* e, int n, const zly_tile* tiles, int n_groups, const zly_merge_config* c, int* max_slots)
{
    if (n < 1 || n > e->cfg.max_batch) return fail(ZLY_ERR_INVALID_ARGUMENT, "batch size out of range");
    if (n_groups < 1 || n_groups > n) return fail(ZLY_ERR_INVALID_ARGUMENT, "n_groups must lie in 1..n");
    if (!tiles) return fail(ZLY_ERR_INVALID_ARGUMENT, "null tiles");
    if (!c) return fail(ZLY_ERR_INVALID_ARGUMENT, "null merge config");
    if (c->metric != ZLY_MERGE_IOU && c->metric != ZLY_MERGE_IOS) return fail(ZLY_ERR_INVALID_ARGUMENT, "unknown merge metric " + std::to_string(c->metric));
    if (!(c->thr >= 0.0f && c->thr < 1.0f)) return fail(ZLY_ERR_INVALID_ARGUMENT, "the merge threshold must lie in [0, 1)");
    std::vector<int> count((size_t)n_groups, 0), first((size_t)n_groups, -1);
    for (int i = 0; i < n; ++i) {
        const zly_tile& t = tiles[i];
        if (t.group < -1 || t.group >= n_groups) return fail(ZLY_ERR_INVALID_ARGUMENT, "tile " + std::to_string(i) + ": group " + std::to_string(t.group) + " out of range");
        if (t.group < 0) continue;
        if (t.W < 1 || t.H < 1 || t.W >= (1 << 24) || t.H >= (1 << 24)) return fail(ZLY_ERR_INVALID_ARGUMENT, "tile " + std::to_string(i) + ": the surface must lie in 1..2^24-1");
        if (t.w < 1 || t.h < 1 || t.x0 < 0 || t.y0 < 0 || (int64_t)t.x0 + t.w > t.W || (int64_t)t.y0 + t.h > t.H)
            return fail(ZLY_ERR_INVALID_ARGUMENT, "tile " + std::to_string(i) + ": the rectangle is not inside its surface");
        int& f = first[(size_t)t.group];
        if (f < 0) f = i;
        else if (tiles[f].W != t.W || tiles[f].H != t.H) return fail(ZLY_ERR_INVALID_ARGUMENT, "tile " + std::to_string(i) + ": the tiles of group " + std::to_string(t.group) + " disagree on W, H");
        count[(size_t)t.group]++;
    }
    int64_t mx = 0;
    for (int g = 0; g < n_groups; ++g) mx = std::max<int64_t>(mx, (int64_t)count[(size_t)g] * e->cfg.max_dets);
    if (mx > ZLY_MERGE_MAX_CANDIDATES) return fail(ZLY_ERR_INVALID_ARGUMENT, "a group's tiles x max_dets exceed ZLY_MERGE_MAX_CANDIDATES");
    *max_slots = (int)mx;
    return ZLY_OK;
}

// the engine's merge state, created on first use: allocations and the kernel's LDS opt-in, alone in the process.  Under e->mu, no gate held.
static int merge_ensure(zly_engine* e)
{
    if (e->merge) return ZLY_OK;
    ExclusiveGate gl;
    HIP_TRY(hipSetDevice(e->dev), ZLY_ERR_SYSTEM);
    Merge* mg = new Merge();
    const bool ok = merge_init() == hipSuccess &&
                    mg->ring.create(sizeof(int) * ((size_t)e->cfg.max_batch * (1 + ZLY_MERGE_TILE_INTS) + 1)) == hipSuccess &&
                    hipMalloc((void**)&mg->d_out, slab_bytes_of(e) * (size_t)e->cfg.max_batch) == hipSuccess &&
                    hipMemset(mg->d_out, 0, slab_bytes_of(e) * (size_t)e->cfg.max_batch) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        (void)merge_free(mg);
        return fail(ZLY_ERR_SYSTEM, "allocation of the merge buffers failed");
    }
    e->merge = mg;
    return ZLY_OK;
}

// Builds the call's tile table in the next ring entry and uploads it on `s`; *ring = the entry.  Under e->mu, enqueue gate held; the arguments are
// validated by the caller (merge_check).  A zoom call uploads on the call's stream, in front of the kernel that patches the table, and launches the
// merge later, on the stream the slabs' NMS ran on.
static int merge_upload(zly_engine* e, int n, const zly_tile* tiles, int n_groups, hipStream_t s, int* ring)
{
    Merge* mg = e->merge;
    int r = 0;
    HIP_TRY(mg->ring.claim(&r), ZLY_ERR_INFERENCE);
    int* t = mg->ring.host<int>(r);
    for (int g = 0; g <= n_groups; ++g) t[g] = 0;
    for (int i = 0; i < n; ++i) if (tiles[i].group >= 0) t[tiles[i].group + 1]++;
    for (int g = 0; g < n_groups; ++g) t[g + 1] += t[g];                             // t[g] = offset of group g, t[n_groups] = members in all
    const int n_members = t[n_groups];
    int* members = t + n_groups + 1;
    std::vector<int> fill(t, t + n_groups);
    for (int i = 0; i < n; ++i) {                                                     // ascending slab index inside every group
        if (tiles[i].group < 0) continue;
        int* m = members + (size_t)fill[(size_t)tiles[i].group]++ * ZLY_MERGE_TILE_INTS;
        m[0] = i; m[1] = tiles[i].x0; m[2] = tiles[i].y0; m[3] = tiles[i].w; m[4] = tiles[i].h; m[5] = tiles[i].W; m[6] = tiles[i].H;
    }
    HIP_TRY(mg->ring.upload(r, sizeof(int) * (size_t)(n_groups + 1 + n_members * ZLY_MERGE_TILE_INTS), s), ZLY_ERR_INFERENCE);
    *ring = r;
    return ZLY_OK;
}

// launches merge_kernel on the uploaded table of ring entry r, on `s` -- the stream the slabs' NMS ran on, or one already ordered behind it (and behind
// the table's upload)
static int merge_launch(zly_engine* e, int r, int n_groups, const zly_merge_config* c, int max_slots, const void* src, void* dst, uint32_t tag0, hipStream_t s)
{
    Merge* mg = e->merge;
    HIP_TRY(launch_merge(mg->ring.dev<int>(r), n_groups, max_slots, src, dst, e->cfg.max_dets, c->metric, c->thr, tag0, s), ZLY_ERR_INFERENCE);
    HIP_TRY(mg->ring.mark(r, s), ZLY_ERR_INFERENCE);
    return ZLY_OK;
}

// upload and launch on one stream: the merge of zly_merge_slabs and zly_detect_tiled
static int merge_enqueue(zly_engine* e, int n, const zly_tile* tiles, int n_groups, const zly_merge_config* c, int max_slots, const void* src, void* dst,
                         uint32_t tag0, hipStream_t s)
{
    int r = 0;
    if (int rc = merge_upload(e, n, tiles, n_groups, s, &r)) return rc;
    return merge_launch(e, r, n_groups, c, max_slots, src, dst, tag0, s);
}

int32_t zly_merge_slabs(zly_engine* e, int32_t n, const zly_tile* tiles, int32_t n_groups, const zly_merge_config* c, void* d_slabs, void* d_out,
                        uint32_t frame_tag0, void* stream)
{
    if (!e) return fail(ZLY_ERR_NOT_INITIALIZED, "Engine not running");
    int max_slots = 0;
    if (int rc = merge_check(e, n, tiles, n_groups, c, &max_slots)) return rc;
    if (d_out && d_out == (void*)e->d_slabs) return fail(ZLY_ERR_INVALID_ARGUMENT, "d_out must not be the engine's own slab buffer");
    std::lock_guard<std::mutex> lk(e->mu);
    if (int rc = merge_ensure(e)) return rc;
    SharedGate gl;
    HIP_TRY(hipSetDevice(e->dev), ZLY_ERR_SYSTEM);
    hipStream_t s = nullptr;
    if (int rc = call_stream(e, stream, &s)) return rc;
    if (int rc = stream_after_detect(e, s)) return rc;
    int rc = merge_enqueue(e, n, tiles, n_groups, c, max_slots, d_slabs ? d_slabs : e->d_slabs, d_out ? d_out : e->merge->d_out, frame_tag0, s);
    if (rc != ZLY_OK) return rc;
    return detect_events_behind(e, s);
}

int32_t zly_read_merged(zly_engine* e, int32_t n_groups, void* host_slabs)
{
    if (!e) return fail(ZLY_ERR_NOT_INITIALIZED, "Engine not running");
    if (!host_slabs || n_groups < 1 || n_groups > e->cfg.max_batch) return fail(ZLY_ERR_INVALID_ARGUMENT, "bad argument");
    std::lock_guard<std::mutex> lk(e->mu);
    Merge* mg = enabled(e->merge, NO_MERGE);
    if (!mg) return ZLY_ERR_INVALID_ARGUMENT;
    auto behind = [&](hipStream_t s) -> int {
        HIP_TRY(mg->ring.wait_last(s), ZLY_ERR_INFERENCE);               // merges of an engine are ordered among themselves
        return join_nms(e, s);
    };
    return read_back(e, behind, {{host_slabs, mg->d_out, slab_bytes_of(e) * (size_t)n_groups}});
}

int32_t zly_detect_tiled(zly_engine* e, const uint8_t* base, size_t buf_bytes, const zly_frame_view* surface, int32_t n, const zly_tile* tiles,
                         const zly_merge_config* c, zly_det* out, int32_t cap, int32_t* n_out)
{
    if (!e) return fail(ZLY_ERR_NOT_INITIALIZED, "Engine not running");
    if (!surface || !out || !n_out || cap < 0) return fail(ZLY_ERR_INVALID_ARGUMENT, "null argument");
    if (!pix_format(surface->fmt)) return fail(ZLY_ERR_INVALID_ARGUMENT, "unknown pixel format " + std::to_string(surface->fmt));
    size_t nbytes = 0;
    if (!view_valid(surface, &nbytes)) return fail(ZLY_ERR_INVALID_INPUT, "invalid surface view");
    if (!base || nbytes > buf_bytes) return fail(ZLY_ERR_INVALID_INPUT, "Invalid image data size: the surface needs " + std::to_string(nbytes) + " bytes, got " + std::to_string(buf_bytes));
    int max_slots = 0;
    if (int rc = merge_check(e, n, tiles, 1, c, &max_slots)) return rc;
    FrameTable ft(n, true);
    for (int i = 0; i < n; ++i) {
        const zly_tile& t = tiles[i];
        if (t.group != 0 || t.W != surface->w || t.H != surface->h)
            return fail(ZLY_ERR_INVALID_ARGUMENT, "tile " + std::to_string(i) + ": zly_detect_tiled needs group = 0 and W, H = the surface's size");
        zly_frame_view v;
        if (int rc = zly_view_crop(surface, t.x0, t.y0, t.w, t.h, &v)) return rc;
        if (int rc = check_view(e->cfg.flags, base, buf_bytes, &v, &g_last_error)) return rc;
        ft.add(v);
    }
    std::lock_guard<std::mutex> lk(e->mu);
    if (int rc = merge_ensure(e)) return rc;
    HIP_TRY(hipSetDevice(e->dev), ZLY_ERR_SYSTEM);
    if (int rc = stage_for(e, nbytes)) return rc;
    memcpy(e->h_stage, base, nbytes);                                    // the surface once, as it is: the front kernel fetches through the tiles' views
    SharedGate gl;
    HIP_TRY(hipMemcpyAsync(e->d_stage, e->h_stage, nbytes, hipMemcpyHostToDevice, e->stream), ZLY_ERR_INFERENCE);
    // not detect_run: a host-synchronous call never defers its NMS and is no call that zly_join or stream_after_detect could order anything behind
    int rc = set_desc(e, ft, e->stream);
    if (rc != ZLY_OK) return rc;
    rc = run_path(e, n, e->d_stage, nullptr, 0, e->stream, true, false, nullptr, ft.front(e));
    if (rc != ZLY_OK) { with_stats(e, [](zly_stats& st) { st.inference_errors++; }); return rc; }
    rc = merge_enqueue(e, n, tiles, 1, c, max_slots, e->d_slabs, e->merge->d_out, 0, e->stream);
    if (rc != ZLY_OK) return rc;
    HIP_TRY(hipMemcpyAsync(e->h_slabs, e->merge->d_out, slab_bytes_of(e), hipMemcpyDeviceToHost, e->stream), ZLY_ERR_INFERENCE);
    gl.release();                                                        // waiting for the device is not an enqueue section
    HIP_TRY(hipStreamSynchronize(e->stream), ZLY_ERR_INFERENCE);
    *n_out = unpack_slab(e->h_slabs, cap, e->cfg.max_dets, now_ms(), out);          // the timestamp: onnx_engine.cpp:813-815
    harvest_timing(e);
    with_stats(e, [&](zly_stats& st) { st.inference_count += (uint64_t)n; });
    return ZLY_OK;
}

// --- resident surfaces (include/zly.h "Resident surfaces"; the rules: surface_rules.h) -----------------
int32_t zly_surfaces_enable(zly_engine* e, int32_t max_surfaces, size_t max_bytes_each)
{
    if (!e) return fail(ZLY_ERR_NOT_INITIALIZED, "Engine not running");
    SurfaceStore st;
    if (int rc = surfaces_plan_store(max_surfaces, max_bytes_each, &st, &g_last_error)) return rc;
    std::lock_guard<std::mutex> lk(e->mu);
    if (e->surf) return fail(ZLY_ERR_INVALID_ARGUMENT, "resident surfaces are already enabled on this engine");
    ExclusiveGate gl;                                  // allocations: alone in the process
    HIP_TRY(hipSetDevice(e->dev), ZLY_ERR_SYSTEM);
    Surfaces* sf = new Surfaces();
    sf->store = st;
    sf->slots.resize((size_t)max_surfaces);
    // cleared once: zly_surface_read of a slot without a keyframe never shows what the memory held before
    const bool ok = hipMalloc((void**)&sf->d_store, st.total) == hipSuccess && hipEventCreateWithFlags(&sf->ev_patch, hipEventDisableTiming) == hipSuccess &&
                    hipEventCreateWithFlags(&sf->ev_read, hipEventDisableTiming) == hipSuccess &&
                    hipMemsetAsync(sf->d_store, 0, st.total, e->stream) == hipSuccess && hipStreamSynchronize(e->stream) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        (void)surfaces_free(sf);
        return fail(ZLY_ERR_SYSTEM, "allocation of the surface store (" + std::to_string(st.total) + " bytes) failed");
    }
    e->surf = sf;
    return ZLY_OK;
}

int32_t zly_surface_define(zly_engine* e, int32_t s, int32_t fmt, int32_t w, int32_t h)
{
    if (!e) return fail(ZLY_ERR_NOT_INITIALIZED, "Engine not running");
    std::lock_guard<std::mutex> lk(e->mu);
    Surfaces* sf = surfaces_of(e);
    if (!sf) return ZLY_ERR_INVALID_ARGUMENT;
    SurfaceSlot sl;
    if (int rc = surface_define(sf->store, s, fmt, w, h, &sl, &g_last_error)) return rc;
    sf->slots[(size_t)s] = sl;
    return ZLY_OK;
}

// Enqueues the update that sf->plan describes (surface_plan_update has accepted it) on the engine's stream: the rectangles' rows tight into pinned staging
// on this thread, ONE copy of pixels + band table, ONE launch.  Under e->mu; takes the gates itself.
static int surface_enqueue_update(zly_engine* e, Surfaces* sf, int n_rects, const zly_surface_rect* rects, const uint8_t* const* bases, const zly_frame_view* src_views)
{
    const SurfacePlan& pl = sf->plan;
    if (pl.bands.size() > (size_t)std::numeric_limits<int>::max()) return fail(ZLY_ERR_INVALID_ARGUMENT, "zly_surface_update: too many bands");
    HIP_TRY(hipSetDevice(e->dev), ZLY_ERR_SYSTEM);
    if (int rc = stage_for(e, pl.stage_bytes)) return rc;
    for (int i = 0; i < n_rects; ++i) copy_view_tight(e->h_stage + pl.stage_off[(size_t)i], bases[i], &src_views[i]);
    memcpy(e->h_stage + pl.table_off, pl.bands.data(), pl.bands.size() * sizeof(SurfaceJob));
    SharedGate gl;
    if (int rc = surfaces_begin_write(e, sf)) return rc;
    HIP_TRY(hipMemcpyAsync(e->d_stage, e->h_stage, pl.stage_bytes, hipMemcpyHostToDevice, e->stream), ZLY_ERR_INFERENCE);
    HIP_TRY(launch_surface_patch(e->d_stage, reinterpret_cast<const SurfaceJob*>(e->d_stage + pl.table_off), (int)pl.bands.size(), sf->d_store, e->sw.num_cus, e->stream),
            ZLY_ERR_INFERENCE);
    if (int rc = surfaces_end_write(e, sf)) return rc;
    for (int i = 0; i < n_rects; ++i) if (pl.covers[(size_t)i]) sf->slots[(size_t)rects[i].surface].valid = true;
    return ZLY_OK;
}

int32_t zly_surface_update(zly_engine* e, int32_t n_rects, const zly_surface_rect* rects, const uint8_t* const* bases, const size_t* buf_bytes,
                           const zly_frame_view* src_views)
{
    if (!e) return fail(ZLY_ERR_NOT_INITIALIZED, "Engine not running");
    std::lock_guard<std::mutex> lk(e->mu);
    Surfaces* sf = surfaces_of(e);
    if (!sf) return ZLY_ERR_INVALID_ARGUMENT;
    if (int rc = surface_plan_update(sf->store, sf->slots.data(), n_rects, rects, bases, buf_bytes, src_views, &sf->plan, &g_last_error)) return rc;
    return surface_enqueue_update(e, sf, n_rects, rects, bases, src_views);
}

int32_t zly_surface_moves_enable(zly_engine* e, size_t scratch_bytes)
{
    if (!e) return fail(ZLY_ERR_NOT_INITIALIZED, "Engine not running");
    std::lock_guard<std::mutex> lk(e->mu);
    Surfaces* sf = surfaces_of(e);
    if (!sf) return ZLY_ERR_INVALID_ARGUMENT;
    if (sf->d_bounce) return fail(ZLY_ERR_INVALID_ARGUMENT, "surface moves are already enabled on this engine");
    const size_t bytes = scratch_bytes ? scratch_bytes : sf->store.stride + 48;  // holds any single move: its planes' bytes, each of up to three rounded up to 16
    ExclusiveGate gl;                                  // an allocation: alone in the process
    HIP_TRY(hipSetDevice(e->dev), ZLY_ERR_SYSTEM);
    if (hipMalloc((void**)&sf->d_bounce, bytes) != hipSuccess) {
        (void)hipGetLastError();
        sf->d_bounce = nullptr;
        return fail(ZLY_ERR_SYSTEM, "allocation of the bounce buffer (" + std::to_string(bytes) + " bytes) failed");
    }
    sf->bounce_bytes = bytes;
    return ZLY_OK;
}

// One call's moves: the phases' band tables through pinned staging in ONE copy, then per phase the move kernel and, if it gathered anything, the patch
// kernel from the bounce buffer -- all on the engine's stream, ordered against detect calls and updates exactly as an update's patch kernel is.
int32_t zly_surface_move(zly_engine* e, int32_t n_moves, const struct zly_surface_move* moves)
{
    if (!e) return fail(ZLY_ERR_NOT_INITIALIZED, "Engine not running");
    std::lock_guard<std::mutex> lk(e->mu);
    Surfaces* sf = surfaces_of(e);
    if (!sf) return ZLY_ERR_INVALID_ARGUMENT;
    if (int rc = surface_plan_moves(sf->store, sf->slots.data(), n_moves, moves, sf->bounce_bytes, &sf->mplan, &g_last_error)) return rc;
    const SurfaceMovePlan& pl = sf->mplan;
    if (pl.a_bands.empty()) return ZLY_OK;                               // identity moves only: nothing to do
    if (pl.a_bands.size() > (size_t)std::numeric_limits<int>::max() || pl.b_bands.size() > (size_t)std::numeric_limits<int>::max())
        return fail(ZLY_ERR_INVALID_ARGUMENT, "zly_surface_move: too many bands");
    HIP_TRY(hipSetDevice(e->dev), ZLY_ERR_SYSTEM);
    if (int rc = stage_for(e, pl.table_bytes)) return rc;
    static_assert(sizeof(SurfaceMoveBand) == 32 && sizeof(SurfaceJob) == 32, "the band records are 32 bytes");
    const size_t b_off = pl.a_bands.size() * sizeof(SurfaceMoveBand);
    memcpy(e->h_stage, pl.a_bands.data(), b_off);
    if (!pl.b_bands.empty()) memcpy(e->h_stage + b_off, pl.b_bands.data(), pl.b_bands.size() * sizeof(SurfaceJob));
    SharedGate gl;
    if (int rc = surfaces_begin_write(e, sf)) return rc;
    HIP_TRY(hipMemcpyAsync(e->d_stage, e->h_stage, pl.table_bytes, hipMemcpyHostToDevice, e->stream), ZLY_ERR_INFERENCE);
    const SurfaceMoveBand* d_a = reinterpret_cast<const SurfaceMoveBand*>(e->d_stage);
    const SurfaceJob* d_b = reinterpret_cast<const SurfaceJob*>(e->d_stage + b_off);
    for (const SurfaceMovePhase& ph : pl.phases) {
        HIP_TRY(launch_surface_move(d_a + ph.a_first, (int)ph.a_count, sf->d_store, sf->d_bounce, e->sw.num_cus, e->stream), ZLY_ERR_INFERENCE);
        HIP_TRY(launch_surface_patch(sf->d_bounce, d_b + ph.b_first, (int)ph.b_count, sf->d_store, e->sw.num_cus, e->stream), ZLY_ERR_INFERENCE);
    }
    return surfaces_end_write(e, sf);
}

int32_t zly_surface_read(zly_engine* e, int32_t s, void* host_out, size_t cap_bytes)
{
    if (!e) return fail(ZLY_ERR_NOT_INITIALIZED, "Engine not running");
    if (!host_out) return fail(ZLY_ERR_INVALID_ARGUMENT, "null output");
    std::lock_guard<std::mutex> lk(e->mu);
    Surfaces* sf = surfaces_of(e);
    if (!sf) return ZLY_ERR_INVALID_ARGUMENT;
    if (int rc = surface_check_slot(sf->store, s, &g_last_error)) return rc;
    const SurfaceSlot& sl = sf->slots[(size_t)s];
    if (!sl.defined) return fail(ZLY_ERR_INVALID_ARGUMENT, "surface " + std::to_string(s) + " is not defined (zly_surface_define)");
    const size_t fb = frame_bytes(sl.fmt, sl.w, sl.h);
    if (cap_bytes < fb) return fail(ZLY_ERR_INVALID_ARGUMENT, "zly_surface_read: the surface holds " + std::to_string(fb) + " bytes, the buffer " + std::to_string(cap_bytes));
    return read_back(e, behind_nothing, {{host_out, sf->d_store + (size_t)s * sf->store.stride, fb}});      // the patch kernels ran on the engine's stream
}

int32_t zly_detect_surfaces(zly_engine* e, int32_t n, const int32_t* surfaces, const zly_roi* rois, void* d_slabs, uint32_t frame_tag0, void* stream)
{
    if (!e) return fail(ZLY_ERR_NOT_INITIALIZED, "Engine not running");
    if (!surfaces) return fail(ZLY_ERR_INVALID_ARGUMENT, "null surfaces");
    if (n < 1 || n > e->cfg.max_batch) return fail(ZLY_ERR_INVALID_ARGUMENT, "batch size out of range");
    std::lock_guard<std::mutex> lk(e->mu);
    StoreFrames src;
    if (int rc = src.open(e)) return rc;
    if (int rc = src.frames(n, surfaces, rois)) return rc;
    return src.read_by([&](const FrameSource& f, hipStream_t* ran) { return detect_device_view_locked(e, n, f, d_slabs, frame_tag0, stream, ran); });
}

int32_t zly_detect_delta(zly_engine* e, int32_t n_rects, const zly_surface_rect* rects, const uint8_t* const* bases, const size_t* buf_bytes,
                         const zly_frame_view* src_views, int32_t n, const int32_t* surfaces, zly_det* out, int32_t cap, int32_t* n_out)
{
    if (!e) return fail(ZLY_ERR_NOT_INITIALIZED, "Engine not running");
    if (!surfaces) return fail(ZLY_ERR_INVALID_ARGUMENT, "null surfaces");
    if (!out || !n_out || cap < 0) return fail(ZLY_ERR_INVALID_ARGUMENT, "null output");
    if (n < 1 || n > e->cfg.max_batch) return fail(ZLY_ERR_INVALID_ARGUMENT, "batch size out of range");
    if (n_rects < 0) return fail(ZLY_ERR_INVALID_ARGUMENT, "negative rectangle count");
    std::lock_guard<std::mutex> lk(e->mu);
    Surfaces* sf = surfaces_of(e);
    if (!sf) return ZLY_ERR_INVALID_ARGUMENT;
    // every check of both halves first, validity as it will be after the update: a refused call enqueues nothing
    std::vector<SurfaceSlot> after = sf->slots;
    if (n_rects > 0) {
        if (int rc = surface_plan_update(sf->store, sf->slots.data(), n_rects, rects, bases, buf_bytes, src_views, &sf->plan, &g_last_error)) return rc;
        for (int i = 0; i < n_rects; ++i) if (sf->plan.covers[(size_t)i]) after[(size_t)rects[i].surface].valid = true;
    }
    std::vector<zly_frame_view> views((size_t)n);
    if (int rc = surface_detect_views(sf->store, after.data(), n, surfaces, nullptr, views.data(), &g_last_error)) return rc;
    for (int i = 0; i < n; ++i)
        if (int rc = check_view(e->cfg.flags, sf->d_store, sf->store.total, &views[(size_t)i], &g_last_error)) return rc;
    if (n_rects > 0)
        if (int rc = surface_enqueue_update(e, sf, n_rects, rects, bases, src_views)) return rc;
    // Not StoreFrames: the views are made against `after`, and the call is on the engine's own stream and waited for below, so the store is told of no reader
    if (int rc = detect_device_view_locked(e, n, FrameSource{sf->d_store, sf->store.total, views.data()}, nullptr, 0, nullptr)) return rc;
    const size_t sb = slab_bytes_of(e);
    {
        SharedGate gl;
        if (int rc = join_nms(e, e->stream)) return rc;                 // ZLY_FLAG_ASYNC_NMS: the call's NMS may run on the engine's NMS stream
        HIP_TRY(hipMemcpyAsync(e->h_slabs, e->d_slabs, sb * (size_t)n, hipMemcpyDeviceToHost, e->stream), ZLY_ERR_INFERENCE);
    }
    HIP_TRY(hipStreamSynchronize(e->stream), ZLY_ERR_INFERENCE);
    const uint64_t ts = now_ms();                                        // onnx_engine.cpp:813-815
    for (int i = 0; i < n; ++i) n_out[i] = unpack_slab(e->h_slabs + sb * (size_t)i, cap, e->cfg.max_dets, ts, out + (size_t)i * cap);
    harvest_timing(e);
    return ZLY_OK;
}

// --- change map (include/zly.h "Change map"; the rules: change_rules.h; the kernels: kernels_change.hip) ----------------
void zly_default_change_config(const zly_engine* e, zly_change_config* c)
{
    if (!c) return;
    change_default_config(e ? e->cfg.model_w : 416, e ? e->cfg.model_h : 416, c);
}

int32_t zly_change_enable(zly_engine* e, const zly_change_config* c, int32_t max_streams)
{
    if (!e) return fail(ZLY_ERR_NOT_INITIALIZED, "Engine not running");
    if (int rc = change_check_config(c, max_streams, &g_last_error)) return rc;
    std::lock_guard<std::mutex> lk(e->mu);
    if (e->change) return fail(ZLY_ERR_INVALID_ARGUMENT, "the change map is already enabled on this engine");
    ExclusiveGate gl;                                  // allocations: alone in the process
    HIP_TRY(hipSetDevice(e->dev), ZLY_ERR_SYSTEM);
    Change* ch = new Change();
    ch->cfg = *c;
    ch->lay = change_layout(c->max_peaks);
    ch->max_streams = max_streams;
    const size_t B = (size_t)e->cfg.max_batch, NS = (size_t)max_streams, grid = sizeof(uint32_t) * ZLY_CHANGE_MAX_CELLS;
    // both arrays 16-byte aligned in every entry
    static_assert(sizeof(ChangeItem) == 16 && alignof(ChipFrame) <= 16 && alignof(ChangeItem) <= 16, "the entry's layout assumes 16-byte items");
    ch->items_off = (sizeof(ChipFrame) * B + 15) / 16 * 16;
    bool ok = ch->ring.create(ch->items_off + sizeof(ChangeItem) * B) == hipSuccess &&
              hipMalloc((void**)&ch->d_sums, grid * B) == hipSuccess &&
              hipMalloc((void**)&ch->d_state, sizeof(ChangeStream) * NS) == hipSuccess &&
              hipMalloc((void**)&ch->d_prev, grid * NS) == hipSuccess &&
              hipMalloc((void**)&ch->d_recs, (size_t)ch->lay.rec_bytes * NS) == hipSuccess &&
              hipMemset(ch->d_sums, 0, grid * B) == hipSuccess &&
              hipMemset(ch->d_state, 0, sizeof(ChangeStream) * NS) == hipSuccess &&
              hipMemset(ch->d_prev, 0, grid * NS) == hipSuccess &&
              hipMemset(ch->d_recs, 0, (size_t)ch->lay.rec_bytes * NS) == hipSuccess &&
              hipDeviceSynchronize() == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        (void)change_free(ch);
        return fail(ZLY_ERR_SYSTEM, "allocation of the change map's buffers failed");
    }
    e->change = ch;
    return ZLY_OK;
}

int32_t zly_change_layout(const zly_engine* e, size_t* rec_bytes, size_t* peaks_off, size_t* activity_off)
{
    if (!e) return fail(ZLY_ERR_NOT_INITIALIZED, "Engine not running");
    std::lock_guard<std::mutex> lk(const_cast<zly_engine*>(e)->mu);
    const Change* ch = enabled(e->change, NO_CHANGE);
    if (!ch) return ZLY_ERR_INVALID_ARGUMENT;
    if (rec_bytes) *rec_bytes = (size_t)ch->lay.rec_bytes;
    if (peaks_off) *peaks_off = (size_t)ch->lay.peaks_off;
    if (activity_off) *activity_off = (size_t)ch->lay.activity_off;
    return ZLY_OK;
}

// The first half of a change call on n checked views v of the device buffer d_base: takes the next ring entry, orders the stream `s` behind the
// change calls so far (they share the scratch grids and the streams' states), uploads the frame records and launches change_sums_kernel.  *ring: the
// entry, for change_enqueue_pick.  Under e->mu, enqueue gate held; every check has been made.
static int change_enqueue_sums(zly_engine* e, Change* ch, int n, const void* d_base, const zly_frame_view* v, const int32_t* streams, hipStream_t s, int* ring)
{
    int r = 0;
    HIP_TRY(ch->ring.claim_behind_last(s, &r), ZLY_ERR_INFERENCE);
    const int rc = [&]() -> int {
        ChipFrame* hf = ch->ring.host<ChipFrame>(r);
        ChangeItem* hi = ch->items(ch->ring.host<unsigned char>(r));
        int max_w = 1, max_h = 1;
        for (int i = 0; i < n; ++i) {
            hf[i] = chip_frame_of(&v[i]);
            hi[i] = ChangeItem{v[i].w, v[i].h, streams[i], 0};
            max_w = std::max(max_w, (int)v[i].w); max_h = std::max(max_h, (int)v[i].h);
        }
        // one copy: the frame records (all max_batch of the entry; the n first matter) and the n items behind them
        HIP_TRY(ch->ring.upload(r, ch->items_off + sizeof(ChangeItem) * (size_t)n, s), ZLY_ERR_INFERENCE);
        HIP_TRY(launch_change_sums((const uint8_t*)d_base, ch->ring.dev<ChipFrame>(r), n, max_w, max_h, ch->cfg.cell, ch->d_sums, s), ZLY_ERR_INFERENCE);
        return ZLY_OK;
    }();
    // The entry's event goes behind whatever has been enqueued, a failed call's too, and behind the sums kernel even if the caller fails before its
    // pick kernel: the next change call, on whichever stream, is ordered behind every user of the entry and of the scratch grids.
    if (ch->ring.mark(r, s) != hipSuccess && rc == ZLY_OK) return fail(ZLY_ERR_INFERENCE, "hipEventRecord failed behind the change map's sums kernel");
    *ring = r;
    return rc;
}

// The second half: change_pick_kernel on the ring entry r, and the entry's event once more, behind it.  zf, desc, tab, plan, K: a zoom call's (null, 0: none)
static int change_enqueue_pick(zly_engine* e, Change* ch, int n, int r, const ZoomFrame* zf, FrameDesc* desc, int* tab, zly_zoom_region* plan, int K, hipStream_t s)
{
    const ChangeItem* di = ch->items(ch->ring.dev<unsigned char>(r));
    HIP_TRY(launch_change_pick(di, n, ch->d_sums, ch->d_state, ch->d_prev, ch->d_recs, ch->cfg, zf, desc, tab, plan, K, s), ZLY_ERR_INFERENCE);
    HIP_TRY(ch->ring.mark(r, s), ZLY_ERR_INFERENCE);
    return ZLY_OK;
}

// The body of zly_change_device_view and zly_change_surfaces: the n views of the source.  Under e->mu, e->change set; takes the enqueue gate itself.
// Every check comes first: a refused call enqueues nothing.  *ran_on (if asked for): the stream the kernels went to.
static int change_locked(zly_engine* e, int32_t n, const FrameSource& f, const int32_t* streams, void* stream, hipStream_t* ran_on = nullptr)
{
    Change* ch = e->change;
    if (int rc = change_check_streams(n, streams, ch->max_streams, &g_last_error)) return rc;
    for (int i = 0; i < n; ++i) {
        if (int rc = chip_check_view(e->cfg.flags, f.base, f.bytes, &f.v[i], &g_last_error)) return rc;
        if (int rc = change_check_size(f.v[i].w, f.v[i].h, ch->cfg.cell, &g_last_error)) return rc;
    }
    SharedGate gl;
    HIP_TRY(hipSetDevice(e->dev), ZLY_ERR_SYSTEM);
    hipStream_t s = nullptr;
    if (int rc = call_stream(e, stream, &s, f.wait_for)) return rc;
    int r = 0;
    if (int rc = change_enqueue_sums(e, ch, n, f.base, f.v, streams, s, &r)) return rc;
    if (int rc = change_enqueue_pick(e, ch, n, r, nullptr, nullptr, nullptr, nullptr, 0, s)) return rc;
    if (ran_on) *ran_on = s;
    return ZLY_OK;
}

int32_t zly_change_device_view(zly_engine* e, int32_t n, const void* d_base, size_t buf_bytes, const zly_frame_view* views, const int32_t* streams, void* stream)
{
    if (!e) return fail(ZLY_ERR_NOT_INITIALIZED, "Engine not running");
    if (int rc = change_check_call(n, e->cfg.max_batch, views, streams, &g_last_error)) return rc;
    std::lock_guard<std::mutex> lk(e->mu);
    if (!change_of(e)) return ZLY_ERR_INVALID_ARGUMENT;
    return change_locked(e, n, FrameSource{d_base, buf_bytes, views}, streams, stream);
}

int32_t zly_change_surfaces(zly_engine* e, int32_t n, const int32_t* surfaces, const int32_t* streams, void* stream)
{
    if (!e) return fail(ZLY_ERR_NOT_INITIALIZED, "Engine not running");
    if (int rc = change_check_call(n, e->cfg.max_batch, surfaces, streams, &g_last_error)) return rc;
    std::lock_guard<std::mutex> lk(e->mu);
    if (!change_of(e)) return ZLY_ERR_INVALID_ARGUMENT;
    StoreFrames src;
    if (int rc = src.open(e)) return rc;
    if (int rc = src.frames(n, surfaces)) return rc;
    return src.read_by([&](const FrameSource& f, hipStream_t* ran) { return change_locked(e, n, f, streams, stream, ran); });
}

int32_t zly_change_read(zly_engine* e, int32_t stream, void* host_out, size_t cap_bytes)
{
    if (!e) return fail(ZLY_ERR_NOT_INITIALIZED, "Engine not running");
    if (!host_out) return fail(ZLY_ERR_INVALID_ARGUMENT, "null output");
    std::lock_guard<std::mutex> lk(e->mu);
    Change* ch = change_of(e);
    if (!ch) return ZLY_ERR_INVALID_ARGUMENT;
    if (stream < 0 || stream >= ch->max_streams) return fail(ZLY_ERR_INVALID_ARGUMENT, "stream " + std::to_string(stream) + " out of range");
    if (cap_bytes < (size_t)ch->lay.activity_off) return fail(ZLY_ERR_INVALID_ARGUMENT, "zly_change_read: the header and the peaks are " + std::to_string(ch->lay.activity_off) + " bytes");
    return read_back(e, behind_ring(ch->ring), {{host_out, ch->d_recs + (size_t)stream * (size_t)ch->lay.rec_bytes, std::min(cap_bytes, (size_t)ch->lay.rec_bytes)}});
}

int32_t zly_change_reset(zly_engine* e, int32_t stream)
{
    if (!e) return fail(ZLY_ERR_NOT_INITIALIZED, "Engine not running");
    std::lock_guard<std::mutex> lk(e->mu);
    Change* ch = change_of(e);
    if (!ch) return ZLY_ERR_INVALID_ARGUMENT;
    if (stream < -1 || stream >= ch->max_streams) return fail(ZLY_ERR_INVALID_ARGUMENT, "stream " + std::to_string(stream) + " out of range");
    HIP_TRY(hipSetDevice(e->dev), ZLY_ERR_SYSTEM);
    SharedGate gl;
    // a ring entry of its own orders the reset among the change calls: behind the last one, in front of the next
    int r = 0;
    HIP_TRY(ch->ring.claim(&r), ZLY_ERR_INFERENCE);
    HIP_TRY(ch->ring.wait_last(e->stream), ZLY_ERR_INFERENCE);
    HIP_TRY(hipMemsetAsync(ch->d_state + (stream < 0 ? 0 : stream), 0, sizeof(ChangeStream) * (size_t)(stream < 0 ? ch->max_streams : 1), e->stream), ZLY_ERR_INFERENCE);
    HIP_TRY(ch->ring.mark(r, e->stream), ZLY_ERR_INFERENCE);
    return ZLY_OK;
}

// --- camera motion (include/zly.h "Camera motion"; the rules: camera_rules.h; the kernels: kernels_camera.hip) ---------
void zly_default_camera_config(zly_camera_config* c)
{
    if (!c) return;
    camera_default_config(c);
}

int32_t zly_camera_enable(zly_engine* e, const zly_camera_config* c, int32_t max_streams)
{
    if (!e) return fail(ZLY_ERR_NOT_INITIALIZED, "Engine not running");
    if (int rc = camera_check_config(c, max_streams, &g_last_error)) return rc;
    std::lock_guard<std::mutex> lk(e->mu);
    if (e->camera) return fail(ZLY_ERR_INVALID_ARGUMENT, "camera motion is already enabled on this engine");
    ExclusiveGate gl;                                  // allocations: alone in the process
    HIP_TRY(hipSetDevice(e->dev), ZLY_ERR_SYSTEM);
    Camera* cm = new Camera();
    cm->cfg = *c;
    cm->lay = camera_layout();
    cm->max_streams = max_streams;
    const size_t B = (size_t)e->cfg.max_batch, NS = (size_t)max_streams, grid = sizeof(uint32_t) * ZLY_CHANGE_MAX_CELLS;
    // both arrays 16-byte aligned in every entry
    static_assert(sizeof(CameraItem) == 16 && alignof(ChipFrame) <= 16 && alignof(CameraItem) <= 16, "the entry's layout assumes 16-byte items");
    cm->items_off = (sizeof(ChipFrame) * B + 15) / 16 * 16;
    bool ok = cm->ring.create(std::max(cm->items_off + sizeof(CameraItem) * B, sizeof(int32_t) * NS)) == hipSuccess &&
              hipMalloc((void**)&cm->d_sums, grid * B) == hipSuccess &&
              hipMalloc((void**)&cm->d_state, sizeof(CameraStream) * NS) == hipSuccess &&
              hipMalloc((void**)&cm->d_prev, grid * NS) == hipSuccess &&
              hipMalloc((void**)&cm->d_recs, (size_t)cm->lay.rec_bytes * NS) == hipSuccess &&
              hipMemset(cm->d_sums, 0, grid * B) == hipSuccess &&
              hipMemset(cm->d_state, 0, sizeof(CameraStream) * NS) == hipSuccess &&
              hipMemset(cm->d_prev, 0, grid * NS) == hipSuccess &&
              hipMemset(cm->d_recs, 0, (size_t)cm->lay.rec_bytes * NS) == hipSuccess &&
              hipDeviceSynchronize() == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        (void)camera_free(cm);
        return fail(ZLY_ERR_SYSTEM, "allocation of the camera motion's buffers failed");
    }
    e->camera = cm;
    return ZLY_OK;
}

int32_t zly_camera_layout(const zly_engine* e, size_t* rec_bytes, size_t* sad_off, size_t* sad_room)
{
    if (!e) return fail(ZLY_ERR_NOT_INITIALIZED, "Engine not running");
    std::lock_guard<std::mutex> lk(const_cast<zly_engine*>(e)->mu);
    const Camera* cm = enabled(e->camera, NO_CAMERA);
    if (!cm) return ZLY_ERR_INVALID_ARGUMENT;
    if (rec_bytes) *rec_bytes = (size_t)cm->lay.rec_bytes;
    if (sad_off) *sad_off = (size_t)cm->lay.sad_off;
    if (sad_room) *sad_room = (size_t)cm->lay.sad_room;
    return ZLY_OK;
}

// The body of zly_camera_device_view and zly_camera_surfaces: the n views of the source.  Under e->mu, e->camera set; takes the enqueue gate itself.
// Every check comes first: a refused call enqueues nothing.  *ran_on (if asked for): the stream the kernels went to.
static int camera_locked(zly_engine* e, int32_t n, const FrameSource& f, const int32_t* streams, void* stream, hipStream_t* ran_on = nullptr)
{
    Camera* cm = e->camera;
    if (int rc = camera_check_streams(n, streams, cm->max_streams, cm->max_streams, &g_last_error)) return rc;
    for (int i = 0; i < n; ++i) {
        if (int rc = chip_check_view(e->cfg.flags, f.base, f.bytes, &f.v[i], &g_last_error)) return rc;
        if (int rc = camera_check_size(f.v[i].w, f.v[i].h, cm->cfg.cell, cm->cfg.radius, &g_last_error)) return rc;
    }
    SharedGate gl;
    HIP_TRY(hipSetDevice(e->dev), ZLY_ERR_SYSTEM);
    hipStream_t s = nullptr;
    if (int rc = call_stream(e, stream, &s, f.wait_for)) return rc;
    int r = 0;
    HIP_TRY(cm->ring.claim_behind_last(s, &r), ZLY_ERR_INFERENCE);      // behind the camera calls so far: they share scratch grids, states and records
    const int rc = [&]() -> int {
        ChipFrame* hf = cm->ring.host<ChipFrame>(r);
        CameraItem* hi = cm->items(cm->ring.host<unsigned char>(r));
        int max_w = 1, max_h = 1;
        for (int i = 0; i < n; ++i) {
            hf[i] = chip_frame_of(&f.v[i]);
            hi[i] = CameraItem{f.v[i].w, f.v[i].h, streams[i], 0};
            max_w = std::max(max_w, (int)f.v[i].w); max_h = std::max(max_h, (int)f.v[i].h);
        }
        // one copy: the frame records (all max_batch of the entry; the n first matter) and the n items behind them
        HIP_TRY(cm->ring.upload(r, cm->items_off + sizeof(CameraItem) * (size_t)n, s), ZLY_ERR_INFERENCE);
        HIP_TRY(launch_change_sums((const uint8_t*)f.base, cm->ring.dev<ChipFrame>(r), n, max_w, max_h, cm->cfg.cell, cm->d_sums, s), ZLY_ERR_INFERENCE);
        HIP_TRY(launch_camera(cm->items(cm->ring.dev<unsigned char>(r)), n, cm->d_sums, cm->d_state, cm->d_prev, cm->d_recs, cm->cfg, s), ZLY_ERR_INFERENCE);
        return ZLY_OK;
    }();
    // the entry's event goes behind whatever has been enqueued, a failed call's too: the next camera call, on whichever stream, is ordered behind it
    if (cm->ring.mark(r, s) != hipSuccess && rc == ZLY_OK) return fail(ZLY_ERR_INFERENCE, "hipEventRecord failed behind the camera motion's kernels");
    if (ran_on) *ran_on = s;
    return rc;
}

int32_t zly_camera_device_view(zly_engine* e, int32_t n, const void* d_base, size_t buf_bytes, const zly_frame_view* views, const int32_t* streams, void* stream)
{
    if (!e) return fail(ZLY_ERR_NOT_INITIALIZED, "Engine not running");
    if (int rc = camera_check_call(n, e->cfg.max_batch, views, streams, &g_last_error)) return rc;
    std::lock_guard<std::mutex> lk(e->mu);
    if (!camera_of(e)) return ZLY_ERR_INVALID_ARGUMENT;
    return camera_locked(e, n, FrameSource{d_base, buf_bytes, views}, streams, stream);
}

int32_t zly_camera_surfaces(zly_engine* e, int32_t n, const int32_t* surfaces, const int32_t* streams, void* stream)
{
    if (!e) return fail(ZLY_ERR_NOT_INITIALIZED, "Engine not running");
    if (int rc = camera_check_call(n, e->cfg.max_batch, surfaces, streams, &g_last_error)) return rc;
    std::lock_guard<std::mutex> lk(e->mu);
    if (!camera_of(e)) return ZLY_ERR_INVALID_ARGUMENT;
    StoreFrames src;
    if (int rc = src.open(e)) return rc;
    if (int rc = src.frames(n, surfaces)) return rc;
    return src.read_by([&](const FrameSource& f, hipStream_t* ran) { return camera_locked(e, n, f, streams, stream, ran); });
}

int32_t zly_camera_read(zly_engine* e, int32_t stream, void* host_out, size_t cap_bytes)
{
    if (!e) return fail(ZLY_ERR_NOT_INITIALIZED, "Engine not running");
    if (!host_out) return fail(ZLY_ERR_INVALID_ARGUMENT, "null output");
    std::lock_guard<std::mutex> lk(e->mu);
    Camera* cm = camera_of(e);
    if (!cm) return ZLY_ERR_INVALID_ARGUMENT;
    if (stream < 0 || stream >= cm->max_streams) return fail(ZLY_ERR_INVALID_ARGUMENT, "stream " + std::to_string(stream) + " out of range");
    if (cap_bytes < (size_t)cm->lay.sad_off) return fail(ZLY_ERR_INVALID_ARGUMENT, "zly_camera_read: the header is " + std::to_string(cm->lay.sad_off) + " bytes");
    return read_back(e, behind_ring(cm->ring), {{host_out, cm->d_recs + (size_t)stream * (size_t)cm->lay.rec_bytes, std::min(cap_bytes, (size_t)cm->lay.rec_bytes)}});
}

int32_t zly_camera_reset(zly_engine* e, int32_t stream)
{
    if (!e) return fail(ZLY_ERR_NOT_INITIALIZED, "Engine not running");
    std::lock_guard<std::mutex> lk(e->mu);
    Camera* cm = camera_of(e);
    if (!cm) return ZLY_ERR_INVALID_ARGUMENT;
    if (stream < -1 || stream >= cm->max_streams) return fail(ZLY_ERR_INVALID_ARGUMENT, "stream " + std::to_string(stream) + " out of range");
    HIP_TRY(hipSetDevice(e->dev), ZLY_ERR_SYSTEM);
    SharedGate gl;
    // a ring entry of its own orders the reset among the camera calls: behind the last one, in front of the next
    int r = 0;
    HIP_TRY(cm->ring.claim_behind_last(e->stream, &r), ZLY_ERR_INFERENCE);
    const hipError_t le = launch_camera_reset(cm->d_state, cm->d_recs, stream < 0 ? 0 : stream, stream < 0 ? cm->max_streams : 1, e->stream);
    HIP_TRY(cm->ring.mark(r, e->stream), ZLY_ERR_INFERENCE);
    HIP_TRY(le, ZLY_ERR_INFERENCE);
    return ZLY_OK;
}

int32_t zly_camera_apply_tracks(zly_engine* e, int32_t n, const int32_t* streams, void* stream)
{
    if (!e) return fail(ZLY_ERR_NOT_INITIALIZED, "Engine not running");
    if (!streams) return fail(ZLY_ERR_INVALID_ARGUMENT, "null streams");
    std::lock_guard<std::mutex> lk(e->mu);
    Camera* cm = camera_of(e);
    if (!cm) return ZLY_ERR_INVALID_ARGUMENT;
    Track* tk = track_of(e);
    if (!tk) return ZLY_ERR_INVALID_ARGUMENT;
    if (n < 1 || n > cm->max_streams) return fail(ZLY_ERR_INVALID_ARGUMENT, "zly_camera_apply_tracks: n must lie in 1.." + std::to_string(cm->max_streams));
    if (int rc = camera_check_streams(n, streams, cm->max_streams, tk->cfg.max_streams, &g_last_error)) return rc;
    SharedGate gl;
    HIP_TRY(hipSetDevice(e->dev), ZLY_ERR_SYSTEM);
    hipStream_t s = nullptr;
    if (int rc = call_stream(e, stream, &s)) return rc;
    // behind the camera calls (the entry) and the tracked calls (the track ring's last mark) enqueued so far, on whichever streams they ran
    int r = 0, tr = 0;
    HIP_TRY(cm->ring.claim_behind_last(s, &r), ZLY_ERR_INFERENCE);      // behind the camera calls so far: they share scratch grids, states and records
    const int rc = [&]() -> int {
        HIP_TRY(tk->ring.wait_last(s), ZLY_ERR_INFERENCE);
        memcpy(cm->ring.host<int32_t>(r), streams, sizeof(int32_t) * (size_t)n);
        HIP_TRY(cm->ring.upload(r, sizeof(int32_t) * (size_t)n, s), ZLY_ERR_INFERENCE);
        HIP_TRY(launch_camera_apply(cm->ring.dev<int>(r), n, cm->d_state, cm->d_recs, tk->d_state, tk->cfg.max_tracks, s), ZLY_ERR_INFERENCE);
        // ... and ahead of every later one: an entry of the track ring, not filled, is marked behind the kernel -- the tracking kernels of an engine
        // with this feature (track_enqueue), the zoom plan and zly_track_read all go behind the ring's last mark
        HIP_TRY(tk->ring.claim(&tr), ZLY_ERR_INFERENCE);
        HIP_TRY(tk->ring.mark(tr, s), ZLY_ERR_INFERENCE);
        return ZLY_OK;
    }();
    if (cm->ring.mark(r, s) != hipSuccess && rc == ZLY_OK) return fail(ZLY_ERR_INFERENCE, "hipEventRecord failed behind the camera motion's apply kernel");
    return rc;
}

// --- zoom regions (include/zly.h "Zoom regions"; the rules: zoom_rules.h; the plan kernel: kernels_zoom.hip) -----------
void zly_default_zoom_config(const zly_engine* e, zly_zoom_config* c)
{
    if (!c) return;
    c->regions = 3;               // chosen, not tuned
    c->region_w = e ? e->cfg.model_w & ~1 : 416;      // 1:1 with the model: the front kernel's resize is the identity
    c->region_h = e ? e->cfg.model_h & ~1 : 416;
    c->max_age = 2;
    c->class_id = -1;
}

int32_t zly_zoom_enable(zly_engine* e, const zly_zoom_config* c)
{
    if (!e) return fail(ZLY_ERR_NOT_INITIALIZED, "Engine not running");
    if (int rc = zoom_check_config(c, &g_last_error)) return rc;
    if (!track_of(e)) return ZLY_ERR_INVALID_ARGUMENT;
    if ((int64_t)(1 + c->regions) * e->cfg.max_dets > ZLY_MERGE_MAX_CANDIDATES)
        return fail(ZLY_ERR_INVALID_ARGUMENT, "(1 + regions) x max_dets exceeds ZLY_MERGE_MAX_CANDIDATES");
    if (1 + c->regions > e->cfg.max_batch) return fail(ZLY_ERR_INVALID_ARGUMENT, "1 + regions exceeds max_batch (" + std::to_string(e->cfg.max_batch) + ")");
    std::lock_guard<std::mutex> lk(e->mu);
    if (e->zoom) return fail(ZLY_ERR_INVALID_ARGUMENT, "zoom regions are already enabled on this engine");
    ExclusiveGate gl;                                  // allocations: alone in the process
    HIP_TRY(hipSetDevice(e->dev), ZLY_ERR_SYSTEM);
    Zoom* zm = new Zoom();
    zm->cfg = *c;
    const size_t B = (size_t)e->cfg.max_batch, n_plan = B + B * (size_t)c->regions;
    const bool ok = zm->ring.create(sizeof(ZoomFrame) * B) == hipSuccess &&
                    hipMalloc((void**)&zm->d_plan, sizeof(zly_zoom_region) * n_plan) == hipSuccess &&
                    hipMemset(zm->d_plan, 0, sizeof(zly_zoom_region) * n_plan) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        (void)zoom_free(zm);
        return fail(ZLY_ERR_SYSTEM, "allocation of the zoom plan buffers failed");
    }
    e->zoom = zm;
    return ZLY_OK;
}

// Uploads the n frame records of a plan in the next ring entry and launches zoom_plan_kernel on `s`, behind the tracking enqueued so far on whichever
// stream that ran.  desc / tab: what the kernel patches (null: the plan alone).  Under e->mu, enqueue gate held.
static int zoom_enqueue_plan(zly_engine* e, Zoom* zm, Track* tk, int n, const ZoomFrame* zf, FrameDesc* desc, int* tab, zly_zoom_region* d_plan, hipStream_t s, int* ring)
{
    HIP_TRY(tk->ring.wait_last(s), ZLY_ERR_INFERENCE);                               // the most recent tracked launch
    int r = 0;
    HIP_TRY(zm->ring.claim(&r), ZLY_ERR_INFERENCE);
    memcpy(zm->ring.host<ZoomFrame>(r), zf, sizeof(ZoomFrame) * (size_t)n);
    HIP_TRY(zm->ring.upload(r, sizeof(ZoomFrame) * (size_t)n, s), ZLY_ERR_INFERENCE);
    HIP_TRY(launch_zoom_plan(tk->d_state, tk->d_motion, zm->ring.dev<ZoomFrame>(r), n, desc, tab, d_plan, zm->cfg.regions, tk->cfg.max_tracks, zm->cfg.region_w,
                             zm->cfg.region_h, zm->cfg.max_age, zm->cfg.class_id, s), ZLY_ERR_INFERENCE);
    HIP_TRY(zm->ring.mark(r, s), ZLY_ERR_INFERENCE);
    *ring = r;
    return ZLY_OK;
}

// The body of zly_detect_device_zoom and zly_detect_surfaces_zoom: n surfaces that are the views of the source.  Under e->mu, e->zoom set; takes the
// enqueue gate itself.  Every check comes first: a refused call enqueues nothing.  *ran_on (if asked for): the stream the call's last kernel went to.
static int detect_zoom_locked(zly_engine* e, int32_t n, const FrameSource& f, const int32_t* streams, const zly_merge_config* mc, void* d_out, uint32_t frame_tag0,
                              void* stream, hipStream_t* ran_on = nullptr)
{
    const zly_frame_view* sv = f.v;
    Zoom* zm = e->zoom;
    Track* tk = e->track.load();
    const int K = zm->cfg.regions, V = 1 + K, nb = n * V;
    for (int i = 0; i < n; ++i) {
        if (streams[i] < 0 || streams[i] >= tk->cfg.max_streams) return fail(ZLY_ERR_INVALID_ARGUMENT, "stream " + std::to_string(streams[i]) + " out of range (a zoomed frame names a stream)");
        for (int k = 0; k < i; ++k)
            if (streams[k] == streams[i]) return fail(ZLY_ERR_INVALID_ARGUMENT, "stream " + std::to_string(streams[i]) + " occurs twice in a zoom call");
    }
    if (d_out && d_out == (void*)e->d_slabs) return fail(ZLY_ERR_INVALID_ARGUMENT, "d_out must not be the engine's own slab buffer");
    Change* ch = e->change && e->change->zoom_on ? e->change : nullptr;      // zly_zoom_use_change: the fallback regions follow the change map
    if (ch)
        if (int rc = change_check_streams(n, streams, ch->max_streams, &g_last_error)) return rc;
    FrameTable t(nb, true);                                                          // the n x (1 + K) views of the batch: frame i's surface, then its regions
    std::vector<zly_tile> tiles((size_t)nb);
    std::vector<ZoomFrame> zf((size_t)n);
    for (int i = 0; i < n; ++i) {
        if (int rc = zoom_check_surface(&sv[i], &g_last_error)) return rc;
        if (int rc = check_view(e->cfg.flags, f.base, f.bytes, &sv[i], &g_last_error)) return rc;
        const int32_t W = sv[i].w, H = sv[i].h;
        const ZoomSize z = zoom_size(zm->cfg.region_w, zm->cfg.region_h, W, H);
        const int32_t fx = zoom_fallback_origin(W, z.rw), fy = zoom_fallback_origin(H, z.rh);
        t.add(sv[i]);
        tiles[(size_t)i * V] = zly_tile{i, 0, 0, W, H, W, H};
        for (int j = 1; j <= K; ++j) {                                              // every region at its fallback origin: the kernel patches what depends on the origin
            zly_frame_view rv;
            if (int rc = view_crop(&sv[i], fx, fy, z.rw, z.rh, &rv, &g_last_error)) return rc;
            if (int rc = check_view(e->cfg.flags, f.base, f.bytes, &rv, &g_last_error)) return rc;
            t.add(rv);
            tiles[(size_t)i * V + j] = zly_tile{i, fx, fy, z.rw, z.rh, W, H};
        }
        zf[(size_t)i] = zoom_frame_of(&sv[i], streams[i]);
        if (ch)
            if (int rc = change_check_size(W, H, ch->cfg.cell, &g_last_error)) return rc;
    }
    int max_slots = 0;
    if (int rc = merge_check(e, nb, tiles.data(), n, mc, &max_slots)) return rc;
    if (int rc = merge_ensure(e)) return rc;
    SharedGate gl;
    HIP_TRY(hipSetDevice(e->dev), ZLY_ERR_SYSTEM);
    hipStream_t s = nullptr;
    if (int rc = call_stream(e, stream, &s, f.wait_for)) return rc;
    // the three tables the plan kernel patches go up first, on the call's stream; what set_desc remembers of d_desc is void from here on: a kernel writes it
    int rc = set_desc(e, t, s);
    e->desc_cache.clear(); e->view_cache.clear(); e->last_desc_n = 0;
    if (rc != ZLY_OK) return rc;
    int mr = 0, zr = 0;
    if ((rc = merge_upload(e, nb, tiles.data(), n, s, &mr)) != ZLY_OK) return rc;
    int cr = 0;
    if (ch && (rc = change_enqueue_sums(e, ch, n, f.base, sv, streams, s, &cr)) != ZLY_OK) return rc;
    int* d_tab = e->merge->ring.dev<int>(mr);
    if ((rc = zoom_enqueue_plan(e, zm, tk, n, zf.data(), e->d_desc, d_tab, zm->d_plan, s, &zr)) != ZLY_OK) return rc;
    if (ch && (rc = change_enqueue_pick(e, ch, n, cr, zm->ring.dev<ZoomFrame>(zr), e->d_desc, d_tab, zm->d_plan, zm->cfg.regions, s)) != ZLY_OK) return rc;
    if (ch) HIP_TRY(zm->ring.mark(zr, s), ZLY_ERR_INFERENCE);      // zly_zoom_read_plan reads the plan as the pick kernel left it
    zm->last_frames = zr; zm->last_n = n;
    // the nb views counted; no completion event yet: the call's events go behind its tracking, below
    if ((rc = detect_run(e, t, f.base, nullptr, 0, s, false)) != ZLY_OK) return rc;
    const hipStream_t ns = e->last_ns;
    // merge, then track, on the stream the NMS ran on -- where zly_merge_slabs and zly_track_slabs would put them
    void* dst = d_out ? d_out : (void*)e->merge->d_out;
    if ((rc = merge_launch(e, mr, n, mc, max_slots, e->d_slabs, dst, frame_tag0, ns)) != ZLY_OK) return rc;
    bool launched = false;
    if ((rc = track_enqueue(e, tk, n, streams, dst, ns, &launched)) != ZLY_OK) return rc;
    // the call's completion events lie behind its tracking: zly_join, zly_read_slabs, zly_read_merged and a later call's NMS wait for all of it
    if ((rc = detect_events_behind(e, ns)) != ZLY_OK) return rc;
    HIP_TRY(e->merge->ring.mark(mr, ns), ZLY_ERR_INFERENCE);
    if (ran_on) *ran_on = ns;
    return ZLY_OK;
}

// the argument checks the two frame entries share, in front of the lock
static int zoom_check_call(const zly_engine* e, int32_t n, const void* frames, const int32_t* streams, const zly_merge_config* mc)
{
    if (!frames) return fail(ZLY_ERR_INVALID_ARGUMENT, "null surfaces");
    if (!streams) return fail(ZLY_ERR_INVALID_ARGUMENT, "null streams");
    if (!mc) return fail(ZLY_ERR_INVALID_ARGUMENT, "null merge config");
    if (n < 1 || n > e->cfg.max_batch) return fail(ZLY_ERR_INVALID_ARGUMENT, "batch size out of range");
    return ZLY_OK;
}

int32_t zly_detect_device_zoom(zly_engine* e, int32_t n, const void* d_base, size_t buf_bytes, const zly_frame_view* surface_views, const int32_t* streams,
                               const zly_merge_config* merge_cfg, void* d_out, uint32_t frame_tag0, void* stream)
{
    if (!e) return fail(ZLY_ERR_NOT_INITIALIZED, "Engine not running");
    if (int rc = zoom_check_call(e, n, surface_views, streams, merge_cfg)) return rc;
    std::lock_guard<std::mutex> lk(e->mu);
    Zoom* zm = zoom_of(e);
    if (!zm) return ZLY_ERR_INVALID_ARGUMENT;
    if ((int64_t)n * (1 + zm->cfg.regions) > e->cfg.max_batch) return fail(ZLY_ERR_INVALID_ARGUMENT, "n x (1 + regions) exceeds max_batch");
    return detect_zoom_locked(e, n, FrameSource{d_base, buf_bytes, surface_views}, streams, merge_cfg, d_out, frame_tag0, stream);
}

int32_t zly_detect_surfaces_zoom(zly_engine* e, int32_t n, const int32_t* surfaces, const int32_t* streams, const zly_merge_config* merge_cfg, void* d_out,
                                 uint32_t frame_tag0, void* stream)
{
    if (!e) return fail(ZLY_ERR_NOT_INITIALIZED, "Engine not running");
    if (int rc = zoom_check_call(e, n, surfaces, streams, merge_cfg)) return rc;
    std::lock_guard<std::mutex> lk(e->mu);
    StoreFrames src;
    if (int rc = src.open(e)) return rc;                                // the store before the feature: the other store entries ask the other way round
    Zoom* zm = zoom_of(e);
    if (!zm) return ZLY_ERR_INVALID_ARGUMENT;
    if ((int64_t)n * (1 + zm->cfg.regions) > e->cfg.max_batch) return fail(ZLY_ERR_INVALID_ARGUMENT, "n x (1 + regions) exceeds max_batch");
    if (int rc = src.frames(n, surfaces)) return rc;
    return src.read_by([&](const FrameSource& f, hipStream_t* ran) { return detect_zoom_locked(e, n, f, streams, merge_cfg, d_out, frame_tag0, stream, ran); });
}

int32_t zly_zoom_plan(zly_engine* e, int32_t n, const int32_t* W, const int32_t* H, const int32_t* streams, zly_zoom_region* out)
{
    if (!e) return fail(ZLY_ERR_NOT_INITIALIZED, "Engine not running");
    if (!W || !H || !streams || !out) return fail(ZLY_ERR_INVALID_ARGUMENT, "null argument");
    if (n < 1 || n > e->cfg.max_batch) return fail(ZLY_ERR_INVALID_ARGUMENT, "batch size out of range");
    std::lock_guard<std::mutex> lk(e->mu);
    Zoom* zm = zoom_of(e);
    if (!zm) return ZLY_ERR_INVALID_ARGUMENT;
    Track* tk = e->track.load();
    std::vector<ZoomFrame> zf((size_t)n);
    for (int i = 0; i < n; ++i) {
        if (W[i] < 2 || H[i] < 2 || W[i] >= (1 << 24) || H[i] >= (1 << 24)) return fail(ZLY_ERR_INVALID_ARGUMENT, "a zoomed surface must be 2..2^24-1 pixels on a side");
        if (streams[i] < 0 || streams[i] >= tk->cfg.max_streams) return fail(ZLY_ERR_INVALID_ARGUMENT, "stream " + std::to_string(streams[i]) + " out of range");
        ZoomFrame z{};
        z.W = W[i]; z.H = H[i]; z.stream = streams[i]; z.planes = 1;
        zf[(size_t)i] = z;
    }
    zly_zoom_region* d_plan = zm->d_plan + (size_t)e->cfg.max_batch;               // its own records: zly_zoom_read_plan keeps the last frame call's
    int zr = 0;
    // `behind` is the plan kernel itself here, no wait: the copy goes behind it in the engine stream's own order
    return read_back(e, [&](hipStream_t s) { return zoom_enqueue_plan(e, zm, tk, n, zf.data(), nullptr, nullptr, d_plan, s, &zr); },
                     {{out, d_plan, sizeof(zly_zoom_region) * (size_t)n * (size_t)zm->cfg.regions}});
}

int32_t zly_zoom_read_plan(zly_engine* e, int32_t n, zly_zoom_region* out)
{
    if (!e) return fail(ZLY_ERR_NOT_INITIALIZED, "Engine not running");
    if (!out) return fail(ZLY_ERR_INVALID_ARGUMENT, "null output");
    std::lock_guard<std::mutex> lk(e->mu);
    Zoom* zm = zoom_of(e);
    if (!zm) return ZLY_ERR_INVALID_ARGUMENT;
    if (zm->last_frames < 0 || n != zm->last_n) return fail(ZLY_ERR_INVALID_ARGUMENT, "zly_zoom_read_plan: n must be the frames of the most recent zoom call");
    auto behind = [&](hipStream_t s) -> int {                            // the frame call's own entry, not wait_last: zly_zoom_plan marks entries too
        HIP_TRY(hipStreamWaitEvent(s, zm->ring.ev[zm->last_frames], 0), ZLY_ERR_INFERENCE);
        return ZLY_OK;
    };
    return read_back(e, behind, {{out, zm->d_plan, sizeof(zly_zoom_region) * (size_t)n * (size_t)zm->cfg.regions}});
}

int32_t zly_zoom_use_change(zly_engine* e, int32_t on)
{
    if (!e) return fail(ZLY_ERR_NOT_INITIALIZED, "Engine not running");
    std::lock_guard<std::mutex> lk(e->mu);
    Zoom* zm = zoom_of(e);
    if (!zm) return ZLY_ERR_INVALID_ARGUMENT;
    Change* ch = change_of(e);
    if (!ch) return ZLY_ERR_INVALID_ARGUMENT;
    if (ch->cfg.window_w != zm->cfg.region_w || ch->cfg.window_h != zm->cfg.region_h)
        return fail(ZLY_ERR_INVALID_ARGUMENT, "zly_zoom_use_change: the change map's window (" + std::to_string(ch->cfg.window_w) + " x " + std::to_string(ch->cfg.window_h) +
                                              ") must be the zoom region (" + std::to_string(zm->cfg.region_w) + " x " + std::to_string(zm->cfg.region_h) + ")");
    ch->zoom_on = on != 0;
    return ZLY_OK;
}

// --- chips (include/zly.h "Chips"; the rules: chip_rules.h; the kernels: kernels_chips.hip) -----------------------------
void zly_default_chip_config(const zly_engine* e, zly_chip_config* c)
{
    if (!c) return;
    chip_default_config(e ? e->cfg.max_dets : 16, c);
}

int32_t zly_chips_enable(zly_engine* e, const zly_chip_config* c)
{
    if (!e) return fail(ZLY_ERR_NOT_INITIALIZED, "Engine not running");
    if (int rc = chip_check_config(c, e->cfg.max_dets, &g_last_error)) return rc;
    std::lock_guard<std::mutex> lk(e->mu);
    if (e->chips) return fail(ZLY_ERR_INVALID_ARGUMENT, "chips are already enabled on this engine");
    ExclusiveGate gl;                                  // allocations: alone in the process
    HIP_TRY(hipSetDevice(e->dev), ZLY_ERR_SYSTEM);
    Chips* cp = new Chips();
    cp->cfg = *c;
    cp->lay = chip_layout(c->chip_w, c->chip_h, c->max_chips, c->layout == ZLY_CHIP_RGB_F32);
    const size_t B = (size_t)e->cfg.max_batch;
    const bool ok = cp->ring.create(sizeof(ChipFrame) * B) == hipSuccess &&
                    hipMalloc((void**)&cp->d_out, (size_t)cp->lay.slab_bytes * B) == hipSuccess &&
                    hipMemset(cp->d_out, 0, (size_t)cp->lay.slab_bytes * B) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        (void)chips_free(cp);
        return fail(ZLY_ERR_SYSTEM, "allocation of the chip buffers failed");
    }
    e->chips = cp;
    return ZLY_OK;
}

int32_t zly_chip_layout(const zly_engine* e, size_t* slab_bytes, size_t* pixels_off, size_t* chip_stride)
{
    if (!e) return fail(ZLY_ERR_NOT_INITIALIZED, "Engine not running");
    const Chips* cp = enabled(e->chips, NO_CHIPS);
    if (!cp) return ZLY_ERR_INVALID_ARGUMENT;
    if (slab_bytes) *slab_bytes = (size_t)cp->lay.slab_bytes;
    if (pixels_off) *pixels_off = (size_t)cp->lay.pixels_off;
    if (chip_stride) *chip_stride = (size_t)cp->lay.chip_stride;
    return ZLY_OK;
}

// The body of zly_chips_device_view and zly_chips_surfaces: the n views of the source.  Under e->mu, e->chips set; takes the enqueue gate itself.
// *ran_on (if asked for): the stream the kernels went to.
static int chips_locked(zly_engine* e, int32_t n, const FrameSource& f, const void* d_slabs, int32_t source, void* d_chips, void* stream, hipStream_t* ran_on = nullptr)
{
    Chips* cp = e->chips;
    if (!d_slabs && source == ZLY_CHIPS_SRC_MERGED && !e->merge) return fail(ZLY_ERR_INVALID_ARGUMENT, std::string("ZLY_CHIPS_SRC_MERGED: ") + NO_MERGE);
    std::vector<ChipFrame> cf((size_t)n);
    for (int i = 0; i < n; ++i) {
        if (int rc = chip_check_view(e->cfg.flags, f.base, f.bytes, &f.v[i], &g_last_error)) return rc;
        cf[(size_t)i] = chip_frame_of(&f.v[i]);
    }
    const void* slabs = d_slabs ? d_slabs : source == ZLY_CHIPS_SRC_MERGED ? (const void*)e->merge->d_out : (const void*)e->d_slabs;
    SharedGate gl;
    HIP_TRY(hipSetDevice(e->dev), ZLY_ERR_SYSTEM);
    // behind the NMS, merge and tracking of the most recent zly_detect_device* call, on whichever stream they ran: the stream chosen there is the one
    // that waits for the source
    hipStream_t s = nullptr;
    if (int rc = call_stream(e, stream, &s)) return rc;
    if (int rc = stream_after_detect(e, s)) return rc;
    if (int rc = wait_if_foreign(e, s, f.wait_for)) return rc;
    // merges of an engine made before any detect call (slabs made elsewhere) are ordered by their own ring event
    if (!d_slabs && source == ZLY_CHIPS_SRC_MERGED) HIP_TRY(e->merge->ring.wait_last(s), ZLY_ERR_INFERENCE);
    int r = 0;
    HIP_TRY(cp->ring.claim(&r), ZLY_ERR_INFERENCE);
    // chip calls of an engine are ordered among themselves: they may share the engine-owned output
    HIP_TRY(cp->ring.wait_last(s), ZLY_ERR_INFERENCE);
    memcpy(cp->ring.host<ChipFrame>(r), cf.data(), sizeof(ChipFrame) * (size_t)n);
    HIP_TRY(cp->ring.upload(r, sizeof(ChipFrame) * (size_t)n, s), ZLY_ERR_INFERENCE);
    HIP_TRY(launch_chips((const uint8_t*)f.base, cp->ring.dev<ChipFrame>(r), n, slabs, slab_bytes_of(e), e->cfg.max_dets, d_chips ? d_chips : (void*)cp->d_out, cp->cfg, s),
            ZLY_ERR_INFERENCE);
    HIP_TRY(cp->ring.mark(r, s), ZLY_ERR_INFERENCE);
    if (int rc = detect_events_behind(e, s)) return rc;
    if (ran_on) *ran_on = s;
    return ZLY_OK;
}

int32_t zly_chips_device_view(zly_engine* e, int32_t n, const void* d_base, size_t buf_bytes, const zly_frame_view* views, const void* d_slabs, int32_t source,
                              void* d_chips, void* stream)
{
    if (!e) return fail(ZLY_ERR_NOT_INITIALIZED, "Engine not running");
    if (int rc = chip_check_call(n, e->cfg.max_batch, views, d_slabs, source, &g_last_error)) return rc;
    std::lock_guard<std::mutex> lk(e->mu);
    if (!chips_of(e)) return ZLY_ERR_INVALID_ARGUMENT;
    return chips_locked(e, n, FrameSource{d_base, buf_bytes, views}, d_slabs, source, d_chips, stream);
}

int32_t zly_chips_surfaces(zly_engine* e, int32_t n, const int32_t* surfaces, const void* d_slabs, int32_t source, void* d_chips, void* stream)
{
    if (!e) return fail(ZLY_ERR_NOT_INITIALIZED, "Engine not running");
    if (int rc = chip_check_call(n, e->cfg.max_batch, surfaces, d_slabs, source, &g_last_error)) return rc;
    std::lock_guard<std::mutex> lk(e->mu);
    if (!chips_of(e)) return ZLY_ERR_INVALID_ARGUMENT;
    StoreFrames src;
    if (int rc = src.open(e)) return rc;
    if (int rc = src.frames(n, surfaces)) return rc;
    return src.read_by([&](const FrameSource& f, hipStream_t* ran) { return chips_locked(e, n, f, d_slabs, source, d_chips, stream, ran); });
}

int32_t zly_read_chips(zly_engine* e, int32_t n, void* host_out)
{
    if (!e) return fail(ZLY_ERR_NOT_INITIALIZED, "Engine not running");
    if (!host_out || n < 1 || n > e->cfg.max_batch) return fail(ZLY_ERR_INVALID_ARGUMENT, "bad argument");
    std::lock_guard<std::mutex> lk(e->mu);
    Chips* cp = chips_of(e);
    if (!cp) return ZLY_ERR_INVALID_ARGUMENT;
    return read_back(e, behind_ring(cp->ring), {{host_out, cp->d_out, (size_t)cp->lay.slab_bytes * (size_t)n}});
}

int32_t zly_preprocess(zly_engine* e, const uint8_t* bgr, size_t nbytes, int32_t w, int32_t h, float* out_nchw)
{
    return zly_preprocess_fmt(e, ZLY_PIX_BGR, bgr, nbytes, w, h, out_nchw);
}

int32_t zly_preprocess_fmt(zly_engine* e, int32_t fmt, const uint8_t* bgr, size_t nbytes, int32_t w, int32_t h, float* out_nchw)
{
    if (!e) return fail(ZLY_ERR_NOT_INITIALIZED, "Engine not running");
    if (!out_nchw) return fail(ZLY_ERR_INVALID_ARGUMENT, "null output");
    if (int rcv = check_frame(fmt, bgr, nbytes, w, h, &g_last_error)) return rcv;
    if (int rcm = check_frame_mode(e->cfg.flags, w, h, &g_last_error)) return rcm;
    std::lock_guard<std::mutex> lk(e->mu);
    ExclusiveGate gl;                                    // parity / debug entry point: allocations and copies, alone in the process
    HIP_TRY(hipSetDevice(e->dev), ZLY_ERR_SYSTEM);
    int rc = ensure_stage(e, nbytes);
    if (rc != ZLY_OK) return rc;
    const size_t elems = (size_t)3 * e->cfg.model_w * e->cfg.model_h;
    rc = ensure_scratch_f32(e, elems);
    if (rc != ZLY_OK) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream), ZLY_ERR_INFERENCE);
    memcpy(e->h_stage, bgr, nbytes);
    HIP_TRY(hipMemcpyAsync(e->d_stage, e->h_stage, nbytes, hipMemcpyHostToDevice, e->stream), ZLY_ERR_INFERENCE);
    size_t off0 = 0;
    rc = set_desc(e, 1, &w, &h, &off0, e->stream, &fmt);
    if (rc != ZLY_OK) return rc;
    const FrontVariant fv = area_front(e, front_of(e, front_level(fmt)));
    const uint8_t* src = e->d_stage; const FrameDesc* desc = e->d_desc;
    HIP_TRY(front_source(e, 1, &src, &desc, e->stream), ZLY_ERR_INFERENCE);
    HIP_TRY(launch_preprocess(e->dtype, src, desc, 1, nullptr, e->d_scratch_f32, e->cfg.model_w, e->cfg.model_h, e->stream, fv), ZLY_ERR_INFERENCE);
    HIP_TRY(hipMemcpyAsync(out_nchw, e->d_scratch_f32, elems * sizeof(float), hipMemcpyDeviceToHost, e->stream), ZLY_ERR_INFERENCE);
    HIP_TRY(hipStreamSynchronize(e->stream), ZLY_ERR_INFERENCE);
    return ZLY_OK;
}

int32_t zly_preprocess_view(zly_engine* e, const uint8_t* base, size_t buf_bytes, const zly_frame_view* v, float* out_nchw)
{
    if (!e) return fail(ZLY_ERR_NOT_INITIALIZED, "Engine not running");
    if (!out_nchw) return fail(ZLY_ERR_INVALID_ARGUMENT, "null output");
    if (int rcv = check_view(e->cfg.flags, base, buf_bytes, v, &g_last_error)) return rcv;
    const size_t nbytes = zly_view_bytes(v);             // the buffer's first bytes as they are: the kernel fetches through the view
    std::lock_guard<std::mutex> lk(e->mu);
    ExclusiveGate gl;                                    // parity / debug entry point: allocations and copies, alone in the process
    HIP_TRY(hipSetDevice(e->dev), ZLY_ERR_SYSTEM);
    int rc = ensure_stage(e, nbytes);
    if (rc != ZLY_OK) return rc;
    const size_t elems = (size_t)3 * e->cfg.model_w * e->cfg.model_h;
    rc = ensure_scratch_f32(e, elems);
    if (rc != ZLY_OK) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream), ZLY_ERR_INFERENCE);
    memcpy(e->h_stage, base, nbytes);
    HIP_TRY(hipMemcpyAsync(e->d_stage, e->h_stage, nbytes, hipMemcpyHostToDevice, e->stream), ZLY_ERR_INFERENCE);
    const size_t off0 = (size_t)v->off[0];
    const ViewRec rec = view_rec(v);
    rc = set_desc(e, 1, &v->w, &v->h, &off0, e->stream, &v->fmt, &rec);
    if (rc != ZLY_OK) return rc;
    const FrontVariant fv = area_front(e, front_of(e, front_level(v->fmt), true));
    const uint8_t* src = e->d_stage; const FrameDesc* desc = e->d_desc;
    HIP_TRY(front_source(e, 1, &src, &desc, e->stream), ZLY_ERR_INFERENCE);
    HIP_TRY(launch_preprocess(e->dtype, src, desc, 1, nullptr, e->d_scratch_f32, e->cfg.model_w, e->cfg.model_h, e->stream, fv), ZLY_ERR_INFERENCE);
    HIP_TRY(hipMemcpyAsync(out_nchw, e->d_scratch_f32, elems * sizeof(float), hipMemcpyDeviceToHost, e->stream), ZLY_ERR_INFERENCE);
    HIP_TRY(hipStreamSynchronize(e->stream), ZLY_ERR_INFERENCE);
    return ZLY_OK;
}

int32_t zly_forward(zly_engine* e, int32_t n, const float* images_nchw, float* head_out)
{
    if (!e) return fail(ZLY_ERR_NOT_INITIALIZED, "Engine not running");
    if (!images_nchw || !head_out) return fail(ZLY_ERR_INVALID_ARGUMENT, "null argument");
    if (n < 1 || n > e->cfg.max_batch) return fail(ZLY_ERR_INVALID_ARGUMENT, "batch size out of range");
    std::lock_guard<std::mutex> lk(e->mu);
    HIP_TRY(hipSetDevice(e->dev), ZLY_ERR_SYSTEM);
    const size_t elems = (size_t)n * 3 * e->cfg.model_w * e->cfg.model_h;
    int rc = ZLY_OK;
    {
        ExclusiveGate x;                                      // scratch allocation: alone in the process
        rc = ensure_scratch_f32(e, elems);
    }
    if (rc != ZLY_OK) return rc;
    SharedGate gl;
    HIP_TRY(hipMemcpyAsync(e->d_scratch_f32, images_nchw, elems * sizeof(float), hipMemcpyHostToDevice, e->stream), ZLY_ERR_INFERENCE);
    HIP_TRY(launch_nchw_to_nhwc8(e->dtype, e->d_scratch_f32, e->bufs[(size_t)e->in_buf].ptr, n, e->cfg.model_w, e->cfg.model_h, e->stream), ZLY_ERR_INFERENCE);
    // frames are model-sized for the purposes of the (unused) decode that follows
    std::vector<int32_t> ws((size_t)n, e->cfg.model_w), hs((size_t)n, e->cfg.model_h);
    std::vector<size_t> offs((size_t)n, 0);
    rc = set_desc(e, n, ws.data(), hs.data(), offs.data(), e->stream);
    if (rc != ZLY_OK) return rc;
    if (e->cfg.flags & ZLY_FLAG_NO_HEAD_TENSOR) return fail(ZLY_ERR_INVALID_ARGUMENT, "engine was created with ZLY_FLAG_NO_HEAD_TENSOR: the head tensor is not materialised");
    rc = run_path(e, n, nullptr, nullptr, 0, e->stream, false, false, nullptr, FrontVariant());     // no front kernel: model.0 is computed from the caller's images
    if (rc != ZLY_OK) return rc;
    HIP_TRY(hipMemcpyAsync(head_out, e->d_head, (size_t)n * (4 + (size_t)e->nc) * e->N * sizeof(float), hipMemcpyDeviceToHost, e->stream), ZLY_ERR_INFERENCE);
    HIP_TRY(hipStreamSynchronize(e->stream), ZLY_ERR_INFERENCE);
    return ZLY_OK;
}

int32_t zly_head_tensor(zly_engine* e, int32_t idx, float* head_out)
{
    if (!e) return fail(ZLY_ERR_NOT_INITIALIZED, "Engine not running");
    if (!head_out || idx < 0 || idx >= e->cfg.max_batch) return fail(ZLY_ERR_INVALID_ARGUMENT, "bad argument");
    std::lock_guard<std::mutex> lk(e->mu);
    SharedGate gl;
    HIP_TRY(hipSetDevice(e->dev), ZLY_ERR_SYSTEM);
    if (e->cfg.flags & ZLY_FLAG_NO_HEAD_TENSOR) return fail(ZLY_ERR_INVALID_ARGUMENT, "engine was created with ZLY_FLAG_NO_HEAD_TENSOR: the head tensor is not materialised");
    const size_t per = (4 + (size_t)e->nc) * e->N;
    HIP_TRY(hipMemcpyAsync(head_out, e->d_head + per * (size_t)idx, per * sizeof(float), hipMemcpyDeviceToHost, e->stream), ZLY_ERR_INFERENCE);
    HIP_TRY(hipStreamSynchronize(e->stream), ZLY_ERR_INFERENCE);
    return ZLY_OK;
}

int32_t zly_postprocess(zly_engine* e, const float* head, int32_t num_classes, int32_t num_boxes, int32_t img_w, int32_t img_h,
                        float conf_thr, float iou_thr, zly_det* out, int32_t cap, int32_t* n_out, int32_t* n_candidates)
{
    if (!e) return fail(ZLY_ERR_NOT_INITIALIZED, "Engine not running");
    if (!head || !out || !n_out || num_classes < 1 || num_classes > 1024 || num_boxes < 0 || cap < 1 || img_w <= 0 || img_h <= 0)
        return fail(ZLY_ERR_INVALID_ARGUMENT, "bad argument");
    std::lock_guard<std::mutex> lk(e->mu);
    ExclusiveGate gl;                                    // parity / debug entry point: allocations and copies, alone in the process
    HIP_TRY(hipSetDevice(e->dev), ZLY_ERR_SYSTEM);
    *n_out = 0;
    if (n_candidates) *n_candidates = 0;
    if (num_boxes == 0) return ZLY_OK;
    const size_t N = (size_t)num_boxes;
    const size_t head_bytes = (4 + (size_t)num_classes) * N * sizeof(float);
    const size_t slab = sizeof(zly_slab_header) + (size_t)cap * sizeof(zly_det);
    // one-off device scratch: [head | cand | scratch | count | desc | slab]
    size_t off_cand = (head_bytes + 255) / 256 * 256;
    size_t off_scr = off_cand + (N * sizeof(Cand) + 255) / 256 * 256;
    size_t off_cnt = off_scr + (N * sizeof(Cand) + 255) / 256 * 256;
    size_t off_desc = off_cnt + 256;
    size_t off_slab = off_desc + 256;
    size_t total = off_slab + slab;
    char* d = nullptr;
    HIP_TRY(hipMalloc((void**)&d, total), ZLY_ERR_SYSTEM);
    std::vector<unsigned char> hslab(slab);
    FrameDesc fd; fd.src_off = 0; fd.w = img_w; fd.h = img_h;
    hipError_t r = hipMemcpyAsync(d, head, head_bytes, hipMemcpyHostToDevice, e->stream);
    if (r == hipSuccess) r = hipMemcpyAsync(d + off_desc, &fd, sizeof fd, hipMemcpyHostToDevice, e->stream);
    if (r == hipSuccess) r = hipMemsetAsync(d + off_cnt, 0, sizeof(int), e->stream);
    if (r == hipSuccess) r = launch_decode((const float*)d, num_classes, num_boxes, 1, (const FrameDesc*)(d + off_desc), conf_thr,
                                           (Cand*)(d + off_cand), (int*)(d + off_cnt), e->stream);
    if (r == hipSuccess) r = launch_nms((const Cand*)(d + off_cand), (int*)(d + off_cnt), num_boxes, 1, iou_thr, num_classes,
                                        (Cand*)(d + off_scr), d + off_slab, cap, 0, e->stream, e->sw.nms_general ? 1 : 0);
    if (r == hipSuccess) r = hipMemcpyAsync(hslab.data(), d + off_slab, slab, hipMemcpyDeviceToHost, e->stream);
    if (r == hipSuccess) r = hipStreamSynchronize(e->stream);
    hipFree(d);
    if (r != hipSuccess) return fail(ZLY_ERR_INFERENCE, std::string("postprocess: ") + hipGetErrorString(r));
    const zly_slab_header* hd = reinterpret_cast<const zly_slab_header*>(hslab.data());
    const zly_det* dd = reinterpret_cast<const zly_det*>(hd + 1);
    const int m = hd->n_kept < cap ? hd->n_kept : cap;
    for (int k = 0; k < m; ++k) out[k] = dd[k];
    *n_out = hd->n_kept;
    if (n_candidates) *n_candidates = hd->n_candidates;
    return ZLY_OK;
}

int32_t zly_debug_tap(zly_engine* e, const char* name, int32_t idx, float* out, size_t cap_floats, int32_t* c, int32_t* h, int32_t* w)
{
    if (!e) return fail(ZLY_ERR_NOT_INITIALIZED, "Engine not running");
    if (!name || !out || idx < 0 || idx >= e->cfg.max_batch) return fail(ZLY_ERR_INVALID_ARGUMENT, "bad argument");
    std::lock_guard<std::mutex> lk(e->mu);
    ExclusiveGate gl;                                    // parity / debug entry point: allocations and copies, alone in the process
    HIP_TRY(hipSetDevice(e->dev), ZLY_ERR_SYSTEM);
    int buf = -1, co = 0, C = 0;
    bool f32 = false;
    if (std::string(name) == "images") { buf = e->in_buf; co = 0; C = 3; }
    else {
        auto it = e->tap_index.find(name);
        auto jt = e->tap_final.find(name);
        if (it != e->tap_index.end()) {
            const Op& op = e->ops[(size_t)it->second.first];
            // where the last call left the op's output: the launch table of its batch size (no call yet: every buffer is in HBM)
            const std::vector<Launch>* t = e->last_n > 0 ? &resolve_launches(e, e->last_n) : nullptr;
            const Launch* L = t ? &(*t)[(size_t)it->second.first] : nullptr;
            switch (L && !L->hbm ? (*t)[(size_t)L->covered_by].kind : LK_NONE) {
            case LK_STEM1:
                if (e->last_front)
                    return fail(ZLY_ERR_INVALID_ARGUMENT, "tap model.0 stays in LDS inside the fused stem kernel; create the engine with ZLY_FLAG_DUMP_LOGITS (or ZLY_FLAG_NO_FUSION)");
                break;
            case LK_C2F:
                return fail(ZLY_ERR_INVALID_ARGUMENT, std::string("tap ") + name + " stays in LDS inside the fused C2f kernel at this batch size; create the engine with " +
                                                          (e->c2fs[(size_t)op.c2f].vis_of(it->second.first) == 1 ? "ZLY_FLAG_DUMP_LOGITS or " : "") + "ZLY_FLAG_NO_FUSION");
            case LK_SPPF_FUSED:
                return fail(ZLY_ERR_INVALID_ARGUMENT, std::string("tap ") + name + " stays in LDS inside the fused SPPF kernel; create the engine with ZLY_FLAG_DUMP_LOGITS or ZLY_FLAG_NO_FUSION");
            case LK_PAIR:
                return fail(ZLY_ERR_INVALID_ARGUMENT, std::string("tap ") + name + " stays in LDS inside the fused bottleneck kernel at this batch size; create the engine with ZLY_FLAG_NO_FUSION");
            case LK_WS_PAIR:
                return fail(ZLY_ERR_INVALID_ARGUMENT, std::string("tap ") + name + " stays in LDS inside the fused bottleneck kernel at this batch size; create the engine with ZLY_FLAG_DUMP_LOGITS or ZLY_FLAG_NO_FUSION");
            case LK_HEAD:
                return fail(ZLY_ERR_INVALID_ARGUMENT, std::string("tap ") + name + " is computed inside the fused Detect kernel, at surviving anchors only, at this batch size; create the engine with ZLY_FLAG_DUMP_LOGITS or ZLY_FLAG_NO_FUSION");
            }
            buf = op.out.buf; co = op.out.co + op.tap_co[(size_t)it->second.second]; C = op.tap_c[(size_t)it->second.second];
            f32 = op.out_f32 != 0;
        } else if (jt != e->tap_final.end()) {
            if (!(e->cfg.flags & ZLY_FLAG_DUMP_LOGITS))
                return fail(ZLY_ERR_INVALID_ARGUMENT, std::string("tap ") + name + " is computed inside the fused Detect kernel; create the engine with ZLY_FLAG_DUMP_LOGITS");
            buf = jt->second.first; co = jt->second.second; C = co == 0 ? 64 : e->nc; f32 = true;
        } else {
            return fail(ZLY_ERR_INVALID_ARGUMENT, std::string("unknown tap: ") + name);
        }
    }
    const Buffer& b = e->bufs[(size_t)buf];
    const size_t elems = (size_t)C * b.H * b.W;
    if (elems > cap_floats) return fail(ZLY_ERR_INVALID_ARGUMENT, "tap output buffer too small");
    int rc = ensure_scratch_f32(e, elems);
    if (rc != ZLY_OK) return rc;
    HIP_TRY(launch_tap_to_nchw(f32 ? ZLY_DTYPE_FP32 : e->dtype, b.ptr, b.C, co, C, b.H, b.W, idx, e->d_scratch_f32, e->stream), ZLY_ERR_INFERENCE);
    HIP_TRY(hipMemcpyAsync(out, e->d_scratch_f32, elems * sizeof(float), hipMemcpyDeviceToHost, e->stream), ZLY_ERR_INFERENCE);
    HIP_TRY(hipStreamSynchronize(e->stream), ZLY_ERR_INFERENCE);
    if (c) *c = C;
    if (h) *h = b.H;
    if (w) *w = b.W;
    return ZLY_OK;
}

int32_t zly_num_classes(const zly_engine* e) { return e ? e->nc : 0; }
int32_t zly_weights_fp8(const zly_engine* e) { return (e && e->model.fp8_weights) ? 1 : 0; }
int32_t zly_num_anchors(const zly_engine* e) { return e ? e->N : 0; }
int32_t zly_num_ops(const zly_engine* e) { return e ? (int32_t)e->ops.size() : 0; }

int32_t zly_op_info_at(const zly_engine* e, int32_t i, zly_op_info* out)
{
    if (!e || !out || i < 0 || i >= (int32_t)e->ops.size()) return fail(ZLY_ERR_INVALID_ARGUMENT, "bad argument");
    const Op& op = e->ops[(size_t)i];
    memset(out, 0, sizeof *out);
    snprintf(out->name, sizeof out->name, "%s", op.name.c_str());
    out->kind = op.kind;
    out->flops_per_frame = op.flops;
    out->bytes_per_frame = op.bytes;
    return ZLY_OK;
}

int32_t zly_op_kernel_name(zly_engine* e, int32_t i, int32_t n, char* out, size_t cap)
{
    if (!e || !out || cap < 8 || i < 0 || i >= (int32_t)e->ops.size() || n < 1 || n > e->cfg.max_batch) return fail(ZLY_ERR_INVALID_ARGUMENT, "bad argument");
    std::lock_guard<std::mutex> lk(e->mu);
    const std::vector<Launch>& t = resolve_launches(e, n);
    const Launch& L = t[(size_t)i];
    const Op& op = e->ops[(size_t)i];
    std::string k;
    switch (L.kind) {
    case LK_NONE:
        switch (t[(size_t)L.covered_by].kind) {
        case LK_STEM: case LK_STEM1: k = op.kind == OP_PREPROCESS ? "(fused into stem_fused_kernel)" : "(fused into the previous launch)"; break;
        case LK_PAIR: case LK_WS_PAIR: k = "(fused into the previous launch)"; break;
        case LK_C2F: k = "(fused into the C2f kernel at " + e->ops[(size_t)L.covered_by].name + ")"; break;
        case LK_SPPF_FUSED: k = "(fused into the SPPF kernel at model.9.cv1)"; break;
        case LK_MULTI: k = "(in a merged Detect launch)"; break;
        case LK_HEAD: k = op.kind == OP_CONV ? "(computed in the Detect tail at surviving anchors)" : "(covered by the last tail launch)"; break;
        }
        break;
    case LK_PREPROCESS: k = L.lb ? "preprocess_kernel<LB> (letterbox)" : "preprocess_kernel"; break;
    case LK_STEM: k = L.lb ? "stem_fused_kernel<LB> (letterbox)" : "stem_fused_kernel"; break;
    case LK_STEM1: k = L.lb ? "stem_model1_kernel<LB> (letterbox preprocess+model.0+model.1)" : "stem_model1_kernel (preprocess+model.0+model.1)"; break;
    case LK_SPPF_POOL: k = L.pool16 ? "sppf_pool16_kernel<DPP row windows, one barrier>" : "sppf_pool_kernel"; break;
    case LK_SPPF_FUSED: k = "sppf_fused_kernel<cv1+3 pools+cv2,SPLIT=" + std::to_string(sppf_split(e->ops[(size_t)e->sppf_cv2].cout, n, e->sw)) + ">"; break;
    case LK_MULTI: k = L.multi_ct == 3 ? "conv_igemm_multi_kernel<CT=3> (the 3 Detect stems)" : "conv_igemm_multi_kernel<CT=2> (the 6 Detect branch convs)"; break;
    case LK_C2F: {
        const C2fGroup& g = e->c2fs[(size_t)op.c2f];
        k = "c2f_kernel<C=" + std::to_string(g.c) + (g.c == 32 ? ",NW=" + std::to_string(L.c2f.nw) : std::string()) +
            (g.mode == 3 ? ",cv1+bottleneck+cv2," : g.mode == 1 ? ",cv1+bottleneck," : ",bottleneck+cv2,") + std::to_string(L.c2f.th) + "x" + std::to_string(L.c2f.tw) + " tiles>";
        break;
    }
    case LK_PAIR: k = "bottleneck_pair_kernel<" + std::to_string(e->pairs[(size_t)op.pair].c) + ">"; break;
    case LK_WS_PAIR: k = std::string("conv3x3_ws_pair_kernel<") + (e->pairs[(size_t)op.pair].res ? "RES," : "") + "64->64->64," + std::to_string(L.ws_pair.g.TH) + "x" + std::to_string(L.ws_pair.g.TW) + " tiles>"; break;
    case LK_CONV_WSK: k = "conv3x3_wsk_kernel<K=720 packed across taps,5 channel tiles>"; break;
    case LK_CONV: {
        const int cin = op.in.C + (op.in2.buf >= 0 ? op.in2.C : 0);
        const ConvPlan& c = L.conv;
        switch (c.kind) {
        case CONV_WS1: k = std::string("conv1x1_ws_kernel<") + (op.in2.buf >= 0 ? "dual-source," : "") + "NK=" + std::to_string(cin / 32) + "," + std::to_string(c.ct) + " channel tiles," + std::to_string(c.pt * 16) + " px>"; break;
        case CONV_WS: k = std::string("conv3x3_ws_kernel<") + (op.stride == 2 ? "S=2," : "") + (c.rowt ? "ROWT," : "") + (c.tpw1 ? "TPW=1," : "TPW=2,") + std::to_string(c.ct) + " channel tiles>"; break;
        case CONV_LDS: k = "conv3x3_lds_kernel<S=" + std::to_string(op.stride) + ",CT=" + std::to_string(c.ct) + ",PT=" + std::to_string(c.pt) + (c.wres ? ",wres>" : ">"); break;
        case CONV_STREAM: k = "conv1x1_stream_kernel<CT=" + std::to_string(c.ct) + ",PT=" + std::to_string(c.pt) + ",NK=" + std::to_string((cin + 31) / 32) + ">"; break;
        default: k = std::string("conv_igemm_kernel<") + (op.ks == 1 ? (op.in2.buf >= 0 ? "1x1 dual-source" : "1x1") : (c.fastk ? "3x3" : "3x3 generic-K")) +
                 ",CT=" + std::to_string(c.ct) + ",PT=" + std::to_string(c.pt) + ",KSPLIT=" + std::to_string(c.ksplit) + ">";
        }
        break;
    }
    case LK_HEAD: {
        k = L.lb ? "head_fused_kernel<LB> (letterbox box mapping)" : "head_fused_kernel";
        std::string lv;
        for (int l = 0; l < 3; ++l)
            if (L.box_mode[l] && (L.only_level < 0 || L.only_level == l)) lv += std::string(lv.empty() ? "" : ",") + "P" + std::to_string(3 + l) + (L.box_mode[l] == 1 ? ":ws" : ":lds");
        if (!lv.empty()) k += " (+ box conv in k-step order " + lv + ")";
        break;
    }
    case LK_NMS: k = "nms_kernel"; break;
    }
    snprintf(out, cap, "%s", k.c_str());
    return ZLY_OK;
}

int32_t zly_launch_info_at(zly_engine* e, int32_t i, int32_t n, zly_launch_info* out)
{
    if (!e || !out || i < 0 || i >= (int32_t)e->ops.size() || n < 1 || n > e->cfg.max_batch) return fail(ZLY_ERR_INVALID_ARGUMENT, "bad argument");
    std::lock_guard<std::mutex> lk(e->mu);
    memset(out, 0, sizeof *out);
    const int nops = (int)e->ops.size();
    const std::vector<Launch>& t = resolve_launches(e, n);
    out->covered_by = t[(size_t)i].covered_by;
    if (out->covered_by != i) return ZLY_OK;
    std::vector<char> in_group((size_t)nops, 0);
    for (int j = 0; j < nops; ++j) in_group[(size_t)j] = t[(size_t)j].covered_by == i ? 1 : 0;
    // channel maps per buffer: written inside the group / read outside the group
    std::map<int, std::vector<char>> written_in, read_out, counted_in, counted_out;
    auto chan = [&](std::map<int, std::vector<char>>& m, int buf) -> std::vector<char>& {
        std::vector<char>& v = m[buf];
        if (v.empty()) v.assign((size_t)e->bufs[(size_t)buf].C + 64, 0);
        return v;
    };
    std::vector<IoView> io;
    for (int j = 0; j < nops; ++j) {
        io.clear();
        if (in_group[(size_t)j]) { op_writes(e, e->ops[(size_t)j], &io); for (const IoView& v : io) for (int c = 0; c < v.C; ++c) chan(written_in, v.buf)[(size_t)(v.co + c)] = 1; }
        else { op_reads(e, e->ops[(size_t)j], &io); for (const IoView& v : io) for (int c = 0; c < v.C; ++c) chan(read_out, v.buf)[(size_t)(v.co + c)] = 1; }
    }
    double ext_in = 0, ext_out = 0, wbytes = 0;
    for (int j = 0; j < nops; ++j) {
        if (!in_group[(size_t)j]) continue;
        const Op& op = e->ops[(size_t)j];
        out->n_ops++;
        // a conv the Detect tail computes at surviving anchors only: its dense flops, bytes and weights are work that is not done, and are not booked on the
        // tail.  Its input view is: the stem buffer's box half is what the tail reads in place of the conv's output (which counts as written inside the
        // group), booked whole -- the bound with every wave surviving; the tail reads the share that survives, plus those tiles' halo
        const bool in_tail = op.kind == OP_CONV && j != i && t[(size_t)i].kind == LK_HEAD;
        if (!in_tail) {
            out->flops_per_frame += op.flops;
            out->bytes_unfused_per_frame += op.bytes;
            wbytes += op.wbytes;
        }
        if (op.kind == OP_PREPROCESS) ext_in += (double)e->cfg.model_w * e->cfg.model_h * 3;          // the u8 frame (model-sized requests)
        if (op.kind == OP_HEAD && !(e->cfg.flags & ZLY_FLAG_NO_HEAD_TENSOR)) ext_out += (double)e->tail.args.lv[op.level].hw * (4 + e->nc) * 4.0;
        io.clear(); op_reads(e, op, &io);
        for (const IoView& v : io) {
            int cext = 0;
            for (int c = 0; c < v.C; ++c) {
                const size_t ch = (size_t)(v.co + c);
                if (chan(written_in, v.buf)[ch] || chan(counted_in, v.buf)[ch]) continue;
                chan(counted_in, v.buf)[ch] = 1; ++cext;
            }
            ext_in += v.px * cext * (double)e->esz * v.scale;
        }
        if (in_tail) continue;                                   // its output exists only under the dump flag, and nothing outside the group reads it
        io.clear(); op_writes(e, op, &io);
        for (const IoView& v : io) {
            int cext = 0;
            for (int c = 0; c < v.C; ++c) {
                const size_t ch = (size_t)(v.co + c);
                if (!chan(read_out, v.buf)[ch] || chan(counted_out, v.buf)[ch]) continue;
                chan(counted_out, v.buf)[ch] = 1; ++cext;
            }
            ext_out += v.px * cext * (double)e->esz * v.scale;
        }
    }
    out->bytes_fused_per_frame = ext_in + ext_out + wbytes;
    out->weight_bytes = wbytes;
    return ZLY_OK;
}

int32_t zly_profile_ops(zly_engine* e, int32_t n, const void* d_frames, int32_t w, int32_t h, int32_t reps, float* ms_out)
{
    if (!e) return fail(ZLY_ERR_NOT_INITIALIZED, "Engine not running");
    if (!d_frames || !ms_out || reps < 1 || n < 1 || n > e->cfg.max_batch || w < 1 || h < 1) return fail(ZLY_ERR_INVALID_ARGUMENT, "bad argument");
    if (int rcm = check_frame_mode(e->cfg.flags, w, h, &g_last_error)) return rcm;
    std::lock_guard<std::mutex> lk(e->mu);
    ExclusiveGate gl;
    HIP_TRY(hipSetDevice(e->dev), ZLY_ERR_SYSTEM);
    std::vector<int32_t> ws((size_t)n, w), hs((size_t)n, h);
    std::vector<size_t> offs((size_t)n);
    for (int i = 0; i < n; ++i) offs[(size_t)i] = (size_t)i * (size_t)w * (size_t)h * 3u;
    int rc = set_desc(e, n, ws.data(), hs.data(), offs.data(), e->stream);
    e->front = area_front(e, front_of(e, ZLY_FRONT_BGR));         // tight BGR frames
    if (rc != ZLY_OK) return rc;
    const size_t nops = e->ops.size();
    const std::vector<Launch>& tab = resolve_launches(e, n);
    std::vector<hipEvent_t> ev(nops + 1);
    for (hipEvent_t& x : ev) HIP_TRY(hipEventCreate(&x), ZLY_ERR_SYSTEM);
    std::vector<double> acc(nops, 0.0);
    int rcode = ZLY_OK;
    // ZLY_PROFILE_INNER=k: every op is launched k times back to back between its two events, and the time is
    // divided by k -- the in-sequence cost of a launch (kernel + boundary) without the ~5 us that an event pair
    // per launch adds; used to study the batch-1 path, where most kernels are shorter than that
    // (read per call, not per engine: bench.py changes it between two calls on one engine)
    Switches now;
    read_switches(&now);
    const int inner = now.profile_inner;
    for (int r = 0; r < reps && rcode == ZLY_OK; ++r) {
        hipEventRecord(ev[0], e->stream);
        for (size_t i = 0; i < nops; ++i) {
            hipError_t hr = hipSuccess;
            // only the idempotent forward ops are repeated: the Detect tail appends candidates and NMS consumes them
            const int reps_i = (e->ops[i].kind == OP_HEAD || e->ops[i].kind == OP_NMS) ? 1 : inner;
            // the detect path's launches: the front kernel's time is booked on the op that launches it, covered ops launch nothing
            for (int k = 0; k < reps_i && hr == hipSuccess; ++k) hr = run_op(e, i, tab[i], n, (const uint8_t*)d_frames, nullptr, 0, e->stream);
            if (hr != hipSuccess) { rcode = fail(ZLY_ERR_INFERENCE, std::string("profile: ") + hipGetErrorString(hr)); break; }
            hipEventRecord(ev[i + 1], e->stream);
        }
        if (rcode != ZLY_OK) break;
        if (hipStreamSynchronize(e->stream) != hipSuccess) { rcode = fail(ZLY_ERR_INFERENCE, "profile: sync failed"); break; }
        for (size_t i = 0; i < nops; ++i) {
            float ms = 0.f;
            hipEventElapsedTime(&ms, ev[i], ev[i + 1]);
            if (tab[i].kind == LK_NONE) ms = 0.f;            // nothing was launched: what the event pair shows is its own cost
            acc[i] += ms / ((e->ops[i].kind == OP_HEAD || e->ops[i].kind == OP_NMS) ? 1 : inner);
        }
    }
    for (hipEvent_t& x : ev) hipEventDestroy(x);
    if (rcode != ZLY_OK) return rcode;
    for (size_t i = 0; i < nops; ++i) {
        ms_out[i] = (float)(acc[i] / reps);
        const int k = e->ops[i].kind;
        with_stats(e, [&](zly_stats& st) {
            if (k == OP_PREPROCESS) st.total_preprocess_ms += acc[i];
            else if (k == OP_NMS) st.total_postprocess_ms += acc[i];
            else st.total_forward_ms += acc[i];
        });
    }
    e->last_n = n; e->last_front = true;
    return ZLY_OK;
}

int32_t zly_get_stats(const zly_engine* e, zly_stats* out)
{
    if (!e || !out) return fail(ZLY_ERR_INVALID_ARGUMENT, "bad argument");
    std::lock_guard<std::mutex> lk(e->stats_mu);           // never held across a device call: does not wait on a running batch
    *out = e->stats;
    return ZLY_OK;
}

}  // extern "C"
