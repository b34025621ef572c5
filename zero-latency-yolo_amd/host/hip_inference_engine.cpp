// hip_inference_engine.cpp -- see hip_inference_engine.h.  Host C++ only; every GPU action is a call
// into the C ABI of include/zly.h.
#include "hip_inference_engine.h"

#include "zly.h"
#include "zly_sha256.hpp"

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <random>
#include <unordered_map>

// The format-taking submit calls are referenced weakly: a host build against a C ABI without them (the link-time stub of
// tests/cpp/test_plugin_stub.cpp) still links, and initialize() refuses a YUV ZLY_INPUT_FORMAT when they are missing.
#pragma weak zly_submit_fmt
#pragma weak zly_submit_try_fmt
// ... and so are the frame-view calls behind ZLY_CROP: initialize() refuses ZLY_CROP when they are missing
#pragma weak zly_view_tight
#pragma weak zly_view_bytes
#pragma weak zly_view_crop
#pragma weak zly_submit_view
#pragma weak zly_submit_try_view
// ... and the tracking calls behind ZLY_TRACK: initialize() refuses ZLY_TRACK when they are missing
#pragma weak zly_default_track_config
#pragma weak zly_track_enable
#pragma weak zly_track_reset
#pragma weak zly_submit_view_tracked
#pragma weak zly_submit_try_view_tracked
// ... and the motion model's calls behind ZLY_TRACK_MOTION: initialize() refuses ZLY_TRACK_MOTION when they are missing
#pragma weak zly_default_track_motion_config
#pragma weak zly_track_motion_enable

namespace zero_latency {

namespace {
uint64_t wallMs()
{
    return (uint64_t)std::chrono::duration_cast<std::chrono::milliseconds>(
               std::chrono::system_clock::now().time_since_epoch()).count();
}
ErrorCode toErrorCode(int32_t rc)
{
    switch (rc) {
        case ZLY_OK: return ErrorCode::OK;
        case ZLY_ERR_INVALID_ARGUMENT: return ErrorCode::INVALID_ARGUMENT;
        case ZLY_ERR_NOT_INITIALIZED: return ErrorCode::NOT_INITIALIZED;
        case ZLY_ERR_MODEL_NOT_FOUND: return ErrorCode::MODEL_NOT_FOUND;
        case ZLY_ERR_MODEL_LOAD: return ErrorCode::MODEL_LOAD_FAILED;
        case ZLY_ERR_INVALID_INPUT: return ErrorCode::INVALID_INPUT;
        case ZLY_ERR_SYSTEM: return ErrorCode::SYSTEM_ERROR;
        default: return ErrorCode::INFERENCE_ERROR;
    }
}
// ZLY_INPUT_FORMAT: bgr (default), nv12, i420 (BT.601), nv12_709, i420_709, rgb, bgra, rgba, yuy2, uyvy (BT.601), yuy2_709, uyvy_709 -> ZLY_PIX_*, -1 = unknown
int32_t parseInputFormat(const char* v)
{
    if (!v || !*v || std::strcmp(v, "bgr") == 0) return ZLY_PIX_BGR;
    if (std::strcmp(v, "nv12") == 0) return ZLY_PIX_NV12_BT601;
    if (std::strcmp(v, "i420") == 0) return ZLY_PIX_I420_BT601;
    if (std::strcmp(v, "nv12_709") == 0) return ZLY_PIX_NV12_BT709;
    if (std::strcmp(v, "i420_709") == 0) return ZLY_PIX_I420_BT709;
    if (std::strcmp(v, "rgb") == 0) return ZLY_PIX_RGB;
    if (std::strcmp(v, "bgra") == 0) return ZLY_PIX_BGRA;
    if (std::strcmp(v, "rgba") == 0) return ZLY_PIX_RGBA;
    if (std::strcmp(v, "yuy2") == 0) return ZLY_PIX_YUY2_BT601;
    if (std::strcmp(v, "uyvy") == 0) return ZLY_PIX_UYVY_BT601;
    if (std::strcmp(v, "yuy2_709") == 0) return ZLY_PIX_YUY2_BT709;
    if (std::strcmp(v, "uyvy_709") == 0) return ZLY_PIX_UYVY_BT709;
    return -1;
}
// YUV 4:2:0 formats: even sizes and even crop origins; the packed formats (BGR, RGB, BGRA, RGBA) have no such rule
bool isYuvFormat(int32_t fmt) { return fmt >= ZLY_PIX_NV12_BT601 && fmt <= ZLY_PIX_I420_BT709; }
// packed YUV 4:2:2 formats: the rule holds along x only (whole macropixels); any height, any y0
bool isYuv422Format(int32_t fmt) { return fmt >= ZLY_PIX_YUY2_BT601 && fmt <= ZLY_PIX_UYVY_BT709; }
const char* inputFormatName(int32_t fmt)
{
    switch (fmt) {
    case ZLY_PIX_NV12_BT601: return "nv12";
    case ZLY_PIX_I420_BT601: return "i420";
    case ZLY_PIX_NV12_BT709: return "nv12_709";
    case ZLY_PIX_I420_BT709: return "i420_709";
    case ZLY_PIX_RGB: return "rgb";
    case ZLY_PIX_BGRA: return "bgra";
    case ZLY_PIX_RGBA: return "rgba";
    case ZLY_PIX_YUY2_BT601: return "yuy2";
    case ZLY_PIX_UYVY_BT601: return "uyvy";
    case ZLY_PIX_YUY2_BT709: return "yuy2_709";
    case ZLY_PIX_UYVY_BT709: return "uyvy_709";
    default: return "bgr";
    }
}
// ZLY_RESIZE: stretch (default: the reference's nearest-neighbour stretch), letterbox (ZLY_FLAG_LETTERBOX), area (ZLY_FLAG_AREA: the stretch geometry
// with the area-average filter), letterbox_area (both flags) -> bit 0 = letterbox geometry, bit 1 = area filter; -1 = unknown
int parseResizeMode(const char* v)
{
    if (!v || !*v || std::strcmp(v, "stretch") == 0) return 0;
    if (std::strcmp(v, "letterbox") == 0) return 1;
    if (std::strcmp(v, "area") == 0) return 2;
    if (std::strcmp(v, "letterbox_area") == 0) return 3;
    return -1;
}
const char* resizeModeName(bool letterbox, bool area) { return letterbox ? (area ? "letterbox_area" : "letterbox") : (area ? "area" : "stretch"); }
// ZLY_CROP=WxH (both >= 1) -> true; unset or empty: no crop (w = h = 0), true; anything else: false
bool parseCrop(const char* v, int32_t* w, int32_t* h)
{
    *w = *h = 0;
    if (!v || !*v) return true;
    char* end = nullptr;
    const long cw = std::strtol(v, &end, 10);
    if (end == v || (*end != 'x' && *end != 'X')) return false;
    const char* hs = end + 1;
    const long ch = std::strtol(hs, &end, 10);
    if (end == hs || *end || cw < 1 || ch < 1 || cw > (1 << 24) || ch > (1 << 24)) return false;
    *w = (int32_t)cw; *h = (int32_t)ch;
    return true;
}
// The box map of ZLY_CROP, single IEEE fp32 operations: a product is rounded to fp32 before it is added to or divided
// (the volatile store keeps a compiler from contracting it into a fused multiply-add)
inline float mulRounded(float a, float b) { volatile float p = a * b; return p; }
void mapCropToFrame(Detection& d, int32_t x0, int32_t y0, int32_t cw, int32_t ch, int32_t fw, int32_t fh)
{
    d.box.x = (mulRounded(d.box.x, (float)cw) + (float)x0) / (float)fw;
    d.box.y = (mulRounded(d.box.y, (float)ch) + (float)y0) / (float)fh;
    d.box.width = mulRounded(d.box.width, (float)cw) / (float)fw;
    d.box.height = mulRounded(d.box.height, (float)ch) / (float)fh;
}
int envInt(const char* name, int fallback)
{
    const char* v = std::getenv(name);
    return (v && *v) ? std::atoi(v) : fallback;
}
}  // namespace

struct HipInferenceEngine::EngineHandle {
    zly_engine* e = nullptr;
    std::atomic<bool> replaced{false};                   // set by reloadModel / shutdown when the handle leaves engines_: its last request hands it to the reaper
    // ZLY_TRACK: which client owns which stream slot of this engine.  A new engine (hot reload) starts empty, like its track tables.
    struct TrackSlot { uint32_t client = 0; uint64_t last_use = 0; bool used = false; };
    std::mutex track_mu;
    std::vector<TrackSlot> track_slots;
    std::unordered_map<uint32_t, int32_t> track_slot_of;
    uint64_t track_clock = 0;
    explicit EngineHandle(zly_engine* p) : e(p) {}
    ~EngineHandle() { if (e) zly_destroy(e); }
    EngineHandle(const EngineHandle&) = delete;
    EngineHandle& operator=(const EngineHandle&) = delete;
};

HipInferenceEngine::HipInferenceEngine(const ServerConfig& config) : config_(config)
{
    max_batch_ = std::max(1, std::min(65535, envInt("ZLY_MAX_BATCH", 64)));
    max_dets_ = std::max(1, envInt("ZLY_MAX_DETS", 256));
}

HipInferenceEngine::~HipInferenceEngine() { shutdown(); }

Result<void> HipInferenceEngine::initialize()
{
    if (running_) return Result<void>::ok();
    simulate_ = envInt("ZLY_SIMULATE", 0) != 0;               // explicit opt-in only: a missing or bad model file is an ERROR below, never a silent fake
    // ZLY_INPUT_FORMAT: requests carry YUV 4:2:0 frames (decoder output), packed RGB / BGRA / RGBA frames (capture surfaces) or packed YUV 4:2:2 frames (capture
    // cards, UVC devices) instead of packed BGR; request.data must then hold
    // zly_frame_bytes(format, width, height) bytes, a request of any other size fails alone with INVALID_INPUT
    input_format_ = parseInputFormat(std::getenv("ZLY_INPUT_FORMAT"));
    if (input_format_ < 0)
        return Result<void>::error(ErrorCode::INVALID_ARGUMENT, std::string("ZLY_INPUT_FORMAT must be bgr, nv12, i420, nv12_709, i420_709, rgb, bgra, rgba, yuy2, uyvy, yuy2_709 or uyvy_709, got '") +
                                                                 std::getenv("ZLY_INPUT_FORMAT") + "'");
    if (input_format_ != ZLY_PIX_BGR && (!zly_submit_fmt || !zly_submit_try_fmt))
        return Result<void>::error(ErrorCode::SYSTEM_ERROR, "ZLY_INPUT_FORMAT: the engine library has no zly_submit_fmt");
    // ZLY_CROP=WxH: every request is detected in the centred W x H window of its frame (x0 = (width - W) / 2, y0 = (height - H) / 2, both rounded down
    // to even for a YUV 4:2:0 ZLY_INPUT_FORMAT, x0 alone for a packed 4:2:2 one) -- a model-sized window around the crosshair is the engine's fast path -- and its boxes are mapped back to
    // fractions of the whole frame before the callback.  A request smaller than the window on either axis is detected whole.
    if (!parseCrop(std::getenv("ZLY_CROP"), &crop_w_, &crop_h_))
        return Result<void>::error(ErrorCode::INVALID_ARGUMENT, std::string("ZLY_CROP must be WxH with W, H >= 1, got '") + std::getenv("ZLY_CROP") + "'");
    if (crop_w_ > 0 && isYuvFormat(input_format_) && ((crop_w_ | crop_h_) & 1))
        return Result<void>::error(ErrorCode::INVALID_ARGUMENT, "ZLY_CROP: a YUV 4:2:0 ZLY_INPUT_FORMAT needs an even window size");
    if (crop_w_ > 0 && isYuv422Format(input_format_) && (crop_w_ & 1))
        return Result<void>::error(ErrorCode::INVALID_ARGUMENT, "ZLY_CROP: a packed YUV 4:2:2 ZLY_INPUT_FORMAT needs an even window width");
    if (crop_w_ > 0 && (!zly_view_tight || !zly_view_bytes || !zly_view_crop || !zly_submit_view || !zly_submit_try_view))
        return Result<void>::error(ErrorCode::SYSTEM_ERROR, "ZLY_CROP: the engine library has no zly_submit_view");
    // ZLY_RESIZE: how every engine of this plugin (a hot reload's new ones included) fits a request into the model's input: the reference's
    // stretch, or the aspect-preserving letterbox an Ultralytics-trained model expects (boxes then are normalised to the request frame itself); and
    // with which filter: one source pixel per model pixel (four in the letterbox), or -- area, letterbox_area -- the average over all of them
    const int resize = parseResizeMode(std::getenv("ZLY_RESIZE"));
    if (resize < 0)
        return Result<void>::error(ErrorCode::INVALID_ARGUMENT, std::string("ZLY_RESIZE must be stretch, letterbox, area or letterbox_area, got '") + std::getenv("ZLY_RESIZE") + "'");
    letterbox_ = (resize & 1) != 0;
    area_ = (resize & 2) != 0;
    // ZLY_TRACK=1: track ids on the GPU (include/zly.h "tracking"); a client is one stream of one engine
    track_ = envInt("ZLY_TRACK", 0) != 0;
    if (track_) {
        if (!zly_default_track_config || !zly_track_enable || !zly_track_reset || !zly_submit_view_tracked || !zly_submit_try_view_tracked || !zly_view_tight ||
            !zly_view_bytes)
            return Result<void>::error(ErrorCode::SYSTEM_ERROR, "ZLY_TRACK: the engine library has no zly_submit_view_tracked");
        track_streams_ = std::max(1, envInt("ZLY_TRACK_STREAMS", 64));
        const char* iou = std::getenv("ZLY_TRACK_IOU");
        track_iou_ = (iou && *iou) ? (float)std::atof(iou) : -1.0f;
        track_max_lost_ = envInt("ZLY_TRACK_MAX_LOST", -1);
        // a tracking engine stores at most 64 detections per frame (one lane per track slot): that is the default then, and a larger ZLY_MAX_DETS an error
        const char* md = std::getenv("ZLY_MAX_DETS");
        if (md && *md && max_dets_ > 64) return Result<void>::error(ErrorCode::INVALID_ARGUMENT, "ZLY_TRACK needs ZLY_MAX_DETS <= 64");
        max_dets_ = std::min(max_dets_, 64);
    }
    // ZLY_TRACK_MOTION=1: the tracker's constant-velocity motion model on every engine (include/zly.h "The motion model"); only with ZLY_TRACK=1
    track_motion_ = envInt("ZLY_TRACK_MOTION", 0) != 0;
    if (track_motion_) {
        if (!track_) return Result<void>::error(ErrorCode::INVALID_ARGUMENT, "ZLY_TRACK_MOTION needs ZLY_TRACK=1");
        if (!zly_default_track_motion_config || !zly_track_motion_enable)
            return Result<void>::error(ErrorCode::SYSTEM_ERROR, "ZLY_TRACK_MOTION: the engine library has no zly_track_motion_enable");
        const char* beta = std::getenv("ZLY_TRACK_BETA");
        track_beta_ = (beta && *beta) ? (float)std::atof(beta) : -1.0f;
        const char* vmax = std::getenv("ZLY_TRACK_VMAX");
        track_vmax_ = (vmax && *vmax) ? (float)std::atof(vmax) : -1.0f;
    }
    const int ndev = simulate_ ? 0 : std::max(1, envInt("ZLY_NUM_DEVICES", 1));
    const int dev0 = std::max(0, envInt("ZLY_FIRST_DEVICE", 0));
    first_device_ = dev0;
    // ZLY_ENGINES_PER_GPU (default 2): several engine instances per GPU, each one chain of launches on its own stream; consecutive
    // requests go to different instances and their batches overlap on the device (one instance leaves the chip idle at every kernel
    // boundary): 67k -> 82k frames/s host to host.  Two compute streams + the shared upload stream + the null stream = the four
    // hardware queues ROCm gives a process; a third instance shares a queue and is slower
    engines_per_gpu_ = std::max(1, std::min(8, envInt("ZLY_ENGINES_PER_GPU", 2)));
    std::vector<std::shared_ptr<EngineHandle>> fresh;
    for (int d = 0; d < ndev * engines_per_gpu_; ++d) {
        int32_t rc = ZLY_OK;
        std::string msg;
        auto e = createEngineOn(dev0 + d / engines_per_gpu_, &rc, &msg);
        if (!e) return Result<void>::error(toErrorCode(rc), "Failed to initialize HIP inference engine: " + msg);
        fresh.push_back(std::move(e));
    }
    {
        std::lock_guard<std::mutex> lk(engines_mutex_);
        engines_ = std::move(fresh);
        std::atomic_store(&engines_snapshot_, std::make_shared<const std::vector<std::shared_ptr<EngineHandle>>>(engines_));
    }
    {
        std::lock_guard<std::mutex> lk(stats_mutex_);
        model_hash_ = simulate_ ? std::string() : sha256File(config_.model_path);
    }
    if (simulate_) {
        // std::random_device like the reference (:1137-1138), or a fixed seed for tests (ZLY_SIMULATE_SEED)
        std::random_device rd;
        const int seed = envInt("ZLY_SIMULATE_SEED", -1);
        for (int i = 0; i < 4; ++i) sim_rng_state_[i] = seed >= 0 ? (uint32_t)seed * 2654435761u + (uint32_t)i : rd();
    }
    model_version_ = 1;
    {
        std::lock_guard<std::mutex> lk(queue_mutex_);
        pending_.assign((size_t)(ndev * engines_per_gpu_) + 1, std::deque<Pending>());     // nothing of a previous run may be emitted under the new sequence numbers
        pending_count_ = 0;
        ring_.assign(1024, Done{});
        ring_full_.assign(1024, 0);
        finished_count_ = 0;
        next_seq_ = 0;
        next_emit_ = 0;
    }
    running_ = true;
    {
        std::lock_guard<std::mutex> lk(reap_mutex_);
        reap_stop_ = false;
    }
    reaper_ = std::thread(&HipInferenceEngine::reaperLoop, this);
    completer_ = std::thread(&HipInferenceEngine::completionLoop, this);
    if (!simulate_ && envInt("ZLY_MODEL_WATCH_MS", 10000) > 0) monitor_ = std::thread(&HipInferenceEngine::monitorLoop, this);
    return Result<void>::ok();
}

std::shared_ptr<HipInferenceEngine::EngineHandle> HipInferenceEngine::createEngineOn(int device, int32_t* rc, std::string* msg) const
{
    zly_config c;
    zly_default_config(&c);
    c.weights_path = config_.model_path.c_str();
    c.model_w = config_.detection.model_width;
    c.model_h = config_.detection.model_height;
    c.conf_thr = config_.confidence_threshold;
    c.iou_thr = config_.nms_threshold;
    c.max_batch = max_batch_;
    c.max_dets = max_dets_;
    c.device = device;
    c.dtype = envInt("ZLY_FP32", 0) ? ZLY_DTYPE_FP32 : ZLY_DTYPE_BF16;
    c.warmup_runs = 3;                                   // onnx_engine.cpp:919-954
    c.use_graph = 1;
    // the server only consumes detections; one engine per GPU: NMS of a batch runs beside the next one; several: one chain each
    c.flags = ZLY_FLAG_NO_HEAD_TENSOR | (engines_per_gpu_ > 1 ? ZLY_FLAG_SINGLE_CHAIN : ZLY_FLAG_ASYNC_NMS) | (letterbox_ ? ZLY_FLAG_LETTERBOX : 0) | (area_ ? ZLY_FLAG_AREA : 0);
    zly_engine* e = nullptr;
    *rc = zly_create(&c, &e);
    if (*rc != ZLY_OK) { *msg = zly_last_error(); return nullptr; }
    auto h = std::make_shared<EngineHandle>(e);
    if (track_) {
        zly_track_config tc;
        zly_default_track_config(&tc);
        tc.max_streams = track_streams_;
        tc.max_tracks = 64;
        if (track_iou_ >= 0.0f) tc.match_iou = track_iou_;
        if (track_max_lost_ >= 0) tc.max_lost = track_max_lost_;
        *rc = zly_track_enable(e, &tc);
        if (*rc != ZLY_OK) { *msg = zly_last_error(); return nullptr; }      // h destroys the engine
        if (track_motion_) {
            zly_track_motion_config mc;
            zly_default_track_motion_config(&mc);
            if (track_beta_ >= 0.0f) mc.beta = track_beta_;
            if (track_vmax_ >= 0.0f) mc.v_max = track_vmax_;
            *rc = zly_track_motion_enable(e, &mc);
            if (*rc != ZLY_OK) { *msg = zly_last_error(); return nullptr; }
        }
        h->track_slots.assign((size_t)track_streams_, EngineHandle::TrackSlot());
    }
    return h;
}

// Build the new engines first (hundreds of milliseconds: weight repack, upload, warm-up, beside the running ones), then
// swap the handles: requests submitted from then on go to the new model, requests already in flight finish on the old
// engine, which is destroyed with its last pending request.  Any failure leaves the running model untouched.
Result<void> HipInferenceEngine::reloadModel()
{
    if (!running_) return Result<void>::error(ErrorCode::NOT_INITIALIZED, "Engine not running");
    if (simulate_) return Result<void>::error(ErrorCode::INVALID_ARGUMENT, "simulation mode has no model to reload");
    std::lock_guard<std::mutex> rl(reload_mutex_);
    const std::string hash = sha256File(config_.model_path);
    size_t count;
    {
        std::lock_guard<std::mutex> lk(engines_mutex_);
        count = engines_.size();
    }
    std::vector<std::shared_ptr<EngineHandle>> fresh;
    for (size_t d = 0; d < count; ++d) {
        int32_t rc = ZLY_OK;
        std::string msg;
        auto e = createEngineOn(first_device_ + (int)d / engines_per_gpu_, &rc, &msg);
        if (!e) return Result<void>::error(toErrorCode(rc), "Failed to reload model: " + msg);
        fresh.push_back(std::move(e));
    }
    {
        std::lock_guard<std::mutex> lk(engines_mutex_);
        engines_.swap(fresh);
        std::atomic_store(&engines_snapshot_, std::make_shared<const std::vector<std::shared_ptr<EngineHandle>>>(engines_));
    }
    for (auto& h : fresh) { h->replaced = true; retire(std::move(h)); }     // old engines go -- on the reaper thread -- when their last pending request is done
    fresh.clear();
    {
        std::lock_guard<std::mutex> lk(stats_mutex_);
        model_hash_ = hash;
    }
    model_version_++;
    return Result<void>::ok();
}

// Engines replaced by a hot reload: the reaper takes a reference of each and KEEPS it until it is the only one left (requests in flight on the old
// engine hold the others), then runs zly_destroy -- on its own thread, never on the completion thread or a submitting thread.
void HipInferenceEngine::retire(std::shared_ptr<EngineHandle>&& h)
{
    if (!h) return;
    {
        std::lock_guard<std::mutex> lk(reap_mutex_);
        retired_.push_back(std::move(h));
    }
    reap_cv_.notify_one();
}

// A finished request lets go of its engine.  That is an atomic decrement and never the last reference: engines_ holds one while the engine serves, the
// reaper holds one from the moment a reload replaces it until every request has let go.  (Round 3 pushed EVERY frame's reference through reap_mutex_
// and the reaper's vector.)
void HipInferenceEngine::release(std::shared_ptr<EngineHandle>&& h) { h.reset(); }

void HipInferenceEngine::reaperLoop()
{
    std::vector<std::shared_ptr<EngineHandle>> mine, dead;
    while (true) {
        bool stop;
        {
            std::unique_lock<std::mutex> lk(reap_mutex_);
            reap_cv_.wait_for(lk, std::chrono::milliseconds(mine.empty() ? 50 : 5), [&] { return reap_stop_ || !retired_.empty(); });
            for (auto& h : retired_) mine.push_back(std::move(h));
            retired_.clear();
            stop = reap_stop_;
        }
        // sole owner = the last request on that engine has been delivered: destroy it here.  At shutdown the completion thread has been joined already;
        // what is still referenced elsewhere (requests dropped by shutdown) is let go and dies with its last reference on the shutting-down thread.
        for (auto& h : mine)
            if (stop || h.use_count() == 1) dead.push_back(std::move(h));
        mine.erase(std::remove(mine.begin(), mine.end(), nullptr), mine.end());
        dead.clear();                                           // zly_destroy runs here
        if (stop) return;
    }
}

void HipInferenceEngine::monitorLoop()
{
    const int period_ms = std::max(50, envInt("ZLY_MODEL_WATCH_MS", 10000));
    int waited = 0;
    while (running_) {
        std::this_thread::sleep_for(std::chrono::milliseconds(50));
        waited += 50;
        if (waited < period_ms) continue;
        waited = 0;
        const std::string now = sha256File(config_.model_path);
        if (now.empty()) continue;                              // file missing: keep serving (onnx_engine.cpp:484-488)
        std::string last;
        {
            std::lock_guard<std::mutex> lk(stats_mutex_);
            last = model_hash_;
        }
        if (now != last) {
            auto r = reloadModel();
            if (r.hasError()) {                                 // remember the bad file so it is not retried every period
                std::lock_guard<std::mutex> lk(stats_mutex_);
                model_hash_ = now;
            }
        }
    }
}

Result<void> HipInferenceEngine::shutdown()
{
    if (!running_.exchange(false)) {
        return Result<void>::ok();
    }
    {
        std::lock_guard<std::mutex> lk(queue_mutex_);
        queue_cv_.notify_all();
    }
    if (completer_.joinable()) completer_.join();               // hands over what is already on the device, then stops
    if (monitor_.joinable()) monitor_.join();
    {
        std::lock_guard<std::mutex> lk(reap_mutex_);
        reap_stop_ = true;
    }
    reap_cv_.notify_all();
    if (reaper_.joinable()) reaper_.join();
    {
        std::lock_guard<std::mutex> lk(queue_mutex_);
        dropped_frames_ += pending_count_;
        for (auto& q : pending_) q.clear();                     // stale results must never be emitted by a later initialize()
        pending_count_ = 0;
        ring_.clear(); ring_full_.clear(); finished_count_ = 0;
    }
    std::vector<std::shared_ptr<EngineHandle>> old;
    {
        std::lock_guard<std::mutex> lk(engines_mutex_);
        old.swap(engines_);
        std::atomic_store(&engines_snapshot_, std::shared_ptr<const std::vector<std::shared_ptr<EngineHandle>>>());
    }
    old.clear();
    return Result<void>::ok();
}

// ZLY_TRACK: the stream slot of a client on its engine.  Known client: its slot.  New client: a slot never used, else the least recently used one,
// whose tracks are cleared (zly_track_reset, ids go on counting) before the new client's first frame.
int32_t HipInferenceEngine::trackSlotFor(EngineHandle& h, uint32_t client_id) const
{
    std::lock_guard<std::mutex> lk(h.track_mu);
    const uint64_t now = ++h.track_clock;
    auto it = h.track_slot_of.find(client_id);
    if (it != h.track_slot_of.end()) { h.track_slots[(size_t)it->second].last_use = now; return it->second; }
    int32_t pick = -1;
    for (size_t i = 0; i < h.track_slots.size() && pick < 0; ++i) if (!h.track_slots[i].used) pick = (int32_t)i;
    if (pick < 0) {
        pick = 0;
        for (size_t i = 1; i < h.track_slots.size(); ++i) if (h.track_slots[i].last_use < h.track_slots[(size_t)pick].last_use) pick = (int32_t)i;
        h.track_slot_of.erase(h.track_slots[(size_t)pick].client);
        if (zly_track_reset(h.e, pick, 0) != ZLY_OK) return -1;
    }
    EngineHandle::TrackSlot& sl = h.track_slots[(size_t)pick];
    sl.client = client_id; sl.last_use = now; sl.used = true;
    h.track_slot_of[client_id] = pick;
    return pick;
}

// Runs on the caller's thread (the UDP receive thread in the reference's server, network_server.cpp:209): the request's
// pixels are copied ONCE, into the engine's pinned staging ring; nothing of `request` is retained.
Result<void> HipInferenceEngine::submitInference(const InferenceRequest& request)
{
    if (!running_) return Result<void>::error(ErrorCode::NOT_INITIALIZED, "Engine not running");
    const uint64_t seq = next_seq_.fetch_add(1);
    Pending p;
    p.seq = seq;
    p.client_id = request.client_id; p.frame_id = request.frame_id; p.timestamp = request.timestamp;
    p.enqueue_ms = wallMs();
    if (simulate_) {
        // the reference's simulation mode checks nothing about the frame (runInference, :524-528)
        p.simulated = true;
    } else {
        const auto snap = std::atomic_load(&engines_snapshot_);                           // immutable snapshot: no lock shared by the submitting threads
        if (!snap || snap->empty()) {
            p.failed = true;
        } else {
            // One frame per engine, round robin -- offered without blocking first: when the engine whose turn it is has every ring slot
            // busy, the frame goes to the next one that has room, and only if all are back-pressured does the caller wait (on the engine whose turn
            // it was).  With the blocking call alone all submitting threads ended up waiting on ONE engine's ring while the other idled (round 4:
            // plugin 72k -> 77k frames/s against the C ABI's 86-94k with threads pinned to engines).  Results are re-ordered by sequence number.
            // A request with the wrong byte count fails alone (INVALID_INPUT, onnx_engine.cpp:659-665): counted, no callback.
            const size_t ne = snap->size(), first = (size_t)(seq % ne);
            int32_t rc = ZLY_PENDING;
            // ZLY_CROP: the window of this request as a view of its (tight) frame; the engine copies the window's rows only
            zly_frame_view win;
            int32_t vrc = ZLY_OK;
            if (crop_w_ > 0 && request.width >= crop_w_ && request.height >= crop_h_) {
                zly_frame_view whole;
                vrc = zly_view_tight(input_format_, request.width, request.height, &whole);
                if (vrc == ZLY_OK && request.data.size() != zly_view_bytes(&whole)) vrc = ZLY_ERR_INVALID_INPUT;     // as a whole frame of the wrong size
                if (vrc == ZLY_OK) {
                    p.crop_x0 = (request.width - crop_w_) / 2; p.crop_y0 = (request.height - crop_h_) / 2;
                    if (isYuvFormat(input_format_)) { p.crop_x0 &= ~1; p.crop_y0 &= ~1; }
                    if (isYuv422Format(input_format_)) p.crop_x0 &= ~1;
                    p.frame_w = request.width; p.frame_h = request.height;
                    vrc = zly_view_crop(&whole, p.crop_x0, p.crop_y0, crop_w_, crop_h_, &win);
                    p.cropped = vrc == ZLY_OK;
                }
            }
            // ZLY_TRACK: the client's engine and its stream slot there; the request as a view (its window, or its whole tight frame)
            int32_t track_slot = -1;
            if (track_ && vrc == ZLY_OK) {
                if (!p.cropped) {
                    vrc = zly_view_tight(input_format_, request.width, request.height, &win);
                    if (vrc == ZLY_OK && request.data.size() != zly_view_bytes(&win)) vrc = ZLY_ERR_INVALID_INPUT;
                    else if (vrc != ZLY_OK) vrc = ZLY_ERR_INVALID_INPUT;             // a size the format does not allow: as a frame of the wrong size
                }
                if (vrc == ZLY_OK) {
                    track_slot = trackSlotFor(*(*snap)[(size_t)(request.client_id % ne)], request.client_id);
                    if (track_slot < 0) vrc = ZLY_ERR_INFERENCE;
                }
            }
            auto offer = [&](zly_engine* e, bool blocking) -> int32_t {
                if (track_)
                    return blocking ? zly_submit_view_tracked(e, request.data.data(), request.data.size(), &win, track_slot, &p.ticket)
                                    : zly_submit_try_view_tracked(e, request.data.data(), request.data.size(), &win, track_slot, &p.ticket);
                if (p.cropped)
                    return blocking ? zly_submit_view(e, request.data.data(), request.data.size(), &win, &p.ticket)
                                    : zly_submit_try_view(e, request.data.data(), request.data.size(), &win, &p.ticket);
                if (input_format_ == ZLY_PIX_BGR)
                    return blocking ? zly_submit(e, request.data.data(), request.data.size(), request.width, request.height, &p.ticket)
                                    : zly_submit_try(e, request.data.data(), request.data.size(), request.width, request.height, &p.ticket);
                return blocking ? zly_submit_fmt(e, input_format_, request.data.data(), request.data.size(), request.width, request.height, &p.ticket)
                                : zly_submit_try_fmt(e, input_format_, request.data.data(), request.data.size(), request.width, request.height, &p.ticket);
            };
            if (vrc != ZLY_OK) rc = vrc;
            if (track_ && rc == ZLY_PENDING) {
                // a client's frames are one stream of ONE engine: no round robin and no spill-over; non-blocking first only to keep the two calls' order of the untracked path
                p.slot = (size_t)(request.client_id % ne);
                p.engine = (*snap)[p.slot];
                rc = offer(p.engine->e, false);
                if (rc == ZLY_PENDING) rc = offer(p.engine->e, true);
            }
            for (size_t k = 0; k < ne && rc == ZLY_PENDING; ++k) {
                p.slot = (first + k) % ne;
                p.engine = (*snap)[p.slot];
                rc = offer(p.engine->e, false);
            }
            if (rc == ZLY_PENDING) {
                p.slot = first;
                p.engine = (*snap)[first];
                rc = offer(p.engine->e, true);
            }
            if (rc != ZLY_OK) { p.failed = true; p.engine.reset(); }
        }
        if (p.failed) inference_errors_++;
    }
    bool wake;
    {
        std::lock_guard<std::mutex> lk(queue_mutex_);
        if (pending_.empty()) return Result<void>::error(ErrorCode::NOT_INITIALIZED, "Engine not running");     // shutdown() got in between
        wake = pending_count_ == 0;                              // the completion thread only sleeps on empty queues
        const size_t qi = (p.failed || p.simulated) ? pending_.size() - 1 : std::min(p.slot, pending_.size() - 2);
        pending_[qi].push_back(std::move(p));
        ++pending_count_;
        const size_t depth = (size_t)(seq + 1 - next_emit_);
        if (depth > queue_high_water_mark_) queue_high_water_mark_ = depth;
    }
    if (wake) queue_cv_.notify_one();
    return Result<void>::ok();
}

void HipInferenceEngine::setCallback(InferenceCallback callback)
{
    std::lock_guard<std::mutex> lk(queue_mutex_);
    callback_ = std::move(callback);
}

size_t HipInferenceEngine::getQueueSize() const
{
    std::lock_guard<std::mutex> lk(queue_mutex_);
    return (size_t)(next_seq_.load() - next_emit_);              // submitted, not yet handed to the callback (or dropped as failed)
}

std::string HipInferenceEngine::getName() const { return "hip"; }

// generateRandomDetections of the reference's simulation mode (onnx_engine.cpp:1133-1177), ZLY_SIMULATE=1 only: 0-5 detections, centre in [0.1, 0.9],
// width in [0.05, 0.2], height = 1.5 x a second draw from that range, confidence in [0.6, 1.0], class in 0..3, track_id = i + 1, timestamp = now (ms).
std::vector<Detection> HipInferenceEngine::generateRandomDetections()
{
    auto next = [this]() {                                       // xoshiro128**: small, seedable state owned by the completion thread
        uint32_t* st = sim_rng_state_;
        const uint32_t x = st[1] * 5u, r = ((x << 7) | (x >> 25)) * 9u, t = st[1] << 9;
        st[2] ^= st[0]; st[3] ^= st[1]; st[1] ^= st[2]; st[0] ^= st[3]; st[2] ^= t; st[3] = (st[3] << 11) | (st[3] >> 21);
        return r;
    };
    auto uni = [&](double lo, double hi) { return lo + (hi - lo) * ((double)(next() >> 8) * (1.0 / 16777216.0)); };
    std::vector<Detection> out((size_t)(next() % 6u));
    const uint64_t now = wallMs();
    for (size_t i = 0; i < out.size(); ++i) {
        Detection& d = out[i];
        d.box.x = (float)uni(0.1, 0.9); d.box.y = (float)uni(0.1, 0.9);
        d.box.width = (float)uni(0.05, 0.2); d.box.height = (float)uni(0.05, 0.2) * 1.5f;
        d.confidence = (float)uni(0.6, 1.0);
        d.class_id = (int)(next() % 4u);
        d.track_id = (uint32_t)i + 1;
        d.timestamp = now;
    }
    return out;
}

// One engine-owned thread hands results to the callback in submission order (reference: the inference thread,
// onnx_engine.cpp:355-364); several GPUs finishing out of order are re-ordered by the sequence number.
// Per wake-up it takes EVERYTHING that is pending (one lock), blocks for the first ticket and then collects, without blocking, every following
// ticket whose batch is back as well (zly_poll): a device batch of 64 frames costs two lock acquisitions on queue_mutex_ and one on stats_mutex_,
// where round 3 paid two + one per FRAME against twelve submitting threads on the same mutex.
void HipInferenceEngine::completionLoop()
{
    std::vector<zly_det> dets((size_t)max_dets_);
    std::vector<std::deque<Pending>> local;                     // per engine slot (the last queue: requests without a ticket), in ticket order
    size_t local_count = 0;
    std::vector<std::pair<uint64_t, Done>> group;               // (sequence number, result) of the frames completed in this round
    std::vector<Done> ready;
    auto take = [&](Pending& p) {                               // consume one request whose result is available (or whose batch this call waits for)
        Done d;
        d.client_id = p.client_id; d.enqueue_ms = p.enqueue_ms;
        if (p.simulated) {
            d.ok = true;
            d.state.frame_id = p.frame_id; d.state.timestamp = p.timestamp;
            d.state.detections = generateRandomDetections();
        } else if (!p.failed) {
            int32_t n = 0;
            const int32_t rc = zly_wait(p.engine->e, p.ticket, dets.data(), max_dets_, &n);
            if (rc == ZLY_OK) {
                d.ok = true;
                d.state.frame_id = p.frame_id;                   // onnx_engine.cpp:520-521
                d.state.timestamp = p.timestamp;
                const int cnt = std::min<int>(n, max_dets_);
                static_assert(sizeof(zly_det) == sizeof(Detection), "zly_det must be layout-identical to Detection");
                d.state.detections.resize((size_t)cnt);
                if (cnt) std::memcpy(d.state.detections.data(), dets.data(), (size_t)cnt * sizeof(Detection));
                if (p.cropped)                                   // boxes came back as fractions of the window: make them fractions of the request frame
                    for (Detection& det : d.state.detections) mapCropToFrame(det, p.crop_x0, p.crop_y0, crop_w_, crop_h_, p.frame_w, p.frame_h);
            } else {
                inference_errors_++;
            }
            release(std::move(p.engine));                        // an engine replaced by a reload goes with its last request -- on the reaper thread
        }
        group.emplace_back(p.seq, std::move(d));
    };
    while (true) {
        {
            std::unique_lock<std::mutex> lk(queue_mutex_);
            if (local_count == 0) {
                queue_cv_.wait_for(lk, std::chrono::milliseconds(100), [&] { return pending_count_ != 0 || !running_; });
                if (pending_count_ == 0) {
                    if (!running_) return;                       // shutting down: everything already in the rings has been handed over
                    continue;
                }
            }
            if (local.size() != pending_.size()) local.resize(pending_.size());
            for (size_t i = 0; i < pending_.size(); ++i)         // everything that is pending, under ONE lock
                while (!pending_[i].empty()) { local[i].push_back(std::move(pending_[i].front())); pending_[i].pop_front(); ++local_count; }
            pending_count_ = 0;
        }
        group.clear();
        // every engine's tickets whose batch is back, without blocking (requests without a ticket are always ready)
        for (size_t i = 0; i < local.size(); ++i)
            while (!local[i].empty()) {
                Pending& p = local[i].front();
                if (!p.failed && !p.simulated && zly_poll(p.engine->e, p.ticket) != ZLY_OK) break;
                take(p);
                local[i].pop_front(); --local_count;
            }
        if (group.empty() && local_count != 0) {
            // nothing is back yet: wait for the oldest request's batch (the one the callback order needs first)
            size_t best = local.size();
            for (size_t i = 0; i < local.size(); ++i)
                if (!local[i].empty() && (best == local.size() || local[i].front().seq < local[best].front().seq)) best = i;
            take(local[best].front());
            local[best].pop_front(); --local_count;
        }
        // hand over in submission order
        ready.clear();
        InferenceCallback cb;
        {
            std::lock_guard<std::mutex> lk(queue_mutex_);
            for (auto& g : group) {
                while (g.first - next_emit_ >= ring_.size()) {   // more sequence numbers outstanding than the ring holds: double it (re-placing what it holds)
                    std::vector<Done> bigger(ring_.size() * 2);
                    std::vector<uint8_t> full(ring_.size() * 2, 0);
                    for (uint64_t q = next_emit_; q < next_emit_ + ring_.size(); ++q)
                        if (ring_full_[q & (ring_.size() - 1)]) { bigger[q & (bigger.size() - 1)] = std::move(ring_[q & (ring_.size() - 1)]); full[q & (bigger.size() - 1)] = 1; }
                    ring_.swap(bigger); ring_full_.swap(full);
                }
                const size_t at = (size_t)(g.first & (ring_.size() - 1));
                ring_[at] = std::move(g.second); ring_full_[at] = 1; ++finished_count_;
            }
            while (ring_full_[next_emit_ & (ring_.size() - 1)]) {
                const size_t at = (size_t)(next_emit_ & (ring_.size() - 1));
                ready.push_back(std::move(ring_[at]));
                ring_full_[at] = 0; --finished_count_;
                ++next_emit_;
            }
            cb = callback_;
        }
        if (ready.empty()) continue;
        {
            std::lock_guard<std::mutex> lk(stats_mutex_);
            const uint64_t now = wallMs();
            for (const Done& r : ready) {
                if (!r.ok) continue;
                const double lat = (double)(now - r.enqueue_ms);
                latency_window_ms_.push_back(lat);
                if (latency_window_ms_.size() > 100) latency_window_ms_.pop_front();
                total_latency_ms_ += lat;
            }
        }
        for (Done& r : ready) {
            if (!r.ok) continue;                                 // not invoked on error results (onnx_engine.cpp:380-388)
            inference_count_++;
            if (cb) cb(r.client_id, r.state);
        }
    }
}

std::unordered_map<std::string, std::string> HipInferenceEngine::getStatus() const
{
    std::unordered_map<std::string, std::string> s;
    s["name"] = getName();
    s["simulation_mode"] = simulate_ ? "true" : "false";
    s["running"] = running_ ? "true" : "false";
    s["model_path"] = config_.model_path;
    s["model_version"] = std::to_string(model_version_.load());
    { std::lock_guard<std::mutex> lk(stats_mutex_); s["model_hash"] = model_hash_; }
    s["int8_quantization"] = "disabled";
    s["zero_copy"] = "disabled";
    s["queue_size"] = std::to_string(getQueueSize());
    s["queue_high_water_mark"] = std::to_string(queue_high_water_mark_.load());
    s["inference_count"] = std::to_string(inference_count_.load());
    s["inference_errors"] = std::to_string(inference_errors_.load());
    s["dropped_frames"] = std::to_string(dropped_frames_.load());
    s["dynamic_batching"] = "enabled";
    s["resize_mode"] = resizeModeName(letterbox_, area_);
    s["input_format"] = inputFormatName(input_format_);
    s["tracking"] = track_ ? "on" : "off";
    s["track_motion"] = track_motion_ ? "on" : "off";
    s["crop"] = crop_w_ > 0 ? std::to_string(crop_w_) + "x" + std::to_string(crop_h_) : "off";
    double avg = 0, p99 = 0;
    {
        std::lock_guard<std::mutex> lk(stats_mutex_);
        if (!latency_window_ms_.empty()) {
            std::vector<double> v(latency_window_ms_.begin(), latency_window_ms_.end());
            std::sort(v.begin(), v.end());
            for (double x : v) avg += x;
            avg /= (double)v.size();
            p99 = v[std::min(v.size() - 1, (size_t)(v.size() * 0.99))];
        }
    }
    s["avg_inference_time_ms"] = std::to_string(avg);
    s["p99_inference_time_ms"] = std::to_string(p99);
    // per-phase device time, sampled by the engine on every 16th batch (the reference accumulates its three phase
    // timers per frame, onnx_engine.cpp:530-557,605-618).  zly_get_stats never waits on a running batch.
    std::vector<std::shared_ptr<EngineHandle>> engines;
    {
        std::lock_guard<std::mutex> lk(engines_mutex_);
        engines = engines_;
    }
    uint64_t frames = 0, batches = 0, replays = 0, eager = 0;
    double pre = 0, fwd = 0, post = 0;
    for (const auto& h : engines) {
        zly_stats st{};
        if (zly_get_stats(h->e, &st) != ZLY_OK) continue;
        frames += st.sampled_frames; batches += st.batches; replays += st.graph_replays; eager += st.eager_batches;
        pre += st.sampled_preprocess_ms; fwd += st.sampled_forward_ms; post += st.sampled_postprocess_ms;
    }
    s["batches"] = std::to_string(batches);
    s["graph_replays"] = std::to_string(replays);          // batches whose forward was one hipGraph replay (lone frames and full batches) ...
    s["eager_batches"] = std::to_string(eager);            // ... or kernel-by-kernel launches (partial batches)
    s["avg_preprocessing_time_ms"] = frames ? std::to_string(pre / (double)frames) : "0";
    s["avg_forward_time_ms"] = frames ? std::to_string(fwd / (double)frames) : "0";
    s["avg_postprocessing_time_ms"] = frames ? std::to_string(post / (double)frames) : "0";
    s["weight_format"] = (!engines.empty() && zly_weights_fp8(engines[0]->e)) ? "fp8_e4m3" : "fp32";      // the reference's "quantised" model claim (README.md:84)
    size_t in_use = 0;
    for (const auto& h : engines) {
        std::lock_guard<std::mutex> lk(h->track_mu);
        in_use += h->track_slot_of.size();
    }
    s["track_streams_in_use"] = std::to_string(in_use);
    s["worker_threads"] = std::to_string(engines.size());
    s["devices"] = std::to_string(engines.size() / (size_t)std::max(1, engines_per_gpu_));
    s["engines_per_gpu"] = std::to_string(engines_per_gpu_);
    return s;
}

std::unique_ptr<IInferenceEngine> HipInferenceEngineFactory::createEngine(const ServerConfig& config)
{
    return std::make_unique<HipInferenceEngine>(config);
}

std::string HipInferenceEngineFactory::getName() const { return "hip"; }

REGISTER_INFERENCE_ENGINE(HipInferenceEngineFactory)

}  // namespace zero_latency
