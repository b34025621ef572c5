// test_plugin_track_motion_stub.cpp -- the plugin's ZLY_TRACK_MOTION (the tracker's motion model on every engine) without a GPU: with the variable the
// plugin calls zly_track_motion_enable once per engine, after zly_track_enable, with ZLY_TRACK_BETA / ZLY_TRACK_VMAX; without it, never; the variable is
// refused without ZLY_TRACK=1, and when the library lacks the call.
// TEST INFRASTRUCTURE, in the manner of test_plugin_track_stub.cpp: host/hip_inference_engine.cpp is compiled into this binary together with a
// link-time stub of the C-ABI entry points it calls.  The stub is not a CPU fallback of the product: its fake engines record the calls and "detect"
// one fixed box per frame.  Built a second time with -DNO_MOTION_SYMBOLS, the stub has the tracking calls but not the motion model's.
//
//   test_plugin_track_motion_stub <report.txt> <motion|defaults|plain|notrack>
#include "../../zero-latency-yolo_amd/host/hip_inference_engine.cpp"

#include <fstream>
#include <sstream>
#include <thread>

// ------------------------------------------------------------------------------------------------ stub of the C ABI
struct zly_engine {
    int index = 0;
    std::mutex mu;
    std::map<uint64_t, int> pending;
    uint64_t next_ticket = 1;
    std::atomic<uint64_t> frames{0};
    int max_dets = 0;
};
namespace {
std::mutex g_mu;
std::vector<std::string> g_log;                          // every enable and every submit, in order
int g_engines = 0, g_motion_calls = 0;
thread_local std::string g_err;

void note(const std::string& s) { std::lock_guard<std::mutex> lg(g_mu); g_log.push_back(s); }
int32_t accept(zly_engine* e, int stream, uint64_t* ticket)
{
    {
        std::lock_guard<std::mutex> lk(e->mu);
        *ticket = e->next_ticket++;
        e->pending[*ticket] = stream;
    }
    std::ostringstream o;
    o << "submit:" << e->index << ":" << stream;
    note(o.str());
    return ZLY_OK;
}
}

extern "C" {
void zly_default_config(zly_config* c) { std::memset(c, 0, sizeof *c); c->model_w = 416; c->model_h = 416; c->conf_thr = 0.5f; c->iou_thr = 0.45f; c->max_batch = 1; c->max_dets = 64; c->warmup_runs = 3; c->use_graph = 1; }
const char* zly_last_error(void) { return g_err.c_str(); }
int32_t zly_create(const zly_config* c, zly_engine** out)
{
    *out = new zly_engine();
    (*out)->max_dets = c->max_dets;
    std::lock_guard<std::mutex> lg(g_mu);
    (*out)->index = g_engines++;
    return ZLY_OK;
}
int32_t zly_destroy(zly_engine* e) { delete e; return ZLY_OK; }
size_t zly_view_bytes(const zly_frame_view* v) { return v->fmt == ZLY_PIX_BGR && v->w >= 1 && v->h >= 1 ? (size_t)v->off[0] + (size_t)(v->h - 1) * (size_t)v->pitch[0] + 3u * (size_t)v->w : 0; }
int32_t zly_view_tight(int32_t fmt, int32_t w, int32_t h, zly_frame_view* out)
{
    if (fmt != ZLY_PIX_BGR || w < 1 || h < 1) return ZLY_ERR_INVALID_ARGUMENT;
    std::memset(out, 0, sizeof *out);
    out->fmt = fmt; out->w = w; out->h = h; out->pitch[0] = 3 * w;
    return ZLY_OK;
}
int32_t zly_submit(zly_engine* e, const uint8_t* bgr, size_t nbytes, int32_t w, int32_t h, uint64_t* ticket)
{
    if (!bgr || nbytes != (size_t)w * (size_t)h * 3) { g_err = "Invalid image data size"; return ZLY_ERR_INVALID_INPUT; }
    return accept(e, -1, ticket);
}
int32_t zly_submit_try(zly_engine* e, const uint8_t* bgr, size_t nbytes, int32_t w, int32_t h, uint64_t* ticket) { return zly_submit(e, bgr, nbytes, w, h, ticket); }
void zly_default_track_config(zly_track_config* c) { c->max_streams = 64; c->max_tracks = 64; c->match_iou = 0.3f; c->max_lost = 6; }
int32_t zly_track_enable(zly_engine* e, const zly_track_config*)
{
    std::ostringstream o;
    o << "enable:" << e->index;
    note(o.str());
    return ZLY_OK;
}
int32_t zly_track_reset(zly_engine*, int32_t, uint32_t) { return ZLY_OK; }
int32_t zly_submit_view_tracked(zly_engine* e, const uint8_t* base, size_t buf_bytes, const zly_frame_view* v, int32_t stream, uint64_t* ticket)
{
    const size_t need = zly_view_bytes(v);
    if (!base || !need || need > buf_bytes) { g_err = "Invalid image data size"; return ZLY_ERR_INVALID_INPUT; }
    return accept(e, stream, ticket);
}
int32_t zly_submit_try_view_tracked(zly_engine* e, const uint8_t* base, size_t buf_bytes, const zly_frame_view* v, int32_t stream, uint64_t* ticket)
{
    return zly_submit_view_tracked(e, base, buf_bytes, v, stream, ticket);
}
#ifndef NO_MOTION_SYMBOLS
void zly_default_track_motion_config(zly_track_motion_config* c) { c->beta = 0.5f; c->v_max = 0.25f; { std::lock_guard<std::mutex> lg(g_mu); ++g_motion_calls; } }
int32_t zly_track_motion_enable(zly_engine* e, const zly_track_motion_config* c)
{
    { std::lock_guard<std::mutex> lg(g_mu); ++g_motion_calls; }
    std::ostringstream o;
    o << "motion:" << e->index << ":" << c->beta << ":" << c->v_max;
    note(o.str());
    return ZLY_OK;
}
#endif
int32_t zly_poll(zly_engine* e, uint64_t ticket)
{
    std::lock_guard<std::mutex> lk(e->mu);
    return e->pending.count(ticket) ? ZLY_OK : ZLY_ERR_INVALID_ARGUMENT;
}
int32_t zly_wait(zly_engine* e, uint64_t ticket, zly_det* out, int32_t cap, int32_t* n_out)
{
    int stream;
    {
        std::lock_guard<std::mutex> lk(e->mu);
        auto it = e->pending.find(ticket);
        if (it == e->pending.end()) return ZLY_ERR_INVALID_ARGUMENT;
        stream = it->second;
        e->pending.erase(it);
    }
    if (cap >= 1) {
        std::memset(out, 0, sizeof *out);
        out[0].x = 0.5f; out[0].y = 0.5f; out[0].w = 0.1f; out[0].h = 0.1f; out[0].confidence = 0.75f; out[0].class_id = 2;
        out[0].track_id = stream < 0 ? 0u : (uint32_t)(100 * (e->index + 1) + stream);
    }
    *n_out = 1;
    e->frames++;
    return ZLY_OK;
}
int32_t zly_get_stats(const zly_engine* e, zly_stats* out) { std::memset(out, 0, sizeof *out); out->batches = e->frames.load(); return ZLY_OK; }
int32_t zly_weights_fp8(const zly_engine*) { return 0; }
}

// ------------------------------------------------------------------------------------------------ the test
using namespace zero_latency;

int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    const std::string mode = argv[2];
    std::ofstream rep(argv[1]);
    setenv("ZLY_NUM_DEVICES", "1", 1); setenv("ZLY_ENGINES_PER_GPU", "2", 1); setenv("ZLY_MODEL_WATCH_MS", "0", 1);
    unsetenv("ZLY_CROP"); unsetenv("ZLY_INPUT_FORMAT"); unsetenv("ZLY_MAX_DETS");
    unsetenv("ZLY_TRACK"); unsetenv("ZLY_TRACK_MOTION"); unsetenv("ZLY_TRACK_BETA"); unsetenv("ZLY_TRACK_VMAX");
    if (mode != "notrack") { setenv("ZLY_TRACK", "1", 1); setenv("ZLY_TRACK_STREAMS", "2", 1); }
    if (mode != "plain") setenv("ZLY_TRACK_MOTION", "1", 1);
    if (mode == "motion") { setenv("ZLY_TRACK_BETA", "0.25", 1); setenv("ZLY_TRACK_VMAX", "0.125", 1); }
    const std::string model = std::string(argv[1]) + ".model";
    { std::ofstream m(model); m << "weights"; }
    ServerConfig config;
    config.model_path = model;
    config.inference_engine = "hip";
    auto engine = InferenceEngineManager::getInstance().createEngine("hip", config);
    if (!engine) return 3;
    std::mutex smu;
    int callbacks = 0;
    engine->setCallback([&](uint32_t, const GameState&) { std::lock_guard<std::mutex> lk(smu); ++callbacks; });
    auto r0 = engine->initialize();
    rep << "init_error=" << (r0.hasError() ? static_cast<int>(r0.error().code) : 0) << "\n";
    if (!r0.hasError()) {
        rep << "status_tracking=" << engine->getStatus()["tracking"] << "\nstatus_motion=" << engine->getStatus()["track_motion"] << "\n";
        const int n = 4;
        for (int i = 0; i < n; ++i) {
            InferenceRequest r;
            r.client_id = (uint32_t)(i % 2); r.frame_id = (uint32_t)i; r.timestamp = 7; r.width = 8; r.height = 8;
            r.data.assign(8 * 8 * 3, (uint8_t)i);
            if (engine->submitInference(r).hasError()) return 5;
        }
        for (int k = 0; k < 4000; ++k) {
            { std::lock_guard<std::mutex> lk(smu); if (callbacks >= n) break; }
            std::this_thread::sleep_for(std::chrono::milliseconds(1));
        }
        engine->shutdown();
        rep << "callbacks=" << callbacks << "\n";
    }
    rep << "motion_calls=" << g_motion_calls << "\n";
    for (size_t i = 0; i < g_log.size(); ++i) rep << "log[" << i << "]=" << g_log[i] << "\n";
    return 0;
}
