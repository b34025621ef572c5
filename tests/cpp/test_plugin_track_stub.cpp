// test_plugin_track_stub.cpp -- the plugin's ZLY_TRACK (track ids on the GPU: a client is one stream of one engine) without a GPU: engine affinity by
// client id, stable stream slots, least-recently-used reuse with a reset before the new client's first frame, and the switch being off by default.
// TEST INFRASTRUCTURE: host/hip_inference_engine.cpp is compiled into this binary together with a link-time stub of the C-ABI entry points it
// calls.  The stub is not a CPU fallback of the product: its fake engines record (engine, stream) of every submit and every reset, and "detect"
// one fixed box per frame.  Built a second time with -DNO_TRACK_SYMBOLS, the stub lacks the tracking calls: initialize() must then refuse ZLY_TRACK.
//
//   test_plugin_track_stub <report.txt> <on|off>
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
std::vector<std::string> g_log;                          // every submit, reset and enable, in order
int g_engines = 0, g_tracked_calls = 0;
thread_local std::string g_err;

void note(const std::string& s) { std::lock_guard<std::mutex> lg(g_mu); g_log.push_back(s); }
int32_t accept(zly_engine* e, int stream, bool tracked, uint64_t* ticket)
{
    {
        std::lock_guard<std::mutex> lk(e->mu);
        *ticket = e->next_ticket++;
        e->pending[*ticket] = stream;
    }
    std::ostringstream o;
    o << "submit:" << e->index << ":" << stream << ":" << (tracked ? 1 : 0);
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
    return accept(e, -1, false, ticket);
}
int32_t zly_submit_try(zly_engine* e, const uint8_t* bgr, size_t nbytes, int32_t w, int32_t h, uint64_t* ticket) { return zly_submit(e, bgr, nbytes, w, h, ticket); }
#ifndef NO_TRACK_SYMBOLS
void zly_default_track_config(zly_track_config* c) { c->max_streams = 64; c->max_tracks = 64; c->match_iou = 0.3f; c->max_lost = 6; { std::lock_guard<std::mutex> lg(g_mu); ++g_tracked_calls; } }
int32_t zly_track_enable(zly_engine* e, const zly_track_config* c)
{
    { std::lock_guard<std::mutex> lg(g_mu); ++g_tracked_calls; }
    if (c->max_tracks < e->max_dets || c->max_tracks > 64) { g_err = "max_tracks"; return ZLY_ERR_INVALID_ARGUMENT; }
    std::ostringstream o;
    o << "enable:" << e->index << ":" << c->max_streams << ":" << c->max_tracks << ":" << c->max_lost << ":" << e->max_dets;
    note(o.str());
    return ZLY_OK;
}
int32_t zly_track_reset(zly_engine* e, int32_t stream, uint32_t first_id)
{
    { std::lock_guard<std::mutex> lg(g_mu); ++g_tracked_calls; }
    std::ostringstream o;
    o << "reset:" << e->index << ":" << stream << ":" << first_id;
    note(o.str());
    return ZLY_OK;
}
int32_t zly_submit_view_tracked(zly_engine* e, const uint8_t* base, size_t buf_bytes, const zly_frame_view* v, int32_t stream, uint64_t* ticket)
{
    { std::lock_guard<std::mutex> lg(g_mu); ++g_tracked_calls; }
    const size_t need = zly_view_bytes(v);
    if (!base || !need || need > buf_bytes) { g_err = "Invalid image data size"; return ZLY_ERR_INVALID_INPUT; }
    return accept(e, stream, true, ticket);
}
int32_t zly_submit_try_view_tracked(zly_engine* e, const uint8_t* base, size_t buf_bytes, const zly_frame_view* v, int32_t stream, uint64_t* ticket)
{
    return zly_submit_view_tracked(e, base, buf_bytes, v, stream, ticket);
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
        out[0].track_id = stream < 0 ? 0u : (uint32_t)(100 * (e->index + 1) + stream);       // what a tracking engine would fill: non-zero, per stream
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
    const bool on = std::string(argv[2]) == "on";
    std::ofstream rep(argv[1]);
    setenv("ZLY_NUM_DEVICES", "1", 1); setenv("ZLY_ENGINES_PER_GPU", "2", 1); setenv("ZLY_MODEL_WATCH_MS", "0", 1);
    unsetenv("ZLY_CROP"); unsetenv("ZLY_INPUT_FORMAT"); unsetenv("ZLY_MAX_DETS");
    if (on) { setenv("ZLY_TRACK", "1", 1); setenv("ZLY_TRACK_STREAMS", "2", 1); setenv("ZLY_TRACK_MAX_LOST", "9", 1); }
    else unsetenv("ZLY_TRACK");
    const std::string model = std::string(argv[1]) + ".model";
    { std::ofstream m(model); m << "weights"; }
    ServerConfig config;
    config.model_path = model;
    config.inference_engine = "hip";
    auto engine = InferenceEngineManager::getInstance().createEngine("hip", config);
    if (!engine) return 3;
    std::mutex smu;
    std::vector<std::pair<uint32_t, uint32_t>> seen;          // (client, track id of its detection)
    engine->setCallback([&](uint32_t client, const GameState& st) {
        std::lock_guard<std::mutex> lk(smu);
        seen.emplace_back(client, st.detections.at(0).track_id);
    });
    auto r0 = engine->initialize();
    rep << "init_error=" << (r0.hasError() ? static_cast<int>(r0.error().code) : 0) << "\n";
    if (r0.hasError()) return 0;
    rep << "status_tracking=" << engine->getStatus()["tracking"] << "\n";
    // two engines, two stream slots each.  Clients 0 and 2 fill engine 0, clients 1 and 3 engine 1; client 4 then finds engine 0 full and takes
    // the slot of client 2 (used longest ago); client 2, back, takes client 4's; client 5 takes client 3's on engine 1
    const uint32_t clients[] = {0, 1, 2, 3, 0, 1, 4, 0, 2, 5, 5, 1};
    const int n = (int)(sizeof clients / sizeof clients[0]);
    for (int i = 0; i < n; ++i) {
        InferenceRequest r;
        r.client_id = clients[i]; r.frame_id = (uint32_t)i; r.timestamp = 7; r.width = 8; r.height = 8;
        r.data.assign(8 * 8 * 3, (uint8_t)i);
        if (engine->submitInference(r).hasError()) return 5;
    }
    // a frame with the wrong byte count fails alone: counted, no callback, no stream slot taken
    {
        InferenceRequest r;
        r.client_id = 9; r.frame_id = 99; r.timestamp = 7; r.width = 8; r.height = 8;
        r.data.assign(8 * 8 * 3 + 1, 0);
        if (engine->submitInference(r).hasError()) return 5;
    }
    for (int k = 0; k < 4000; ++k) {
        { std::lock_guard<std::mutex> lk(smu); if ((int)seen.size() >= n) break; }
        std::this_thread::sleep_for(std::chrono::milliseconds(1));
    }
    auto st = engine->getStatus();
    engine->shutdown();
    rep << "callbacks=" << seen.size() << "\nstatus_errors=" << st["inference_errors"] << "\nstreams_in_use=" << st["track_streams_in_use"]
        << "\ntracked_calls=" << g_tracked_calls << "\n";
    for (size_t i = 0; i < g_log.size(); ++i) rep << "log[" << i << "]=" << g_log[i] << "\n";
    for (size_t i = 0; i < seen.size(); ++i) rep << "seen[" << i << "]=" << seen[i].first << ":" << seen[i].second << "\n";
    return 0;
}
