// test_plugin_area_stub.cpp -- the plugin's resize modes (ZLY_RESIZE=stretch / letterbox / area / letterbox_area) without a GPU: each name produces
// the expected zly_config.flags, near misses are refused by initialize(), and getStatus() reports the mode.
// TEST INFRASTRUCTURE: host/hip_inference_engine.cpp is compiled into this binary together with a link-time stub of the C-ABI entry points it
// calls.  The stub is not a CPU fallback of the product.  Its zly_create records the configuration it is handed.
//
//   test_plugin_area_stub <report.txt>          (ZLY_RESIZE is set by the driver itself)
#include "../../zero-latency-yolo_amd/host/hip_inference_engine.cpp"

#include <fstream>

// ------------------------------------------------------------------------------------------------ stub of the C ABI
struct zly_engine { int unused; };
namespace {
std::mutex g_mu;
std::vector<int32_t> g_flags;                            // the flags of every zly_create, in order
thread_local std::string g_err;
}

extern "C" {
void zly_default_config(zly_config* c) { std::memset(c, 0, sizeof *c); c->model_w = 416; c->model_h = 416; c->conf_thr = 0.5f; c->iou_thr = 0.45f; c->max_batch = 1; c->max_dets = 64; c->warmup_runs = 3; c->use_graph = 1; }
const char* zly_last_error(void) { return g_err.c_str(); }
int32_t zly_create(const zly_config* c, zly_engine** out)
{
    std::lock_guard<std::mutex> lk(g_mu);
    g_flags.push_back(c->flags);
    *out = new zly_engine();
    return ZLY_OK;
}
int32_t zly_destroy(zly_engine* e) { delete e; return ZLY_OK; }
size_t zly_view_bytes(const zly_frame_view*) { return 0; }
int32_t zly_view_tight(int32_t, int32_t, int32_t, zly_frame_view*) { return ZLY_ERR_INVALID_ARGUMENT; }
int32_t zly_view_crop(const zly_frame_view*, int32_t, int32_t, int32_t, int32_t, zly_frame_view*) { return ZLY_ERR_INVALID_ARGUMENT; }
int32_t zly_submit_fmt(zly_engine*, int32_t, const uint8_t*, size_t, int32_t, int32_t, uint64_t*) { g_err = "the stub takes no frames"; return ZLY_ERR_INVALID_INPUT; }
int32_t zly_submit_try_fmt(zly_engine* e, int32_t fmt, const uint8_t* frame, size_t nbytes, int32_t w, int32_t h, uint64_t* ticket) { return zly_submit_fmt(e, fmt, frame, nbytes, w, h, ticket); }
int32_t zly_submit(zly_engine* e, const uint8_t* bgr, size_t nbytes, int32_t w, int32_t h, uint64_t* ticket) { return zly_submit_fmt(e, ZLY_PIX_BGR, bgr, nbytes, w, h, ticket); }
int32_t zly_submit_try(zly_engine* e, const uint8_t* bgr, size_t nbytes, int32_t w, int32_t h, uint64_t* ticket) { return zly_submit_fmt(e, ZLY_PIX_BGR, bgr, nbytes, w, h, ticket); }
int32_t zly_submit_view(zly_engine*, const uint8_t*, size_t, const zly_frame_view*, uint64_t*) { g_err = "the stub takes no frames"; return ZLY_ERR_INVALID_INPUT; }
int32_t zly_submit_try_view(zly_engine* e, const uint8_t* base, size_t buf_bytes, const zly_frame_view* v, uint64_t* ticket) { return zly_submit_view(e, base, buf_bytes, v, ticket); }
int32_t zly_poll(zly_engine*, uint64_t) { return ZLY_ERR_INVALID_ARGUMENT; }
int32_t zly_wait(zly_engine*, uint64_t, zly_det*, int32_t, int32_t*) { return ZLY_ERR_INVALID_ARGUMENT; }
int32_t zly_get_stats(const zly_engine*, zly_stats* out) { std::memset(out, 0, sizeof *out); return ZLY_OK; }
int32_t zly_weights_fp8(const zly_engine*) { return 0; }
}

// ------------------------------------------------------------------------------------------------ the test
using namespace zero_latency;

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    std::ofstream rep(argv[1]);
    setenv("ZLY_NUM_DEVICES", "1", 1); setenv("ZLY_ENGINES_PER_GPU", "1", 1); setenv("ZLY_MODEL_WATCH_MS", "0", 1);
    unsetenv("ZLY_CROP"); unsetenv("ZLY_INPUT_FORMAT"); unsetenv("ZLY_TRACK");
    const std::string model = std::string(argv[1]) + ".model";
    { std::ofstream m(model); m << "weights"; }
    ServerConfig config;
    config.model_path = model;
    config.inference_engine = "hip";
    // mode[name] = initialize()'s error code (0 = none), the flags every engine was created with (OR over the creates, and AND: they agree), the status
    for (const char* name : {"", "stretch", "letterbox", "area", "letterbox_area", "Area", "letterbox-area", "area_letterbox", "AREA", "area "}) {
        if (*name) setenv("ZLY_RESIZE", name, 1); else unsetenv("ZLY_RESIZE");
        { std::lock_guard<std::mutex> lk(g_mu); g_flags.clear(); }
        auto eng = InferenceEngineManager::getInstance().createEngine("hip", config);
        if (!eng) return 3;
        auto r = eng->initialize();
        int32_t any = 0, all = -1;
        size_t creates;
        { std::lock_guard<std::mutex> lk(g_mu); for (int32_t f : g_flags) { any |= f; all &= f; } creates = g_flags.size(); }
        rep << "mode[" << name << "]=" << (r.hasError() ? static_cast<int>(r.error().code) : 0) << "," << creates << "," << any << "," << (creates ? all : 0) << ","
            << (r.hasError() ? std::string("-") : eng->getStatus()["resize_mode"]) << "\n";
        if (r.hasError()) rep << "message[" << name << "]=" << r.error().message << "\n";
        eng->shutdown();
    }
    return 0;
}
