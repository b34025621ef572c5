// test_plugin_yuv422_stub.cpp -- the plugin's packed YUV 4:2:2 input (ZLY_INPUT_FORMAT=yuy2 / uyvy / yuy2_709 / uyvy_709) without a GPU: the four
// names parse and are reported by getStatus(), a request of the wrong size fails alone, and ZLY_CROP follows the format's x-only evenness rule (W even,
// any H; x0 rounded down to even, y0 as it is).
// TEST INFRASTRUCTURE: host/hip_inference_engine.cpp is compiled into this binary together with a link-time stub of the C-ABI entry points it
// calls, among them the frame-view calls.  The stub is not a CPU fallback of the product.  Its fake engine records the view it is handed and
// "detects" one fixed box per frame.
//
//   test_plugin_yuv422_stub <report.txt>          (ZLY_CROP / ZLY_INPUT_FORMAT are set by the driver itself)
#include "../../zero-latency-yolo_amd/host/hip_inference_engine.cpp"

#include <fstream>
#include <thread>

// ------------------------------------------------------------------------------------------------ stub of the C ABI
struct Submitted { bool view; zly_frame_view v; size_t buf_bytes; int32_t w, h, fmt; };
struct zly_engine {
    std::mutex mu;
    std::map<uint64_t, Submitted> pending;
    uint64_t next_ticket = 1;
    std::atomic<uint64_t> frames{0};
};
namespace {
std::mutex g_mu;
std::vector<Submitted> g_log;                            // every accepted submit, in order
thread_local std::string g_err;
const float BOX[4] = {0.25f, 0.625f, 0.1f, 0.3f};        // what the fake engine detects: centre x, centre y, w, h as fractions of what it was handed

int planes_of(int32_t fmt, int32_t w, int32_t h, int64_t rows[3], int64_t rb[3])
{
    const bool y422 = fmt >= ZLY_PIX_YUY2_BT601 && fmt <= ZLY_PIX_UYVY_BT709;
    if ((fmt != ZLY_PIX_BGR && !y422) || w < 1 || h < 1) return 0;
    if (y422 && (w < 2 || (w & 1))) return 0;
    rows[0] = h; rb[0] = (y422 ? 2 : 3) * (int64_t)w;
    return 1;
}
int32_t accept(zly_engine* e, const Submitted& s, uint64_t* ticket)
{
    std::lock_guard<std::mutex> lk(e->mu);
    *ticket = e->next_ticket++;
    e->pending[*ticket] = s;
    std::lock_guard<std::mutex> lg(g_mu);
    g_log.push_back(s);
    return ZLY_OK;
}
}

extern "C" {
void zly_default_config(zly_config* c) { std::memset(c, 0, sizeof *c); c->model_w = 416; c->model_h = 416; c->conf_thr = 0.5f; c->iou_thr = 0.45f; c->max_batch = 1; c->max_dets = 64; c->warmup_runs = 3; c->use_graph = 1; }
const char* zly_last_error(void) { return g_err.c_str(); }
int32_t zly_create(const zly_config*, zly_engine** out) { *out = new zly_engine(); return ZLY_OK; }
int32_t zly_destroy(zly_engine* e) { delete e; return ZLY_OK; }
size_t zly_view_bytes(const zly_frame_view* v)
{
    int64_t rows[3], rb[3];
    const int np = planes_of(v->fmt, v->w, v->h, rows, rb);
    size_t most = 0;
    for (int p = 0; p < np; ++p) {
        if (v->pitch[p] < rb[p]) return 0;
        most = std::max<size_t>(most, (size_t)v->off[p] + (size_t)((rows[p] - 1) * v->pitch[p] + rb[p]));
    }
    return most;
}
int32_t zly_view_tight(int32_t fmt, int32_t w, int32_t h, zly_frame_view* out)
{
    int64_t rows[3], rb[3];
    const int np = planes_of(fmt, w, h, rows, rb);
    if (!np) return ZLY_ERR_INVALID_ARGUMENT;
    std::memset(out, 0, sizeof *out);
    out->fmt = fmt; out->w = w; out->h = h;
    uint64_t off = 0;
    for (int p = 0; p < np; ++p) { out->off[p] = off; out->pitch[p] = (int32_t)rb[p]; off += (uint64_t)(rows[p] * rb[p]); }
    return ZLY_OK;
}
int32_t zly_view_crop(const zly_frame_view* s, int32_t x0, int32_t y0, int32_t w, int32_t h, zly_frame_view* out)
{
    if (x0 < 0 || y0 < 0 || w < 1 || h < 1 || x0 + w > s->w || y0 + h > s->h) return ZLY_ERR_INVALID_ARGUMENT;
    zly_frame_view v = *s;
    v.w = w; v.h = h;
    if (v.fmt == ZLY_PIX_BGR) v.off[0] += (uint64_t)y0 * v.pitch[0] + (uint64_t)x0 * 3;
    else {
        if ((x0 | w) & 1) return ZLY_ERR_INVALID_ARGUMENT;
        v.off[0] += (uint64_t)y0 * v.pitch[0] + (uint64_t)x0 * 2;
    }
    *out = v;
    return ZLY_OK;
}
int32_t zly_submit_fmt(zly_engine* e, int32_t fmt, const uint8_t* frame, size_t nbytes, int32_t w, int32_t h, uint64_t* ticket)
{
    zly_frame_view t;
    if (!frame || zly_view_tight(fmt, w, h, &t) != ZLY_OK || nbytes != zly_view_bytes(&t)) { g_err = "Invalid image data size"; return ZLY_ERR_INVALID_INPUT; }
    return accept(e, Submitted{false, t, nbytes, w, h, fmt}, ticket);
}
int32_t zly_submit_try_fmt(zly_engine* e, int32_t fmt, const uint8_t* frame, size_t nbytes, int32_t w, int32_t h, uint64_t* ticket) { return zly_submit_fmt(e, fmt, frame, nbytes, w, h, ticket); }
int32_t zly_submit(zly_engine* e, const uint8_t* bgr, size_t nbytes, int32_t w, int32_t h, uint64_t* ticket) { return zly_submit_fmt(e, ZLY_PIX_BGR, bgr, nbytes, w, h, ticket); }
int32_t zly_submit_try(zly_engine* e, const uint8_t* bgr, size_t nbytes, int32_t w, int32_t h, uint64_t* ticket) { return zly_submit_fmt(e, ZLY_PIX_BGR, bgr, nbytes, w, h, ticket); }
int32_t zly_submit_view(zly_engine* e, const uint8_t* base, size_t buf_bytes, const zly_frame_view* v, uint64_t* ticket)
{
    const size_t need = zly_view_bytes(v);
    if (!base || !need || need > buf_bytes) { g_err = "Invalid image data size"; return ZLY_ERR_INVALID_INPUT; }
    return accept(e, Submitted{true, *v, buf_bytes, v->w, v->h, v->fmt}, ticket);
}
int32_t zly_submit_try_view(zly_engine* e, const uint8_t* base, size_t buf_bytes, const zly_frame_view* v, uint64_t* ticket) { return zly_submit_view(e, base, buf_bytes, v, ticket); }
int32_t zly_poll(zly_engine* e, uint64_t ticket)
{
    std::lock_guard<std::mutex> lk(e->mu);
    return e->pending.count(ticket) ? ZLY_OK : ZLY_ERR_INVALID_ARGUMENT;
}
int32_t zly_wait(zly_engine* e, uint64_t ticket, zly_det* out, int32_t cap, int32_t* n_out)
{
    {
        std::lock_guard<std::mutex> lk(e->mu);
        if (!e->pending.erase(ticket)) return ZLY_ERR_INVALID_ARGUMENT;
    }
    if (cap >= 1) {
        std::memset(out, 0, sizeof *out);
        out[0].x = BOX[0]; out[0].y = BOX[1]; out[0].w = BOX[2]; out[0].h = BOX[3]; out[0].confidence = 0.75f; out[0].class_id = 2;
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
    if (argc < 2) return 2;
    std::ofstream rep(argv[1]);
    setenv("ZLY_NUM_DEVICES", "1", 1); setenv("ZLY_ENGINES_PER_GPU", "1", 1); setenv("ZLY_MODEL_WATCH_MS", "0", 1);
    const std::string model = std::string(argv[1]) + ".model";
    { std::ofstream m(model); m << "weights"; }
    ServerConfig config;
    config.model_path = model;
    config.inference_engine = "hip";
    // the four names parse and come back from getStatus(); near misses are refused by initialize()
    unsetenv("ZLY_CROP");
    for (const char* name : {"yuy2", "uyvy", "yuy2_709", "uyvy_709", "yuyv", "uyvy_601", "YUY2"}) {
        setenv("ZLY_INPUT_FORMAT", name, 1);
        auto eng = InferenceEngineManager::getInstance().createEngine("hip", config);
        auto r = eng->initialize();
        rep << "format[" << name << "]=" << (r.hasError() ? static_cast<int>(r.error().code) : 0) << "," << (r.hasError() ? std::string("-") : eng->getStatus()["input_format"]) << "\n";
        eng->shutdown();
    }
    // ZLY_CROP: W must be even, H may be anything
    setenv("ZLY_INPUT_FORMAT", "yuy2", 1);
    for (const char* crop : {"415x416", "416x415", "415x415", "2x1"}) {
        setenv("ZLY_CROP", crop, 1);
        auto eng = InferenceEngineManager::getInstance().createEngine("hip", config);
        auto r = eng->initialize();
        rep << "crop[" << crop << "]=" << (r.hasError() ? static_cast<int>(r.error().code) : 0) << "\n";
        eng->shutdown();
    }
    // requests through a 416 x 415 window of UYVY (BT.709) frames
    setenv("ZLY_INPUT_FORMAT", "uyvy_709", 1);
    setenv("ZLY_CROP", "416x415", 1);
    auto engine = InferenceEngineManager::getInstance().createEngine("hip", config);
    if (!engine) return 3;
    std::mutex smu;
    std::vector<uint32_t> seen;
    engine->setCallback([&](uint32_t, const GameState& st) {
        std::lock_guard<std::mutex> lk(smu);
        seen.push_back(st.frame_id);
    });
    if (engine->initialize().hasError()) return 4;
    rep << "status_crop=" << engine->getStatus()["crop"] << "\nstatus_format=" << engine->getStatus()["input_format"] << "\n";
    // frame sizes: odd y margin with even / odd x margin, an odd height, exactly the window, smaller on one axis (detected whole, odd height)
    const int sizes[][2] = {{1920, 1081}, {1918, 1081}, {1250, 838}, {416, 415}, {400, 1081}, {1920, 301}};
    const int nsz = (int)(sizeof sizes / sizeof sizes[0]);
    int submitted = 0;
    for (int i = 0; i < nsz; ++i) {
        InferenceRequest r;
        r.client_id = 1; r.frame_id = (uint32_t)i; r.timestamp = 7; r.width = (uint32_t)sizes[i][0]; r.height = (uint32_t)sizes[i][1];
        r.data.assign((size_t)sizes[i][0] * sizes[i][1] * 2, (uint8_t)i);
        if (engine->submitInference(r).hasError()) return 5;
        ++submitted;
    }
    // requests of the wrong size fail alone, cropped or not (frame ids nsz ..): a byte too many (window-sized and small), a BGR-sized frame, an odd width
    const int bad[][3] = {{1920, 1081, 1920 * 1081 * 2 + 1}, {100, 62, 100 * 62 * 2 + 1}, {640, 480, 640 * 480 * 3}, {641, 480, 641 * 480 * 2}, {101, 62, 101 * 62 * 2}};
    const int nbad = (int)(sizeof bad / sizeof bad[0]);
    for (int k = 0; k < nbad; ++k) {
        InferenceRequest r;
        r.client_id = 1; r.frame_id = (uint32_t)(nsz + k); r.timestamp = 7; r.width = (uint32_t)bad[k][0]; r.height = (uint32_t)bad[k][1];
        r.data.assign((size_t)bad[k][2], 0);
        if (engine->submitInference(r).hasError()) return 5;
    }
    // ... and a good one behind them is still served
    {
        InferenceRequest r;
        r.client_id = 1; r.frame_id = (uint32_t)(nsz + nbad); r.timestamp = 7; r.width = 100; r.height = 63;
        r.data.assign((size_t)100 * 63 * 2, 1);
        if (engine->submitInference(r).hasError()) return 5;
        ++submitted;
    }
    for (int k = 0; k < 4000; ++k) {
        { std::lock_guard<std::mutex> lk(smu); if ((int)seen.size() >= submitted) break; }
        std::this_thread::sleep_for(std::chrono::milliseconds(1));
    }
    std::this_thread::sleep_for(std::chrono::milliseconds(20));
    auto st = engine->getStatus();
    engine->shutdown();
    rep << "callbacks=" << seen.size() << "\nstatus_errors=" << st["inference_errors"] << "\nlogged=" << g_log.size() << "\n";
    for (size_t i = 0; i < g_log.size() && i < seen.size(); ++i) {
        const Submitted& s = g_log[i];
        rep << "req[" << i << "]=" << (s.view ? 1 : 0) << "," << s.w << "," << s.h << "," << s.fmt << "," << s.v.off[0] << "," << s.v.pitch[0] << "," << s.buf_bytes << "," << seen[i] << "\n";
    }
    return 0;
}
