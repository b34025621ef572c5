// test_plugin_crop_stub.cpp -- the plugin's ZLY_CROP (detect every request in the centred W x H window of its frame) without a GPU: the window
// arithmetic, the even rounding for YUV input, the small-request rule, and the map of the boxes back to fractions of the request frame.
// TEST INFRASTRUCTURE: the plugin against the link-time stub of the C ABI of plugin_abi_stub.hpp, whose fake engine records the view it is handed
// and "detects" one fixed box (in window coordinates) per frame.
//
//   test_plugin_crop_stub <report.txt> <bgr|nv12>          (ZLY_CROP / ZLY_INPUT_FORMAT are set by the driver itself)
#include "plugin_abi_stub.hpp"

// ------------------------------------------------------------------------------------------------ the test
using namespace zero_latency;

static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    const bool nv12 = std::string(argv[2]) == "nv12";
    std::ofstream rep(argv[1]);
    setenv("ZLY_NUM_DEVICES", "1", 1); setenv("ZLY_ENGINES_PER_GPU", "1", 1); setenv("ZLY_MODEL_WATCH_MS", "0", 1);
    setenv("ZLY_INPUT_FORMAT", nv12 ? "nv12" : "bgr", 1);
    const std::string model = std::string(argv[1]) + ".model";
    { std::ofstream m(model); m << "weights"; }
    ServerConfig config;
    config.model_path = model;
    config.inference_engine = "hip";
    // a malformed switch is refused by initialize()
    for (const char* bad : {"416", "416x", "x416", "0x416", "416x-2", "416x416x3", "abc"}) {
        setenv("ZLY_CROP", bad, 1);
        auto eng = InferenceEngineManager::getInstance().createEngine("hip", config);
        auto r = eng->initialize();
        rep << "bad_crop[" << bad << "]=" << (r.hasError() ? static_cast<int>(r.error().code) : 0) << "\n";
        eng->shutdown();
    }
    if (nv12) {
        setenv("ZLY_CROP", "415x416", 1);
        auto eng = InferenceEngineManager::getInstance().createEngine("hip", config);
        auto r = eng->initialize();
        rep << "odd_crop_yuv=" << (r.hasError() ? static_cast<int>(r.error().code) : 0) << "\n";
        eng->shutdown();
    }
    setenv("ZLY_CROP", "416x416", 1);
    auto engine = InferenceEngineManager::getInstance().createEngine("hip", config);
    if (!engine) return 3;
    std::mutex smu;
    std::vector<std::pair<uint32_t, Detection>> seen;
    engine->setCallback([&](uint32_t, const GameState& st) {
        std::lock_guard<std::mutex> lk(smu);
        seen.emplace_back(st.frame_id, st.detections.at(0));
    });
    if (engine->initialize().hasError()) return 4;
    rep << "status_crop=" << engine->getStatus()["crop"] << "\n";
    // frame sizes: the headline capture, odd margins (the window origin is odd before the YUV rounding), exactly the window, smaller on one axis / both
    const int sizes[][2] = {{1920, 1080}, {1918, 1082}, {1250, 838}, {416, 416}, {418, 416}, {400, 1080}, {1920, 300}, {100, 62}};
    const int nsz = (int)(sizeof sizes / sizeof sizes[0]);
    int submitted = 0;
    for (int i = 0; i < nsz; ++i) {
        InferenceRequest r;
        r.client_id = 1; r.frame_id = (uint32_t)i; r.timestamp = 7; r.width = (uint32_t)sizes[i][0]; r.height = (uint32_t)sizes[i][1];
        r.data.assign((size_t)sizes[i][0] * sizes[i][1] * 3 / (nv12 ? 2 : 1), (uint8_t)i);
        if (engine->submitInference(r).hasError()) return 5;
        ++submitted;
    }
    // a frame with the wrong byte count fails alone, cropped or not (frame ids nsz, nsz + 1): counted, no callback
    for (int k = 0; k < 2; ++k) {
        InferenceRequest r;
        r.client_id = 1; r.frame_id = (uint32_t)(nsz + k); r.timestamp = 7; r.width = k ? 100 : 1920; r.height = k ? 62 : 1080;
        r.data.assign((size_t)r.width * r.height * 3 / (nv12 ? 2 : 1) + 1, 0);
        if (engine->submitInference(r).hasError()) return 5;
    }
    for (int k = 0; k < 4000; ++k) {
        { std::lock_guard<std::mutex> lk(smu); if ((int)seen.size() >= submitted) break; }
        std::this_thread::sleep_for(std::chrono::milliseconds(1));
    }
    std::this_thread::sleep_for(std::chrono::milliseconds(20));
    auto st = engine->getStatus();
    engine->shutdown();
    const std::vector<stub::Event> g_log = stub::log(stub::Event::SUBMIT);      // every accepted submit, in order
    rep << "callbacks=" << seen.size() << "\nstatus_errors=" << st["inference_errors"] << "\nlogged=" << g_log.size() << "\n";
    for (size_t i = 0; i < g_log.size() && i < seen.size(); ++i) {
        const stub::Event& s = g_log[i];
        const Detection& d = seen[i].second;
        rep << "req[" << i << "]=" << sizes[i][0] << "," << sizes[i][1] << "," << (s.view ? 1 : 0) << "," << s.w << "," << s.h << "," << s.fmt << ","
            << s.v.off[0] << "," << s.v.off[1] << "," << s.v.pitch[0] << "," << s.v.pitch[1] << "," << s.buf_bytes << ","
            << bits(d.box.x) << "," << bits(d.box.y) << "," << bits(d.box.width) << "," << bits(d.box.height) << "," << seen[i].first << "\n";
    }
    return 0;
}
