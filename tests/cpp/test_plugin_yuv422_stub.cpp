// test_plugin_yuv422_stub.cpp -- the plugin's packed YUV 4:2:2 input (ZLY_INPUT_FORMAT=yuy2 / uyvy / yuy2_709 / uyvy_709) without a GPU: the four
// names parse and are reported by getStatus(), a request of the wrong size fails alone, and ZLY_CROP follows the format's x-only evenness rule (W even,
// any H; x0 rounded down to even, y0 as it is).
// TEST INFRASTRUCTURE: the plugin against the link-time stub of the C ABI of plugin_abi_stub.hpp, whose fake engine records the view it is handed
// and "detects" one fixed box per frame.
//
//   test_plugin_yuv422_stub <report.txt>          (ZLY_CROP / ZLY_INPUT_FORMAT are set by the driver itself)
#include "plugin_abi_stub.hpp"

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
    const std::vector<stub::Event> g_log = stub::log(stub::Event::SUBMIT);      // every accepted submit, in order
    rep << "callbacks=" << seen.size() << "\nstatus_errors=" << st["inference_errors"] << "\nlogged=" << g_log.size() << "\n";
    for (size_t i = 0; i < g_log.size() && i < seen.size(); ++i) {
        const stub::Event& s = g_log[i];
        rep << "req[" << i << "]=" << (s.view ? 1 : 0) << "," << s.w << "," << s.h << "," << s.fmt << "," << s.v.off[0] << "," << s.v.pitch[0] << "," << s.buf_bytes << "," << seen[i] << "\n";
    }
    return 0;
}
