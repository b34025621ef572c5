// test_plugin_track_motion_stub.cpp -- the plugin's ZLY_TRACK_MOTION (the tracker's motion model on every engine) without a GPU: with the variable the
// plugin calls zly_track_motion_enable once per engine, after zly_track_enable, with ZLY_TRACK_BETA / ZLY_TRACK_VMAX; without it, never; the variable is
// refused without ZLY_TRACK=1, and when the library lacks the call.
// TEST INFRASTRUCTURE, in the manner of test_plugin_track_stub.cpp: the plugin against the link-time stub of the C ABI of plugin_abi_stub.hpp, whose
// fake engines record the calls and "detect" one fixed box per frame.  Built a second time with -DNO_MOTION_SYMBOLS, the stub has the tracking calls
// but not the motion model's.
//
//   test_plugin_track_motion_stub <report.txt> <motion|defaults|plain|notrack>
#include "plugin_abi_stub.hpp"

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
    rep << "motion_calls=" << stub::g_motion_calls << "\n";
    // every enable and every submit, in order
    size_t i = 0;
    for (const stub::Event& ev : stub::log()) {
        if (ev.kind == stub::Event::CREATE || ev.kind == stub::Event::TRACK_RESET) continue;
        rep << "log[" << i++ << "]=";
        if (ev.kind == stub::Event::SUBMIT) rep << "submit:" << ev.engine << ":" << ev.stream;
        if (ev.kind == stub::Event::TRACK_ENABLE) rep << "enable:" << ev.engine;
        if (ev.kind == stub::Event::MOTION_ENABLE) rep << "motion:" << ev.engine << ":" << ev.motion.beta << ":" << ev.motion.v_max;
        rep << "\n";
    }
    return 0;
}
