// test_plugin_track_stub.cpp -- the plugin's ZLY_TRACK (track ids on the GPU: a client is one stream of one engine) without a GPU: engine affinity by
// client id, stable stream slots, least-recently-used reuse with a reset before the new client's first frame, and the switch being off by default.
// TEST INFRASTRUCTURE: the plugin against the link-time stub of the C ABI of plugin_abi_stub.hpp, whose fake engines record (engine, stream) of every
// submit and every reset, and "detect" one fixed box per frame.  Built a second time with -DNO_TRACK_SYMBOLS, the stub lacks the tracking calls:
// initialize() must then refuse ZLY_TRACK.
//
//   test_plugin_track_stub <report.txt> <on|off>
#include "plugin_abi_stub.hpp"

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
        << "\ntracked_calls=" << stub::g_track_calls << "\n";
    // every submit, reset and enable, in order
    size_t i = 0;
    for (const stub::Event& ev : stub::log()) {
        if (ev.kind == stub::Event::CREATE) continue;
        rep << "log[" << i++ << "]=";
        if (ev.kind == stub::Event::SUBMIT) rep << "submit:" << ev.engine << ":" << ev.stream << ":" << (ev.tracked ? 1 : 0);
        if (ev.kind == stub::Event::TRACK_ENABLE) rep << "enable:" << ev.engine << ":" << ev.track.max_streams << ":" << ev.track.max_tracks << ":" << ev.track.max_lost << ":" << ev.cfg.max_dets;
        if (ev.kind == stub::Event::TRACK_RESET) rep << "reset:" << ev.engine << ":" << ev.stream << ":" << ev.first_id;
        rep << "\n";
    }
    for (size_t i = 0; i < seen.size(); ++i) rep << "seen[" << i << "]=" << seen[i].first << ":" << seen[i].second << "\n";
    return 0;
}
