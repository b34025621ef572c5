// test_plugin_area_stub.cpp -- the plugin's resize modes (ZLY_RESIZE=stretch / letterbox / area / letterbox_area) without a GPU: each name produces
// the expected zly_config.flags, near misses are refused by initialize(), and getStatus() reports the mode.
// TEST INFRASTRUCTURE: the plugin against the link-time stub of the C ABI of plugin_abi_stub.hpp, whose zly_create records the configuration it is handed.
//
//   test_plugin_area_stub <report.txt>          (ZLY_RESIZE is set by the driver itself)
#include "plugin_abi_stub.hpp"

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
        stub::clear_log();
        auto eng = InferenceEngineManager::getInstance().createEngine("hip", config);
        if (!eng) return 3;
        auto r = eng->initialize();
        int32_t any = 0, all = -1;
        const std::vector<stub::Event> made = stub::log(stub::Event::CREATE);
        const size_t creates = made.size();
        for (const stub::Event& ev : made) { any |= ev.cfg.flags; all &= ev.cfg.flags; }
        rep << "mode[" << name << "]=" << (r.hasError() ? static_cast<int>(r.error().code) : 0) << "," << creates << "," << any << "," << (creates ? all : 0) << ","
            << (r.hasError() ? std::string("-") : eng->getStatus()["resize_mode"]) << "\n";
        if (r.hasError()) rep << "message[" << name << "]=" << r.error().message << "\n";
        eng->shutdown();
    }
    return 0;
}
