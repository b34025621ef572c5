// test_hip_engine_pix.cpp -- the plugin (host/hip_inference_engine.cpp) fed packed RGB / BGRA / RGBA requests, as an embedder that hands a capture
// surface to IInferenceEngine::submitInference directly does: ZLY_INPUT_FORMAT (any name the plugin knows: bgr, nv12, i420, nv12_709, i420_709, rgb,
// bgra, rgba) and ZLY_CROP are read by initialize().
//
//   test_hip_engine_pix <weights.zlyw> <frames.bin> <out.json>
//
// frames.bin as tests/cpp/test_hip_engine.cpp reads it: u32 count, then per frame {u16 width, u16 height, u32 nbytes, bytes[nbytes]}.  A frame whose
// nbytes is not zly_frame_bytes(format, w, h) must fail alone: no callback, one inference error.  Writes the detections every callback delivered
// (exact float bits) and getStatus(); ZLY_TEST_CONF_THR sets ServerConfig::confidence_threshold. tests/test_gpu_packed_formats.py compares them with zly_detect_fmt / zly_detect_view on the same frames.
#include "zly_compat.hpp"
#include "hip_inference_engine.h"
#include "zly.h"

#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <mutex>
#include <sstream>
#include <thread>

using namespace zero_latency;

struct Frame { uint16_t w, h; std::vector<uint8_t> data; };

static bool readFrames(const char* path, std::vector<Frame>* out)
{
    std::ifstream f(path, std::ios::binary);
    if (!f) return false;
    uint32_t n = 0;
    f.read(reinterpret_cast<char*>(&n), 4);
    for (uint32_t i = 0; i < n; ++i) {
        Frame fr;
        uint32_t nb = 0;
        f.read(reinterpret_cast<char*>(&fr.w), 2);
        f.read(reinterpret_cast<char*>(&fr.h), 2);
        f.read(reinterpret_cast<char*>(&nb), 4);
        fr.data.resize(nb);
        f.read(reinterpret_cast<char*>(fr.data.data()), nb);
        if (!f) return false;
        out->push_back(std::move(fr));
    }
    return true;
}

int main(int argc, char** argv)
{
    if (argc < 4) { std::fprintf(stderr, "usage: %s weights frames.bin out.json\n", argv[0]); return 2; }
    std::vector<Frame> frames;
    if (!readFrames(argv[2], &frames)) { std::fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
    ServerConfig config;
    config.model_path = argv[1];
    config.inference_engine = "hip";
    if (const char* thr = std::getenv("ZLY_TEST_CONF_THR")) config.confidence_threshold = (float)std::atof(thr);   // small windows of synthetic frames: a low threshold, so that boxes exist to compare
    std::unique_ptr<IInferenceEngine> engine = InferenceEngineManager::getInstance().createEngine("hip", config);
    if (!engine) { std::fprintf(stderr, "factory 'hip' not registered\n"); return 3; }

    std::mutex mu;
    std::condition_variable cv;
    struct Got { uint32_t frame_id; std::vector<Detection> dets; };
    std::vector<Got> got;
    engine->setCallback([&](uint32_t, const GameState& st) {
        std::lock_guard<std::mutex> lk(mu);
        got.push_back(Got{st.frame_id, st.detections});
        cv.notify_all();
    });
    auto init = engine->initialize();
    if (init.hasError()) { std::fprintf(stderr, "initialize failed: %s\n", init.error().toString().c_str()); return 4; }
    const char* fmt_name = std::getenv("ZLY_INPUT_FORMAT");
    static const struct { const char* name; int32_t fmt; } kFormats[] = {
        {"bgr", ZLY_PIX_BGR}, {"nv12", ZLY_PIX_NV12_BT601}, {"i420", ZLY_PIX_I420_BT601}, {"nv12_709", ZLY_PIX_NV12_BT709}, {"i420_709", ZLY_PIX_I420_BT709},
        {"rgb", ZLY_PIX_RGB}, {"bgra", ZLY_PIX_BGRA}, {"rgba", ZLY_PIX_RGBA}};
    int32_t fmt = ZLY_PIX_BGR;
    for (const auto& f : kFormats)
        if (fmt_name && !std::strcmp(fmt_name, f.name)) fmt = f.fmt;
    size_t expected = 0;
    for (size_t i = 0; i < frames.size(); ++i) {
        InferenceRequest r;
        r.client_id = 1;
        r.frame_id = (uint32_t)i;
        r.timestamp = 1000 + i;
        r.width = frames[i].w; r.height = frames[i].h;
        r.data = frames[i].data;
        if (r.data.size() == zly_frame_bytes(fmt, r.width, r.height)) ++expected;
        auto res = engine->submitInference(r);
        if (res.hasError()) { std::fprintf(stderr, "submit failed: %s\n", res.error().toString().c_str()); return 5; }
    }
    {
        std::unique_lock<std::mutex> lk(mu);
        if (!cv.wait_for(lk, std::chrono::seconds(60), [&] { return got.size() >= expected; })) {
            std::fprintf(stderr, "timeout: %zu of %zu callbacks\n", got.size(), expected);
            return 6;
        }
    }
    std::this_thread::sleep_for(std::chrono::milliseconds(50));          // a wrongly delivered extra callback would show up here
    std::ostringstream js;
    js << "{\"status\":{";
    bool first = true;
    for (const auto& kv : engine->getStatus()) { js << (first ? "" : ",") << "\"" << kv.first << "\":\"" << kv.second << "\""; first = false; }
    js << "},\"results\":[";
    {
        std::lock_guard<std::mutex> lk(mu);
        for (size_t i = 0; i < got.size(); ++i) {
            js << (i ? "," : "") << "{\"frame_id\":" << got[i].frame_id << ",\"dets\":[";
            for (size_t k = 0; k < got[i].dets.size(); ++k) {
                const Detection& d = got[i].dets[k];
                uint32_t bits[5];
                std::memcpy(bits, &d, 20);
                js << (k ? "," : "") << "[" << bits[0] << "," << bits[1] << "," << bits[2] << "," << bits[3] << "," << bits[4] << "," << d.class_id << "]";
            }
            js << "]}";
        }
    }
    js << "]}";
    engine->shutdown();
    std::ofstream(argv[3]) << js.str() << "\n";
    return 0;
}
