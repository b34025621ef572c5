// plugin_abi_stub.hpp -- the link-time stub of the C ABI (include/zly.h) behind the plugin's CPU tests test_plugin_{crop,yuv422,track,track_motion,area}_stub.cpp.
// TEST INFRASTRUCTURE: host/hip_inference_engine.cpp is compiled into the including binary together with these definitions of the entry points it
// calls.  The stub is not a CPU fallback of the product.  Its fake engines have a ring that is never full, record every call in one event log
// (stub::log()) and "detect" one fixed box per frame; what a frame or a view must look like to be accepted is the product's own rule
// (csrc/frame_rules.h), for every format.
//   -DNO_TRACK_SYMBOLS    the ABI lacks the tracking calls (and with them the motion model's): the plugin's weak references stay null
//   -DNO_MOTION_SYMBOLS   the ABI has the tracking calls but not the motion model's
// (test_plugin_stub.cpp keeps a stub of its own: per-engine delays, out-of-order completion, and an ABI without the _fmt and view calls.)
#pragma once
#include "../../zero-latency-yolo_amd/host/hip_inference_engine.cpp"
#include "frame_rules.h"

#include <fstream>
#include <sstream>
#include <thread>

namespace stub {
struct Event {
    enum Kind { CREATE, SUBMIT, TRACK_ENABLE, TRACK_RESET, MOTION_ENABLE } kind;
    int engine;                          // the engine's index, in the order of zly_create
    zly_config cfg;                      // the zly_config that engine was created with
    // SUBMIT: the view (of a frame submit: the frame's tight view), the caller's buffer size, and the stream (-1: untracked)
    bool view, tracked;
    zly_frame_view v;
    size_t buf_bytes;
    int32_t w, h, fmt, stream;           // stream: also TRACK_RESET's
    zly_track_config track;              // TRACK_ENABLE
    uint32_t first_id;                   // TRACK_RESET
    zly_track_motion_config motion;      // MOTION_ENABLE
};
const float BOX[4] = {0.25f, 0.625f, 0.1f, 0.3f};        // what a fake engine detects: centre x, centre y, w, h as fractions of what it was handed

inline std::mutex g_mu;
inline std::vector<Event> g_log;                         // every accepted call, in order
inline int g_engines = 0, g_track_calls = 0, g_motion_calls = 0;      // engines created; calls of the tracking ABI / the motion model's, refused ones and the default-config getters included
inline thread_local std::string g_err;

inline std::vector<Event> log(int kind = -1)             // a copy of the log, or of its events of one kind
{
    std::lock_guard<std::mutex> lg(g_mu);
    std::vector<Event> out;
    for (const Event& ev : g_log) if (kind < 0 || ev.kind == kind) out.push_back(ev);
    return out;
}
inline void clear_log() { std::lock_guard<std::mutex> lg(g_mu); g_log.clear(); }
inline void count(int* calls) { std::lock_guard<std::mutex> lg(g_mu); ++*calls; }
}  // namespace stub

struct zly_engine {
    int index = 0;
    zly_config cfg{};
    std::mutex mu;
    std::map<uint64_t, int> pending;                     // ticket -> stream
    uint64_t next_ticket = 1;
    std::atomic<uint64_t> frames{0};
};

namespace stub {
inline Event event(const zly_engine* e, Event::Kind kind) { Event ev{}; ev.kind = kind; ev.engine = e->index; ev.cfg = e->cfg; ev.stream = -1; return ev; }
inline void note(const Event& ev) { std::lock_guard<std::mutex> lg(g_mu); g_log.push_back(ev); }
inline int32_t accept(zly_engine* e, bool view, const zly_frame_view& v, size_t buf_bytes, int32_t stream, bool tracked, uint64_t* ticket)
{
    {
        std::lock_guard<std::mutex> lk(e->mu);
        *ticket = e->next_ticket++;
        e->pending[*ticket] = stream;
    }
    Event ev = event(e, Event::SUBMIT);
    ev.view = view; ev.tracked = tracked; ev.v = v; ev.buf_bytes = buf_bytes; ev.w = v.w; ev.h = v.h; ev.fmt = v.fmt; ev.stream = stream;
    note(ev);
    return ZLY_OK;
}
}  // namespace stub

extern "C" {
void zly_default_config(zly_config* c) { std::memset(c, 0, sizeof *c); c->model_w = 416; c->model_h = 416; c->conf_thr = 0.5f; c->iou_thr = 0.45f; c->max_batch = 1; c->max_dets = 64; c->warmup_runs = 3; c->use_graph = 1; }
const char* zly_last_error(void) { return stub::g_err.c_str(); }
int32_t zly_create(const zly_config* c, zly_engine** out)
{
    zly_engine* e = new zly_engine();
    e->cfg = *c;
    { std::lock_guard<std::mutex> lg(stub::g_mu); e->index = stub::g_engines++; }
    stub::note(stub::event(e, stub::Event::CREATE));
    *out = e;
    return ZLY_OK;
}
int32_t zly_destroy(zly_engine* e) { delete e; return ZLY_OK; }
size_t zly_view_bytes(const zly_frame_view* v) { return zly::view_bytes(v); }
int32_t zly_view_tight(int32_t fmt, int32_t w, int32_t h, zly_frame_view* out) { return zly::view_tight(fmt, w, h, out, &stub::g_err); }
int32_t zly_view_crop(const zly_frame_view* s, int32_t x0, int32_t y0, int32_t w, int32_t h, zly_frame_view* out) { return zly::view_crop(s, x0, y0, w, h, out, &stub::g_err); }
int32_t zly_submit_fmt(zly_engine* e, int32_t fmt, const uint8_t* frame, size_t nbytes, int32_t w, int32_t h, uint64_t* ticket)
{
    if (int rc = zly::check_frame(fmt, frame, nbytes, w, h, &stub::g_err)) return rc;
    zly_frame_view t;
    zly::view_tight(fmt, w, h, &t, nullptr);
    return stub::accept(e, false, t, nbytes, -1, false, ticket);
}
int32_t zly_submit_try_fmt(zly_engine* e, int32_t fmt, const uint8_t* frame, size_t nbytes, int32_t w, int32_t h, uint64_t* ticket) { return zly_submit_fmt(e, fmt, frame, nbytes, w, h, ticket); }
int32_t zly_submit(zly_engine* e, const uint8_t* bgr, size_t nbytes, int32_t w, int32_t h, uint64_t* ticket) { return zly_submit_fmt(e, ZLY_PIX_BGR, bgr, nbytes, w, h, ticket); }
int32_t zly_submit_try(zly_engine* e, const uint8_t* bgr, size_t nbytes, int32_t w, int32_t h, uint64_t* ticket) { return zly_submit_fmt(e, ZLY_PIX_BGR, bgr, nbytes, w, h, ticket); }
int32_t zly_submit_view(zly_engine* e, const uint8_t* base, size_t buf_bytes, const zly_frame_view* v, uint64_t* ticket)
{
    if (int rc = zly::check_view(e->cfg.flags, base, buf_bytes, v, &stub::g_err)) return rc;
    return stub::accept(e, true, *v, buf_bytes, -1, false, ticket);
}
int32_t zly_submit_try_view(zly_engine* e, const uint8_t* base, size_t buf_bytes, const zly_frame_view* v, uint64_t* ticket) { return zly_submit_view(e, base, buf_bytes, v, ticket); }
#ifndef NO_TRACK_SYMBOLS
void zly_default_track_config(zly_track_config* c) { c->max_streams = 64; c->max_tracks = 64; c->match_iou = 0.3f; c->max_lost = 6; stub::count(&stub::g_track_calls); }
int32_t zly_track_enable(zly_engine* e, const zly_track_config* c)
{
    stub::count(&stub::g_track_calls);
    if (c->max_tracks < e->cfg.max_dets || c->max_tracks > 64) { stub::g_err = "max_tracks"; return ZLY_ERR_INVALID_ARGUMENT; }
    stub::Event ev = stub::event(e, stub::Event::TRACK_ENABLE);
    ev.track = *c;
    stub::note(ev);
    return ZLY_OK;
}
int32_t zly_track_reset(zly_engine* e, int32_t stream, uint32_t first_id)
{
    stub::count(&stub::g_track_calls);
    stub::Event ev = stub::event(e, stub::Event::TRACK_RESET);
    ev.stream = stream; ev.first_id = first_id;
    stub::note(ev);
    return ZLY_OK;
}
int32_t zly_submit_view_tracked(zly_engine* e, const uint8_t* base, size_t buf_bytes, const zly_frame_view* v, int32_t stream, uint64_t* ticket)
{
    stub::count(&stub::g_track_calls);
    if (int rc = zly::check_view(e->cfg.flags, base, buf_bytes, v, &stub::g_err)) return rc;
    return stub::accept(e, true, *v, buf_bytes, stream, true, ticket);
}
int32_t zly_submit_try_view_tracked(zly_engine* e, const uint8_t* base, size_t buf_bytes, const zly_frame_view* v, int32_t stream, uint64_t* ticket)
{
    return zly_submit_view_tracked(e, base, buf_bytes, v, stream, ticket);
}
#ifndef NO_MOTION_SYMBOLS
void zly_default_track_motion_config(zly_track_motion_config* c) { c->beta = 0.5f; c->v_max = 0.25f; stub::count(&stub::g_motion_calls); }
int32_t zly_track_motion_enable(zly_engine* e, const zly_track_motion_config* c)
{
    stub::count(&stub::g_motion_calls);
    stub::Event ev = stub::event(e, stub::Event::MOTION_ENABLE);
    ev.motion = *c;
    stub::note(ev);
    return ZLY_OK;
}
#endif
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
        out[0].x = stub::BOX[0]; out[0].y = stub::BOX[1]; out[0].w = stub::BOX[2]; out[0].h = stub::BOX[3]; out[0].confidence = 0.75f; out[0].class_id = 2;
        out[0].track_id = stream < 0 ? 0u : (uint32_t)(100 * (e->index + 1) + stream);       // what a tracking engine would fill: non-zero, per stream
    }
    *n_out = 1;
    e->frames++;
    return ZLY_OK;
}
int32_t zly_get_stats(const zly_engine* e, zly_stats* out) { std::memset(out, 0, sizeof *out); out->batches = e->frames.load(); return ZLY_OK; }
int32_t zly_weights_fp8(const zly_engine*) { return 0; }
}
