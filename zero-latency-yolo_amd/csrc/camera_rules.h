// camera_rules.h -- the host side of the camera motion estimate (include/zly.h "Camera motion"): the config and call checks, and the HOST TWIN of the
// kernels (kernels_camera.hip) -- the same functions of camera_device.h, walked candidate by candidate and cell by cell in loops.  Nothing here
// touches a device or the engine, as change_rules.h does not: engine.cpp and a stand-alone test program (tests/cpp/test_camera_rules.cpp) compile
// the same text.
#pragma once
#include <cstddef>
#include <cstring>
#include <vector>
#include "change_rules.h"
#include "camera_device.h"

namespace zly {

static_assert(sizeof(zly_camera_header) == ZLY_CAMERA_HDR_BYTES && ZLY_CAMERA_HDR == ZLY_CAMERA_HDR_BYTES, "camera_device.h's offsets are include/zly.h's record");
static_assert(offsetof(zly_camera_header, n_applied) == 44 && offsetof(zly_camera_header, sad_min) == 48 && offsetof(zly_camera_header, pend_x_q4) == 64 &&
              offsetof(zly_camera_header, pad) == 80, "the header has no hidden padding");
static_assert(ZLY_CAMERA_R_MAX == ZLY_CAMERA_MAX_RADIUS && ZLY_CAMERA_SIDE_MAX * ZLY_CAMERA_SIDE_MAX == ZLY_CAMERA_SAD_ROOM, "the table's room");
static_assert(ZLY_CAMERA_F_FIRST == ZLY_CAMERA_FIRST && ZLY_CAMERA_F_LOST == ZLY_CAMERA_LOST && ZLY_CAMERA_F_CLIPPED == ZLY_CAMERA_CLIPPED, "the flags");
static_assert(sizeof(CameraItem) == 16 && sizeof(CameraStream) == 32, "uploaded and kept as arrays");

inline void camera_default_config(zly_camera_config* c)
{
    c->cell = 16;
    c->radius = 4;
    c->max_residual_q4 = 64;                     // four luma levels per pixel: chosen, not tuned
}

inline int camera_check_config(const zly_camera_config* c, int32_t max_streams, std::string* err)
{
    if (!c) return refuse(err, ZLY_ERR_INVALID_ARGUMENT, "null camera config");
    if (!change_cell_ok(c->cell)) return refuse(err, ZLY_ERR_INVALID_ARGUMENT, "cell must be 8, 16, 32 or 64");
    if (!camera_radius_ok(c->radius)) return refuse(err, ZLY_ERR_INVALID_ARGUMENT, "radius must lie in 1..8");
    if (c->max_residual_q4 < 0 || c->max_residual_q4 > 4080) return refuse(err, ZLY_ERR_INVALID_ARGUMENT, "max_residual_q4 must lie in 0..4080");
    if (max_streams < 1) return refuse(err, ZLY_ERR_INVALID_ARGUMENT, "max_streams must be >= 1");
    return ZLY_OK;
}

// the arguments of a frame call that need no engine state
inline int camera_check_call(int32_t n, int32_t max_batch, const void* frames, const int32_t* streams, std::string* err)
{
    if (n < 1 || n > max_batch) return refuse(err, ZLY_ERR_INVALID_ARGUMENT, "camera call: batch size out of range");
    if (!frames) return refuse(err, ZLY_ERR_INVALID_ARGUMENT, "camera call: null views");
    if (!streams) return refuse(err, ZLY_ERR_INVALID_ARGUMENT, "camera call: null streams");
    return ZLY_OK;
}

// streams[0 .. n): inside both tables, each once.  max_b: the other table's size (an apply: the track tables'), or max_a again
inline int camera_check_streams(int32_t n, const int32_t* streams, int32_t max_a, int32_t max_b, std::string* err)
{
    for (int i = 0; i < n; ++i) {
        if (streams[i] < 0 || streams[i] >= max_a || streams[i] >= max_b)
            return refuse(err, ZLY_ERR_INVALID_ARGUMENT, "stream " + std::to_string(streams[i]) + " out of range (the camera has " + std::to_string(max_a) +
                                                         (max_b != max_a ? ", the tracker " + std::to_string(max_b) : std::string()) + ")");
        for (int k = 0; k < i; ++k)
            if (streams[k] == streams[i]) return refuse(err, ZLY_ERR_INVALID_ARGUMENT, "stream " + std::to_string(streams[i]) + " occurs twice in a camera call");
    }
    return ZLY_OK;
}

// the size of a (valid) view's grid: the change map's limits, and room for the window at every candidate
inline int camera_check_size(int32_t W, int32_t H, int32_t C, int32_t R, std::string* err)
{
    if (int rc = change_check_size(W, H, C, err)) return rc;
    const int32_t gw = change_cells_axis(W, C), gh = change_cells_axis(H, C);
    if (!camera_grid_ok(gw, gh, R))
        return refuse(err, ZLY_ERR_INVALID_INPUT, std::to_string(W) + " x " + std::to_string(H) + " at cell " + std::to_string(C) + " is " + std::to_string(gw) + " x " +
                                                  std::to_string(gh) + " cells, below the " + std::to_string(2 * R + 1) + " a radius of " + std::to_string(R) + " needs");
    return ZLY_OK;
}

// a stream as the kernels keep it: state, previous grid, record (header + SAD table)
struct CameraStateHost {
    CameraStream st{};
    std::vector<uint32_t> prev;
    std::vector<uint8_t> rec;
    CameraStateHost() : rec((size_t)camera_layout().rec_bytes, 0) {}
    zly_camera_header header() const { zly_camera_header h; std::memcpy(&h, rec.data(), sizeof h); return h; }
    uint64_t* table() { return reinterpret_cast<uint64_t*>(rec.data() + camera_layout().sad_off); }
};

// ---- the host twin of camera_search_kernel and camera_pick_kernel for one frame with the grid S ----
inline void camera_frame_host(CameraStateHost& s, const uint32_t* S, int32_t W, int32_t H, const zly_camera_config& c)
{
    const int32_t C = c.cell, R = c.radius, gw = change_cells_axis(W, C), gh = change_cells_axis(H, C), side = 2 * R + 1;
    const bool first = camera_first(s.st, W, H, C);
    const zly_camera_header old = s.header();
    zly_camera_header h{};
    h.step = s.st.step + 1u; h.gw = gw; h.gh = gh;
    h.n_lost = old.n_lost; h.n_applied = old.n_applied;
    h.pend_x_q4 = old.pend_x_q4; h.pend_y_q4 = old.pend_y_q4;
    s.prev.resize((size_t)ZLY_CHANGE_MAX_CELLS, 0u);
    if (first) {
        h.flags = ZLY_CAMERA_FIRST;
        h.pend_x_q4 = h.pend_y_q4 = 0;
    } else {
        uint64_t* tab = s.table();
        for (int32_t dy = -R; dy <= R; ++dy)
            for (int32_t dx = -R; dx <= R; ++dx) {
                uint64_t sad = 0;
                for (int32_t cy = R; cy < gh - R; ++cy)
                    for (int32_t cx = R; cx < gw - R; ++cx)
                        sad += change_absdiff(S[cy * gw + cx], s.prev[(size_t)((cy - dy) * gw + (cx - dx))]);
                tab[camera_entry(dx, dy, R)] = sad;
            }
        uint64_t best = tab[0];
        uint32_t rank = camera_rank(-R, -R, R);
        for (int32_t i = 1; i < side * side; ++i) {
            const uint32_t rk = camera_rank(i % side - R, i / side - R, R);
            if (camera_less(tab[i], rk, best, rank)) { best = tab[i]; rank = rk; }
        }
        const int32_t dx = camera_rank_dx(rank, R), dy = camera_rank_dy(rank, R);
        const bool clip_x = camera_abs(dx) == R, clip_y = camera_abs(dy) == R;
        h.dx = dx; h.dy = dy;
        h.fx = camera_fit(dx, R, best, clip_x ? 0u : tab[camera_entry(dx - 1, dy, R)], clip_x ? 0u : tab[camera_entry(dx + 1, dy, R)]);
        h.fy = camera_fit(dy, R, best, clip_y ? 0u : tab[camera_entry(dx, dy - 1, R)], clip_y ? 0u : tab[camera_entry(dx, dy + 1, R)]);
        h.sx_q4 = camera_shift_q4(dx, h.fx, C); h.sy_q4 = camera_shift_q4(dy, h.fy, C);
        h.sad_min = best; h.sad_zero = tab[camera_entry(0, 0, R)];
        const bool lost = camera_lost(best, (uint32_t)c.max_residual_q4, camera_npix(gw, gh, R, C));
        h.flags = (lost ? ZLY_CAMERA_LOST : 0u) | (clip_x || clip_y ? ZLY_CAMERA_CLIPPED : 0u);
        if (lost) h.n_lost += 1u;
        else { h.pend_x_q4 += h.sx_q4; h.pend_y_q4 += h.sy_q4; }
    }
    std::memcpy(s.rec.data(), &h, sizeof h);
    for (int32_t i = 0; i < gw * gh; ++i) s.prev[(size_t)i] = S[i];
    s.st.W = W; s.st.H = H; s.st.C = C; s.st.have_prev = 1; s.st.step += 1u;
}

// ---- zly_camera_reset ----
inline void camera_reset_host(CameraStateHost& s)
{
    s.st = CameraStream{};
    zly_camera_header h = s.header();
    h.pend_x_q4 = h.pend_y_q4 = 0;
    std::memcpy(s.rec.data(), &h, sizeof h);
}

// ---- the host twin of camera_apply_kernel for one stream: x, y, live of the T slots of its track table.  Compile with contraction off. ----
inline void camera_apply_host(CameraStateHost& s, float* x, float* y, const uint32_t* live, int T)
{
    if (s.st.W < 1) return;                                          // no geometry
    zly_camera_header h = s.header();
    const float nx = camera_norm(h.pend_x_q4, s.st.W), ny = camera_norm(h.pend_y_q4, s.st.H);
    for (int t = 0; t < T; ++t)
        if (live[t]) { x[t] = x[t] + nx; y[t] = y[t] + ny; }
    h.pend_x_q4 = h.pend_y_q4 = 0; h.n_applied += 1u;
    std::memcpy(s.rec.data(), &h, sizeof h);
}

}  // namespace zly
