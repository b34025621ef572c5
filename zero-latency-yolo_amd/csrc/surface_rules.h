// surface_rules.h -- the host-side rules of the resident surfaces (include/zly.h "Resident surfaces"): the store's geometry, what a define and an
// update may ask for, the table of jobs and bands an update hands to the patch kernel (kernels_surface.hip), the phases and tables of a call of moves,
// and the views a detect call reads the store through.  Like frame_rules.h, on which it builds: plain C++, nothing of HIP or the engine, so that engine.cpp and a stand-alone test program
// (tests/cpp/test_surface_rules.cpp, test_surface_moves.cpp) compile the same text.  A refusal hands back its ZLY_ERR_* code and, through `err`, its message.
#pragma once
#include <vector>
#include "frame_rules.h"
#include "surface_device.h"

namespace zly {

struct SurfaceSlot {
    int32_t fmt = 0, w = 0, h = 0;
    bool defined = false;     // zly_surface_define has given the slot a format and a size
    bool valid = false;       // a rectangle has covered it whole since
};

// The store: max_surfaces slots, `stride` bytes apart, in ONE allocation of `total` bytes -- one d_base serves a whole view call.
// The largest store: a view's plane-0 offset rides in the low 56 bits of FrameDesc::src_off (zly_internal.h: the top byte holds the format), the
// offsets of planes 1 and 2 are 64-bit (ViewRec), and everything behind a plane's base is a 32-bit offset (view_valid: a plane extends over less than
// 2^31 bytes).  So every byte of a store of up to 2^56 bytes can be addressed, and a larger one is refused.
struct SurfaceStore {
    int32_t max_surfaces = 0;
    size_t  max_bytes_each = 0, stride = 0, total = 0;
};

inline int32_t surfaces_plan_store(int32_t max_surfaces, size_t max_bytes_each, SurfaceStore* out, std::string* err)
{
    if (max_surfaces < 1 || max_bytes_each < 1) return refuse(err, ZLY_ERR_INVALID_ARGUMENT, "zly_surfaces_enable: max_surfaces and max_bytes_each must be positive");
    const uint64_t A = ZLY_SURFACE_ALIGN;
    if ((uint64_t)max_bytes_each > ZLY_SURFACE_STORE_MAX) return refuse(err, ZLY_ERR_INVALID_ARGUMENT, "zly_surfaces_enable: the store would exceed 2^56 bytes");
    const uint64_t stride = ((uint64_t)max_bytes_each + A - 1) / A * A;
    if (stride > ZLY_SURFACE_STORE_MAX / (uint64_t)max_surfaces)
        return refuse(err, ZLY_ERR_INVALID_ARGUMENT, "zly_surfaces_enable: the store would exceed 2^56 bytes, the most a frame view's offset addresses");
    out->max_surfaces = max_surfaces; out->max_bytes_each = max_bytes_each;
    out->stride = (size_t)stride; out->total = (size_t)(stride * (uint64_t)max_surfaces);
    return ZLY_OK;
}

inline int32_t surface_check_slot(const SurfaceStore& st, int32_t s, std::string* err)
{
    if (s < 0 || s >= st.max_surfaces) return refuse(err, ZLY_ERR_INVALID_ARGUMENT, "surface " + std::to_string(s) + " out of range");
    return ZLY_OK;
}

// zly_surface_define: the slot's new state at *out (the caller stores it)
inline int32_t surface_define(const SurfaceStore& st, int32_t s, int32_t fmt, int32_t w, int32_t h, SurfaceSlot* out, std::string* err)
{
    if (int rc = surface_check_slot(st, s, err)) return rc;
    if (!pix_format(fmt)) return refuse(err, ZLY_ERR_INVALID_ARGUMENT, "unknown pixel format " + std::to_string(fmt));
    zly_frame_view v;
    size_t need = 0;
    if (view_tight(fmt, w, h, &v, nullptr) != ZLY_OK || !view_valid(&v, &need))
        return refuse(err, ZLY_ERR_INVALID_INPUT, "zly_surface_define: invalid size " + std::to_string(w) + " x " + std::to_string(h) + " for format " + std::to_string(fmt));
    if (need > st.max_bytes_each)
        return refuse(err, ZLY_ERR_INVALID_INPUT, "zly_surface_define: the surface needs " + std::to_string(need) + " bytes, a slot holds " + std::to_string(st.max_bytes_each));
    out->fmt = fmt; out->w = w; out->h = h; out->defined = true; out->valid = false;
    return ZLY_OK;
}

// the tight view of a defined slot, with offsets from the STORE's base
inline zly_frame_view surface_view(const SurfaceStore& st, const SurfaceSlot& sl, int32_t s)
{
    zly_frame_view v{};
    view_tight(sl.fmt, sl.w, sl.h, &v, nullptr);
    for (int p = 0; p < 3; ++p) v.off[p] += (uint64_t)s * (uint64_t)st.stride;
    return v;
}

// What an update enqueues.  stage_off[i]: where rectangle i's tight bytes (copy_view_tight of its source view) go in the staging buffer, 16-byte
// aligned; jobs: one per (rectangle, plane); bands: the jobs cut into bands, in job order -- what the kernel reads; table_off: where the band table
// goes, behind the pixels; stage_bytes: pixels + table; covers[i]: rectangle i covers its whole surface.
struct SurfacePlan {
    std::vector<size_t> stage_off;
    std::vector<SurfaceJob> jobs, bands;
    std::vector<char> covers;
    size_t pixel_bytes = 0, table_off = 0, stage_bytes = 0;
};

// a job's bands: max(1, ZLY_SURFACE_BAND_BYTES / row_bytes) whole rows each, the last one the rest
inline void surface_bands(const SurfaceJob& j, std::vector<SurfaceJob>* out)
{
    const uint32_t per = std::max<uint32_t>(1u, (uint32_t)ZLY_SURFACE_BAND_BYTES / j.row_bytes);
    for (uint32_t r = 0; r < j.rows; r += per) {
        SurfaceJob b = j;
        b.src_off = j.src_off + (uint64_t)r * j.row_bytes;
        b.dst_off = j.dst_off + (uint64_t)r * j.pitch;
        b.rows = std::min(per, j.rows - r);
        out->push_back(b);
    }
}

// Rectangles of one call that name the same surface must be disjoint.  A sweep instead of all pairs: the rectangles (each already inside its surface)
// are sorted by (surface, y0), and a rectangle is compared only with those behind it that begin above its last row -- n log n plus the pairs that
// share rows.  1024 single pixels spread over a surface cost some thousand comparisons where all pairs cost 520 000; 1024 rectangles in ONE row of
// one surface are still all pairs.  The pair is reported as "rectangle <later index>: overlaps rectangle <earlier index>".
inline int32_t surface_check_disjoint(int32_t n_rects, const zly_surface_rect* rects, const zly_frame_view* src_views, std::string* err)
{
    std::vector<int32_t> order((size_t)n_rects);
    for (int32_t i = 0; i < n_rects; ++i) order[(size_t)i] = i;
    std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {
        if (rects[a].surface != rects[b].surface) return rects[a].surface < rects[b].surface;
        if (rects[a].y0 != rects[b].y0) return rects[a].y0 < rects[b].y0;
        return a < b;
    });
    for (size_t p = 0; p < order.size(); ++p) {
        const int32_t a = order[p];
        const int64_t ay1 = (int64_t)rects[a].y0 + src_views[a].h, ax1 = (int64_t)rects[a].x0 + src_views[a].w;
        for (size_t q = p + 1; q < order.size(); ++q) {
            const int32_t b = order[q];
            if (rects[b].surface != rects[a].surface || rects[b].y0 >= ay1) break;      // sorted: nobody further on shares a row with a
            if (rects[b].x0 < ax1 && rects[a].x0 < (int64_t)rects[b].x0 + src_views[b].w)
                return refuse(err, ZLY_ERR_INVALID_ARGUMENT, "rectangle " + std::to_string(std::max(a, b)) + ": overlaps rectangle " + std::to_string(std::min(a, b)) +
                                                             " of the same surface (make two calls)");
        }
    }
    return ZLY_OK;
}

// zly_surface_update's checks and its table.  slots: the store's max_surfaces slots.  Nothing is modified: the caller applies plan->covers to the
// slots once the work is enqueued.
inline int32_t surface_plan_update(const SurfaceStore& st, const SurfaceSlot* slots, int32_t n_rects, const zly_surface_rect* rects, const uint8_t* const* bases,
                                   const size_t* buf_bytes, const zly_frame_view* src_views, SurfacePlan* plan, std::string* err)
{
    if (n_rects < 1 || n_rects > ZLY_SURFACE_MAX_RECTS)
        return refuse(err, ZLY_ERR_INVALID_ARGUMENT, "zly_surface_update: " + std::to_string(n_rects) + " rectangles, a call takes 1.." + std::to_string(ZLY_SURFACE_MAX_RECTS));
    if (!rects || !bases || !buf_bytes || !src_views) return refuse(err, ZLY_ERR_INVALID_ARGUMENT, "null argument");
    plan->stage_off.assign((size_t)n_rects, 0); plan->covers.assign((size_t)n_rects, 0);
    plan->jobs.clear(); plan->bands.clear();
    size_t total = 0;
    for (int i = 0; i < n_rects; ++i) {
        const zly_surface_rect& r = rects[i];
        const std::string who = "rectangle " + std::to_string(i) + ": ";
        if (int rc = surface_check_slot(st, r.surface, err)) return rc;
        const SurfaceSlot& sl = slots[r.surface];
        if (!sl.defined) return refuse(err, ZLY_ERR_INVALID_ARGUMENT, who + "surface " + std::to_string(r.surface) + " is not defined (zly_surface_define)");
        const zly_frame_view* sv = &src_views[i];
        std::string why;
        if (int rc = check_view(0, bases[i], buf_bytes[i], sv, &why)) return refuse(err, rc, who + why);
        if (sv->fmt != sl.fmt)
            return refuse(err, ZLY_ERR_INVALID_ARGUMENT, who + "format " + std::to_string(sv->fmt) + " is not the surface's (" + std::to_string(sl.fmt) + ")");
        const zly_frame_view whole = surface_view(st, sl, r.surface);
        zly_frame_view dst;
        if (view_crop(&whole, r.x0, r.y0, sv->w, sv->h, &dst, &why) != ZLY_OK) return refuse(err, ZLY_ERR_INVALID_ARGUMENT, who + why);
        plan->covers[(size_t)i] = r.x0 == 0 && r.y0 == 0 && sv->w == sl.w && sv->h == sl.h;
        plan->stage_off[(size_t)i] = total;
        int64_t rows[3], rb[3];
        const int np = plane_shape(sv->fmt, sv->w, sv->h, rows, rb);
        uint64_t src = total;
        for (int p = 0; p < np; ++p) {                          // the planes of the staged rectangle follow each other tight, as copy_view_tight writes them
            SurfaceJob j;
            j.src_off = src; j.dst_off = dst.off[p];
            j.row_bytes = (uint32_t)rb[p]; j.rows = (uint32_t)rows[p]; j.pitch = (uint32_t)dst.pitch[p]; j.pad_ = 0;
            plan->jobs.push_back(j);
            surface_bands(j, &plan->bands);
            src += (uint64_t)rows[p] * (uint64_t)rb[p];
        }
        total = (size_t)((src + 15u) / 16u * 16u);
    }
    if (int rc = surface_check_disjoint(n_rects, rects, src_views, err)) return rc;
    plan->pixel_bytes = total;
    plan->table_off = total;                                    // a multiple of 16
    plan->stage_bytes = total + plan->bands.size() * sizeof(SurfaceJob);
    return ZLY_OK;
}

// ---- moves (include/zly.h "Resident surfaces", MOVES) ----
typedef struct zly_surface_move SurfaceMoveReq;      // (the header keeps the plain name for the call)

inline bool surface_rects_meet(int64_t ax, int64_t ay, int64_t bx, int64_t by, int64_t w_a, int64_t h_a, int64_t w_b, int64_t h_b)
{
    return ax < bx + w_b && bx < ax + w_a && ay < by + h_b && by < ay + h_a;
}
inline bool surface_move_identity(const SurfaceMoveReq& m) { return m.sx == m.dx && m.sy == m.dy; }
// source and destination intersect (an identity move does, too; it is dropped before anyone asks)
inline bool surface_move_self_overlaps(const SurfaceMoveReq& m) { return surface_rects_meet(m.sx, m.sy, m.dx, m.dy, m.w, m.h, m.w, m.h); }
// two moves of one call conflict: the same surface, and a source meets the other's destination, or the destinations meet.  In surface pixels: the
// planes follow by the formats' evenness rules.
inline bool surface_moves_conflict(const SurfaceMoveReq& a, const SurfaceMoveReq& b)
{
    if (a.surface != b.surface) return false;
    return surface_rects_meet(a.sx, a.sy, b.dx, b.dy, a.w, a.h, b.w, b.h) || surface_rects_meet(a.dx, a.dy, b.sx, b.sy, a.w, a.h, b.w, b.h) ||
           surface_rects_meet(a.dx, a.dy, b.dx, b.dy, a.w, a.h, b.w, b.h);
}

// One phase: moves [first, first + count) of the call, launch A = a_bands [a_first, a_first + a_count) through surface_move_kernel, launch B =
// b_bands [b_first, b_first + b_count) through surface_patch_kernel with the bounce buffer as its staging (b_count = 0: nothing was gathered, no
// launch).  bounce_bytes: what the phase uses of the bounce buffer.  A phase of identity moves alone has no launch at all.
struct SurfaceMovePhase {
    int32_t first = 0, count = 0;
    size_t a_first = 0, a_count = 0, b_first = 0, b_count = 0, bounce_bytes = 0;
};

// What a zly_surface_move call enqueues.  a_jobs / b_jobs: one per (move, plane), before they are cut into a_bands / b_bands (in job order); via[i]:
// 0 move i is an identity and appears in no table, 1 it is copied store -> store, 2 it goes through the bounce buffer; phase_of[i]: its phase.  The
// tables go to the device as [a_bands][b_bands], both of 32-byte records: table_bytes.
struct SurfaceMovePlan {
    std::vector<SurfaceMovePhase> phases;
    std::vector<SurfaceMoveBand> a_jobs, a_bands;
    std::vector<SurfaceJob> b_jobs, b_bands;
    std::vector<char> via;
    std::vector<int32_t> phase_of;
    size_t table_bytes = 0;
};

// a move job's bands: as surface_bands cuts a patch job
inline void surface_move_bands(const SurfaceMoveBand& j, std::vector<SurfaceMoveBand>* out)
{
    const uint32_t per = std::max<uint32_t>(1u, (uint32_t)ZLY_SURFACE_BAND_BYTES / j.row_bytes);
    for (uint32_t r = 0; r < j.rows; r += per) {
        SurfaceMoveBand b = j;
        b.src_off = j.src_off + (uint64_t)r * j.src_pitch;
        b.dst_off = j.dst_off + (uint64_t)r * j.dst_pitch;      // (the bounce flag rides along: the sum stays far below bit 63)
        b.rows = std::min(per, j.rows - r);
        out->push_back(b);
    }
}

// zly_surface_move's checks, its phases and its tables.  bounce_bytes: the bounce buffer's size, 0 if the engine has none.  Nothing is modified.
// A move is compared with every move of the current phase: n^2 / 2 comparisons of three rectangle pairs at worst (1024 independent moves: half a
// million, about a millisecond), a handful for what a capture API hands out.
inline int32_t surface_plan_moves(const SurfaceStore& st, const SurfaceSlot* slots, int32_t n_moves, const SurfaceMoveReq* moves, size_t bounce_bytes, SurfaceMovePlan* plan,
                                  std::string* err)
{
    if (n_moves < 1 || n_moves > ZLY_SURFACE_MAX_MOVES)
        return refuse(err, ZLY_ERR_INVALID_ARGUMENT, "zly_surface_move: " + std::to_string(n_moves) + " moves, a call takes 1.." + std::to_string(ZLY_SURFACE_MAX_MOVES));
    if (!moves) return refuse(err, ZLY_ERR_INVALID_ARGUMENT, "null argument");
    if (bounce_bytes < 1) return refuse(err, ZLY_ERR_INVALID_ARGUMENT, "zly_surface_move: the engine has no bounce buffer (zly_surface_moves_enable)");
    plan->phases.clear(); plan->a_jobs.clear(); plan->a_bands.clear(); plan->b_jobs.clear(); plan->b_bands.clear();
    plan->via.assign((size_t)n_moves, 0); plan->phase_of.assign((size_t)n_moves, 0);
    SurfaceMovePhase ph;
    auto close_phase = [&](int32_t next_first) {
        ph.count = next_first - ph.first;
        ph.a_count = plan->a_bands.size() - ph.a_first; ph.b_count = plan->b_bands.size() - ph.b_first;
        plan->phases.push_back(ph);
        ph = SurfaceMovePhase();
        ph.first = next_first; ph.a_first = plan->a_bands.size(); ph.b_first = plan->b_bands.size();
    };
    for (int32_t i = 0; i < n_moves; ++i) {
        const SurfaceMoveReq& m = moves[i];
        const std::string who = "move " + std::to_string(i) + ": ";
        if (int rc = surface_check_slot(st, m.surface, err)) return rc;
        const SurfaceSlot& sl = slots[m.surface];
        if (!sl.defined) return refuse(err, ZLY_ERR_INVALID_ARGUMENT, who + "surface " + std::to_string(m.surface) + " is not defined (zly_surface_define)");
        if (!sl.valid) return refuse(err, ZLY_ERR_INVALID_INPUT, who + "surface " + std::to_string(m.surface) + " is not valid: it needs a rectangle that covers it whole (a keyframe)");
        const zly_frame_view whole = surface_view(st, sl, m.surface);
        zly_frame_view src, dst;
        std::string why;
        if (view_crop(&whole, m.sx, m.sy, m.w, m.h, &src, &why) != ZLY_OK) return refuse(err, ZLY_ERR_INVALID_ARGUMENT, who + "source: " + why);
        if (view_crop(&whole, m.dx, m.dy, m.w, m.h, &dst, &why) != ZLY_OK) return refuse(err, ZLY_ERR_INVALID_ARGUMENT, who + "destination: " + why);
        if (surface_move_identity(m)) { plan->phase_of[(size_t)i] = (int32_t)plan->phases.size(); continue; }
        int64_t rows[3], rb[3];
        const int np = plane_shape(sl.fmt, m.w, m.h, rows, rb);
        const bool self = surface_move_self_overlaps(m);
        size_t need = 0;                                        // of the bounce buffer: every job's start is 16-byte aligned
        if (self) {
            for (int p = 0; p < np; ++p) need += (size_t)(((uint64_t)rows[p] * (uint64_t)rb[p] + 15u) / 16u * 16u);
            if (need > bounce_bytes)
                return refuse(err, ZLY_ERR_INVALID_ARGUMENT, who + "it overlaps itself and needs " + std::to_string(need) + " bytes of the bounce buffer, which has " + std::to_string(bounce_bytes));
        }
        bool open_next = self && ph.bounce_bytes + need > bounce_bytes;
        for (int32_t k = ph.first; k < i && !open_next; ++k)
            open_next = plan->via[(size_t)k] != 0 && surface_moves_conflict(moves[k], m);
        if (open_next) close_phase(i);
        plan->phase_of[(size_t)i] = (int32_t)plan->phases.size();
        plan->via[(size_t)i] = self ? 2 : 1;
        for (int p = 0; p < np; ++p) {
            SurfaceMoveBand a;
            a.src_off = src.off[p]; a.row_bytes = (uint32_t)rb[p]; a.rows = (uint32_t)rows[p]; a.src_pitch = (uint32_t)src.pitch[p];
            if (self) {
                a.dst_off = ZLY_SURFACE_MOVE_TO_BOUNCE | (uint64_t)ph.bounce_bytes; a.dst_pitch = a.row_bytes;
                SurfaceJob b;
                b.src_off = ph.bounce_bytes; b.dst_off = dst.off[p]; b.row_bytes = a.row_bytes; b.rows = a.rows; b.pitch = (uint32_t)dst.pitch[p]; b.pad_ = 0;
                plan->b_jobs.push_back(b);
                surface_bands(b, &plan->b_bands);
                ph.bounce_bytes += (size_t)(((uint64_t)rows[p] * (uint64_t)rb[p] + 15u) / 16u * 16u);
            } else {
                a.dst_off = dst.off[p]; a.dst_pitch = (uint32_t)dst.pitch[p];
            }
            plan->a_jobs.push_back(a);
            surface_move_bands(a, &plan->a_bands);
        }
    }
    close_phase(n_moves);
    plan->table_bytes = (plan->a_bands.size() + plan->b_bands.size()) * sizeof(SurfaceJob);
    return ZLY_OK;
}

// zly_detect_surfaces: the n views into the store.  rois: null (whole surfaces) or n rectangles
inline int32_t surface_detect_views(const SurfaceStore& st, const SurfaceSlot* slots, int32_t n, const int32_t* surfaces, const zly_roi* rois, zly_frame_view* out,
                                    std::string* err)
{
    if (!surfaces) return refuse(err, ZLY_ERR_INVALID_ARGUMENT, "null surfaces");
    for (int i = 0; i < n; ++i) {
        if (int rc = surface_check_slot(st, surfaces[i], err)) return rc;
        const SurfaceSlot& sl = slots[surfaces[i]];
        if (!sl.defined) return refuse(err, ZLY_ERR_INVALID_ARGUMENT, "surface " + std::to_string(surfaces[i]) + " is not defined (zly_surface_define)");
        if (!sl.valid) return refuse(err, ZLY_ERR_INVALID_INPUT, "surface " + std::to_string(surfaces[i]) + " is not valid: it needs a rectangle that covers it whole (a keyframe)");
        out[i] = surface_view(st, sl, surfaces[i]);
        if (rois) {
            std::string why;
            if (view_crop(&out[i], rois[i].x0, rois[i].y0, rois[i].w, rois[i].h, &out[i], &why) != ZLY_OK)
                return refuse(err, ZLY_ERR_INVALID_ARGUMENT, "region " + std::to_string(i) + ": " + why);
        }
    }
    return ZLY_OK;
}

}  // namespace zly
