// zoom_rules.h -- the host side of the zoom regions (include/zly.h "Zoom regions"): the config check, the record a frame's plan kernel is given
// (from the surface's view and the format table), and the HOST TWIN of the plan kernel -- the same functions of zoom_device.h, walked slot by slot in
// a loop.  Nothing here touches a device or the engine, as frame_rules.h does not: engine.cpp and a stand-alone test program
// (tests/cpp/test_zoom_plan.cpp) compile the same text.
#pragma once
#include "frame_rules.h"
#include "zoom_device.h"

namespace zly {

#define ZLY_ZOOM_MAX_REGION_DIM 16384

inline int zoom_check_config(const zly_zoom_config* c, std::string* err)
{
    if (!c) return refuse(err, ZLY_ERR_INVALID_ARGUMENT, "null zoom config");
    if (c->regions < 1 || c->regions > ZLY_ZOOM_MAX_REGIONS) return refuse(err, ZLY_ERR_INVALID_ARGUMENT, "zoom regions must lie in 1..15");
    if (c->region_w < 2 || c->region_h < 2 || c->region_w > ZLY_ZOOM_MAX_REGION_DIM || c->region_h > ZLY_ZOOM_MAX_REGION_DIM || ((c->region_w | c->region_h) & 1))
        return refuse(err, ZLY_ERR_INVALID_ARGUMENT, "a zoom region's width and height must be even and lie in 2..16384");
    if (c->max_age < 0) return refuse(err, ZLY_ERR_INVALID_ARGUMENT, "max_age must be >= 0");
    if (c->class_id < -1) return refuse(err, ZLY_ERR_INVALID_ARGUMENT, "class_id must be -1 or a class");
    return ZLY_OK;
}

// the surface of a zoom frame: a known format, 2 <= w, h < 2^24 (the view itself is checked by check_view)
inline int zoom_check_surface(const zly_frame_view* v, std::string* err)
{
    if (!v) return refuse(err, ZLY_ERR_INVALID_ARGUMENT, "null view");
    if (!pix_format(v->fmt)) return refuse(err, ZLY_ERR_INVALID_ARGUMENT, "unknown pixel format " + std::to_string(v->fmt));
    if (v->w < 2 || v->h < 2 || v->w >= (1 << 24) || v->h >= (1 << 24))
        return refuse(err, ZLY_ERR_INVALID_ARGUMENT, "a zoomed surface must be 2..2^24-1 pixels on a side, got " + std::to_string(v->w) + " x " + std::to_string(v->h));
    return ZLY_OK;
}

// the plan kernel's record of a frame on the (valid) surface view v: view_crop's offsets, as steps and shifts per plane
inline ZoomFrame zoom_frame_of(const zly_frame_view* v, int32_t stream)
{
    const PixFormat* f = pix_format(v->fmt);
    ZoomFrame z{};
    z.W = v->w; z.H = v->h; z.stream = stream; z.fmt = v->fmt; z.planes = f->planes;
    for (int p = 0; p < f->planes; ++p) { z.off[p] = v->off[p]; z.pitch[p] = v->pitch[p]; }
    z.xstep[0] = (uint8_t)f->bpp;
    if (f->chroma == CHROMA_NV12) { z.xstep[1] = 2; z.xsh[1] = 1; z.ysh[1] = 1; }
    if (f->chroma == CHROMA_I420) { z.xstep[1] = z.xstep[2] = 1; z.xsh[1] = z.xsh[2] = 1; z.ysh[1] = z.ysh[2] = 1; }
    return z;
}

// A stream's table as the plan reads it (the fields of TrackStream and TrackMotion it needs; vx = vy = 0 without the motion model)
struct ZoomTable {
    uint32_t frame_no;
    uint32_t live[64];
    float    x[64], y[64], w[64], h[64], vx[64], vy[64];
    int32_t  cls[64];
    uint32_t id[64], last_seen[64];
};

// The host twin of zoom_plan_kernel: out[0 .. K) for one frame of a W x H surface.  T: the table's slots
inline void zoom_plan_host(const ZoomTable& t, int T, const zly_zoom_config& c, int32_t W, int32_t H, zly_zoom_region* out)
{
    const ZoomSize z = zoom_size(c.region_w, c.region_h, W, H);
    const uint32_t F = t.frame_no;
    int order[64], n_elig = 0;
    uint32_t age[64], key[64];
    for (int s = 0; s < T && s < 64; ++s) {
        if (!zoom_eligible(t.live[s] != 0u, t.cls[s], F, t.last_seen[s], t.w[s], t.h[s], W, H, z, c.max_age, c.class_id)) continue;
        age[s] = F - t.last_seen[s]; key[s] = zoom_area_key(t.w[s], t.h[s]);
        int k = n_elig++;                                                               // insertion by zoom_before
        while (k > 0 && zoom_before(age[s], key[s], s, age[order[k - 1]], key[order[k - 1]], order[k - 1])) { order[k] = order[k - 1]; --k; }
        order[k] = s;
    }
    int chosen = 0;
    for (int r = 0; r < n_elig && chosen < c.regions; ++r) {
        const int s = order[r];
        const float px = zoom_predict(t.x[s], t.vx[s], F, t.last_seen[s]), py = zoom_predict(t.y[s], t.vy[s], F, t.last_seen[s]);
        bool covered = false;
        for (int j = 0; j < chosen && !covered; ++j)
            covered = zoom_covered_axis(px, t.w[s], out[j].x0, z.rw, W) && zoom_covered_axis(py, t.h[s], out[j].y0, z.rh, H);
        if (covered) continue;
        zly_zoom_region& o = out[chosen++];
        o.x0 = zoom_origin(px, W, z.rw, z.xmax); o.y0 = zoom_origin(py, H, z.rh, z.ymax);
        o.w = z.rw; o.h = z.rh; o.slot = s; o.track_id = t.id[s];
    }
    for (; chosen < c.regions; ++chosen) {
        zly_zoom_region& o = out[chosen];
        o.x0 = zoom_fallback_origin(W, z.rw); o.y0 = zoom_fallback_origin(H, z.rh);
        o.w = z.rw; o.h = z.rh; o.slot = -1; o.track_id = 0u;
    }
}

}  // namespace zly
