// test_zoom_plan -- the plan of the zoom regions (csrc/zoom_device.h, walked by the host twin of csrc/zoom_rules.h) on its own: no GPU, nothing of the
// engine.  tests/test_zoom_plan.py drives it.
//   test_zoom_plan plan      reads cases from stdin, prints their plans:
//                              in:  "<cases>", then per case "T K region_w region_h max_age class_id W H frame_no" and T lines
//                                   "live cls id last_seen x y w h vx vy" (the six floats as hex bit patterns)
//                              out: per case K lines "x0 y0 w h slot track_id"
//   test_zoom_plan offsets   for all twelve pixel formats, tight and pitched surfaces with plane offsets: every even origin of a grid of regions through
//                            zoom_frame_of + zoom_plane_off against view_crop; prints "offsets ok <count>" or the first mismatch (exit 1)
//   test_zoom_plan selftest  the offsets walk and a few thousand pseudo-random tables through the twin with its outputs checked against the rule's
//                            invariants (even origins inside the surface, at most one region per slot): what the sanitizer build runs
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "zoom_rules.h"

using namespace zly;

static float bits_f(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

static int run_plan()
{
    int cases = 0;
    if (scanf("%d", &cases) != 1 || cases < 0) { fprintf(stderr, "bad case count\n"); return 2; }
    for (int c = 0; c < cases; ++c) {
        int T = 0;
        zly_zoom_config cfg{};
        int32_t W = 0, H = 0;
        ZoomTable t{};
        if (scanf("%d %d %d %d %d %d %d %d %u", &T, &cfg.regions, &cfg.region_w, &cfg.region_h, &cfg.max_age, &cfg.class_id, &W, &H, &t.frame_no) != 9 || T < 0 || T > 64) {
            fprintf(stderr, "case %d: bad header\n", c);
            return 2;
        }
        if (zoom_check_config(&cfg, nullptr) != ZLY_OK || W < 2 || H < 2 || W >= (1 << 24) || H >= (1 << 24)) { fprintf(stderr, "case %d: refused config or surface\n", c); return 2; }
        for (int s = 0; s < T; ++s) {
            uint32_t b[6];
            if (scanf("%u %d %u %u %x %x %x %x %x %x", &t.live[s], &t.cls[s], &t.id[s], &t.last_seen[s], &b[0], &b[1], &b[2], &b[3], &b[4], &b[5]) != 10) {
                fprintf(stderr, "case %d: bad slot %d\n", c, s);
                return 2;
            }
            t.x[s] = bits_f(b[0]); t.y[s] = bits_f(b[1]); t.w[s] = bits_f(b[2]); t.h[s] = bits_f(b[3]); t.vx[s] = bits_f(b[4]); t.vy[s] = bits_f(b[5]);
        }
        zly_zoom_region out[ZLY_ZOOM_MAX_REGIONS];
        zoom_plan_host(t, T, cfg, W, H, out);
        for (int j = 0; j < cfg.regions; ++j) printf("%d %d %d %d %d %u\n", out[j].x0, out[j].y0, out[j].w, out[j].h, out[j].slot, out[j].track_id);
    }
    return 0;
}

static int run_offsets()
{
    static const int32_t fmts[12] = {ZLY_PIX_BGR, ZLY_PIX_NV12_BT601, ZLY_PIX_I420_BT601, ZLY_PIX_NV12_BT709, ZLY_PIX_I420_BT709, ZLY_PIX_YUY2_BT601,
                                     ZLY_PIX_UYVY_BT601, ZLY_PIX_YUY2_BT709, ZLY_PIX_UYVY_BT709, ZLY_PIX_RGB, ZLY_PIX_BGRA, ZLY_PIX_RGBA};
    long count = 0;
    for (int32_t fmt : fmts)
        for (int pitched = 0; pitched < 2; ++pitched) {
            const int32_t W = 102, H = 76;
            zly_frame_view sv;
            std::string err;
            if (view_tight(fmt, W, H, &sv, &err) != ZLY_OK) { printf("view_tight refused format %d: %s\n", fmt, err.c_str()); return 1; }
            if (pitched) {                                                           // padded rows, planes apart, the surface not at the buffer's start
                for (int p = 2; p >= 0; --p) { sv.off[p] = sv.off[p] * 3 + 4096u * (uint64_t)(p + 1); sv.pitch[p] = sv.pitch[p] * 2 + 64; }
            }
            const ZoomFrame zf = zoom_frame_of(&sv, 0);
            const int32_t rw = 40, rh = 30;
            for (int32_t y0 = 0; y0 + rh <= H; y0 += 2)
                for (int32_t x0 = 0; x0 + rw <= W; x0 += 2) {
                    zly_frame_view cv;
                    if (view_crop(&sv, x0, y0, rw, rh, &cv, &err) != ZLY_OK) { printf("view_crop refused format %d at %d, %d: %s\n", fmt, x0, y0, err.c_str()); return 1; }
                    for (int p = 0; p < zf.planes; ++p) {
                        const uint64_t got = zoom_plane_off(zf, p, x0, y0);
                        if (got != cv.off[p]) {
                            printf("format %d pitched %d plane %d at %d, %d: %llu, view_crop %llu\n", fmt, pitched, p, x0, y0, (unsigned long long)got, (unsigned long long)cv.off[p]);
                            return 1;
                        }
                        ++count;
                    }
                    if (zf.planes != pix_format(fmt)->planes) { printf("format %d: %d planes\n", fmt, zf.planes); return 1; }
                }
        }
    printf("offsets ok %ld\n", count);
    return 0;
}

static uint32_t lcg(uint32_t* s) { *s = *s * 1664525u + 1013904223u; return *s >> 8; }

static int run_selftest()
{
    if (int rc = run_offsets()) return rc;
    uint32_t seed = 12345u;
    for (int c = 0; c < 4000; ++c) {
        ZoomTable t{};
        const int T = 1 + (int)(lcg(&seed) % 64u);
        zly_zoom_config cfg{};
        cfg.regions = 1 + (int)(lcg(&seed) % 15u);
        cfg.region_w = 2 * (1 + (int)(lcg(&seed) % 300u)); cfg.region_h = 2 * (1 + (int)(lcg(&seed) % 300u));
        cfg.max_age = (int)(lcg(&seed) % 4u); cfg.class_id = (int)(lcg(&seed) % 3u) - 1;
        const int32_t W = 2 + (int32_t)(lcg(&seed) % 700u), H = 2 + (int32_t)(lcg(&seed) % 500u);
        t.frame_no = lcg(&seed) % 8u;
        for (int s = 0; s < T; ++s) {
            t.live[s] = lcg(&seed) % 4u != 0u; t.cls[s] = (int)(lcg(&seed) % 2u); t.id[s] = 1u + lcg(&seed) % 1000u;
            t.last_seen[s] = t.frame_no - lcg(&seed) % 4u;
            t.x[s] = (float)(lcg(&seed) % 1200u) / 1000.f - 0.1f; t.y[s] = (float)(lcg(&seed) % 1200u) / 1000.f - 0.1f;
            t.w[s] = (float)(lcg(&seed) % 500u) / 1000.f; t.h[s] = (float)(lcg(&seed) % 500u) / 1000.f;
            t.vx[s] = ((float)(lcg(&seed) % 200u) - 100.f) / 1000.f; t.vy[s] = ((float)(lcg(&seed) % 200u) - 100.f) / 1000.f;
        }
        zly_zoom_region out[ZLY_ZOOM_MAX_REGIONS];
        zoom_plan_host(t, T, cfg, W, H, out);
        const ZoomSize z = zoom_size(cfg.region_w, cfg.region_h, W, H);
        bool seen[64] = {};
        for (int j = 0; j < cfg.regions; ++j) {
            const zly_zoom_region& o = out[j];
            const bool inside = o.x0 >= 0 && o.y0 >= 0 && !((o.x0 | o.y0) & 1) && o.w == z.rw && o.h == z.rh && o.x0 + o.w <= W && o.y0 + o.h <= H;
            const bool slot_ok = o.slot == -1 ? o.track_id == 0u : (o.slot >= 0 && o.slot < T && !seen[o.slot] && t.live[o.slot] && o.track_id == t.id[o.slot]);
            if (!inside || !slot_ok) { printf("selftest case %d region %d: %d %d %d %d slot %d on %d x %d\n", c, j, o.x0, o.y0, o.w, o.h, o.slot, W, H); return 1; }
            if (o.slot >= 0) seen[o.slot] = true;
        }
    }
    printf("selftest ok\n");
    return 0;
}

int main(int argc, char** argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "plan") return run_plan();
    if (mode == "offsets") return run_offsets();
    if (mode == "selftest") return run_selftest();
    fprintf(stderr, "usage: test_zoom_plan plan | offsets | selftest\n");
    return 2;
}
