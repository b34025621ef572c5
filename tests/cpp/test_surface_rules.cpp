// test_surface_rules.cpp -- csrc/surface_rules.h (+ surface_device.h, frame_rules.h) on its own: the headers and the standard library, nothing of the
// engine, no GPU.  It keeps a store in host memory and runs a script of the calls of include/zly.h's "Resident surfaces" against the rules; for every
// update it prints the verdict and the job and band tables, and EXECUTES the band table twice on host arrays -- once row by row with memcpy, once
// item by item as the patch kernel walks it (surface_device.h: granules, clipped heads and tails, store widths), checking on the way that every wide
// store is aligned and that no access leaves its row.  tests/test_surface_rules.py drives it and compares the store with the numpy oracle.
// TEST INFRASTRUCTURE.
//
//   test_surface_rules SCRIPT      one command per line:
//       store MAX_SURFACES MAX_BYTES_EACH
//       define S FMT W H
//       update N FILE              then N lines "S X0 Y0 FMT W H": the rectangles' tight bytes lie one behind the other in FILE
//       views N ROIS               then N lines "S" or (ROIS = 1) "S X0 Y0 W H"
//       dump S FILE                the slot's whole stride
//   test_surface_rules selftest    a built-in walk over every format (also built with -fsanitize=address,undefined: make surface_rules_san)
#include "surface_rules.h"

#include <stdio.h>
#include <stdlib.h>
#include <fstream>
#include <sstream>
#include <vector>

using namespace zly;

static const uint8_t POISON = 0xEE;       // what the host store holds before anything is written

struct World {
    SurfaceStore st;
    std::vector<SurfaceSlot> slots;
    std::vector<uint8_t> store;
    bool enabled = false;
};

// the band table row by row: the plain meaning of a band
static void execute_rows(const std::vector<SurfaceJob>& bands, const std::vector<uint8_t>& stage, std::vector<uint8_t>* store)
{
    for (const SurfaceJob& b : bands)
        for (uint32_t r = 0; r < b.rows; ++r)
            memcpy(store->data() + b.dst_off + (uint64_t)r * b.pitch, stage.data() + b.src_off + (uint64_t)r * b.row_bytes, b.row_bytes);
}

// ... and item by item as surface_patch_kernel does; the number of violations (a misaligned store, an access outside its row or its array)
static int execute_items(const std::vector<SurfaceJob>& bands, const std::vector<uint8_t>& stage, size_t pixel_bytes, std::vector<uint8_t>* store, std::vector<uint8_t>* hits)
{
    int bad = 0;
    for (const SurfaceJob& j : bands) {
        const uint32_t n = j.row_bytes, G = surface_row_granules(n);
        const uint64_t items = (uint64_t)j.rows * G;
        for (uint64_t i = 0; i < items; ++i) {
            const uint32_t r = j.rows == 1 ? 0 : (uint32_t)i / G, g = j.rows == 1 ? (uint32_t)i : (uint32_t)i - r * G;
            const uint64_t drow = j.dst_off + (uint64_t)r * j.pitch;
            uint32_t lo, hi;
            if (!surface_granule(drow, n, g, &lo, &hi)) continue;
            uint64_t s = j.src_off + (uint64_t)r * n + lo, d = drow + lo;
            uint32_t k = hi - lo;
            if (hi > n || lo >= hi || k > 16 || s + k > pixel_bytes || d + k > store->size()) { ++bad; continue; }
            while (k) {
                const uint32_t wd = k == 16 ? 16 : surface_edge_width((uint32_t)d, k);
                if (d % wd || wd > k) ++bad;
                for (uint32_t t = 0; t < wd; ++t) { (*store)[d + t] = stage[s + t]; if ((*hits)[d + t]++) ++bad; }      // no byte is written twice
                d += wd; s += wd; k -= wd;
            }
        }
    }
    return bad;
}

// bands tile their jobs: in job order, whole rows, each row once, within the band size
static int check_bands(const SurfacePlan& pl)
{
    int bad = 0;
    size_t k = 0;
    for (const SurfaceJob& j : pl.jobs) {
        uint32_t r = 0;
        while (r < j.rows) {
            if (k >= pl.bands.size()) return bad + 1;
            const SurfaceJob& b = pl.bands[k++];
            if (b.row_bytes != j.row_bytes || b.pitch != j.pitch || b.rows < 1 || b.src_off != j.src_off + (uint64_t)r * j.row_bytes || b.dst_off != j.dst_off + (uint64_t)r * j.pitch) ++bad;
            if (b.rows > 1 && (uint64_t)b.rows * b.row_bytes > ZLY_SURFACE_BAND_BYTES) ++bad;
            if (r + b.rows < j.rows && (uint64_t)(b.rows + 1) * b.row_bytes <= ZLY_SURFACE_BAND_BYTES) ++bad;       // a band that is not the last is full
            r += b.rows;
        }
        if (r != j.rows) ++bad;
    }
    return bad + (k != pl.bands.size());
}

struct RectIn { int s, x0, y0, fmt, w, h; };

// one update against the world; prints the verdict (and, if asked, the tables); the return code of the rules
static int run_update(World& W, const std::vector<RectIn>& in, const std::vector<uint8_t>& pixels, bool print)
{
    const int n = (int)in.size();
    std::vector<zly_surface_rect> rects((size_t)n);
    std::vector<zly_frame_view> views((size_t)n);
    std::vector<const uint8_t*> bases((size_t)n, pixels.data());
    std::vector<size_t> sizes((size_t)n, pixels.size());
    uint64_t at = 0;
    for (int i = 0; i < n; ++i) {
        rects[(size_t)i] = {in[(size_t)i].s, in[(size_t)i].x0, in[(size_t)i].y0};
        zly_frame_view v{};
        if (view_tight(in[(size_t)i].fmt, in[(size_t)i].w, in[(size_t)i].h, &v, nullptr) != ZLY_OK) { v.fmt = in[(size_t)i].fmt; v.w = in[(size_t)i].w; v.h = in[(size_t)i].h; }
        for (int p = 0; p < 3; ++p) v.off[p] += at;
        at += frame_bytes(v.fmt, v.w, v.h);
        views[(size_t)i] = v;
    }
    SurfacePlan pl;
    std::string err;
    const int rc = surface_plan_update(W.st, W.slots.data(), n, n ? rects.data() : nullptr, bases.data(), sizes.data(), views.data(), &pl, &err);
    if (rc != ZLY_OK) { if (print) printf("update %d\nerror %s\n", rc, err.c_str()); return rc; }
    if (print) {
        printf("update 0 %zu %zu %zu %zu\n", pl.jobs.size(), pl.bands.size(), pl.pixel_bytes, pl.stage_bytes);
        for (const SurfaceJob& j : pl.jobs) printf("job %llu %llu %u %u %u\n", (unsigned long long)j.src_off, (unsigned long long)j.dst_off, j.row_bytes, j.rows, j.pitch);
        for (const SurfaceJob& j : pl.bands) printf("band %llu %llu %u %u %u\n", (unsigned long long)j.src_off, (unsigned long long)j.dst_off, j.row_bytes, j.rows, j.pitch);
        printf("covers");
        for (char c : pl.covers) printf(" %d", (int)c);
        printf("\n");
    }
    // the staging buffer as the engine fills it: the rectangles tight at their offsets, the band table behind them
    std::vector<uint8_t> stage(pl.stage_bytes, 0x77);
    for (int i = 0; i < n; ++i) copy_view_tight(stage.data() + pl.stage_off[(size_t)i], pixels.data(), &views[(size_t)i]);
    if (!pl.bands.empty()) memcpy(stage.data() + pl.table_off, pl.bands.data(), pl.bands.size() * sizeof(SurfaceJob));
    std::vector<uint8_t> by_rows = W.store, hits(W.store.size(), 0);
    execute_rows(pl.bands, stage, &by_rows);
    int bad = execute_items(pl.bands, stage, pl.pixel_bytes, &W.store, &hits);
    bad += check_bands(pl);
    bad += pl.table_off % 16 != 0;
    for (size_t o : pl.stage_off) bad += o % 16 != 0;
    const bool same = by_rows == W.store;
    for (int i = 0; i < n; ++i) if (pl.covers[(size_t)i]) W.slots[(size_t)rects[(size_t)i].surface].valid = true;
    if (print) printf("exec %s %d\n", same ? "same" : "DIFFER", bad);
    return same && bad == 0 ? ZLY_OK : -1;
}

static int run_script(const char* path)
{
    std::ifstream f(path);
    if (!f) { fprintf(stderr, "cannot open %s\n", path); return 2; }
    World W;
    std::string line;
    while (std::getline(f, line)) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd) || cmd[0] == '#') continue;
        std::string err;
        if (cmd == "store") {
            long long s = 0; unsigned long long b = 0;
            in >> s >> b;
            SurfaceStore st;
            const int rc = W.enabled ? ZLY_ERR_INVALID_ARGUMENT : surfaces_plan_store((int32_t)s, (size_t)b, &st, &err);
            if (rc == ZLY_OK && st.total <= (1u << 28)) { W.st = st; W.slots.assign((size_t)s, SurfaceSlot()); W.store.assign(st.total, POISON); W.enabled = true; }
            printf("store %d %zu %zu\n", rc, rc ? (size_t)0 : st.stride, rc ? (size_t)0 : st.total);
        } else if (cmd == "define") {
            int s = 0, fmt = 0, w = 0, h = 0;
            in >> s >> fmt >> w >> h;
            SurfaceSlot sl;
            const int rc = surface_define(W.st, s, fmt, w, h, &sl, &err);
            if (rc == ZLY_OK) W.slots[(size_t)s] = sl;
            printf("define %d\n", rc);
        } else if (cmd == "update") {
            int n = 0; std::string file;
            in >> n >> file;
            std::vector<RectIn> rs;
            for (int i = 0; i < n && std::getline(f, line); ++i) {
                std::istringstream q(line);
                RectIn r{};
                q >> r.s >> r.x0 >> r.y0 >> r.fmt >> r.w >> r.h;
                rs.push_back(r);
            }
            std::ifstream pf(file, std::ios::binary);
            std::vector<uint8_t> pixels((std::istreambuf_iterator<char>(pf)), std::istreambuf_iterator<char>());
            if (pixels.empty()) pixels.push_back(0);
            run_update(W, rs, pixels, true);
        } else if (cmd == "views") {
            int n = 0, with = 0;
            in >> n >> with;
            std::vector<int32_t> ss; std::vector<zly_roi> rois;
            for (int i = 0; i < n && std::getline(f, line); ++i) {
                std::istringstream q(line);
                int s = 0; zly_roi r{};
                q >> s;
                if (with) q >> r.x0 >> r.y0 >> r.w >> r.h;
                ss.push_back(s); rois.push_back(r);
            }
            std::vector<zly_frame_view> out((size_t)n);
            const int rc = surface_detect_views(W.st, W.slots.data(), n, ss.data(), with ? rois.data() : nullptr, out.data(), &err);
            printf("views %d\n", rc);
            if (rc == ZLY_OK)
                for (const zly_frame_view& v : out)
                    printf("view %d %d %d %llu %llu %llu %d %d %d %zu\n", v.fmt, v.w, v.h, (unsigned long long)v.off[0], (unsigned long long)v.off[1], (unsigned long long)v.off[2],
                           v.pitch[0], v.pitch[1], v.pitch[2], view_bytes(&v));
        } else if (cmd == "dump") {
            int s = 0; std::string file;
            in >> s >> file;
            std::ofstream of(file, std::ios::binary);
            of.write((const char*)W.store.data() + (size_t)s * W.st.stride, (std::streamsize)W.st.stride);
            printf("dump %d\n", s);
        } else {
            printf("unknown %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}

// every format: a keyframe, then seeded legal rectangles, many per call and disjoint by construction (a grid of cells); both executions must agree
static int selftest()
{
    int failed = 0, calls = 0;
    const int fmts[] = {ZLY_PIX_BGR, ZLY_PIX_NV12_BT601, ZLY_PIX_I420_BT709, ZLY_PIX_YUY2_BT601, ZLY_PIX_UYVY_BT709, ZLY_PIX_RGB, ZLY_PIX_BGRA, ZLY_PIX_RGBA};
    uint32_t seed = 12345;
    auto rnd = [&](uint32_t m) { seed = seed * 1664525u + 1013904223u; return (seed >> 8) % m; };
    for (int fmt : fmts)
        for (int big = 0; big < 2; ++big) {
            const PixFormat* pf = pix_format(fmt);
            const int Wd = big ? 1922 : (pf->even_w ? 38 : 37), Ht = big ? 36 : (pf->even_h ? 30 : 29);
            World W;
            std::string err;
            if (surfaces_plan_store(3, frame_bytes(fmt, Wd, Ht) + 5, &W.st, &err) != ZLY_OK) return 1;
            W.slots.assign(3, SurfaceSlot()); W.store.assign(W.st.total, POISON);
            if (surface_define(W.st, 1, fmt, Wd, Ht, &W.slots[1], &err) != ZLY_OK) return 1;
            std::vector<uint8_t> pixels(frame_bytes(fmt, Wd, Ht) * 2);
            for (size_t i = 0; i < pixels.size(); ++i) pixels[i] = (uint8_t)(i * 31 + (i >> 7));
            failed += run_update(W, {{1, 0, 0, fmt, Wd, Ht}}, pixels, false) != ZLY_OK; ++calls;
            failed += !W.slots[1].valid;
            for (int round = 0; round < 6; ++round) {
                const int cw = 2 * (1 + (int)rnd(big ? 300 : 5)), chh = 2 * (1 + (int)rnd(5));      // cells of even size: legal origins for every format
                std::vector<RectIn> rs;
                for (int y = 0; y + chh <= Ht; y += chh)
                    for (int x = 0; x + cw <= Wd && (int)rs.size() < ZLY_SURFACE_MAX_RECTS; x += cw) {
                        if (rnd(3) == 0) continue;
                        int w = cw, h = chh, dx = 0, dy = 0;
                        if (!pf->even_w) { w = 1 + (int)rnd((uint32_t)cw); dx = (int)rnd((uint32_t)(cw - w + 1)); }
                        if (!pf->even_h) { h = 1 + (int)rnd((uint32_t)chh); dy = (int)rnd((uint32_t)(chh - h + 1)); }
                        rs.push_back({1, x + dx, y + dy, fmt, w, h});
                    }
                if (rs.empty()) continue;
                failed += run_update(W, rs, pixels, false) != ZLY_OK; ++calls;
            }
            // the neighbours and the slack behind the frame are as they were
            const size_t fb = frame_bytes(fmt, Wd, Ht);
            for (size_t i = 0; i < W.store.size(); ++i)
                if ((i < W.st.stride || i >= W.st.stride + fb) && W.store[i] != POISON) { ++failed; break; }
        }
    printf("%d updates, %d failed\n", calls, failed);
    return failed ? 1 : 0;
}

int main(int argc, char** argv)
{
    if (argc == 2 && std::string(argv[1]) == "selftest") return selftest();
    if (argc == 2) return run_script(argv[1]);
    fprintf(stderr, "usage: test_surface_rules SCRIPT | selftest\n");
    return 2;
}
