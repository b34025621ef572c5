// test_frame_rules.cpp -- csrc/frame_rules.h on its own: the header and the standard library, nothing of the engine, no GPU.  It walks the case
// families of tests/frame_rules_cases.py (whose recorded answers tests/test_frame_rules_golden.py replays through libzly.so) and checks what needs
// no recording: the format table, tight view = frame bytes, crops fit their surface and compose, the tight copy of a crop is a slice of the
// surface's tight copy, and every refusal.  One line per failed check; exit status 1 if any failed.  TEST INFRASTRUCTURE.
//
//   test_frame_rules            (also built with -fsanitize=address,undefined: make frame_rules_san)
#include "frame_rules.h"

#include <stdio.h>
#include <limits.h>
#include <vector>

using namespace zly;

static int g_checks = 0, g_failed = 0;
#define CHECK(cond, ...) do { ++g_checks; if (!(cond)) { ++g_failed; printf("FAILED %s:%d  %s  [", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("]\n"); } } while (0)

// the test's own copy of the twelve formats: planes, bytes per pixel of plane 0, 0 / 1 (NV12) / 2 (I420), even width, even height, level
struct Row { int fmt, planes, bpp, chroma, even_w, even_h, front; };
static const Row ROWS[12] = {{0, 1, 3, 0, 0, 0, 0},  {1, 2, 1, 1, 1, 1, 1},  {2, 3, 1, 2, 1, 1, 1},  {3, 2, 1, 1, 1, 1, 1},  {4, 3, 1, 2, 1, 1, 1},  {10, 1, 2, 0, 1, 0, 3},
                            {11, 1, 2, 0, 1, 0, 3}, {12, 1, 2, 0, 1, 0, 3}, {13, 1, 2, 0, 1, 0, 3}, {16, 1, 3, 0, 0, 0, 2}, {17, 1, 4, 0, 0, 0, 2}, {18, 1, 4, 0, 0, 0, 2}};
static const Row* row_of(int fmt) { for (const Row& r : ROWS) if (r.fmt == fmt) return &r; return nullptr; }
// front_level as zly_internal.h had it, by ranges
static int old_front_level(int fmt) { return fmt == 0 ? 0 : fmt >= 1 && fmt <= 4 ? 1 : fmt >= 10 && fmt <= 13 ? 3 : 2; }

static bool same(const zly_frame_view& a, const zly_frame_view& b)
{
    return a.fmt == b.fmt && a.w == b.w && a.h == b.h && !memcmp(a.off, b.off, sizeof a.off) && !memcmp(a.pitch, b.pitch, sizeof a.pitch);
}
static zly_frame_view untouched() { zly_frame_view v; memset(&v, 0x5A, sizeof v); return v; }
static bool is_untouched(const zly_frame_view& v) { const zly_frame_view u = untouched(); return !memcmp(&v, &u, sizeof v); }

// a w x h surface of format fmt whose pitches are the rows' bytes + extra, planes behind each other
static zly_frame_view surface(int fmt, int w, int h, int extra)
{
    zly_frame_view v{};
    int64_t rows[3], rb[3];
    const int np = plane_shape(fmt, w, h, rows, rb);
    v.fmt = fmt; v.w = w; v.h = h;
    uint64_t at = 0;
    for (int p = 0; p < np; ++p) { v.off[p] = at; v.pitch[p] = (int32_t)rb[p] + extra; at += (uint64_t)rows[p] * (uint64_t)v.pitch[p]; }
    return v;
}

static void test_table()
{
    int known = 0;
    for (int64_t f : {(int64_t)INT32_MIN, (int64_t)INT32_MAX}) CHECK(!pix_format((int32_t)f), "fmt %lld", (long long)f);
    for (int fmt = -8; fmt <= 64; ++fmt) {
        const PixFormat* f = pix_format(fmt);
        const Row* r = row_of(fmt);
        CHECK((f != nullptr) == (r != nullptr), "fmt %d", fmt);
        CHECK(front_level(fmt) == old_front_level(fmt), "fmt %d: level %d", fmt, front_level(fmt));
        if (!f || !r) continue;
        ++known;
        CHECK(f->fmt == fmt && f->planes == r->planes && (int)f->bpp == r->bpp && (int)f->chroma == r->chroma && f->even_w == (r->even_w != 0) &&
              f->even_h == (r->even_h != 0) && f->front == r->front, "fmt %d", fmt);
    }
    CHECK(known == 12, "%d formats", known);
    CHECK(ZLY_FRONT_BGR == 0 && ZLY_FRONT_YUV == 1 && ZLY_FRONT_PACKED == 2 && ZLY_FRONT_YUV422 == 3, "levels");
}

static void test_frames()
{
    const int v[] = {0, -1, 1, 2, 3, 4, 416, 417, 1080, 1920, 32768, INT32_MAX - 1, INT32_MAX};
    for (int fmt = -1; fmt <= 20; ++fmt)
        for (int w : v)
            for (int h : v) {
                const Row* r = row_of(fmt);
                const bool ok = r && w >= 1 && h >= 1 && !(r->even_w && (w & 1)) && !(r->even_h && (h & 1));
                const size_t fb = frame_bytes(fmt, w, h);
                const uint64_t want = !ok ? 0 : r->chroma ? (uint64_t)w * (uint64_t)h * 3 / 2 : (uint64_t)w * (uint64_t)h * (uint64_t)r->bpp;
                CHECK(fb == want, "fmt %d %d x %d: %zu", fmt, w, h, fb);
                zly_frame_view t = untouched();
                std::string err;
                const int rc = view_tight(fmt, w, h, &t, &err);
                if (!ok) {
                    CHECK(rc == ZLY_ERR_INVALID_ARGUMENT && err == "zly_view_tight: unknown format or invalid size" && is_untouched(t), "fmt %d %d x %d: rc %d", fmt, w, h, rc);
                    std::string e2;
                    CHECK(check_frame(fmt, (const uint8_t*)"", 1, w, h, &e2) == (r ? ZLY_ERR_INVALID_INPUT : ZLY_ERR_INVALID_ARGUMENT), "fmt %d %d x %d", fmt, w, h);
                    CHECK(e2.find(r ? "Invalid image data size: expected " : "unknown pixel format ") == 0, "%s", e2.c_str());
                    continue;
                }
                CHECK(rc == ZLY_OK && err.empty() && t.fmt == fmt && t.w == w && t.h == h, "fmt %d %d x %d: rc %d", fmt, w, h, rc);
                // a plane of 2 GiB or more makes no valid view; below that, the tight view needs exactly the frame's bytes
                const bool fits = (uint64_t)w * (uint64_t)h * (uint64_t)r->bpp < (1ull << 31);
                CHECK(view_bytes(&t) == (fits ? fb : 0), "fmt %d %d x %d: %zu, frame %zu", fmt, w, h, view_bytes(&t), fb);
                std::string e2;
                CHECK(check_frame(fmt, (const uint8_t*)"", fb, w, h, &e2) == ZLY_OK && e2.empty(), "fmt %d %d x %d", fmt, w, h);
                CHECK(check_frame(fmt, (const uint8_t*)"", fb + 1, w, h, &e2) == ZLY_ERR_INVALID_INPUT &&
                      e2 == "Invalid image data size: expected " + std::to_string(fb) + ", got " + std::to_string(fb + 1), "%s", e2.c_str());
                CHECK(check_frame(fmt, nullptr, fb, w, h, &e2) == ZLY_ERR_INVALID_INPUT, "fmt %d: null frame", fmt);
            }
    std::string e;
    CHECK(check_frame(ZLY_PIX_NV12_BT601, (const uint8_t*)"", 9, 3, 2, &e) == ZLY_ERR_INVALID_INPUT &&
          e == "Invalid image data size: expected 9, got 9 (YUV 4:2:0 needs even width and height >= 2)", "%s", e.c_str());
    CHECK(check_frame(ZLY_PIX_UYVY_BT709, (const uint8_t*)"", 12, 3, 2, &e) == ZLY_ERR_INVALID_INPUT &&
          e == "Invalid image data size: expected 12, got 12 (packed YUV 4:2:2 needs even width >= 2)", "%s", e.c_str());
    // the resize modes bound a request's sides
    e.clear();
    CHECK(check_frame_mode(0, 1 << 20, 1 << 20, &e) == ZLY_OK && e.empty(), "stretch");
    CHECK(check_frame_mode(ZLY_FLAG_LETTERBOX | ZLY_FLAG_AREA, ZLY_LETTERBOX_MAX_DIM, ZLY_AREA_MAX_DIM, &e) == ZLY_OK && e.empty(), "at the bound");
    CHECK(check_frame_mode(ZLY_FLAG_LETTERBOX, ZLY_LETTERBOX_MAX_DIM + 1, 8, &e) == ZLY_ERR_INVALID_INPUT &&
          e == "letterbox mode takes frames of at most 16384 pixels on a side, got 16385 x 8", "%s", e.c_str());
    CHECK(check_frame_mode(ZLY_FLAG_AREA, 8, ZLY_AREA_MAX_DIM + 1, &e) == ZLY_ERR_INVALID_INPUT &&
          e == "area mode takes frames of at most 16384 pixels on a side, got 8 x 16385", "%s", e.c_str());
}

// rows [y0, y0 + h) x columns [x0, x0 + w) of the tight W x H frame `whole`, plane by plane, by the test's own arithmetic
static std::vector<uint8_t> slice(const Row& r, const std::vector<uint8_t>& whole, int W, int H, int x0, int y0, int w, int h)
{
    std::vector<uint8_t> out;
    auto take = [&](size_t base, size_t pitch, int first_row, int rows, size_t first_byte, size_t bytes) {
        for (int y = first_row; y < first_row + rows; ++y) out.insert(out.end(), whole.begin() + base + y * pitch + first_byte, whole.begin() + base + y * pitch + first_byte + bytes);
    };
    take(0, (size_t)W * r.bpp, y0, h, (size_t)x0 * r.bpp, (size_t)w * r.bpp);
    const size_t ysz = (size_t)W * H;
    if (r.chroma == 1) take(ysz, W, y0 / 2, h / 2, x0, w);
    if (r.chroma == 2) { take(ysz, W / 2, y0 / 2, h / 2, x0 / 2, w / 2); take(ysz + ysz / 4, W / 2, y0 / 2, h / 2, x0 / 2, w / 2); }
    return out;
}

static void test_views()
{
    const int W = 64, H = 48;
    const int rects[][4] = {{0, 0, 32, 24}, {0, 0, 64, 48}, {8, 6, 32, 24}, {9, 6, 32, 24}, {8, 7, 32, 24}, {8, 6, 31, 24}, {8, 6, 32, 23}, {32, 24, 32, 24}, {63, 47, 1, 1},
                            {-1, 0, 32, 24}, {0, -1, 32, 24}, {33, 24, 32, 24}, {32, 25, 32, 24}, {-2, 0, 32, 24}, {0, -2, 32, 24}, {34, 24, 32, 24}, {32, 26, 32, 24},
                            {8, 6, 0, 24}, {8, 6, 32, 0}, {8, 6, -1, 24}, {8, 6, 32, -2},
                            {2, 0, INT32_MAX, 24}, {INT32_MAX, 0, 2, 24}, {0, 2, 32, INT32_MAX}, {0, INT32_MAX - 1, 32, 2}, {INT32_MAX - 1, INT32_MAX - 1, 2, 2}};
    const int second[][4] = {{4, 2, 16, 12}, {0, 0, 32, 24}, {16, 12, 16, 12}, {3, 2, 16, 12}, {4, 1, 16, 12}, {18, 2, 16, 12}, {5, 3, 7, 5}};
    for (const Row& r : ROWS)
        for (int extra : {0, 1, 64}) {
            const zly_frame_view s = surface(r.fmt, W, H, extra);
            size_t need = 0;
            CHECK(view_valid(&s, &need) && need == view_bytes(&s) && need >= frame_bytes(r.fmt, W, H), "fmt %d + %d", r.fmt, extra);
            std::string e;
            CHECK(check_view(0, "", need, &s, &e) == ZLY_OK && e.empty(), "fmt %d + %d", r.fmt, extra);
            CHECK(check_view(0, "", need - 1, &s, &e) == ZLY_ERR_INVALID_INPUT &&
                  e == "Invalid image data size: the view needs " + std::to_string(need) + " bytes, got " + std::to_string(need - 1), "%s", e.c_str());
            CHECK(check_view(0, nullptr, need, &s, &e) == ZLY_ERR_INVALID_INPUT, "null base");
            // a buffer of distinct bytes (no two neighbours in a row or a column alike), and its tight copy
            std::vector<uint8_t> buf(need), whole(frame_bytes(r.fmt, W, H));
            for (size_t i = 0; i < need; ++i) buf[i] = (uint8_t)((i * 2654435761u) >> 13 ^ i);
            copy_view_tight(whole.data(), buf.data(), &s);
            for (const auto& q : rects) {
                const int x0 = q[0], y0 = q[1], w = q[2], h = q[3];
                const bool inside = x0 >= 0 && y0 >= 0 && w >= 1 && h >= 1 && (int64_t)x0 + w <= W && (int64_t)y0 + h <= H;
                const bool even = !(r.even_w && ((x0 | w) & 1)) && !(r.even_h && ((y0 | h) & 1));
                zly_frame_view c = untouched();
                e.clear();
                const int rc = view_crop(&s, x0, y0, w, h, &c, &e);
                if (!inside || !even) {
                    const char* text = !inside ? "zly_view_crop: the rectangle is not inside the surface" :
                                       r.even_h ? "zly_view_crop: a YUV 4:2:0 rectangle needs even x0, y0, w, h" : "zly_view_crop: a packed YUV 4:2:2 rectangle needs even x0 and w";
                    CHECK(rc == ZLY_ERR_INVALID_ARGUMENT && e == text && is_untouched(c), "fmt %d + %d (%d, %d, %d, %d): rc %d, %s", r.fmt, extra, x0, y0, w, h, rc, e.c_str());
                    continue;
                }
                size_t cneed = 0;
                CHECK(rc == ZLY_OK && e.empty() && c.fmt == r.fmt && c.w == w && c.h == h && !memcmp(c.pitch, s.pitch, sizeof c.pitch), "fmt %d + %d (%d, %d, %d, %d): rc %d", r.fmt, extra, x0, y0, w, h, rc);
                CHECK(view_valid(&c, &cneed) && cneed <= need, "fmt %d + %d (%d, %d, %d, %d): %zu of %zu", r.fmt, extra, x0, y0, w, h, cneed, need);
                // the crop's tight copy is the slice of the surface's
                std::vector<uint8_t> part(frame_bytes(r.fmt, w, h));
                copy_view_tight(part.data(), buf.data(), &c);
                CHECK(part == slice(r, whole, W, H, x0, y0, w, h), "fmt %d + %d (%d, %d, %d, %d)", r.fmt, extra, x0, y0, w, h);
                // crops compose, also in place
                for (const auto& q2 : second) {
                    if (q2[0] + q2[2] > w || q2[1] + q2[3] > h) continue;
                    zly_frame_view a = untouched(), b = untouched(), in_place = c;
                    std::string ea, eb;
                    const int ra = view_crop(&c, q2[0], q2[1], q2[2], q2[3], &a, &ea), rb = view_crop(&s, x0 + q2[0], y0 + q2[1], q2[2], q2[3], &b, &eb);
                    CHECK(ra == rb && ea == eb && (ra != ZLY_OK || same(a, b)), "fmt %d + %d (%d, %d, %d, %d) then (%d, %d, %d, %d): %d, %d", r.fmt, extra, x0, y0, w, h, q2[0], q2[1], q2[2], q2[3], ra, rb);
                    CHECK(view_crop(&in_place, q2[0], q2[1], q2[2], q2[3], &in_place, &ea) == ra && (ra == ZLY_OK ? same(in_place, a) : same(in_place, c)), "in place, fmt %d", r.fmt);
                }
            }
            // the limits of a view: a pitch below its row, a plane that reaches 2 GiB, an offset that wraps
            int64_t rows[3], rb[3];
            const int np = plane_shape(r.fmt, W, H, rows, rb);
            CHECK(np == r.planes, "fmt %d: %d planes", r.fmt, np);
            for (int p = 0; p < np; ++p) {
                const zly_frame_view t = surface(r.fmt, W, H, 0);
                zly_frame_view v = t, out = untouched();
                v.pitch[p] = (int32_t)rb[p] - 1;
                CHECK(!view_valid(&v, &need) && view_bytes(&v) == 0, "fmt %d plane %d: pitch below the row", r.fmt, p);
                CHECK(check_view(0, "", SIZE_MAX, &v, &e) == ZLY_ERR_INVALID_INPUT && e.find("invalid frame view (size 64 x 48: ") == 0, "%s", e.c_str());
                CHECK(view_crop(&v, 0, 0, 2, 2, &out, &e) == ZLY_ERR_INVALID_ARGUMENT && e == "zly_view_crop: invalid surface view" && is_untouched(out), "%s", e.c_str());
                const int64_t reach = ((1ll << 31) - rb[p] + rows[p] - 2) / (rows[p] - 1);       // the least pitch whose extent reaches 2^31
                v = t; v.pitch[p] = (int32_t)reach;
                CHECK(!view_valid(&v, &need), "fmt %d plane %d: extent 2^31", r.fmt, p);
                v.pitch[p] = (int32_t)reach - 1;
                CHECK(view_valid(&v, &need), "fmt %d plane %d: extent below 2^31", r.fmt, p);
                const uint64_t ext = (uint64_t)rows[p] * (uint64_t)rb[p];
                v = t; v.off[p] = UINT64_MAX - ext;
                CHECK(view_valid(&v, &need) && need == SIZE_MAX, "fmt %d plane %d: the last offset", r.fmt, p);
                v.off[p] = UINT64_MAX - ext + 1;
                CHECK(!view_valid(&v, &need), "fmt %d plane %d: a wrapping offset", r.fmt, p);
            }
        }
    for (int fmt : {-1, 5, 9, 14, 15, 19, 20, INT32_MAX}) {
        zly_frame_view v = surface(ZLY_PIX_BGR, W, H, 0), out = untouched();
        v.fmt = fmt;
        size_t need = 0;
        std::string e;
        CHECK(!view_valid(&v, &need) && view_bytes(&v) == 0, "fmt %d", fmt);
        CHECK(check_view(0, "", SIZE_MAX, &v, &e) == ZLY_ERR_INVALID_ARGUMENT && e == "unknown pixel format " + std::to_string(fmt), "%s", e.c_str());
        CHECK(view_crop(&v, 0, 0, 2, 2, &out, &e) == ZLY_ERR_INVALID_ARGUMENT && e == "zly_view_crop: invalid surface view" && is_untouched(out), "%s", e.c_str());
    }
    std::string e;
    size_t need = 0;
    CHECK(!view_valid(nullptr, &need) && view_bytes(nullptr) == 0 && check_view(0, "", 1, nullptr, &e) == ZLY_ERR_INVALID_ARGUMENT && e == "null view", "%s", e.c_str());
    // a view that passes is still bound by the engine's resize mode
    const zly_frame_view big = surface(ZLY_PIX_BGR, ZLY_LETTERBOX_MAX_DIM + 1, 2, 0);
    CHECK(check_view(ZLY_FLAG_LETTERBOX, "", SIZE_MAX, &big, &e) == ZLY_ERR_INVALID_INPUT && e.find("letterbox") == 0, "%s", e.c_str());
    CHECK(check_view(ZLY_FLAG_AREA, "", SIZE_MAX, &big, &e) == ZLY_ERR_INVALID_INPUT && e.find("area mode") == 0, "%s", e.c_str());
}

static void test_letterbox()
{
    const int req[][2] = {{1, 1}, {2, 1}, {416, 416}, {1920, 1080}, {1080, 1920}, {16384, 16384}, {INT32_MAX, INT32_MAX}, {INT32_MAX, 1}, {1, INT32_MAX}};
    const int model[][2] = {{416, 416}, {640, 384}, {1, 1}};
    for (const auto& q : req)
        for (const auto& m : model) {
            int32_t nw = -7, nh = -7, px = -7, py = -7;
            std::string e;
            CHECK(letterbox_geometry(q[0], q[1], m[0], m[1], &nw, &nh, &px, &py, &e) == ZLY_OK && e.empty(), "%d x %d", q[0], q[1]);
            // the content fills one axis, is at least one pixel on the other, and is centred (the odd pixel goes right / below)
            CHECK(nw >= 1 && nh >= 1 && nw <= m[0] && nh <= m[1] && (nw == m[0] || nh == m[1]) && px == (m[0] - nw) / 2 && py == (m[1] - nh) / 2,
                  "%d x %d into %d x %d: %d x %d at %d, %d", q[0], q[1], m[0], m[1], nw, nh, px, py);
        }
    const int bad[][4] = {{0, 1080, 416, 416}, {1920, 0, 416, 416}, {1920, 1080, 0, 416}, {1920, 1080, 416, 0}, {-1, 1080, 416, 416}, {1920, 1080, 416, -416}, {0, 0, 0, 0}};
    for (const auto& b : bad) {
        int32_t o[4] = {-7, -7, -7, -7};
        std::string e;
        CHECK(letterbox_geometry(b[0], b[1], b[2], b[3], &o[0], &o[1], &o[2], &o[3], &e) == ZLY_ERR_INVALID_ARGUMENT && e == "zly_letterbox_geometry: sizes must be positive" &&
              o[0] == -7 && o[1] == -7 && o[2] == -7 && o[3] == -7, "%d x %d into %d x %d", b[0], b[1], b[2], b[3]);
        CHECK(letterbox_geometry(b[0], b[1], b[2], b[3], nullptr, nullptr, nullptr, nullptr, &e) == ZLY_ERR_INVALID_ARGUMENT && e == "zly_letterbox_geometry: sizes must be positive", "%s", e.c_str());
    }
    for (int mask : {1, 2, 4, 8, 15}) {
        int32_t o[4] = {-7, -7, -7, -7};
        std::string e;
        CHECK(letterbox_geometry(1920, 1080, 416, 416, mask & 1 ? nullptr : &o[0], mask & 2 ? nullptr : &o[1], mask & 4 ? nullptr : &o[2], mask & 8 ? nullptr : &o[3], &e) ==
              ZLY_ERR_INVALID_ARGUMENT && e == "null output" && o[0] == -7 && o[1] == -7 && o[2] == -7 && o[3] == -7, "mask %d", mask);
    }
}

static void test_tiles()
{
    const char* refused = "zly_tile_grid: the surface must lie in 1..2^24-1, a tile be >= 1 and its overlap in [0, tile); even surfaces need even sizes";
    for (int extent : {1, 2, 415, 416, 417, 1920, (1 << 24) - 1, 1 << 24})
        for (int tile : {0, 1, 416, extent + 1})
            for (int overlap : {-1, 0, 32, tile - 1, tile})
                for (int even : {0, 1}) {
                    const bool ok = extent < (1 << 24) && tile >= 1 && overlap >= 0 && overlap < tile && !(even && ((extent | tile) & 1));
                    int64_t count = 0;
                    int32_t size = 0, step = 0, n = -7;
                    std::string e;
                    CHECK(grid_axis(extent, tile, overlap, even != 0, &count, &size, &step) == ok, "extent %d tile %d overlap %d even %d", extent, tile, overlap, even);
                    if (!ok) {
                        CHECK(tile_grid(extent, 416, tile, 416, overlap, 0, even, nullptr, 0, &n, &e) == ZLY_ERR_INVALID_ARGUMENT && e == refused && n == -7, "%s", e.c_str());
                        CHECK(tile_grid(416, extent, 416, tile, 0, overlap, even, nullptr, 0, &n, &e) == ZLY_ERR_INVALID_ARGUMENT && e == refused && n == -7, "%s", e.c_str());
                        continue;
                    }
                    // the tiles of an axis are of one size, start inside, reach the end, and no step is wider than a tile less its overlap
                    CHECK(size == std::min(tile, extent) && step == tile - overlap && count >= 1 && (count - 1) * (int64_t)step + size >= extent &&
                          (count == 1 || (count - 2) * (int64_t)step + size < extent), "extent %d tile %d overlap %d: %lld x %d", extent, tile, overlap, (long long)count, size);
                    CHECK(tile_grid(extent, 416, tile, 416, overlap, 0, even, nullptr, 0, &n, &e) == ZLY_OK && n == count && e.empty(), "cap 0: %d", n);
                    const int32_t full = count < 4096 ? (int32_t)count : 0;
                    for (int32_t cap : {(int32_t)std::min<int64_t>(3, count - 1), full}) {
                        std::vector<zly_tile> t((size_t)cap + 1);
                        memset(t.data(), 0xA5, t.size() * sizeof(zly_tile));
                        const zly_tile guard = t[(size_t)cap];
                        n = -7;
                        CHECK(tile_grid(extent, 416, tile, 416, overlap, 0, even, t.data(), cap, &n, &e) == ZLY_OK && n == count, "cap %d: %d", cap, n);
                        CHECK(!memcmp(&t[(size_t)cap], &guard, sizeof guard), "cap %d: written behind the array", cap);
                        bool good = true;
                        for (int32_t k = 0; k < cap; ++k) {
                            const zly_tile& q = t[(size_t)k];
                            const int64_t x = std::min<int64_t>((int64_t)k * step, extent - size) & ~(int64_t)(even ? 1 : 0);
                            good = good && q.group == 0 && q.x0 == x && q.y0 == 0 && q.w == size && q.h == 416 && q.W == extent && q.H == 416 && q.x0 >= 0 && q.x0 + q.w <= extent;
                        }
                        CHECK(good, "extent %d tile %d overlap %d even %d cap %d", extent, tile, overlap, even, cap);
                        if (cap == count && cap > 0) CHECK(t[(size_t)cap - 1].x0 + size == extent, "the last tile ends at the edge");
                    }
                }
    for (int even : {0, 1}) {
        int32_t n = -7;
        std::string e;
        CHECK(tile_grid((1 << 24) - 1 - even, (1 << 24) - 1 - even, 1 + even, 1 + even, 0, 0, even, nullptr, 0, &n, &e) == ZLY_ERR_INVALID_ARGUMENT && e == "zly_tile_grid: too many tiles" && n == -7, "%s", e.c_str());
        e.clear();
        CHECK(tile_grid((1 << 24) - 2, (1 << 24) - 2, 512, 512, 0, 0, even, nullptr, 0, &n, &e) == ZLY_OK && n == 1 << 30 && e.empty(), "%d", n);
        // both axes: row-major, every tile inside, the grid covers the surface
        std::vector<zly_tile> t(64);
        CHECK(tile_grid(1920, 1080, 416, 416, 32, 32, even, t.data(), 64, &n, &e) == ZLY_OK && n == 15, "%d", n);
        bool good = n == 15;
        for (int k = 0; good && k < n; ++k)
            good = t[k].w == 416 && t[k].h == 416 && t[k].x0 == std::min(k % 5 * 384, 1920 - 416) && t[k].y0 == std::min(k / 5 * 384, 1080 - 416) && t[k].W == 1920 && t[k].H == 1080;
        CHECK(good, "1920 x 1080 in tiles of 416 with overlap 32");
    }
}

int main()
{
    test_table();
    test_frames();
    test_views();
    test_letterbox();
    test_tiles();
    printf("%d checks, %d failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
