// frame_rules.h -- the host-side rules of a request frame: what a frame of format fmt and size w x h is (planes, bytes per row, which sizes must be
// even, which front-kernel level it asks for), what makes a frame view valid, and the request checks built on them.  Nothing here touches a device or
// the engine: plain C++ (include/zly.h, front_variants.h for the ZLY_FRONT_* levels, the standard library), so that engine.cpp, the stubs of the C ABI
// under tests/cpp/ and a stand-alone test program (tests/cpp/test_frame_rules.cpp) all compile the same text.
//
// A refusal hands back its ZLY_ERR_* code and, through `err`, its message; a call that succeeds leaves *err alone.  engine.cpp passes its
// zly_last_error slot.  The kernels keep predicates of their own on the device side (yuv_device.h, planes_device.h).
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include <algorithm>
#include <string>
#include "zly.h"
#include "front_variants.h"

namespace zly {

// ---- the format table: one row per ZLY_PIX_* value.  The known formats are a set, not a range (include/zly.h): 5..9, 14, 15 and 17 up are unknown.
//      Adding a format: DESIGN.md, "Adding a pixel format".
enum Chroma { CHROMA_NONE, CHROMA_NV12, CHROMA_I420 };    // no chroma planes / one plane of interleaved U,V pairs / a U plane and a V plane; both 2 x 2 subsampled
struct PixFormat {
    int32_t  fmt;               // ZLY_PIX_*
    int      planes;
    uint32_t bpp;               // bytes per pixel of plane 0 (packed 4:2:2: 2, in macropixels of two)
    Chroma   chroma;
    bool     even_w, even_h;    // must the width / the height (and a rectangle's x0 / y0) be even?
    int      front;             // ZLY_FRONT_*: the format level a frame of this format asks of the front kernels
};

inline const PixFormat* pix_format(int32_t fmt)
{
    static const PixFormat table[] = {
        {ZLY_PIX_BGR,        1, 3, CHROMA_NONE, false, false, ZLY_FRONT_BGR},
        {ZLY_PIX_NV12_BT601, 2, 1, CHROMA_NV12, true,  true,  ZLY_FRONT_YUV},
        {ZLY_PIX_I420_BT601, 3, 1, CHROMA_I420, true,  true,  ZLY_FRONT_YUV},
        {ZLY_PIX_NV12_BT709, 2, 1, CHROMA_NV12, true,  true,  ZLY_FRONT_YUV},
        {ZLY_PIX_I420_BT709, 3, 1, CHROMA_I420, true,  true,  ZLY_FRONT_YUV},
        {ZLY_PIX_YUY2_BT601, 1, 2, CHROMA_NONE, true,  false, ZLY_FRONT_YUV422},
        {ZLY_PIX_UYVY_BT601, 1, 2, CHROMA_NONE, true,  false, ZLY_FRONT_YUV422},
        {ZLY_PIX_YUY2_BT709, 1, 2, CHROMA_NONE, true,  false, ZLY_FRONT_YUV422},
        {ZLY_PIX_UYVY_BT709, 1, 2, CHROMA_NONE, true,  false, ZLY_FRONT_YUV422},
        {ZLY_PIX_RGB,        1, 3, CHROMA_NONE, false, false, ZLY_FRONT_PACKED},
        {ZLY_PIX_BGRA,       1, 4, CHROMA_NONE, false, false, ZLY_FRONT_PACKED},
        {ZLY_PIX_RGBA,       1, 4, CHROMA_NONE, false, false, ZLY_FRONT_PACKED},
    };
    for (const PixFormat& f : table) if (f.fmt == fmt) return &f;
    return nullptr;
}

// callers ask after the request checks, so of known formats only; an unknown one gets the level that serves every format
inline int front_level(int32_t fmt) { const PixFormat* f = pix_format(fmt); return f ? f->front : ZLY_FRONT_PACKED; }

inline int refuse(std::string* err, int code, const std::string& msg) { if (err) *err = msg; return code; }

// ---- frames ----
// planes of a w x h frame of format fmt: rows and bytes per row of each; 0 for an unknown format or invalid dimensions (YUV 4:2:0: one chroma sample
// per 2 x 2 block; packed 4:2:2: whole macropixels of two pixels, any height)
inline int plane_shape(int32_t fmt, int32_t w, int32_t h, int64_t rows[3], int64_t row_bytes[3])
{
    const PixFormat* f = pix_format(fmt);
    if (!f || w < 1 || h < 1) return 0;
    if ((f->even_w && (w & 1)) || (f->even_h && (h & 1))) return 0;
    rows[0] = h; row_bytes[0] = (int64_t)f->bpp * (int64_t)w;
    if (f->chroma == CHROMA_NV12) { rows[1] = h / 2; row_bytes[1] = w; }      // 2 * (w/2)
    if (f->chroma == CHROMA_I420) { rows[1] = rows[2] = h / 2; row_bytes[1] = row_bytes[2] = w / 2; }
    return f->planes;
}

// zly_frame_bytes
inline size_t frame_bytes(int32_t fmt, int32_t w, int32_t h)
{
    int64_t rows[3], rb[3];
    if (!plane_shape(fmt, w, h, rows, rb)) return 0;
    const PixFormat* f = pix_format(fmt);
    return f->chroma == CHROMA_NONE ? (size_t)w * (size_t)h * f->bpp : (size_t)w * (size_t)h * 3u / 2u;
}

// ---- frame views (include/zly.h zly_frame_view) ----
// include/zly.h's validity rule; *need = the smallest buffer that holds the view
inline bool view_valid(const zly_frame_view* v, size_t* need)
{
    int64_t rows[3], rb[3];
    const int np = v ? plane_shape(v->fmt, v->w, v->h, rows, rb) : 0;
    if (!np) return false;
    uint64_t most = 0;
    for (int p = 0; p < np; ++p) {
        if ((int64_t)v->pitch[p] < rb[p]) return false;
        const uint64_t ext = (uint64_t)(rows[p] - 1) * (uint64_t)v->pitch[p] + (uint64_t)rb[p];
        if (ext >= (1ull << 31)) return false;
        if (v->off[p] > UINT64_MAX - ext) return false;
        most = std::max<uint64_t>(most, v->off[p] + ext);
    }
    if (most > (uint64_t)SIZE_MAX) return false;
    *need = (size_t)most;
    return true;
}

// zly_view_bytes
inline size_t view_bytes(const zly_frame_view* v)
{
    size_t need = 0;
    return view_valid(v, &need) ? need : 0;
}

// zly_view_tight
inline int32_t view_tight(int32_t fmt, int32_t w, int32_t h, zly_frame_view* out, std::string* err)
{
    int64_t rows[3], rb[3];
    const int np = plane_shape(fmt, w, h, rows, rb);
    if (!np) return refuse(err, ZLY_ERR_INVALID_ARGUMENT, "zly_view_tight: unknown format or invalid size");
    zly_frame_view v{};
    v.fmt = fmt; v.w = w; v.h = h;
    uint64_t off = 0;
    for (int p = 0; p < np; ++p) {                       // the planes follow each other without padding, rows without pitch
        v.off[p] = off; v.pitch[p] = (int32_t)rb[p];
        off += (uint64_t)rows[p] * (uint64_t)rb[p];
    }
    *out = v;
    return ZLY_OK;
}

// zly_view_crop
inline int32_t view_crop(const zly_frame_view* surface, int32_t x0, int32_t y0, int32_t w, int32_t h, zly_frame_view* out, std::string* err)
{
    size_t need = 0;
    if (!view_valid(surface, &need)) return refuse(err, ZLY_ERR_INVALID_ARGUMENT, "zly_view_crop: invalid surface view");
    if (x0 < 0 || y0 < 0 || w < 1 || h < 1 || (int64_t)x0 + w > surface->w || (int64_t)y0 + h > surface->h)
        return refuse(err, ZLY_ERR_INVALID_ARGUMENT, "zly_view_crop: the rectangle is not inside the surface");
    zly_frame_view v = *surface;                         // (out may be the surface itself: crops compose)
    v.w = w; v.h = h;
    const PixFormat* f = pix_format(v.fmt);
    if ((f->even_w && ((x0 | w) & 1)) || (f->even_h && ((y0 | h) & 1)))
        return refuse(err, ZLY_ERR_INVALID_ARGUMENT, f->even_h ? "zly_view_crop: a YUV 4:2:0 rectangle needs even x0, y0, w, h" :
                                                                 "zly_view_crop: a packed YUV 4:2:2 rectangle needs even x0 and w");
    v.off[0] += (uint64_t)y0 * (uint64_t)v.pitch[0] + (uint64_t)x0 * f->bpp;
    if (f->chroma == CHROMA_NV12) v.off[1] += (uint64_t)(y0 / 2) * (uint64_t)v.pitch[1] + (uint64_t)(x0 / 2) * 2u;
    if (f->chroma == CHROMA_I420) {
        v.off[1] += (uint64_t)(y0 / 2) * (uint64_t)v.pitch[1] + (uint64_t)(x0 / 2);
        v.off[2] += (uint64_t)(y0 / 2) * (uint64_t)v.pitch[2] + (uint64_t)(x0 / 2);
    }
    *out = v;
    return ZLY_OK;
}

// the region's rows, plane by plane, as the tight frame of frame_bytes(fmt, w, h) at dst: the one host copy of a view request
inline void copy_view_tight(uint8_t* dst, const uint8_t* base, const zly_frame_view* v)
{
    int64_t rows[3], rb[3];
    const int np = plane_shape(v->fmt, v->w, v->h, rows, rb);
    for (int p = 0; p < np; ++p) {
        const uint8_t* q = base + v->off[p];
        if ((int64_t)v->pitch[p] == rb[p]) { memcpy(dst, q, (size_t)(rows[p] * rb[p])); dst += rows[p] * rb[p]; continue; }
        for (int64_t r = 0; r < rows[p]; ++r, q += v->pitch[p], dst += rb[p]) memcpy(dst, q, (size_t)rb[p]);
    }
}

// ---- the request checks ----
// of every entry point that takes host frames (onnx_engine.cpp:659-665): an unknown format is an argument error; a byte count that is not
// frame_bytes(fmt, w, h) -- odd or too small YUV sizes included -- is ZLY_ERR_INVALID_INPUT
inline int check_frame(int32_t fmt, const uint8_t* p, size_t nbytes, int32_t w, int32_t h, std::string* err)
{
    const PixFormat* f = pix_format(fmt);
    if (!f) return refuse(err, ZLY_ERR_INVALID_ARGUMENT, "unknown pixel format " + std::to_string(fmt));
    const size_t want = frame_bytes(fmt, w, h);
    if (!p || want == 0 || nbytes != want) {
        const bool yuv420 = f->chroma != CHROMA_NONE, yuv422 = !yuv420 && f->even_w;
        const size_t shown = want ? want : (size_t)(w > 0 ? w : 0) * (size_t)(h > 0 ? h : 0) * (yuv420 ? 3u : 2u * f->bpp) / 2u;
        return refuse(err, ZLY_ERR_INVALID_INPUT, "Invalid image data size: expected " + std::to_string(shown) + ", got " + std::to_string(nbytes) +
                                                  (yuv420 && (w < 2 || h < 2 || (w | h) & 1) ? " (YUV 4:2:0 needs even width and height >= 2)" :
                                                   yuv422 && (w < 2 || (w & 1)) ? " (packed YUV 4:2:2 needs even width >= 2)" : ""));
    }
    return ZLY_OK;
}

// flags: the engine's zly_config.flags.  A letterbox engine's fixed-point resize fits int32 for requests of up to ZLY_LETTERBOX_MAX_DIM pixels on a
// side (include/zly.h)
inline int check_frame_mode(int32_t flags, int32_t w, int32_t h, std::string* err)
{
    if ((flags & ZLY_FLAG_LETTERBOX) && (w > ZLY_LETTERBOX_MAX_DIM || h > ZLY_LETTERBOX_MAX_DIM))
        return refuse(err, ZLY_ERR_INVALID_INPUT, "letterbox mode takes frames of at most " + std::to_string(ZLY_LETTERBOX_MAX_DIM) + " pixels on a side, got " +
                                                  std::to_string(w) + " x " + std::to_string(h));
    // so does an area engine's exact average (the products of the footprint arithmetic stay below 2^28)
    if ((flags & ZLY_FLAG_AREA) && (w > ZLY_AREA_MAX_DIM || h > ZLY_AREA_MAX_DIM))
        return refuse(err, ZLY_ERR_INVALID_INPUT, "area mode takes frames of at most " + std::to_string(ZLY_AREA_MAX_DIM) + " pixels on a side, got " +
                                                  std::to_string(w) + " x " + std::to_string(h));
    return ZLY_OK;
}

// of every entry point that takes a view: an unknown format is an argument error; an otherwise invalid view, or one that does not fit the caller's
// buffer, is ZLY_ERR_INVALID_INPUT (as a wrong byte count is); letterbox and area engines bound the view's size
inline int check_view(int32_t flags, const void* base, size_t buf_bytes, const zly_frame_view* v, std::string* err)
{
    if (!v) return refuse(err, ZLY_ERR_INVALID_ARGUMENT, "null view");
    if (!pix_format(v->fmt)) return refuse(err, ZLY_ERR_INVALID_ARGUMENT, "unknown pixel format " + std::to_string(v->fmt));
    size_t need = 0;
    if (!view_valid(v, &need)) return refuse(err, ZLY_ERR_INVALID_INPUT, "invalid frame view (size " + std::to_string(v->w) + " x " + std::to_string(v->h) +
                                                                         ": YUV 4:2:0 needs even width and height >= 2, packed 4:2:2 even width >= 2, every pitch at least its row's bytes, every plane below 2 GiB)");
    if (!base || need > buf_bytes) return refuse(err, ZLY_ERR_INVALID_INPUT, "Invalid image data size: the view needs " + std::to_string(need) + " bytes, got " + std::to_string(buf_bytes));
    return check_frame_mode(flags, v->w, v->h, err);
}

// ---- zly_letterbox_geometry ----
inline int32_t letterbox_geometry(int32_t w, int32_t h, int32_t model_w, int32_t model_h, int32_t* nw, int32_t* nh, int32_t* pad_x, int32_t* pad_y, std::string* err)
{
    if (w < 1 || h < 1 || model_w < 1 || model_h < 1) return refuse(err, ZLY_ERR_INVALID_ARGUMENT, "zly_letterbox_geometry: sizes must be positive");
    if (!nw || !nh || !pad_x || !pad_y) return refuse(err, ZLY_ERR_INVALID_ARGUMENT, "null output");
    const int64_t W = w, H = h, TW = model_w, TH = model_h;
    int64_t cw, ch;
    if (TW * H <= TH * W) { cw = TW; ch = std::max<int64_t>(1, (2 * H * TW + W) / (2 * W)); }      // the width binds
    else                  { ch = TH; cw = std::max<int64_t>(1, (2 * W * TH + H) / (2 * H)); }
    *nw = (int32_t)cw; *nh = (int32_t)ch;
    *pad_x = (int32_t)((TW - cw) >> 1); *pad_y = (int32_t)((TH - ch) >> 1);
    return ZLY_OK;
}

// ---- zly_tile_grid ----
// one axis: the number of tiles and their size; false when the arguments are refused
inline bool grid_axis(int32_t extent, int32_t tile, int32_t overlap, bool even, int64_t* count, int32_t* size, int32_t* step)
{
    if (extent < 1 || extent >= (1 << 24) || tile < 1 || overlap < 0 || overlap >= tile) return false;
    if (even && ((extent | tile) & 1)) return false;
    *step = tile - overlap;
    if (tile >= extent) { *count = 1; *size = extent; return true; }
    *size = tile;
    *count = ((int64_t)(extent - tile) + *step - 1) / *step + 1;
    return true;
}

// the grid: the first min(cap, count) tiles at out (cap >= 0; out may be null when cap is 0), the count at *n_out
inline int32_t tile_grid(int32_t W, int32_t H, int32_t tile_w, int32_t tile_h, int32_t overlap_x, int32_t overlap_y, int32_t even, zly_tile* out,
                         int32_t cap, int32_t* n_out, std::string* err)
{
    int64_t nx = 0, ny = 0;
    int32_t tw = 0, th = 0, sx = 0, sy = 0;
    if (!grid_axis(W, tile_w, overlap_x, even != 0, &nx, &tw, &sx) || !grid_axis(H, tile_h, overlap_y, even != 0, &ny, &th, &sy))
        return refuse(err, ZLY_ERR_INVALID_ARGUMENT, "zly_tile_grid: the surface must lie in 1..2^24-1, a tile be >= 1 and its overlap in [0, tile); even surfaces need even sizes");
    if (nx * ny > 0x7fffffff) return refuse(err, ZLY_ERR_INVALID_ARGUMENT, "zly_tile_grid: too many tiles");
    int64_t k = 0;
    for (int64_t j = 0; j < ny && k < cap; ++j)
        for (int64_t i = 0; i < nx && k < cap; ++i, ++k) {
            int64_t x0 = std::min<int64_t>(i * sx, W - tw), y0 = std::min<int64_t>(j * sy, H - th);
            if (even) { x0 &= ~(int64_t)1; y0 &= ~(int64_t)1; }
            zly_tile t;
            t.group = 0; t.x0 = (int32_t)x0; t.y0 = (int32_t)y0; t.w = tw; t.h = th; t.W = W; t.H = H;
            out[k] = t;
        }
    *n_out = (int32_t)(nx * ny);
    return ZLY_OK;
}

}  // namespace zly
