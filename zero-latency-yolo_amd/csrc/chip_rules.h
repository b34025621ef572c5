// chip_rules.h -- the host side of the chips (include/zly.h "Chips"): the config and call checks, and the record the kernels are given of a frame
// (from the frame's checked view and the format table of frame_rules.h).  Nothing here touches a device or the engine, as frame_rules.h does not:
// engine.cpp and a stand-alone test program (tests/cpp/test_chip_rules.cpp) compile the same text.
#pragma once
#include "frame_rules.h"
#include "chip_device.h"

namespace zly {

static_assert(sizeof(zly_chip_header) == ZLY_CHIP_HDR_BYTES && sizeof(zly_chip_rec) == ZLY_CHIP_REC_BYTES, "chip_device.h's offsets are include/zly.h's records");
static_assert(sizeof(ChipFrame) == 88, "the frame record is uploaded as an array");

inline void chip_default_config(int32_t max_dets, zly_chip_config* c)
{
    c->chip_w = 64; c->chip_h = 64;              // chosen, not tuned
    c->max_chips = max_dets < 16 ? max_dets : 16;
    c->class_id = -1;
    c->scale = 1.25f;                            // chosen, not tuned
    c->layout = ZLY_CHIP_BGR8;
}

inline int chip_check_config(const zly_chip_config* c, int32_t max_dets, std::string* err)
{
    if (!c) return refuse(err, ZLY_ERR_INVALID_ARGUMENT, "null chip config");
    if (c->chip_w < 1 || c->chip_h < 1 || c->chip_w > ZLY_CHIP_MAX_DIM || c->chip_h > ZLY_CHIP_MAX_DIM)
        return refuse(err, ZLY_ERR_INVALID_ARGUMENT, "a chip's width and height must lie in 1..256");
    if (c->max_chips < 1 || c->max_chips > max_dets) return refuse(err, ZLY_ERR_INVALID_ARGUMENT, "max_chips must lie in 1..max_dets (" + std::to_string(max_dets) + ")");
    if (c->class_id < -1) return refuse(err, ZLY_ERR_INVALID_ARGUMENT, "class_id must be -1 or a class");
    if (!(c->scale >= 1.0f && c->scale <= 4.0f)) return refuse(err, ZLY_ERR_INVALID_ARGUMENT, "scale must be finite and lie in [1, 4]");      // a NaN fails both
    if (c->layout != ZLY_CHIP_BGR8 && c->layout != ZLY_CHIP_RGB_F32) return refuse(err, ZLY_ERR_INVALID_ARGUMENT, "unknown chip layout " + std::to_string(c->layout));
    return ZLY_OK;
}

// the arguments of a call that need no engine state: n, the source, the view array
inline int chip_check_call(int32_t n, int32_t max_batch, const void* frames, const void* d_slabs, int32_t source, std::string* err)
{
    if (n < 1 || n > max_batch) return refuse(err, ZLY_ERR_INVALID_ARGUMENT, "batch size out of range");
    if (!frames) return refuse(err, ZLY_ERR_INVALID_ARGUMENT, "null views");
    if (source != ZLY_CHIPS_SRC_SLABS && source != ZLY_CHIPS_SRC_MERGED) return refuse(err, ZLY_ERR_INVALID_ARGUMENT, "unknown chip source " + std::to_string(source));
    if (d_slabs && source != ZLY_CHIPS_SRC_SLABS) return refuse(err, ZLY_ERR_INVALID_ARGUMENT, "source must be 0 when d_slabs names the slabs");
    return ZLY_OK;
}

// a frame's view: what zly_detect_device_view refuses (flags: the engine's), and the filter's size limit
inline int chip_check_view(int32_t flags, const void* base, size_t buf_bytes, const zly_frame_view* v, std::string* err)
{
    if (int rc = check_view(flags, base, buf_bytes, v, err)) return rc;
    if (v->w > ZLY_AREA_MAX_DIM || v->h > ZLY_AREA_MAX_DIM)
        return refuse(err, ZLY_ERR_INVALID_INPUT, "chips are cut from frames of at most " + std::to_string(ZLY_AREA_MAX_DIM) + " pixels on a side, got " +
                                                  std::to_string(v->w) + " x " + std::to_string(v->h));
    return ZLY_OK;
}

// the kernels' record of a frame on the (valid) view v
inline ChipFrame chip_frame_of(const zly_frame_view* v)
{
    const PixFormat* f = pix_format(v->fmt);
    int64_t rows[3], rb[3];
    const int np = plane_shape(v->fmt, v->w, v->h, rows, rb);
    ChipFrame c{};
    c.W = v->w; c.H = v->h; c.fmt = v->fmt; c.planes = np; c.bpp = (int32_t)f->bpp;
    c.fam = f->chroma == CHROMA_NV12 ? ZLY_CHIP_FAM_NV12 : f->chroma == CHROMA_I420 ? ZLY_CHIP_FAM_I420 : f->even_w ? ZLY_CHIP_FAM_Y422 : ZLY_CHIP_FAM_PACKED;
    for (int p = 0; p < np; ++p) {
        c.off[p] = v->off[p]; c.pitch[p] = v->pitch[p];
        c.ext[p] = (uint64_t)(rows[p] - 1) * (uint64_t)v->pitch[p] + (uint64_t)rb[p];
    }
    return c;
}

}  // namespace zly
