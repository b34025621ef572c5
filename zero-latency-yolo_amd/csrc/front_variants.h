// front_variants.h -- THE list of the front kernels' input variants, and which object each one is compiled in.
//
// The front kernels (preprocess_kernel in kernels_misc.hip; stem_fused_kernel and stem_model1_kernel in kernels_stem.hip) are templates over four flags:
//   YUV   the instantiation for batches with a frame that is not plain BGR: a YUV 4:2:0 frame's pixel becomes the B, G, R bytes of its integer
//         conversion (yuv_device.h) and then takes the BGR path.  It serves the batch's BGR frames as well.
//   LB    the instantiation of a letterbox engine (ZLY_FLAG_LETTERBOX, letterbox_device.h): padding test + four-tap bilinear blend in place of the
//         nearest-neighbour pick.
//   VIEW  the instantiation for calls whose frames are frame views (zly_frame_view: pitched surfaces, regions of interest): every fetch takes its
//         row pitch and plane bases from the frame's ViewRec (planes_device.h).  Always YUV-capable: it serves BGR views too.
//   PK    with YUV: the instantiation that serves every format, packed RGB / BGRA / RGBA included (the BGR fetch with the frame's pixel size,
//         bytes 0 and 2 exchanged for the R-first layouts).
//   Y2    with YUV and PK: the instantiation that serves packed YUV 4:2:2 (YUY2 / UYVY) as well: one 4-byte macropixel load per pixel, Y, U, V picked by
//         one permute, then the YUV path's conversion.  Y2 is NOT a fifth flag of the kernels -- one more parameter would rename every kernel that
//         exists.  The stem kernels carry it as ZLY_FRONT_Y2_TAG on an int parameter they have (stem_fused_kernel's NT, stem_model1_kernel's VAR): an
//         existing instantiation keeps its name, text and code.  (With their text moved behind a device template and entry kernels in front of it
//         -- what preprocess_kernel, which has no int parameter, does: preprocess_body, preprocess_y422_kernel<T, LB, VIEW> -- the stem kernels'
//         existing instantiations came out with another schedule and register allocation: tools/isa_diff.py.)
// A launch does not name flags but a FrontVariant -- the batch's format level, the engine's resize mode, tight frames or views -- and YUV, PK and Y2
// follow from the level.  The fourteen rows of ZLY_FRONT_VARIANTS exist; a launch of any other combination is an error.
//
// Why several objects: instantiated next to each other, the variants of one kernel changed each other's register allocation (same resources,
// different code), and every kernel that existed before a variant was added is to compile to exactly the code it compiled to.  So the variants are
// compiled in groups, one translation unit per group: kernels_misc.hip / kernels_stem.hip as the main units, and kernels_stem_yuv.hip, kernels_lb.hip,
// kernels_view.hip, kernels_pix.hip, kernels_pix_view.hip, kernels_y422.hip, kernels_y422_view.hip, which define ZLY_FRONT_TU and include the main units' text.  A unit instantiates the
// variants the table gives it, per kernel family (preprocess_kernel's YUV variant lives in kernels_misc.o, the stem kernels' in kernels_stem_yuv.o),
// and exports one getter per family; the main units hold the launchers, whose pickers ask the owning unit's getter.  kernels_lb.hip also holds the
// Detect tail's letterbox instantiations (kernels_head.hip).  tools/isa_diff.py checks that a change left every kernel of every object as it was.
#pragma once

// ---- which translation unit is being compiled --------------------------------------------------------------------------------------------------
#define ZLY_TU_ALL      0      // one-unit diagnostic builds (tools/stem_bench.hip, tools/head_bench.hip): this unit owns every variant
#define ZLY_TU_MAIN     1      // kernels_misc.hip, kernels_stem.hip, kernels_head.hip compiled as themselves: launchers, pickers, tables
#define ZLY_TU_YUV      2      // kernels_stem_yuv.hip
#define ZLY_TU_LB       3      // kernels_lb.hip
#define ZLY_TU_VIEW     4      // kernels_view.hip
#define ZLY_TU_PIX      5      // kernels_pix.hip
#define ZLY_TU_PIX_VIEW 6      // kernels_pix_view.hip
#define ZLY_TU_Y422     7      // kernels_y422.hip
#define ZLY_TU_Y422_VIEW 8     // kernels_y422_view.hip
#ifndef ZLY_FRONT_TU
#if defined(ZLY_STEM_DIAG) || defined(ZLY_HEAD_DIAG)
#define ZLY_FRONT_TU ZLY_TU_ALL
#else
#define ZLY_FRONT_TU ZLY_TU_MAIN
#endif
#endif
#define ZLY_FRONT_OWNS(tu)  (ZLY_FRONT_TU == ZLY_TU_ALL || ZLY_FRONT_TU == (tu))      // does this unit compile what the table gives unit tu?
#define ZLY_FRONT_LAUNCHERS ZLY_FRONT_OWNS(ZLY_TU_MAIN)      // this unit holds the launchers and everything that is not a front-kernel instantiation

// ---- the variants ----------------------------------------------------------------------------------------------------------------------------
// The format level of a batch: the highest of its frames'.  A level serves the levels below it as well.
#define ZLY_FRONT_BGR    0      // plain BGR frames only: the headline kernels (YUV = PK = false)
#define ZLY_FRONT_YUV    1      // at least one YUV 4:2:0 frame, no packed RGB / BGRA / RGBA frame (YUV = true)
#define ZLY_FRONT_PACKED 2      // at least one packed RGB / BGRA / RGBA frame, no packed 4:2:2 frame (YUV = PK = true)
#define ZLY_FRONT_YUV422 3      // at least one packed YUV 4:2:2 frame (YUY2 / UYVY) (YUV = PK = Y2 = true)

// X(level, lb, view, unit that owns preprocess_kernel's instantiations, unit that owns stem_fused_kernel's and stem_model1_kernel's)
#define ZLY_FRONT_VARIANTS(X) \
    X(ZLY_FRONT_BGR,    false, false, ZLY_TU_MAIN,     ZLY_TU_MAIN)     \
    X(ZLY_FRONT_YUV,    false, false, ZLY_TU_MAIN,     ZLY_TU_YUV)      \
    X(ZLY_FRONT_BGR,    true,  false, ZLY_TU_LB,       ZLY_TU_LB)       \
    X(ZLY_FRONT_YUV,    true,  false, ZLY_TU_LB,       ZLY_TU_LB)       \
    X(ZLY_FRONT_YUV,    false, true,  ZLY_TU_VIEW,     ZLY_TU_VIEW)     \
    X(ZLY_FRONT_YUV,    true,  true,  ZLY_TU_VIEW,     ZLY_TU_VIEW)     \
    X(ZLY_FRONT_PACKED, false, false, ZLY_TU_PIX,      ZLY_TU_PIX)      \
    X(ZLY_FRONT_PACKED, true,  false, ZLY_TU_PIX,      ZLY_TU_PIX)      \
    X(ZLY_FRONT_PACKED, false, true,  ZLY_TU_PIX_VIEW, ZLY_TU_PIX_VIEW) \
    X(ZLY_FRONT_PACKED, true,  true,  ZLY_TU_PIX_VIEW, ZLY_TU_PIX_VIEW) \
    X(ZLY_FRONT_YUV422, false, false, ZLY_TU_Y422,     ZLY_TU_Y422)     \
    X(ZLY_FRONT_YUV422, true,  false, ZLY_TU_Y422,     ZLY_TU_Y422)     \
    X(ZLY_FRONT_YUV422, false, true,  ZLY_TU_Y422_VIEW, ZLY_TU_Y422_VIEW) \
    X(ZLY_FRONT_YUV422, true,  true,  ZLY_TU_Y422_VIEW, ZLY_TU_Y422_VIEW)
// the kernels' <YUV, LB, VIEW, PK> of a row, and the tag its level adds to the stem kernels' int parameter
#define ZLY_FRONT_FLAGS(level, lb, view) ((level) >= ZLY_FRONT_YUV), lb, view, ((level) >= ZLY_FRONT_PACKED)
#define ZLY_FRONT_Y2_TAG 16
#define ZLY_FRONT_Y2(level) ((level) >= ZLY_FRONT_YUV422 ? ZLY_FRONT_Y2_TAG : 0)

namespace zly {

// What a front-kernel launch is for.  The constructor is the one place that knows the rules: a view is served by at least the YUV level (there is
// no BGR-only VIEW instantiation); that a packed level is YUV-capable is ZLY_FRONT_FLAGS.
struct FrontVariant {
    int level;                  // ZLY_FRONT_*
    bool lb, view;
    constexpr FrontVariant(int level_ = ZLY_FRONT_BGR, bool lb_ = false, bool view_ = false)
        : level(view_ && level_ < ZLY_FRONT_YUV ? ZLY_FRONT_YUV : level_), lb(lb_), view(view_) {}
    constexpr bool operator==(const FrontVariant& o) const { return level == o.level && lb == o.lb && view == o.view; }
};

#define ZLY_FRONT_ROW(level, lb, view, pre_tu, stem_tu) FrontVariant(level, lb, view),
static constexpr FrontVariant FRONT_VARIANTS[] = { ZLY_FRONT_VARIANTS(ZLY_FRONT_ROW) };
#undef ZLY_FRONT_ROW

// The unit whose getter serves a row owned by `tu`: that unit, or this one when it owns everything.
constexpr int front_owner(int tu) { return ZLY_FRONT_OWNS(tu) ? ZLY_FRONT_TU : tu; }

}  // namespace zly
