// kernels_view.hip -- the VIEW unit of front_variants.h: the front kernels' instantiations for calls on frame views (include/zly.h zly_frame_view)
// of BGR and YUV 4:2:0 frames, stretch and letterbox.  The Detect tail does not change (FrameDesc::w, h hold the view's size).
#define ZLY_FRONT_TU ZLY_TU_VIEW
#include "kernels_misc.hip"
#include "kernels_stem.hip"
