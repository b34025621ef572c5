// kernels_view.hip -- the VIEW = true instantiations of the front kernels (preprocess_kernel, stem_fused_kernel, stem_model1_kernel; stretch and
// letterbox forms) for calls whose frames are frame views (include/zly.h zly_frame_view: pitched surfaces and regions of interest), in a translation
// unit of their own so that the instantiations every other call launches compile exactly as before (see kernels_stem.hip).  They are YUV-capable and
// serve BGR views too; the Detect tail does not change (FrameDesc::w, h hold the view's size).
#define ZLY_VIEW_TU 1
#define ZLY_STEM_VIEW_TU 1
#include "kernels_misc.hip"
#include "kernels_stem.hip"
