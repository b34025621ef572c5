// kernels_lb.hip -- the LB = true instantiations of the front kernels (preprocess_kernel, stem_fused_kernel, stem_model1_kernel) and of the Detect
// tail (head_fused_kernel: the box mapping) for letterbox engines (include/zly.h ZLY_FLAG_LETTERBOX), in a translation unit of their own so that the instantiations every other engine launches compile
// exactly as before (see kernels_stem.hip).
#define ZLY_LB_TU 1
#define ZLY_STEM_LB_TU 1
#include "kernels_misc.hip"
#include "kernels_stem.hip"
#include "kernels_head.hip"          // last: it switches FP contraction off for the rest of the translation unit
