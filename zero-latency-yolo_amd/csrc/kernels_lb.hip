// kernels_lb.hip -- the LB unit of front_variants.h: the front kernels' instantiations for tight frames in a letterbox engine (include/zly.h
// ZLY_FLAG_LETTERBOX), and the Detect tail's (head_fused_kernel: the box mapping out of the letterbox).
#define ZLY_FRONT_TU ZLY_TU_LB
#include "kernels_misc.hip"
#include "kernels_stem.hip"
#include "kernels_head.hip"          // last: it switches FP contraction off for the rest of the translation unit
