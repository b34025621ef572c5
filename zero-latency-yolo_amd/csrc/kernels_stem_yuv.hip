// kernels_stem_yuv.hip -- the YUV = true instantiations of kernels_stem.hip's front kernels (batches with YUV 4:2:0 frames, include/zly.h
// ZLY_PIX_*), in a translation unit of their own so that the BGR instantiations compile exactly as before (see kernels_stem.hip).
#define ZLY_STEM_YUV_TU 1
#include "kernels_stem.hip"
