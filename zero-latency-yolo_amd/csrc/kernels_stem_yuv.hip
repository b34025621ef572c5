// kernels_stem_yuv.hip -- the YUV unit of front_variants.h: the stem kernels' instantiations for tight stretch batches with a YUV 4:2:0 frame.
#define ZLY_FRONT_TU ZLY_TU_YUV
#include "kernels_stem.hip"
