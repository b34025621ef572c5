// kernels_y422.hip -- the Y422 unit of front_variants.h: the front kernels' entries that serve every pixel format, packed YUV 4:2:2 (YUY2 / UYVY:
// capture cards, UVC devices) included (include/zly.h ZLY_PIX_*), on tight frames, stretch and letterbox.
#define ZLY_FRONT_TU ZLY_TU_Y422
#include "kernels_misc.hip"
#include "kernels_stem.hip"
