// kernels_pix.hip -- the PIX unit of front_variants.h: the front kernels' instantiations that serve every pixel format, packed RGB / BGRA / RGBA
// included (include/zly.h ZLY_PIX_*), on tight frames, stretch and letterbox.
#define ZLY_FRONT_TU ZLY_TU_PIX
#include "kernels_misc.hip"
#include "kernels_stem.hip"
