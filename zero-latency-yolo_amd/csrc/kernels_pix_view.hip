// kernels_pix_view.hip -- the PIX_VIEW unit of front_variants.h: kernels_pix.hip's counterpart for calls on frame views -- a region of a BGRA capture
// surface detected in place --, split off so that the two compile side by side.
#define ZLY_FRONT_TU ZLY_TU_PIX_VIEW
#include "kernels_misc.hip"
#include "kernels_stem.hip"
