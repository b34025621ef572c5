// kernels_y422_view.hip -- the Y422_VIEW unit of front_variants.h: kernels_y422.hip's counterpart for calls on frame views -- a pitched capture surface, a
// region or a tile of one, detected in place --, split off so that the two compile side by side.
#define ZLY_FRONT_TU ZLY_TU_Y422_VIEW
#include "kernels_misc.hip"
#include "kernels_stem.hip"
