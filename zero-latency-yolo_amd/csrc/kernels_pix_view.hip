// kernels_pix_view.hip -- the PK = true, VIEW = true instantiations of the front kernels: frame views (zly_frame_view) of every pixel format, packed
// RGB / BGRA / RGBA included -- a region of a BGRA capture surface detected in place.  The counterpart of kernels_pix.hip for calls on views, split off
// so that the two compile side by side.
#define ZLY_PIX_VIEW_TU 1
#define ZLY_STEM_PIX_VIEW_TU 1
#include "kernels_misc.hip"
#include "kernels_stem.hip"
