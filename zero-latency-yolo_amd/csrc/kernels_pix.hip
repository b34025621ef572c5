// kernels_pix.hip -- the PK = true instantiations of the front kernels (preprocess_kernel, stem_fused_kernel, stem_model1_kernel) on tight frames: the
// ones that serve every pixel format, packed RGB / BGRA / RGBA included (include/zly.h ZLY_PIX_*; yuv_device.h has the three format levels).  A batch
// runs them when it holds at least one frame of the packed family.  In a translation unit of their own so that the instantiations every other batch
// launches compile exactly as before (see kernels_stem.hip); frame views are in kernels_pix_view.hip.
#define ZLY_PIX_TU 1
#define ZLY_STEM_PIX_TU 1
#include "kernels_misc.hip"
#include "kernels_stem.hip"
