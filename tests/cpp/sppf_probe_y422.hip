// sppf_probe_y422.hip -- TEST INFRASTRUCTURE, a second object of libsppf_probe.so (Makefile) beside sppf_probe.hip: kernels_misc.o's preprocess picker also
// asks the two units of the packed 4:2:2 level (front_variants.h: kernels_y422.hip, kernels_y422_view.hip) for their instantiations.  Those objects are
// not linked into the probe and no preprocess kernel is ever launched from it: as sppf_probe.hip's, their getters answer "no such kernel".
#include "zly_internal.h"

namespace zly {
template <int TU> const void* preprocess_kernel_in(FrontVariant v, int dtype);
template <> const void* preprocess_kernel_in<ZLY_TU_Y422>(FrontVariant, int) { return nullptr; }
template <> const void* preprocess_kernel_in<ZLY_TU_Y422_VIEW>(FrontVariant, int) { return nullptr; }
}  // namespace zly
