// Adapter v2 instantiations (AFF: per-column scale and bias in the epilogue) of the GEMV kernels for
// weight format WF_W4G (gemv_impl.h).
#include "gemv_impl.h"

namespace llj {
int gemv_launch_aff_w4g(int am, int ep, const GemvParams& p, hipStream_t s) {
  return launch_fmt<WF_W4G, true>(am, ep, p, s);
}
}  // namespace llj
