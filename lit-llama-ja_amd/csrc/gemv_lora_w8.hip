// LoRA instantiations (LORA: the unmerged low-rank term in the QKV epilogue) of the GEMV kernels for
// weight format WF_W8 (gemv_impl.h).
#include "gemv_impl.h"

namespace llj {
int gemv_launch_lora_w8(int am, const GemvParams& p, hipStream_t s) {
  return launch_lora_fmt<WF_W8>(am, p, s);
}
}  // namespace llj
