// LoRA (reference lit_llama/lora.py): the eval-time merge of the low-rank update into the dense c_attn
// weight (lora.py:241-278), in place. Runs once per checkpoint load; one coalesced pass over the rows of
// the enabled groups, the group's slab of lora_A staged through LDS. The unmerged forward lives in the
// kernels that produce c_attn's output (gemv_impl.h, gemm.hip, generic.hip: their LORA forms).
#include "common.h"
#include "lit_llama_amd.h"

namespace llj {

constexpr int kLmK = 128;    // weight columns per workgroup (one per thread of a half block)
constexpr int kLmRows = 32;  // weight rows per workgroup, two at a time
constexpr int kLmR = 64;     // largest rank

template <typename T>
__device__ __forceinline__ float lm_ld(const T* p, size_t i) {
  if constexpr (sizeof(T) == 2) return bf2f(p[i]);
  else return p[i];
}
template <typename T>
__device__ __forceinline__ float lm_rnd(float v) {
  if constexpr (sizeof(T) == 2) return round_bf(v);
  else return v;
}

// W[n, k] += sign * rnd(scaling * rnd(sum_j B[n', j] A[gi r + j, k])) for the rows n of enabled group
// blockIdx.z (gi: among the enabled ones); rnd = to T, the reference's three rounding points on tensors of
// T (the conv1d output, delta_w * scaling, the in-place sum). The sum over j runs in index order in fp32.
template <typename T>
__global__ __launch_bounds__(256) void lora_merge_kernel(T* __restrict__ W, const T* __restrict__ A,
                                                         const T* __restrict__ B, int Ng, int K, int r, int mask,
                                                         float scaling, float sign) {
  __shared__ float As[kLmR * kLmK];
  const int tid = threadIdx.x, kk = tid & (kLmK - 1), rsub = tid >> 7;
  const int gi = blockIdx.z;
  int g = 0;  // the gi-th enabled group
  for (int seen = 0; g < 3; ++g)
    if ((mask >> g) & 1) {
      if (seen == gi) break;
      ++seen;
    }
  const int k0 = blockIdx.x * kLmK;
  for (int e = tid; e < r * kLmK; e += 256) {
    const int j = e / kLmK, c = e - j * kLmK;
    As[e] = k0 + c < K ? lm_ld(A, (size_t)(gi * r + j) * K + k0 + c) : 0.f;
  }
  __syncthreads();
  const int k = k0 + kk;
  const int row_end = min(Ng, (int)(blockIdx.y + 1) * kLmRows);
  for (int nl = blockIdx.y * kLmRows + rsub; nl < row_end; nl += 2) {
    const T* br = B + ((size_t)gi * Ng + nl) * r;
    float d = 0.f;
    for (int j = 0; j < r; ++j) d = fmaf(lm_ld(br, j), As[j * kLmK + kk], d);
    float dl = lm_rnd<T>(d) * scaling;
    asm volatile("" : "+v"(dl));  // (fp32: the product is rounded on its own, not contracted into the sum)
    dl = sign * lm_rnd<T>(dl);
    if (k < K) {
      const size_t wi = ((size_t)g * Ng + nl) * K + k;
      const float w = lm_rnd<T>(lm_ld(W, wi) + dl);
      if constexpr (sizeof(T) == 2) W[wi] = f2bf(w);
      else W[wi] = w;
    }
  }
}

}  // namespace llj

using namespace llj;

extern "C" {

int llj_lora_merge(void* W, const void* lora_A, const void* lora_B, int N, int K, int r, int enable_mask,
                   float scaling, int sign, int dt, void* stream) {
  LLJ_REQUIRE(W && lora_A && lora_B && N > 0 && K > 0 && N % 3 == 0 && r >= 1 && r <= kLmR);
  LLJ_REQUIRE(enable_mask >= 1 && enable_mask <= 7 && (sign == 1 || sign == -1) && (dt == 0 || dt == 1));
  const int Ng = N / 3;
  const int n_en = (enable_mask & 1) + ((enable_mask >> 1) & 1) + ((enable_mask >> 2) & 1);
  const dim3 grid((K + kLmK - 1) / kLmK, (Ng + kLmRows - 1) / kLmRows, n_en);
  LLJ_REQUIRE(grid.y <= 65535);
  hipStream_t s = (hipStream_t)stream;
  if (dt == 0)
    hipLaunchKernelGGL(lora_merge_kernel<bf16_t>, grid, dim3(256), 0, s, (bf16_t*)W, (const bf16_t*)lora_A,
                       (const bf16_t*)lora_B, Ng, K, r, enable_mask, scaling, (float)sign);
  else
    hipLaunchKernelGGL(lora_merge_kernel<float>, grid, dim3(256), 0, s, (float*)W, (const float*)lora_A,
                       (const float*)lora_B, Ng, K, r, enable_mask, scaling, (float)sign);
  LLJ_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
