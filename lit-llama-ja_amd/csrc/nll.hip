// Per-row negative log-likelihood over logits (the evaluate scripts' scoring step: the summed cross entropy
// of reference evaluate/full.py:121-123, per token): row_nll[m] = logsumexp(logits[m, :V]) - logits[m, t[m]]
// in fp32, for bf16 logits (llj_nll) and fp32 ones (llj_g_nll), plus a fixed-order double sum of the rows.
//
// One workgroup of 256 threads per row, the row read once. A thread takes 16-byte chunks (8 bf16 / 4 fp32
// columns; on the element path the same number of columns at a stride of 256) and keeps an online
// (max, sum): per chunk one maximum, at most one rescale of the running sum, and the chunk's exp terms.
// The 256 pairs are combined by a butterfly inside each wave and then wave by wave in LDS by thread 0.
// Every order is fixed, nothing is accumulated with atomics: the same inputs give the same bits.
//
// Special values: a -inf logit adds exp(-inf) = 0 (while a thread's maximum is still -inf the subtracted
// value is 0 and the rescale factor 1, so no inf - inf is formed); a NaN logit makes the sum, and so the
// row, NaN (fmaxf drops it from the maximum, exp keeps it in the sum).
#include "common.h"
#include "lit_llama_amd.h"

#include <math.h>

namespace llj {

struct MaxSum {
  float m, s;
};

// exp(a - m) for a <= m, with exp(-inf - -inf) = 1 (the sum it scales is 0 or NaN then)
__device__ __forceinline__ float nll_factor(float a, float m) { return a == m ? 1.f : expf(a - m); }

template <int E>
__device__ __forceinline__ void nll_absorb(MaxSum& st, const float (&x)[E]) {
  float cm = x[0];
#pragma unroll
  for (int j = 1; j < E; ++j) cm = fmaxf(cm, x[j]);
  const float mn = fmaxf(st.m, cm);
  const float sub = mn == -INFINITY ? 0.f : mn;
  float acc = 0.f;
#pragma unroll
  for (int j = 0; j < E; ++j) acc += expf(x[j] - sub);
  st.s = st.s * nll_factor(st.m, mn) + acc;
  st.m = mn;
}

__device__ __forceinline__ MaxSum nll_merge(MaxSum a, MaxSum b) {
  const float m = fmaxf(a.m, b.m);
  return MaxSum{m, a.s * nll_factor(a.m, m) + b.s * nll_factor(b.m, m)};
}

__device__ __forceinline__ float nll_ld(const bf16_t* p) { return bf2f(*p); }
__device__ __forceinline__ float nll_ld(const float* p) { return *p; }
__device__ __forceinline__ void nll_ld16(const bf16_t* p, float (&x)[8]) {
  const u32x4 w = *reinterpret_cast<const u32x4*>(p);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    x[2 * j] = bflo(w[j]);
    x[2 * j + 1] = bfhi(w[j]);
  }
}
__device__ __forceinline__ void nll_ld16(const float* p, float (&x)[4]) {
  const f32x4 w = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
  for (int j = 0; j < 4; ++j) x[j] = w[j];
}

// VEC: every row base is 16-byte aligned (the host checks the pointer and ldl). Columns >= V are never read.
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void nll_rows_kernel(const T* __restrict__ logits, int ldl, int V,
                                                       const int* __restrict__ targets, float* __restrict__ row_nll) {
  constexpr int E = 16 / sizeof(T);
  __shared__ float sm[4], ss[4];
  const int m = blockIdx.x, tid = threadIdx.x;
  const int t = targets[m];
  if (t < 0 || t >= V) {  // ignored row: 0; a target outside the row: NaN (the row is not read)
    if (tid == 0) row_nll[m] = t < 0 ? 0.f : __builtin_nanf("");
    return;
  }
  const T* row = logits + (size_t)m * ldl;
  MaxSum st{-INFINITY, 0.f};
  float x[E];
  if constexpr (VEC) {
    const int nfull = V / E;
    for (int c = tid; c < nfull; c += 256) {
      nll_ld16(row + (size_t)c * E, x);
      nll_absorb<E>(st, x);
    }
    const int v = nfull * E + tid;  // the V % E columns after the last whole chunk
    if (v < V) {
#pragma unroll
      for (int j = 1; j < E; ++j) x[j] = -INFINITY;
      x[0] = nll_ld(row + v);
      nll_absorb<E>(st, x);
    }
  } else {
    for (size_t base = 0; base < (size_t)V; base += 256 * E) {
#pragma unroll
      for (int j = 0; j < E; ++j) {
        const size_t v = base + j * 256 + tid;
        x[j] = v < (size_t)V ? nll_ld(row + v) : -INFINITY;
      }
      nll_absorb<E>(st, x);
    }
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) st = nll_merge(st, MaxSum{__shfl_xor(st.m, o, 64), __shfl_xor(st.s, o, 64)});
  if ((tid & 63) == 0) {
    sm[tid >> 6] = st.m;
    ss[tid >> 6] = st.s;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 4; ++w) st = nll_merge(st, MaxSum{sm[w], ss[w]});
    const float sub = st.m == -INFINITY ? 0.f : st.m;
    row_nll[m] = (sub + logf(st.s)) - nll_ld(row + t);
  }
}

// total[0] += sum of the counted rows' NLL (double, fixed order: thread i adds rows i, i + 256, ... in
// order, then a pairwise tree over the 256 partial sums), total[1] += rows counted (targets[m] >= 0).
__global__ __launch_bounds__(256) void nll_total_kernel(const float* __restrict__ row_nll,
                                                        const int* __restrict__ targets, int M,
                                                        double* __restrict__ total) {
  __shared__ double sd[256];
  __shared__ int sc[256];
  const int tid = threadIdx.x;
  double a = 0.0;
  int c = 0;
  for (int m = tid; m < M; m += 256)
    if (targets[m] >= 0) {
      a += (double)row_nll[m];
      ++c;
    }
  sd[tid] = a;
  sc[tid] = c;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
      sd[tid] += sd[tid + o];
      sc[tid] += sc[tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    total[0] += sd[0];
    total[1] += (double)sc[0];
  }
}

template <typename T>
static int nll_launch(const T* logits, int ldl, int M, int V, const int* targets, float* row_nll, double* total,
                      hipStream_t s) {
  LLJ_REQUIRE(logits && targets && row_nll && M > 0 && V > 0 && ldl >= V);
  const bool vec = (reinterpret_cast<uintptr_t>(logits) % 16 == 0) && (((size_t)ldl * sizeof(T)) % 16 == 0);
  if (vec)
    hipLaunchKernelGGL((nll_rows_kernel<T, true>), dim3(M), dim3(256), 0, s, logits, ldl, V, targets, row_nll);
  else
    hipLaunchKernelGGL((nll_rows_kernel<T, false>), dim3(M), dim3(256), 0, s, logits, ldl, V, targets, row_nll);
  LLJ_CHECK_LAUNCH();
  if (total) {
    hipLaunchKernelGGL(nll_total_kernel, dim3(1), dim3(256), 0, s, (const float*)row_nll, targets, M, total);
    LLJ_CHECK_LAUNCH();
  }
  return 0;
}

}  // namespace llj

using namespace llj;

extern "C" {

int llj_nll(const void* logits, int ldl, int M, int V, const int* targets, float* row_nll, double* total,
            void* stream) {
  return nll_launch((const bf16_t*)logits, ldl, M, V, targets, row_nll, total, (hipStream_t)stream);
}

int llj_g_nll(const float* logits, int ldl, int M, int V, const int* targets, float* row_nll, double* total,
              void* stream) {
  return nll_launch(logits, ldl, M, V, targets, row_nll, total, (hipStream_t)stream);
}

}  // extern "C"
