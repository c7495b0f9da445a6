// LLaMA-Adapter inference (reference lit_llama/adapter.py:149-165): attention over the learned
// prefix of the adapted layers, y += gating_factor[h] * softmax(q . AK^T / sqrt(hs)) . AV with
// AK, AV = the K / V thirds of c_attn(adapter_wte.weight) -- aT <= 64 keys and values per head, no
// RoPE, no mask, the same for every row.
//   llj_attention_adapter   decode attention (attention.h) with the prefix term in the same launch
//   llj_adapter_prefix_add  the prefix term added to rows another attention kernel wrote (flash
//                           prefill, split-K, the any-shape / fp32 kernels)
#include "common.h"
#include "attention.h"
#include "lit_llama_amd.h"

namespace llj {

template <int HS, int U, int NTH, int SPECU>
__global__ __launch_bounds__(NTH) void attention_adapter_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ kc,
                                                                const bf16_t* __restrict__ vc, bf16_t* __restrict__ y,
                                                                const int* __restrict__ pos, int T, int S, int nh,
                                                                float scale_log2, int spec_ok,
                                                                const bf16_t* __restrict__ ak,
                                                                const bf16_t* __restrict__ av,
                                                                const float* __restrict__ gate, int aT) {
  __shared__ float lds[attention_lds_floats<HS, NTH, true>()];
  attention_body<HS, U, NTH, false, SPECU, false, true>(q, kc, vc, y, pos, T, S, nh, scale_log2, blockIdx.x, blockIdx.y,
                                                        lds, 1, 0, nullptr, nullptr, 0.f, nullptr, 0, spec_ok != 0, ak,
                                                        av, gate, aT);
}

// ---- the prefix term on its own: a streaming kernel (q read once, y read and written once).
// Workgroup (head h, tile of kPaRows rows): the head's aT keys staged once in LDS as fp32 (row
// stride hs + 1: lane j reads key j), each wave takes rows of the tile -- lane j scores key j
// against the row's q (an LDS broadcast), the softmax over the wave's lanes leaves normalized
// probabilities in LDS -- then the head's values replace the keys in the same LDS and each wave
// adds sum_j p_j av[j, d] to its rows of y, 16 bytes per lane when VEC.
// bf16 rounding points are the reference's on bf16 tensors: bf16(bf16(y) + bf16(gate * bf16(ay))).
constexpr int kPaNT = 256, kPaWaves = kPaNT / 64, kPaRows = 16;

__device__ __forceinline__ float pa_ld(const bf16_t* p) { return bf2f(*p); }
__device__ __forceinline__ float pa_ld(const float* p) { return *p; }
__device__ __forceinline__ float pa_add(bf16_t y, float g, float ay) { return round_bf(bf2f(y) + round_bf(g * round_bf(ay))); }
__device__ __forceinline__ float pa_add(float y, float g, float ay) { return y + g * ay; }
__device__ __forceinline__ void pa_st(bf16_t* p, float v) { *p = f2bf(v); }
__device__ __forceinline__ void pa_st(float* p, float v) { *p = v; }

constexpr int pa_lds_floats(int hs, int aT) {
  return ((aT * (hs + 1) + 3) & ~3) + kPaRows * 64 + kPaWaves * ((hs + 3) & ~3);
}

template <typename T, bool VEC>
__global__ __launch_bounds__(kPaNT) void adapter_prefix_add_kernel(const T* __restrict__ q, const T* __restrict__ ak,
                                                                   const T* __restrict__ av,
                                                                   const float* __restrict__ gate, T* __restrict__ y,
                                                                   int M, int nh, int hs, int aT, float scale_log2) {
  extern __shared__ __attribute__((aligned(16))) float pa_sm[];
  constexpr int VW = 16 / (int)sizeof(T);  // elements per 16-byte access
  const int h = blockIdx.x, m0 = blockIdx.y * kPaRows;
  const int rows = min(kPaRows, M - m0);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int ks = hs + 1;
  float* kv_s = pa_sm;                              // [aT][hs + 1] keys, then [aT][hs] values
  float* p_s = kv_s + ((aT * ks + 3) & ~3);         // [kPaRows][64] probabilities
  float* q_s = p_s + kPaRows * 64 + wv * ((hs + 3) & ~3);  // this wave's query row
  const size_t C = (size_t)nh * hs;
  const T* akh = ak + (size_t)h * aT * hs;
  const T* avh = av + (size_t)h * aT * hs;
  const float g = gate[h];
  for (int i = threadIdx.x; i < aT * hs; i += kPaNT) kv_s[(i / hs) * ks + i % hs] = pa_ld(akh + i);
  // scores and softmax: the same trip count in every wave (a wave past the tile's rows repeats the
  // last row and writes nothing)
  for (int r0 = 0; r0 < rows; r0 += kPaWaves) {
    const int r = r0 + wv, rc = r < rows ? r : rows - 1;
    const T* qr = q + (size_t)(m0 + rc) * C + (size_t)h * hs;
    if constexpr (VEC) {
      for (int c = lane; c < hs / VW; c += 64) {
        const uint4 w = *reinterpret_cast<const uint4*>(qr + c * VW);
        float* d = q_s + c * VW;
        if constexpr (sizeof(T) == 2) {
          d[0] = bflo(w.x); d[1] = bfhi(w.x); d[2] = bflo(w.y); d[3] = bfhi(w.y);
          d[4] = bflo(w.z); d[5] = bfhi(w.z); d[6] = bflo(w.w); d[7] = bfhi(w.w);
        } else {
          d[0] = __uint_as_float(w.x); d[1] = __uint_as_float(w.y);
          d[2] = __uint_as_float(w.z); d[3] = __uint_as_float(w.w);
        }
      }
    } else {
      for (int d = lane; d < hs; d += 64) q_s[d] = pa_ld(qr + d);
    }
    __syncthreads();  // the staged keys (first trip) and this wave's query row
    float s = -INFINITY;
    if (lane < aT) {
      const float* kr = kv_s + lane * ks;
      float acc = 0.f;
      for (int i = 0; i < hs; ++i) acc += q_s[i] * kr[i];
      s = acc * scale_log2;
    }
    const float mx = wave_max(s);
    const float pj = lane < aT ? exp2f(s - mx) : 0.f;
    const float l = wave_sum(pj);  // >= 1: the maximum's own term
    if (r < rows) p_s[r * 64 + lane] = pj / l;
    __syncthreads();  // q_s is rewritten on the next trip
  }
  for (int i = threadIdx.x; i < aT * hs; i += kPaNT) kv_s[i] = pa_ld(avh + i);
  __syncthreads();
  for (int r = wv; r < rows; r += kPaWaves) {
    T* yr = y + (size_t)(m0 + r) * C + (size_t)h * hs;
    const float* pr = p_s + r * 64;
    if constexpr (VEC) {
      for (int c = lane; c < hs / VW; c += 64) {
        float acc[VW];
#pragma unroll
        for (int k = 0; k < VW; ++k) acc[k] = 0.f;
        for (int j = 0; j < aT; ++j) {
          const float p = pr[j];
          const float4* vr = reinterpret_cast<const float4*>(kv_s + j * hs + c * VW);
#pragma unroll
          for (int k4 = 0; k4 < VW / 4; ++k4) {
            const float4 v = vr[k4];
            acc[4 * k4] += p * v.x; acc[4 * k4 + 1] += p * v.y;
            acc[4 * k4 + 2] += p * v.z; acc[4 * k4 + 3] += p * v.w;
          }
        }
        uint4* yp = reinterpret_cast<uint4*>(yr + c * VW);
        const uint4 w = *yp;
        uint4 o;
        if constexpr (sizeof(T) == 2) {
          o.x = pack2bf(pa_add((bf16_t)(w.x & 0xFFFFu), g, acc[0]), pa_add((bf16_t)(w.x >> 16), g, acc[1]));
          o.y = pack2bf(pa_add((bf16_t)(w.y & 0xFFFFu), g, acc[2]), pa_add((bf16_t)(w.y >> 16), g, acc[3]));
          o.z = pack2bf(pa_add((bf16_t)(w.z & 0xFFFFu), g, acc[4]), pa_add((bf16_t)(w.z >> 16), g, acc[5]));
          o.w = pack2bf(pa_add((bf16_t)(w.w & 0xFFFFu), g, acc[6]), pa_add((bf16_t)(w.w >> 16), g, acc[7]));
        } else {
          o.x = __float_as_uint(pa_add(__uint_as_float(w.x), g, acc[0]));
          o.y = __float_as_uint(pa_add(__uint_as_float(w.y), g, acc[1]));
          o.z = __float_as_uint(pa_add(__uint_as_float(w.z), g, acc[2]));
          o.w = __float_as_uint(pa_add(__uint_as_float(w.w), g, acc[3]));
        }
        *yp = o;
      }
    } else {
      for (int d = lane; d < hs; d += 64) {
        float acc = 0.f;
        for (int j = 0; j < aT; ++j) acc += pr[j] * kv_s[j * hs + d];
        pa_st(yr + d, pa_add(yr[d], g, acc));
      }
    }
  }
}

}  // namespace llj

using namespace llj;

extern "C" {

int llj_attention_adapter(const void* q, const void* kcache, const void* vcache, void* y, const int* pos, int B, int T,
                          int n_head, int head_size, int S, const void* ak, const void* av, const float* gate, int aT,
                          void* stream) {
  LLJ_REQUIRE(q && kcache && vcache && y && pos && ak && av && gate);
  LLJ_REQUIRE(B > 0 && T > 0 && n_head > 0 && S > 0 && aT >= 1 && aT <= kAdpMaxT);
  LLJ_REQUIRE(head_size == 64 || head_size == 128);
  LLJ_REQUIRE((((uintptr_t)ak | (uintptr_t)av) & 15) == 0);
  const float sl2 = 1.4426950408889634f / sqrtf((float)head_size);
  dim3 grid(n_head, B * T);
  // the speculative first pass as llj_attention (ops.hip attention_run)
  const bool full = opt(LLJ_OPT_ATT_SPEC_FULL) == 1;
  const int sb = opt(LLJ_OPT_ATT_SPEC_BATCH);
  const int spec_ok = (int)grid.x * (int)grid.y <= 64 || (!full && (sb < 0 ? LLJ_ATT_SPEC_BATCH : sb) != 0);
  hipStream_t st_ = (hipStream_t)stream;
#define LLJ_ADP_LAUNCH(HS_, SU_)                                                                                       \
  hipLaunchKernelGGL((attention_adapter_kernel<HS_, LLJ_ATT_U, LLJ_ATT_NTH, SU_>), grid, dim3(LLJ_ATT_NTH), 0, st_,   \
                     (const bf16_t*)q, (const bf16_t*)kcache, (const bf16_t*)vcache, (bf16_t*)y, pos, T, S, n_head,  \
                     sl2, spec_ok, (const bf16_t*)ak, (const bf16_t*)av, gate, aT)
  if (head_size == 128) {
    if (full) LLJ_ADP_LAUNCH(128, LLJ_ATT_U); else LLJ_ADP_LAUNCH(128, LLJ_ATT_U / 2);
  } else {
    if (full) LLJ_ADP_LAUNCH(64, LLJ_ATT_U); else LLJ_ADP_LAUNCH(64, LLJ_ATT_U / 2);
  }
#undef LLJ_ADP_LAUNCH
  LLJ_CHECK_LAUNCH();
  return 0;
}

int llj_adapter_prefix_add(const void* q, const void* ak, const void* av, const float* gate, void* y, int M, int n_head,
                           int head_size, int aT, int dt, void* stream) {
  LLJ_REQUIRE(q && ak && av && gate && y && M > 0 && n_head > 0 && head_size > 0 && (dt == 0 || dt == 1));
  LLJ_REQUIRE(aT >= 1 && aT <= kAdpMaxT);
  const size_t lds = (size_t)pa_lds_floats(head_size, aT) * sizeof(float);
  LLJ_REQUIRE(lds <= 64 * 1024 && (M + kPaRows - 1) / kPaRows <= 65535);
  const float sl2 = 1.4426950408889634f / sqrtf((float)head_size);
  const int vw = dt == 0 ? 8 : 4;
  const bool vec = head_size % vw == 0 && (((uintptr_t)q | (uintptr_t)y) & 15) == 0;
  const dim3 grid(n_head, (M + kPaRows - 1) / kPaRows);
  hipStream_t s = (hipStream_t)stream;
#define LLJ_PA_LAUNCH(T_, V_)                                                                                     \
  hipLaunchKernelGGL((adapter_prefix_add_kernel<T_, V_>), grid, dim3(kPaNT), lds, s, (const T_*)q, (const T_*)ak, \
                     (const T_*)av, gate, (T_*)y, M, n_head, head_size, aT, sl2)
  if (dt == 0) {
    if (vec) LLJ_PA_LAUNCH(bf16_t, true); else LLJ_PA_LAUNCH(bf16_t, false);
  } else {
    if (vec) LLJ_PA_LAUNCH(float, true); else LLJ_PA_LAUNCH(float, false);
  }
#undef LLJ_PA_LAUNCH
  LLJ_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
