// Decode attention of B rows that share a prompt prefix (llj_attention_shared; one prompt sampled B times:
// DecodeSession.prefill_shared). Row b at position p attends keys 0 .. p; the keys j < P are the prompt's and
// are the same in every row's cache, so they are read from row 0's cache only, once per head for a group of
// up to 8 rows, instead of once per row; the keys P <= j <= p are row b's own.
//
// One launch of 256-thread blocks on a grid (n_head, nsplit + 8, ceil(B / 8)) and the combine launch of
// attention.h:
//   y < nsplit   prefix block: key range `y` of nsplit equal ranges of [0, P) (at least one pass of 64 keys
//                each; the ranges past P stay empty) of row 0's cache against the <= 8 rows of group z. The
//                layout is attention.h's: 16 lanes per key (HS / 16 dims each), 16 key groups, U = 4 keys per
//                group and pass, all K / V loads of a pass (16 or 8 bytes each, straight to VGPRs) issued
//                before any use, the first pass before the position is read. Every K / V row is loaded once
//                and scored against the 8 query rows (scaled fp32 in LDS, read back per row and pass); each
//                row keeps an online softmax of its own in registers with one rescale per pass.
//   y >= nsplit  suffix block of row 8 z + (y - nsplit): the same loop with one query row over the keys
//                [P, p] of that row's cache.
// Every block merges its key groups as attention_body does (lane swaps inside a wave, the four waves through
// LDS in wave order) and writes an unnormalized partial (outputs, max, sum) per row in the kAttPart record
// layout: nsplit + 1 records per (row, head), the suffix last. attention_combine_kernel merges them in record
// order (empty ranges have max = -inf and add nothing). No atomics: the same inputs give the same bits.
//
// The position is read on the device. The caller guarantees P - 1 <= p < S; whatever it holds, the prefix
// reads stay below P <= S (host-checked) and the suffix below S, and a key outside a block's range is loaded
// from slot 0 of row 0 and weighted 0, so no row's slots below P are touched except row 0's.
#include "attention.h"
#include "lit_llama_amd.h"

#include <math.h>

namespace llj {

constexpr int kShNTH = 256;                // threads per block
constexpr int kShU = 4;                    // keys per 16-lane group per pass
constexpr int kShRows = 8;                 // query rows per prefix block
constexpr int kShPass = kShNTH / 16 * kShU;  // keys per pass (the smallest prefix range)
constexpr int kShMaxSplit = 64;

template <int HS, int R>
constexpr int shared_lds_floats() {
  return (kShNTH / 64) * R * (HS + 2);  // per wave and row: max, sum, HS outputs
}

// One block's key range against the R query rows m0 .. m0 + R - 1 (rows >= B repeat row B - 1 and are not
// written); partial record `rec` of nrec per (row, head). kv_off: element offset of (row, head, slot 0) of the
// cache rows read; safe_off: an offset that may always be read (row 0, slot 0 of this head).
// PREFIX: keys [jbeg, min(jcap, keys valid at the position)), jcap <= P known on the host. The slots below P
// exist whatever the position is, so the first pass is loaded before the position is read (one memory latency
// instead of two; keys past the valid range are masked). Otherwise (suffix): keys [min(P, valid), valid).
template <int HS, int R, bool PREFIX>
__device__ __forceinline__ void shared_range(const bf16_t* __restrict__ q, const bf16_t* __restrict__ kc,
                                             const bf16_t* __restrict__ vc, const int* __restrict__ pos, int P, int S,
                                             size_t kv_off, size_t safe_off, int jbeg, int jcap, int m0, int B,
                                             int nh, int h, float scale_log2, int nrec, int rec,
                                             float* __restrict__ part, float* lds, float* lq) {
  constexpr int DPL = HS / 16;
  constexpr int NG = kShNTH / 16;
  constexpr int NWV = kShNTH / 64;
  constexpr int U = kShU;
  const int sub = threadIdx.x & 15, kg = threadIdx.x >> 4;
  const int C = nh * HS;
  // the R query rows, scaled, as fp32 in LDS (key group r loads row r): every pass reads them back per row,
  // 64 VGPRs less than holding them, which keeps two blocks per CU resident
  if (kg < R) {
    const int m = m0 + kg < B ? m0 + kg : B - 1;
    const size_t qo = (size_t)m * C + h * HS + sub * DPL;
    float* dst = lq + kg * HS + sub * DPL;
    if constexpr (DPL == 8) {
      const uint4 a = *reinterpret_cast<const uint4*>(q + qo);
      const uint32_t w[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        dst[2 * i] = bflo(w[i]) * scale_log2;
        dst[2 * i + 1] = bfhi(w[i]) * scale_log2;
      }
    } else {
      const uint2 a = *reinterpret_cast<const uint2*>(q + qo);
      dst[0] = bflo(a.x) * scale_log2;
      dst[1] = bfhi(a.x) * scale_log2;
      dst[2] = bflo(a.y) * scale_log2;
      dst[3] = bfhi(a.y) * scale_log2;
    }
  }
  float mx[R], l[R], o[R][DPL];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    mx[r] = -INFINITY;
    l[r] = 0.f;
#pragma unroll
    for (int i = 0; i < DPL; ++i) o[r][i] = 0.f;
  }
  uint32_t kw[U][DPL / 2], vw[U][DPL / 2];
  // K / V rows of one pass (U keys of this group), every load first; keys at or past `bound`: the safe row
  auto load_pass = [&](int j0, int bound) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = j0 + NG * u;
      const size_t eo = (j < bound ? kv_off + (size_t)j * HS : safe_off) + sub * DPL;
      if constexpr (DPL == 8) {
        const uint4 a = *reinterpret_cast<const uint4*>(kc + eo);
        const uint4 c = *reinterpret_cast<const uint4*>(vc + eo);
        kw[u][0] = a.x; kw[u][1] = a.y; kw[u][2] = a.z; kw[u][3] = a.w;
        vw[u][0] = c.x; vw[u][1] = c.y; vw[u][2] = c.z; vw[u][3] = c.w;
      } else {
        const uint2 a = *reinterpret_cast<const uint2*>(kc + eo);
        const uint2 c = *reinterpret_cast<const uint2*>(vc + eo);
        kw[u][0] = a.x; kw[u][1] = a.y;
        vw[u][0] = c.x; vw[u][1] = c.y;
      }
    }
  };
  if constexpr (PREFIX) load_pass(jbeg + kg, jcap);
  const int ps = pos[0];
  const int nvalid = ps < 0 ? 0 : ps < S ? ps + 1 : S;  // keys 0 .. p, inside the cache whatever p holds
  const int pe = nvalid < P ? nvalid : P;               // = P under the caller's contract (p >= P - 1)
  if constexpr (!PREFIX) jbeg = pe;
  const int jend = PREFIX ? min(pe, jcap) : nvalid;
  __syncthreads();  // the query rows
  bool first = PREFIX;
  for (int j0 = jbeg + kg; j0 < jend; j0 += NG * U) {  // key u = 0 of a pass that runs is inside the range
    if (!first) load_pass(j0, jend);
    first = false;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      float qf[DPL];
#pragma unroll
      for (int i = 0; i < DPL / 4; ++i) {
        const f32x4 w = *reinterpret_cast<const f32x4*>(lq + r * HS + sub * DPL + 4 * i);
        qf[4 * i] = w[0]; qf[4 * i + 1] = w[1]; qf[4 * i + 2] = w[2]; qf[4 * i + 3] = w[3];
      }
      float s[U];
      float mn = mx[r];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        float a = 0.f;
#pragma unroll
        for (int i = 0; i < DPL / 2; ++i) a += qf[2 * i] * bflo(kw[u][i]) + qf[2 * i + 1] * bfhi(kw[u][i]);
        a = row16_sum(a);  // the 16 lanes of this key
        s[u] = j0 + NG * u < jend ? a : -INFINITY;
        mn = fmaxf(mn, s[u]);
      }
      const float corr = exp2f(mx[r] - mn);  // mn is finite (key u = 0); exp2(-inf) = 0 on the first pass
      float pj[U];
      float ls = 0.f;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        pj[u] = exp2f(s[u] - mn);
        ls += pj[u];
      }
      l[r] = l[r] * corr + ls;
#pragma unroll
      for (int i = 0; i < DPL / 2; ++i) {
        float a = o[r][2 * i] * corr, b = o[r][2 * i + 1] * corr;
#pragma unroll
        for (int u = 0; u < U; ++u) {
          a += pj[u] * bflo(vw[u][i]);
          b += pj[u] * bfhi(vw[u][i]);
        }
        o[r][2 * i] = a;
        o[r][2 * i + 1] = b;
      }
      mx[r] = mn;
    }
  }
  // the four key groups of a wave with lane swaps (attention_body's merge, per row), then the waves through LDS
  const int wv = threadIdx.x >> 6;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    float mlo, mhi, llo, lhi, olo[DPL], ohi[DPL];
    lane_halves<false>(mx[r], mlo, mhi);
    lane_halves<false>(l[r], llo, lhi);
#pragma unroll
    for (int i = 0; i < DPL; ++i) lane_halves<false>(o[r][i], olo[i], ohi[i]);
    softmax_merge<DPL>(mx[r], l[r], o[r], mlo, mhi, llo, lhi, olo, ohi);
    lane_halves<true>(mx[r], mlo, mhi);
    lane_halves<true>(l[r], llo, lhi);
#pragma unroll
    for (int i = 0; i < DPL; ++i) lane_halves<true>(o[r][i], olo[i], ohi[i]);
    softmax_merge<DPL>(mx[r], l[r], o[r], mlo, mhi, llo, lhi, olo, ohi);
    if (kg % 4 == 0) {  // the first 16 lanes of each wave
      float* dst = lds + (wv * R + r) * (HS + 2);
#pragma unroll
      for (int i = 0; i < DPL; ++i) dst[2 + sub * DPL + i] = o[r][i];
      if (sub == 0) {
        dst[0] = mx[r];
        dst[1] = l[r];
      }
    }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < R * HS; e += kShNTH) {
    const int r = e / HS, d = e % HS;
    if (m0 + r >= B) break;  // rows ascend with e
    float M = -INFINITY;
#pragma unroll
    for (int w = 0; w < NWV; ++w) M = fmaxf(M, lds[(w * R + r) * (HS + 2)]);
    float L = 0.f, O = 0.f;
#pragma unroll
    for (int w = 0; w < NWV; ++w) {
      const float* src = lds + (w * R + r) * (HS + 2);
      const float f = src[0] == -INFINITY ? 0.f : exp2f(src[0] - M);
      L += src[1] * f;
      O += src[2 + d] * f;
    }
    float* dst = part + ((size_t)((m0 + r) * nh + h) * nrec + rec) * kAttPart<HS>;
    dst[d] = O;
    if (d == 0) {
      dst[HS] = M;
      dst[HS + 1] = L;
    }
  }
}

template <int HS>
__global__ __launch_bounds__(kShNTH) void attention_shared_kernel(const bf16_t* __restrict__ q,
                                                                  const bf16_t* __restrict__ kc,
                                                                  const bf16_t* __restrict__ vc,
                                                                  const int* __restrict__ pos, int B, int P, int S,
                                                                  int nh, float scale_log2, int nsplit,
                                                                  float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float lds[shared_lds_floats<HS, kShRows>() + kShRows * HS];
  float* lq = lds + shared_lds_floats<HS, kShRows>();  // the query rows (16-byte aligned)
  const int h = blockIdx.x, y = blockIdx.y, m0 = blockIdx.z * kShRows;
  const size_t head0 = (size_t)h * S * HS;  // row 0, this head, slot 0
  if (y < nsplit) {
    const int chunk = max((P + nsplit - 1) / nsplit, kShPass);
    const int jbeg = y * chunk;
    shared_range<HS, kShRows, true>(q, kc, vc, pos, P, S, head0, head0, jbeg, min(P, jbeg + chunk), m0, B, nh, h,
                                    scale_log2, nsplit + 1, y, part, lds, lq);
  } else {
    const int m = m0 + (y - nsplit);
    if (m >= B) return;
    shared_range<HS, 1, false>(q, kc, vc, pos, P, S, ((size_t)(m * nh + h) * S) * HS, head0, 0, 0, m, B, nh, h,
                               scale_log2, nsplit + 1, nsplit, part, lds, lq);
  }
}

}  // namespace llj

using namespace llj;

extern "C" {

size_t llj_attention_shared_ws_bytes(int B, int n_head, int head_size, int nsplit) {
  if (B < 1 || n_head < 1 || head_size < 1) return 0;
  return (size_t)B * n_head * ((nsplit < 1 ? 1 : nsplit) + 1) * (head_size + 4) * sizeof(float);  // kAttPart
}

int llj_attention_shared(const void* q, const void* kcache, const void* vcache, void* y, const int* pos, int B, int P,
                         int n_head, int head_size, int S, int nsplit, void* ws, void* stream) {
  LLJ_REQUIRE(q && kcache && vcache && y && pos && ws);
  LLJ_REQUIRE(head_size == 64 || head_size == 128);
  LLJ_REQUIRE(B >= 1 && n_head >= 1 && P >= 1 && P <= S && nsplit >= 1 && nsplit <= kShMaxSplit);
  LLJ_REQUIRE(B <= 65535 && n_head <= 65535);  // grid dimensions
  const int groups = (B + kShRows - 1) / kShRows;
  const float sl2 = 1.4426950408889634f / sqrtf((float)head_size);
  const dim3 grid(n_head, nsplit + kShRows, groups), cgrid(n_head, B);
  hipStream_t s = (hipStream_t)stream;
  if (head_size == 128) {
    hipLaunchKernelGGL((attention_shared_kernel<128>), grid, dim3(kShNTH), 0, s, (const bf16_t*)q,
                       (const bf16_t*)kcache, (const bf16_t*)vcache, pos, B, P, S, n_head, sl2, nsplit, (float*)ws);
    LLJ_CHECK_LAUNCH();
    hipLaunchKernelGGL((attention_combine_kernel<128>), cgrid, dim3(128), 0, s, (const float*)ws, (bf16_t*)y, n_head,
                       nsplit + 1, (uint32_t*)nullptr, 0.f, (uint32_t*)nullptr, 0);
  } else {
    hipLaunchKernelGGL((attention_shared_kernel<64>), grid, dim3(kShNTH), 0, s, (const bf16_t*)q,
                       (const bf16_t*)kcache, (const bf16_t*)vcache, pos, B, P, S, n_head, sl2, nsplit, (float*)ws);
    LLJ_CHECK_LAUNCH();
    hipLaunchKernelGGL((attention_combine_kernel<64>), cgrid, dim3(64), 0, s, (const float*)ws, (bf16_t*)y, n_head,
                       nsplit + 1, (uint32_t*)nullptr, 0.f, (uint32_t*)nullptr, 0);
  }
  LLJ_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
