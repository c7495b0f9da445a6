// Decode attention of B rows that each stand at a position of their own (llj_attention_ragged; prompts of
// different lengths decoded as one batch: DecodeSession.prefill_ragged). The step counter *pos is shared; row b
// is at p = *pos - off[b], with off fixed for the session. One launch does what the c_attn epilogue (EP_QKV in
// gemv_impl.h) and llj_attention do for rows at one position: RoPE on q and k at the row's angle, k / v into
// slot p of the row's cache, attention over the row's keys 0 .. p.
//
// One 512-thread block per (head, row), attention.h's block. Prologue: three 16-lane groups of wave 0 take the
// head's q, k and v (HS / 16 contiguous dims per lane, one 16- or 8-byte load each, the q / k groups one or two
// 16-byte loads of the RoPE row as well), rotate the interleaved pairs in fp32 on the bf16 inputs, round once
// and store q' to q_out and k', v to slot p. A workgroup barrier follows; attention_body (attention.h, unchanged)
// then reads q' and slots 0 .. p back, the current key among them. No load of a cache slot is issued before the
// barrier: the speculative first pass stays off (spec_ok = false). The row's position reaches attention_body
// through a pointer to a register copy (T = 1: it reads pos[0]).
//
// p is clamped into [0, S - 1] (S <= rope_rows is host-checked), so whatever *pos and off hold, every read and
// write stays inside row b's cache rows, the RoPE table and the (B, C) buffers. No atomics: the same inputs give
// the same bits. Slots above p, other rows' slots, and slots other than p are never written; slots above p are
// never read.
#include "attention.h"
#include "lit_llama_amd.h"

#include <math.h>

namespace llj {

template <int HS>
__global__ __launch_bounds__(LLJ_ATT_NTH) void attention_ragged_kernel(const bf16_t* __restrict__ qkv, bf16_t* q_out,
                                                                       bf16_t* kc, bf16_t* vc, bf16_t* y,
                                                                       const float* __restrict__ rope,
                                                                       const int* __restrict__ pos,
                                                                       const int* __restrict__ off, int S, int nh,
                                                                       float scale_log2) {
  __shared__ float lds[attention_lds_floats<HS, LLJ_ATT_NTH>()];
  constexpr int DPL = HS / 16;
  const int h = blockIdx.x, b = blockIdx.y;
  int p = pos[0] - off[b];
  p = p < 0 ? 0 : (p > S - 1 ? S - 1 : p);
  const int C = nh * HS;
  const int sub = threadIdx.x & 15, part = threadIdx.x >> 4;  // part 0 q, 1 k, 2 v
  if (part < 3) {
    const bf16_t* src = qkv + (size_t)b * 3 * C + (size_t)part * C + h * HS + sub * DPL;
    uint32_t w[DPL / 2];
    if constexpr (DPL == 8) {
      const uint4 a = *reinterpret_cast<const uint4*>(src);
      w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
    } else {
      const uint2 a = *reinterpret_cast<const uint2*>(src);
      w[0] = a.x; w[1] = a.y;
    }
    if (part < 2) {
      // c_attn's bf16 output, RoPE in fp32 on interleaved pairs, one rounding (model.py:318-329; EP_QKV)
      const float* rp = rope + ((size_t)p * (HS / 2) + sub * (DPL / 2)) * 2;  // (cos, sin) of this lane's pairs
#pragma unroll
      for (int i = 0; i < DPL / 4; ++i) {
        const f32x4 cs = *reinterpret_cast<const f32x4*>(rp + 4 * i);
        const float a0 = bflo(w[2 * i]), a1 = bfhi(w[2 * i]);
        const float b0 = bflo(w[2 * i + 1]), b1 = bfhi(w[2 * i + 1]);
        w[2 * i] = pack2bf(a0 * cs[0] - a1 * cs[1], a1 * cs[0] + a0 * cs[1]);
        w[2 * i + 1] = pack2bf(b0 * cs[2] - b1 * cs[3], b1 * cs[2] + b0 * cs[3]);
      }
    }
    bf16_t* dst;
    if (part == 0)
      dst = q_out + (size_t)b * C + h * HS + sub * DPL;
    else
      dst = (part == 1 ? kc : vc) + (((size_t)b * nh + h) * S + p) * HS + sub * DPL;
    if constexpr (DPL == 8)
      *reinterpret_cast<uint4*>(dst) = make_uint4(w[0], w[1], w[2], w[3]);
    else
      *reinterpret_cast<uint2*>(dst) = make_uint2(w[0], w[1]);
  }
  __syncthreads();  // q' and slot p are written before any thread of the block reads them back
  const int pl = p;
  attention_body<HS, LLJ_ATT_U, LLJ_ATT_NTH>(q_out, kc, vc, y, &pl, 1, S, nh, scale_log2, h, b, lds);
}

}  // namespace llj

using namespace llj;

extern "C" {

int llj_attention_ragged(const void* qkv, void* q_out, void* kcache, void* vcache, void* y, const float* rope,
                         const int* pos, const int* off, int B, int n_head, int head_size, int S, int rope_rows,
                         void* stream) {
  LLJ_REQUIRE(qkv && q_out && kcache && vcache && y && rope && pos && off);
  LLJ_REQUIRE(head_size == 64 || head_size == 128);
  LLJ_REQUIRE(B >= 1 && B <= 65535);  // grid dimension
  LLJ_REQUIRE(n_head >= 1 && S >= 1 && rope_rows >= 1 && S <= rope_rows);
  const float sl2 = 1.4426950408889634f / sqrtf((float)head_size);
  const dim3 grid(n_head, B);
  hipStream_t s = (hipStream_t)stream;
  if (head_size == 128)
    hipLaunchKernelGGL((attention_ragged_kernel<128>), grid, dim3(LLJ_ATT_NTH), 0, s, (const bf16_t*)qkv,
                       (bf16_t*)q_out, (bf16_t*)kcache, (bf16_t*)vcache, (bf16_t*)y, rope, pos, off, S, n_head, sl2);
  else
    hipLaunchKernelGGL((attention_ragged_kernel<64>), grid, dim3(LLJ_ATT_NTH), 0, s, (const bf16_t*)qkv,
                       (bf16_t*)q_out, (bf16_t*)kcache, (bf16_t*)vcache, (bf16_t*)y, rope, pos, off, S, n_head, sl2);
  LLJ_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
