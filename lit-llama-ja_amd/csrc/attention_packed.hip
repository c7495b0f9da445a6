// Prefill of B prompts of different lengths packed into M = sum T_b rows (LLaMA._run_packed): row cu[b] + t is
// token t of prompt b. Everything but two steps of a layer works on a flat list of rows; these are the two.
//
// llj_rope_kv_packed: what the c_attn epilogue (EP_QKV in gemv_impl.h, the QKV epilogue of gemm.hip) does for
// rows of equal-length sequences, from c_attn's stored (M, 3C) output: RoPE on q and k at the row's own position
// t, q' into q_out[m], k' / v into slot t of cache row b. One block per packed row; the block finds its sequence
// by a binary search of cu (wave-uniform, <= 16 reads), then each lane takes 8 contiguous dims of q, k or v: one
// 16-byte load, for q / k two 16-byte loads of the RoPE row, fp32 arithmetic on the bf16 inputs, one rounding,
// one 16-byte store (llj_attention_ragged's first phase).
//
// llj_attention_prefill_packed: causal flash attention of one 64-query block of one sequence per workgroup; the
// tile list (b, qb) comes from the host, longest first. The body is the walk of flash_prefill_kernel<HS, 1, false,
// 4> (attention_prefill.hip, see there for the operand layout) at p0 = 0: the same 64-key tiles in ascending
// order, the same softmax and roundings, so every (sequence, query, head) output is bitwise what
// llj_attention_prefill(B = 1, T = T_b, pos = arange) gives on the same q rows and cache row.
//
// Containment, whatever cu and tiles hold on the device: sequence indices are clamped into [0, B - 1], row
// indices into [0, M - 1], lengths into [1, min(M - row, S)] and slots into [0, S - 1] (S <= rope_rows is
// host-checked), so no read or write leaves the (M, .) buffers, cache row b or the RoPE table. No atomics: the
// same inputs give the same bits on every run.
#include "common.h"
#include "lit_llama_amd.h"

#include <math.h>

namespace llj {

template <int HS>
__global__ __launch_bounds__(256) void rope_kv_packed_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ q_out,
                                                             bf16_t* __restrict__ kc, bf16_t* __restrict__ vc,
                                                             const float* __restrict__ rope,
                                                             const int* __restrict__ cu, int B, int S, int nh) {
  constexpr int LH = HS / 8;  // lanes per head
  const int m = blockIdx.x;
  // the last sequence whose first row is <= m (cu ascending; indices 1 .. B - 1 only are read)
  int lo = 0, hi = B - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (cu[mid] <= m) lo = mid;
    else hi = mid - 1;
  }
  const int b = lo;
  int t = m - cu[b];
  t = t < 0 ? 0 : (t > S - 1 ? S - 1 : t);
  const int C = nh * HS;
  const int per = C / 8;  // lanes per third of the row
  const bf16_t* row = qkv + (size_t)m * 3 * C;
  for (int item = threadIdx.x; item < 3 * per; item += 256) {
    const int part = item / per, rem = item - part * per;  // part 0 q, 1 k, 2 v
    const int h = rem / LH, j = rem - h * LH;
    const uint4 a = *reinterpret_cast<const uint4*>(row + (size_t)part * C + rem * 8);
    uint32_t w[4] = {a.x, a.y, a.z, a.w};
    if (part < 2) {
      // c_attn's bf16 output, RoPE in fp32 on interleaved pairs, one rounding (model.py:318-329; EP_QKV)
      const float* rp = rope + ((size_t)t * (HS / 2) + j * 4) * 2;  // (cos, sin) of this lane's 4 pairs
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const f32x4 cs = *reinterpret_cast<const f32x4*>(rp + 4 * i);
        const float a0 = bflo(w[2 * i]), a1 = bfhi(w[2 * i]);
        const float b0 = bflo(w[2 * i + 1]), b1 = bfhi(w[2 * i + 1]);
        w[2 * i] = pack2bf(a0 * cs[0] - a1 * cs[1], a1 * cs[0] + a0 * cs[1]);
        w[2 * i + 1] = pack2bf(b0 * cs[2] - b1 * cs[3], b1 * cs[2] + b0 * cs[3]);
      }
    }
    bf16_t* dst;
    if (part == 0)
      dst = q_out + (size_t)m * C + rem * 8;
    else
      dst = (part == 1 ? kc : vc) + (((size_t)b * nh + h) * S + t) * HS + j * 8;
    *reinterpret_cast<uint4*>(dst) = make_uint4(w[0], w[1], w[2], w[3]);
  }
}

constexpr int kPK = 64;  // keys per tile, queries per workgroup
typedef short pk_s16x4 __attribute__((ext_vector_type(4)));

template <int HS>
__global__ __launch_bounds__(256, 3) void flash_packed_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ kc,
                                                              const bf16_t* __restrict__ vc, bf16_t* __restrict__ y,
                                                              const int* __restrict__ cu,
                                                              const int* __restrict__ tiles, int B, int M, int S,
                                                              int nh, float sl2) {
  constexpr int KP = HS + 8;   // K tile pitch (elements): 16-B row reads
  constexpr int VP = HS + 16;  // V tile pitch: 8 rows x 4 lanes x 8 B of a transposed read on distinct banks
  constexpr int KS = HS / 32;  // MFMA k-steps over the head dim
  constexpr int DB = HS / 16;  // 16-row output blocks of O^T
  constexpr int NT = 256;
  __shared__ __attribute__((aligned(16))) bf16_t Ks[kPK * KP];
  __shared__ __attribute__((aligned(16))) bf16_t Vs[kPK * VP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, g = lane >> 4;
  const int h = blockIdx.y;
  // this workgroup's (sequence, query block), clamped so that nothing below leaves the buffers (all uniform)
  int b = tiles[2 * blockIdx.x], qb = tiles[2 * blockIdx.x + 1];
  b = b < 0 ? 0 : (b > B - 1 ? B - 1 : b);
  int r0 = cu[b];
  const int r1 = cu[b + 1];
  r0 = r0 < 0 ? 0 : (r0 > M - 1 ? M - 1 : r0);
  int T = r1 - r0;
  const int tcap = min(M - r0, S);
  T = T < 1 ? 1 : (T > tcap ? tcap : T);
  const int nqb = (T + kPK - 1) / kPK;
  qb = qb < 0 ? 0 : (qb > nqb - 1 ? nqb - 1 : qb);
  const int C = nh * HS;
  // Q^T fragments: lane holds Q[t][32 kk + 8 g .. + 8] (a row past T is computed on a copy, never stored)
  const int t = qb * kPK + wave * 16 + col;
  u32x4 qf[KS];
  {
    const int tq = t < T ? t : T - 1;
    const bf16_t* qrow = q + ((size_t)r0 + tq) * C + h * HS;
#pragma unroll
    for (int kk = 0; kk < KS; ++kk) qf[kk] = *reinterpret_cast<const u32x4*>(qrow + 32 * kk + 8 * g);
  }
  const int kmax = min(T, qb * kPK + kPK) - 1;  // last key any query of the block attends
  const int ntile = kmax / kPK + 1;
  const bf16_t* kbase = kc + (((size_t)b * nh + h) * S) * HS;
  const bf16_t* vbase = vc + (((size_t)b * nh + h) * S) * HS;
  // staging map: 64 keys x HS/8 vectors = 64 * HS / 8 16-B pieces over NT threads
  constexpr int PV = kPK * HS / 8 / NT;
  u32x4 kA[PV], vA[PV], kB[PV], vB[PV];
  auto load_into = [&](int kt, u32x4 (&kr)[PV], u32x4 (&vr)[PV]) {
#pragma unroll
    for (int i = 0; i < PV; ++i) {
      const int piece = tid + NT * i;
      const int key = piece / (HS / 8), v8 = piece % (HS / 8);
      int slot = kt * kPK + key;
      slot = slot <= kmax ? slot : kmax;  // clamped: masked below
      kr[i] = *reinterpret_cast<const u32x4*>(kbase + (size_t)slot * HS + 8 * v8);
      vr[i] = *reinterpret_cast<const u32x4*>(vbase + (size_t)slot * HS + 8 * v8);
    }
  };
  float m_run = -INFINITY, l_run = 0.f;
  f32x4 acc_o[DB];
#pragma unroll
  for (int d = 0; d < DB; ++d) acc_o[d] = f32x4{0.f, 0.f, 0.f, 0.f};
  // every wave takes every step of the walk, so the barriers and the transposing LDS reads run with all lanes
  auto step = [&](int kt, u32x4 (&kr)[PV], u32x4 (&vr)[PV], u32x4 (&kn)[PV], u32x4 (&vn)[PV]) {
    __syncthreads();  // the previous tile's readers are done with Ks / Vs
#pragma unroll
    for (int i = 0; i < PV; ++i) {
      const int piece = tid + NT * i;
      const int key = piece / (HS / 8), v8 = piece % (HS / 8);
      *reinterpret_cast<u32x4*>(Ks + key * KP + 8 * v8) = kr[i];
      *reinterpret_cast<u32x4*>(Vs + key * VP + 8 * v8) = vr[i];
    }
    __syncthreads();
    if (kt + 1 < ntile) load_into(kt + 1, kn, vn);  // in flight during this tile's MFMAs
    // S^T = K . Q^T for the tile's four 16-key blocks
    f32x4 s[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      s[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < KS; ++kk) {
        const bf16x8 a = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(Ks + (16 * j + col) * KP + 32 * kk + 8 * g));
        s[j] = mfma_bf16(a, __builtin_bit_cast(bf16x8, qf[kk]), s[j]);
      }
    }
    uint32_t pb[4][2];  // bf16 P^T pairs per key block: (r0, r1), (r2, r3)
    // only the tiles that reach past the wave's first query need the causal mask (wave-uniform)
    const bool masked = kt * kPK + kPK - 1 > qb * kPK + wave * 16;
    if (masked) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int key = kt * kPK + 16 * j + 4 * g + r;
          s[j][r] = key <= t ? s[j][r] : -INFINITY;
        }
    }
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) mx = fmaxf(mx, s[j][r]);
    {  // max over the 4 lane groups holding this query's keys (lanes col, col+16, col+32, col+48)
      float lo, hi;
      lane_halves<false>(mx, lo, hi);
      mx = fmaxf(lo, hi);
      lane_halves<true>(mx, lo, hi);
      mx = fmaxf(lo, hi);
    }
    // finite: key 0 of tile 0 is visible to every query, so no tile leaves m_new at -inf
    const float m_new = fmaxf(m_run, mx * sl2);
    const float corr = m_run == -INFINITY ? 0.f : exp2f(m_run - m_new);
    float psum = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float pr[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
#pragma clang fp contract(off)
        // the scaled score rounded before the subtraction (no fma contraction), v_exp_f32 directly
        const float sc = s[j][r] * sl2;
        pr[r] = __builtin_amdgcn_exp2f(sc - m_new);
        psum += pr[r];
      }
      pb[j][0] = pack2bf(pr[0], pr[1]);
      pb[j][1] = pack2bf(pr[2], pr[3]);
    }
    {
      float lo, hi;
      lane_halves<false>(psum, lo, hi);
      psum = lo + hi;
      lane_halves<true>(psum, lo, hi);
      psum = lo + hi;
    }
    l_run = l_run * corr + psum;
    m_run = m_new;
    if (__any(corr != 1.f)) {  // the running max moved for some query of the wave
#pragma unroll
      for (int d = 0; d < DB; ++d)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc_o[d][r] *= corr;
    }
    // O^T += V^T . P^T, two 32-key steps
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const u32x4 bw = {pb[2 * u][0], pb[2 * u][1], pb[2 * u + 1][0], pb[2 * u + 1][1]};
      const bf16x8 bfrag = __builtin_bit_cast(bf16x8, bw);
#pragma unroll
      for (int d = 0; d < DB; ++d) {
        // lane 4q + p of group g addresses keys 32u + 4g + q (+16), dims 16d + 4p .. +3; lane col
        // receives dim 16d + col of those 4 keys
        const bf16_t* vr = Vs + (32 * u + 4 * g + ((lane >> 2) & 3)) * VP + 16 * d + 4 * (lane & 3);
        const pk_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) pk_s16x4*)vr);
        const pk_s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) pk_s16x4*)(vr + 16 * VP));
        const uint2 l2 = __builtin_bit_cast(uint2, lo), h2 = __builtin_bit_cast(uint2, hi);
        const u32x4 aw = {l2.x, l2.y, h2.x, h2.y};
        acc_o[d] = mfma_bf16(__builtin_bit_cast(bf16x8, aw), bfrag, acc_o[d]);
      }
    }
  };
  load_into(0, kA, vA);
  for (int kt = 0; kt < ntile; kt += 2) {
    step(kt, kA, vA, kB, vB);
    if (kt + 1 < ntile) step(kt + 1, kB, vB, kA, vA);
  }
  // y[r0 + t][h*HS + d] = O / l; lane holds d = 16 db + 4 g + r of its query
  if (t < T) {
    const float inv = 1.f / l_run;
    bf16_t* yrow = y + ((size_t)r0 + t) * C + h * HS;
#pragma unroll
    for (int d = 0; d < DB; ++d) {
      const uint2 o = make_uint2(pack2bf(acc_o[d][0] * inv, acc_o[d][1] * inv),
                                 pack2bf(acc_o[d][2] * inv, acc_o[d][3] * inv));
      *reinterpret_cast<uint2*>(yrow + 16 * d + 4 * g) = o;
    }
  }
}

}  // namespace llj

using namespace llj;

extern "C" {

int llj_rope_kv_packed(const void* qkv, void* q_out, void* kcache, void* vcache, const float* rope, const int* cu,
                       int B, int M, int n_head, int head_size, int S, int rope_rows, void* stream) {
  LLJ_REQUIRE(qkv && q_out && kcache && vcache && rope && cu);
  LLJ_REQUIRE(head_size == 64 || head_size == 128);
  LLJ_REQUIRE(B >= 1 && B <= 65535 && M >= B);
  LLJ_REQUIRE(n_head >= 1 && S >= 1 && rope_rows >= 1 && S <= rope_rows);
  hipStream_t s = (hipStream_t)stream;
  if (head_size == 128)
    hipLaunchKernelGGL((rope_kv_packed_kernel<128>), dim3(M), dim3(256), 0, s, (const bf16_t*)qkv, (bf16_t*)q_out,
                       (bf16_t*)kcache, (bf16_t*)vcache, rope, cu, B, S, n_head);
  else
    hipLaunchKernelGGL((rope_kv_packed_kernel<64>), dim3(M), dim3(256), 0, s, (const bf16_t*)qkv, (bf16_t*)q_out,
                       (bf16_t*)kcache, (bf16_t*)vcache, rope, cu, B, S, n_head);
  LLJ_CHECK_LAUNCH();
  return 0;
}

int llj_attention_prefill_packed(const void* q, const void* kcache, const void* vcache, void* y, const int* cu,
                                 const int* tiles, int n_tiles, int B, int M, int n_head, int head_size, int S,
                                 void* stream) {
  LLJ_REQUIRE(q && kcache && vcache && y && cu && tiles);
  LLJ_REQUIRE(head_size == 64 || head_size == 128);
  LLJ_REQUIRE(B >= 1 && B <= 65535 && M >= B);
  LLJ_REQUIRE(n_head >= 1 && n_head <= 65535 && S >= 1 && n_tiles >= 1);  // (n_head: grid dimension y)
  const float sl2 = 1.4426950408889634f / sqrtf((float)head_size);
  const dim3 grid(n_tiles, n_head);
  hipStream_t s = (hipStream_t)stream;
  if (head_size == 128)
    hipLaunchKernelGGL((flash_packed_kernel<128>), grid, dim3(256), 0, s, (const bf16_t*)q, (const bf16_t*)kcache,
                       (const bf16_t*)vcache, (bf16_t*)y, cu, tiles, B, M, S, n_head, sl2);
  else
    hipLaunchKernelGGL((flash_packed_kernel<64>), grid, dim3(256), 0, s, (const bf16_t*)q, (const bf16_t*)kcache,
                       (const bf16_t*)vcache, (bf16_t*)y, cu, tiles, B, M, S, n_head, sl2);
  LLJ_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
