/* Entry points for prefilling prompts of different lengths as one packed batch, part of the C ABI of
 * lit_llama_amd.h, which includes this file (same conventions: every function returns 0, a hipError_t, or
 * LLJ_EINVAL; `stream` is a hipStream_t). Kept in a header of its own, as lit_llama_amd_lora.h, lit_llama_amd_nll.h,
 * lit_llama_amd_samples.h and lit_llama_amd_ragged.h are, so that lit_llama_amd.h's declaration list stays what it
 * was. */
#ifndef LIT_LLAMA_AMD_PACKED_H
#define LIT_LLAMA_AMD_PACKED_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- packed prefill: B sequences in M rows
 * B prompts of T_b >= 1 tokens are concatenated into M = sum T_b rows: row cu[b] + t is token t of prompt b.
 *   cu: B + 1 int32 on the device, cu[0] = 0, cu[b + 1] - cu[b] = T_b, cu[B] = M;
 *   kcache, vcache: (B, n_head, S, head_size) bf16; rope: (rope_rows, head_size / 2, 2) fp32 [cos, sin];
 *   C = n_head * head_size. bf16 throughout, head_size 64 or 128.
 * Whatever cu and tiles hold on the device, nothing is read or written outside the buffers: sequence indices
 * are clamped into [0, B - 1], rows into [0, M - 1], slots into [0, min(S, rope_rows) - 1]. The caller
 * guarantees T_b <= S. No atomics: the same inputs give the same bits on every run.
 * LLJ_EINVAL before any launch: a NULL pointer other than stream, head_size not 64 or 128, B < 1 or > 65535,
 * M < B, n_head < 1, S < 1, n_tiles < 1, rope_rows < 1, S > rope_rows. */

/* RoPE and the KV write of the packed rows from c_attn's stored output qkv (M, 3 * C): for row m = cu[b] + t
 *   q' = bf16(rope(q, t)), k' = bf16(rope(k, t)) on interleaved pairs, fp32 arithmetic on the bf16 inputs and one
 *   rounding (as llj_norm_qkv_rope's epilogue and llj_attention_ragged); q_out[m, h] = q' (q_out: (M, C)),
 *   kcache[b, h, t] = k', vcache[b, h, t] = v. Exactly the slots [0, T_b) of cache row b are written. */
int llj_rope_kv_packed(const void* qkv, void* q_out, void* kcache, void* vcache, const float* rope, const int* cu,
                       int B, int M, int n_head, int head_size, int S, int rope_rows, void* stream);

/* Causal attention of the packed rows, each over the slots 0 .. t of its own sequence's cache row: q, y (M, C).
 *   tiles: (n_tiles, 2) int32 on the device, (b, qb): the 64-query block qb < ceil(T_b / 64) of sequence b, each
 *   exactly once, in any order (the launch starts them in list order: longest first balances the causal work).
 * One workgroup per (tile, head) walks 64-key tiles in ascending order exactly as llj_attention_prefill does, so
 * the rows of sequence b are bitwise those of llj_attention_prefill(B = 1, T = T_b, pos = 0 .. T_b - 1) on the
 * same q rows and cache row. No slot >= T_b and no other sequence's cache row is read. */
int llj_attention_prefill_packed(const void* q, const void* kcache, const void* vcache, void* y, const int* cu,
                                 const int* tiles, int n_tiles, int B, int M, int n_head, int head_size, int S,
                                 void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LIT_LLAMA_AMD_PACKED_H */
