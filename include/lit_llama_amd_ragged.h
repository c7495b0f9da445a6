/* Entry point for decoding prompts of different lengths as one batch, part of the C ABI of lit_llama_amd.h,
 * which includes this file (same conventions: every function returns 0, a hipError_t, or LLJ_EINVAL; `stream`
 * is a hipStream_t). Kept in a header of its own, as lit_llama_amd_lora.h, lit_llama_amd_nll.h and
 * lit_llama_amd_samples.h are, so that lit_llama_amd.h's declaration list stays what it was. */
#ifndef LIT_LLAMA_AMD_RAGGED_H
#define LIT_LLAMA_AMD_RAGGED_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- decode attention at a position per row
 * B decode rows (one per sequence, T = 1) that share the step counter *pos (device) but each stand at a position
 * of their own: row b at p = *pos - off[b], off: B int32 on the device. One launch, one workgroup per (row,
 * head), does RoPE, the KV write and the attention of that row:
 *   qkv: (B, 3 * C) bf16, c_attn's output, C = n_head * head_size; q_out, y: (B, C) bf16;
 *   kcache, vcache: (B, n_head, S, head_size) bf16; rope: (rope_rows, head_size / 2, 2) fp32 [cos, sin].
 *   q' = bf16(rope(q, p)), k' = bf16(rope(k, p)) on interleaved pairs, fp32 arithmetic on the bf16 inputs and one
 *   rounding (as llj_norm_qkv_rope's epilogue and llj_g_rope_kv); q_out[b, h] = q', kcache[b, h, p] = k',
 *   vcache[b, h, p] = v; y[b, h] = bf16(softmax(q' . K[0..p] / sqrt(head_size)) . V[0..p]) with K[p], V[p] the
 *   bf16 values just written: fp32 scores, a max-subtracted softmax, llj_attention's arithmetic up to summation
 *   order.
 * The caller guarantees 0 <= p < S for every row (the ring never wraps); p is clamped into [0, S - 1] on the
 * device whatever *pos and off hold, so no read or write leaves row b's cache rows, the RoPE table or the (B, C)
 * buffers. No slot above p is read, no slot but p written, no other row touched. No atomics: the same inputs
 * give the same bits on every run.
 * LLJ_EINVAL before any launch: a NULL pointer other than stream, head_size not 64 or 128, B < 1 or > 65535,
 * n_head < 1, S < 1, rope_rows < 1, S > rope_rows. */
int llj_attention_ragged(const void* qkv, void* q_out, void* kcache, void* vcache, void* y, const float* rope,
                         const int* pos, const int* off, int B, int n_head, int head_size, int S, int rope_rows,
                         void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LIT_LLAMA_AMD_RAGGED_H */
