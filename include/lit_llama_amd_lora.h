/* LoRA entry points of _lljamd.so: part of the C ABI of lit_llama_amd.h, which includes this file
 * (same conventions: every function returns 0, a hipError_t, or LLJ_EINVAL; `stream` is a hipStream_t).
 * Kept in a header of its own so that lit_llama_amd.h's declaration list stays what it was. */
#ifndef LIT_LLAMA_AMD_LORA_H
#define LIT_LLAMA_AMD_LORA_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- LoRA (inference)
 * The reference's LoRA (lit_llama/lora.py) gives c_attn two low-rank matrices over the enabled ones
 * of its three output groups q, k, v (enable_lora; n_en = their count):
 *   lora_A (r * n_en, K)          one r-row slab per enabled group, in group order
 *   lora_B (n_en * N / 3, r)      one N / 3-row slab per enabled group
 * and scaling = lora_alpha / r. enable_mask: bit g set = group g enabled (1..7).
 *
 * llj_lora_merge: the reference's eval-time merge (lora.py:241-278) in place on the dense weight
 * W (N, K) row-major, N % 3 == 0, dt 0 bf16 / 1 fp32 (W, A and B of that type):
 *   W[n, k] += sign * round(scaling * round(sum_j B[n', j] * A[g_i * r + j, k]))
 * for the rows n of enabled groups (g_i: the group's index among the enabled ones, n' its row of
 * lora_B), sign +1 (merge) or -1 (unmerge); round = to W's type at the reference's three points
 * (the conv1d output, the product with scaling, the sum). Rows of disabled groups are not touched.
 * 1 <= r <= 64. */
int llj_lora_merge(void* W, const void* lora_A, const void* lora_B, int N, int K, int r, int enable_mask,
                   float scaling, int sign, int dt, void* stream);
/* The unmerged forward (lora.py:310-323) of the ops that produce c_attn's output: the op of the same
 * name, with the low-rank term added to the Linear's own rounded output y before the epilogue
 * consumes it (RoPE, the q store and the KV write; the store):
 *   d = bf16(sum_j t[m, g_i * r + j] * B[n', j]);   y = bf16(y + bf16(d * scaling))
 * for the columns of enabled groups; columns of disabled groups are bitwise the base op's. lora_t
 * (rows x ldt, the activation type) = the down-projection x_n . lora_A^T of the same rows, computed
 * by the caller with the existing Linear ops (row m of lora_t belongs to row m of the call: for the
 * QKV ops, global row row0 + m is at lora_t + (row0 + m) * ldt); lora_B as above, contiguous.
 * All of lora_t, lora_B NULL (and r 0) = the op above; a partial set, r outside 1..64, an empty or
 * out-of-range mask = LLJ_EINVAL. wfmt 0 (with and without LLJ_WF_ZINT), 1, 3 and grouped int4;
 * wfmt 2 (LLM.int8) returns LLJ_EINVAL. In fp32 (llj_g_linear_lora, dt 1) the expression is
 * evaluated as written. */
int llj_norm_qkv_rope_lora(int wfmt, const void* x, const void* norm_w, float eps, const void* W, const void* sz,
                           void* q_out, void* kcache, void* vcache, const float* rope, const int* pos, int B, int T,
                           int C, int n_head, int S, int row0, int rows, const void* i8ws, const float* rowsum,
                           const float* nstat, int npart, void* stream, const void* lora_t, int ldt,
                           const void* lora_B, int r, int enable_mask, float scaling);
int llj_gemm_qkv_rope_lora(int wfmt, const void* x, const void* W, const void* sz, void* q_out, void* kcache,
                           void* vcache, const float* rope, const int* pos, int B, int T, int C, int n_head, int S,
                           void* stream, const void* lora_t, int ldt, const void* lora_B, int r, int enable_mask,
                           float scaling);
/* llj_g_linear with the term (any shape with N % 3 == 0, bf16 or fp32, wkind 0 / 1; no residual). */
int llj_g_linear_lora(int wkind, const void* x, int ldx, int M, int K, const void* W, const float* scales,
                      const float* zeros, int bits, int group, int N, void* y, int ldy, const void* resid, int ldr,
                      int dt, void* stream, const void* lora_t, int ldt, const void* lora_B, int r, int enable_mask,
                      float scaling);

#ifdef __cplusplus
}
#endif

#endif /* LIT_LLAMA_AMD_LORA_H */
