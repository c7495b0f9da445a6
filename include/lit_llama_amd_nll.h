/* Scoring entry points of _lljamd.so: part of the C ABI of lit_llama_amd.h, which includes this file
 * (same conventions: every function returns 0, a hipError_t, or LLJ_EINVAL; `stream` is a hipStream_t).
 * Kept in a header of its own, as lit_llama_amd_lora.h is, so that lit_llama_amd.h's declaration list
 * stays what it was. */
#ifndef LIT_LLAMA_AMD_NLL_H
#define LIT_LLAMA_AMD_NLL_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- per-token negative log-likelihood
 * The scoring step of the evaluate scripts (reference evaluate/full.py:121-123 before its sum):
 *   row_nll[m] = logsumexp(logits[m, 0:V]) - logits[m, targets[m]]
 * in fp32 on the exactly converted bf16 logits (M, V), row stride ldl >= V of any value. One block of
 * 256 threads per row; the row is read once with an online (max, sum) per thread and a block combine,
 * with 16-byte loads when the base pointer and ldl allow them and an element path otherwise; columns
 * >= V are never read. The maximum is subtracted, so logits of +-80 do not overflow.
 *   targets[m] < 0    the row is ignored: row_nll[m] = 0, not counted, not read
 *   targets[m] >= V   row_nll[m] = NaN, nothing is read
 *   a -inf logit      adds 0 to the sum (also as the first value a thread sees)
 *   a NaN logit       makes its row NaN
 * total (may be NULL): a second launch of one block on the same stream adds the M values in a fixed
 * order in double, total[0] += the sum over the counted rows, total[1] += the rows counted -- stream
 * order lets a caller score many windows and read the pair once. No floating-point atomics anywhere:
 * the same inputs give the same bits on every run.
 * NULL logits / targets / row_nll, M <= 0, V <= 0 or ldl < V: LLJ_EINVAL. */
int llj_nll(const void* logits, int ldl, int M, int V, const int* targets, float* row_nll, double* total,
            void* stream);
/* The same over fp32 logits (the float32 model, on the any-shape path), as llj_g_argmax is to llj_argmax. */
int llj_g_nll(const float* logits, int ldl, int M, int V, const int* targets, float* row_nll, double* total,
              void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LIT_LLAMA_AMD_NLL_H */
