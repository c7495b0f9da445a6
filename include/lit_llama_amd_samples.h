/* Entry points for sampling one prompt many times, part of the C ABI of lit_llama_amd.h, which includes this
 * file (same conventions: every function returns 0, a hipError_t, or LLJ_EINVAL; `stream` is a hipStream_t).
 * Kept in a header of its own, as lit_llama_amd_lora.h and lit_llama_amd_nll.h are, so that lit_llama_amd.h's
 * declaration list stays what it was. */
#ifndef LIT_LLAMA_AMD_SAMPLES_H
#define LIT_LLAMA_AMD_SAMPLES_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- decode attention over a shared prompt prefix
 * B decode rows (one per sequence, T = 1) whose caches hold the same first P keys / values (one prompt, prefilled
 * once and copied: DecodeSession.prefill_shared). q, y: (B, n_head * head_size) bf16; kcache, vcache:
 * (B, n_head, S, head_size) bf16 as for llj_attention; *pos: the rows' common position p on the device.
 * Row b attends keys 0 .. p: keys j < P are read from row 0's cache only (the other rows' slots below P are
 * never touched), once per head for a group of up to 8 rows; keys P <= j <= p from row b's own cache. Same
 * arithmetic as llj_attention up to summation order: fp32 scores scaled by 1 / sqrt(head_size), a
 * max-subtracted softmax over all p + 1 keys, y = bf16(O / L).
 * The prefix keys are split into nsplit equal ranges (1 <= nsplit <= 64; each at least 64 keys, so ranges past
 * P stay empty) of one block each per (head, row group); the keys [P, p] of every (row, head) are one more
 * block. Each writes an unnormalized partial (outputs, max, sum) into ws, nsplit + 1 records of
 * (head_size + 4) floats per (row, head), merged in record order by a second launch. No atomics: the same
 * inputs give the same bits on every run.
 * The caller guarantees P - 1 <= p < S (the ring has not wrapped); the position is not known on the host, and
 * the kernel clamps every read into the cache whatever it holds.
 * ws: llj_attention_shared_ws_bytes(B, n_head, head_size, nsplit) bytes, written whole apart from two pad
 * floats per record.
 * LLJ_EINVAL before any launch: NULL q / kcache / vcache / y / pos / ws, head_size not 64 or 128, B < 1 or
 * > 65535, n_head < 1, P < 1, P > S, nsplit < 1 or > 64. */
size_t llj_attention_shared_ws_bytes(int B, int n_head, int head_size, int nsplit);
int llj_attention_shared(const void* q, const void* kcache, const void* vcache, void* y, const int* pos, int B,
                         int P, int n_head, int head_size, int S, int nsplit, void* ws, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LIT_LLAMA_AMD_SAMPLES_H */
