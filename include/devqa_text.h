/* C ABI of the sentence-encoder kernels of libdevqa_hip.so (csrc/text_ops.hip): the two ends of a BERT-family text tower.
 * The middle of the tower (q|k|v / output / feed-forward GEMMs, LayerNorm with an add, packed attention) is include/devqa.h.
 *
 * Conventions are those of devqa.h: every function returns 0 or a negative DEVQA_E_* code, never throws, never synchronises
 * the device; the message of the last failure is in the library's error string; `stream` is a hipStream_t; null pointers and
 * unsupported dimensions are rejected on the host before anything is launched.
 */
#ifndef DEVQA_TEXT_H
#define DEVQA_TEXT_H
#include "devqa.h"

#ifdef __cplusplus
extern "C" {
#endif

/* BertEmbeddings in one pass: for row r
 *     e = (word[token[r]] + type0) + position[pos[r]]            (fp32 sums of the table values)
 *     y = (e - mean(e)) * rsqrt(var(e) + eps) * gamma + beta      (two-pass statistics, biased variance, as nn.LayerNorm)
 * token, pos int32 [R]; word [V, D], position [P, D], type0 [D] (row 0 of token_type_embeddings) in the table dtype;
 * gamma, beta fp32 [D].  out_f32 fp32 [R, D] (the residual stream) and / or out_bf16 [R, D] (the next GEMM's operand, the
 * fp32 value rounded to nearest even); at least one of the two.  D % 4 == 0, D <= 4096.
 * The caller checks 0 <= token[r] < V and 0 <= pos[r] < P on the host; the kernel clamps an index outside its table. */
int devqa_text_embed_ln(const int32_t* token, const int32_t* pos, const devqa_bf16* word, const devqa_bf16* position,
                        const devqa_bf16* type0, const float* gamma, const float* beta, int R, int D, int V, int P, float eps,
                        devqa_bf16* out_bf16, float* out_f32, void* stream);
int devqa_text_embed_ln_f32(const int32_t* token, const int32_t* pos, const float* word, const float* position,
                            const float* type0, const float* gamma, const float* beta, int R, int D, int V, int P, float eps,
                            devqa_bf16* out_bf16, float* out_f32, void* stream);

/* Sentence pooling over packed rows: x fp32 [R, D]; sequence s owns rows [seq_start[s], seq_start[s] + seq_len[s])
 * (int32 [S] each, device; rows at or beyond R are not read).  out fp32 [S, D]:
 *     DEVQA_POOL_MEAN  sum of the rows / max(seq_len, 1e-9)        (sentence-transformers Pooling, every token counted)
 *     DEVQA_POOL_CLS   the first row (zeros for an empty sequence)
 *     DEVQA_POOL_MAX   column maximum, starting from -inf (an empty sequence gives -inf)
 * normalize != 0: out[s] /= max(||out[s]||_2, 1e-12) (sentence-transformers Normalize; a zero row stays zero); an empty sequence
 * (seq_len <= 0, or no row below R) is not rescaled: it keeps its zeros (mean, cls) or its -inf (max), never NaN.
 * A column is reduced in a fixed order (up to four interleaved row groups, each in ascending row order, combined in group order)
 * and the norm in a fixed tree: no atomics, the same bits on every run.  D % 4 == 0. */
#define DEVQA_POOL_MEAN 0
#define DEVQA_POOL_CLS 1
#define DEVQA_POOL_MAX 2
int devqa_seq_pool(const float* x, const int32_t* seq_start, const int32_t* seq_len, int R, int S, int D, int mode, int normalize,
                   float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
