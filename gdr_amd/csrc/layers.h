// Internal launchers of the embed, pack, gather / scatter and norm kernels (layers.hip), shared by encoder.hip / bert.hip / decode.hip.
// The attention family has a header of its own (attention.h).
#pragma once
#include "common.h"

namespace gdr {

int launch_embed(const float* table, const int64_t* ids, int64_t rows, int d, int vocab, float* out,
                 hipStream_t stream);
// Ragged batches (encoder.hip): which token rows of a [B,L] batch are computed at all.
//   seq_len[b] = number of leading ones of mask row b when the row is a non-empty prefix of ones (right padding, what the
//                tokenizer produces), else L: such a sequence keeps all its positions and its mask (a fully masked row
//                attends uniformly over PAD keys too, modeling_utils.py:271-272, so nothing of it may be dropped);
//   seq_off[b] = exclusive prefix sum (seq_off[B] = total), row_src[r] = b*L + pos of packed row r, *rows_total = total.
int launch_pack_plan(const int64_t* mask, int B, int L, int32_t* seq_len, int32_t* seq_off, int32_t* row_src,
                     int64_t* rows_total, hipStream_t stream);
// out[r] = table[ids[row_src[r]]] for r < *rows_dev (grid sized for max_rows)
int launch_embed_packed(const float* table, const int64_t* ids, const int32_t* row_src, const int64_t* rows_dev,
                        int64_t max_rows, int d, int vocab, float* out, hipStream_t stream);
// the same gather from two tables by one token id: out2[r] = table2[ids[row_src[r]]] (rows of e floats) beside out[r]
int launch_embed_packed2(const float* table, const float* table2, const int64_t* ids, const int32_t* row_src,
                         const int64_t* rows_dev, int64_t max_rows, int d, int e, int vocab, float* out, float* out2,
                         hipStream_t stream);
// dst[i] = src[idx[i]] (rows of d floats), i < n
int launch_gather_rows(const float* src, const int32_t* idx, int n, int d, float* dst, hipStream_t stream);
// dst[idx[i]] = src[i] (dense rows of d floats into rows of dst that are ldd floats apart), i < n
int launch_scatter_rows_strided(const float* src, const int32_t* idx, int n, int d, float* dst, int64_t ldd, hipStream_t stream);
// dst[row_src[r]] = src[r] for r < *rows_dev: packed rows back into the [B*L, d] layout (dst pre-zeroed by the caller)
int launch_scatter_rows(const float* src, const int32_t* row_src, const int64_t* rows_dev, int64_t max_rows, int d,
                        float* dst, hipStream_t stream);
// y = x / sqrt(mean(x^2) + eps) * w     (T5LayerNorm, modeling_t5.py:164-171); optional second output
// `pooled` receives rows r with r % pool_every == 0 (CLS pool h[:,0]) when non-null.
// y16 (optional, everywhere below): the same output once more, rounded to bf16 (RNE) — the operand of a bf16-mode linear
int launch_rmsnorm(const float* x, const float* w, float* y, int64_t rows, int d, float eps, float* pooled,
                   int pool_every, hipStream_t stream, void* y16 = nullptr);
// x[b, j, :] = 0 for j >= seq_len[b]  (x is [B, L, d])
int launch_zero_dead_rows(float* x, const int32_t* seq_len, int B, int L, int d, hipStream_t stream);
// same over the first *rows_dev rows (a device-side count; the grid is sized for max_rows)
int launch_rmsnorm_dev(const float* x, const float* w, float* y, const int64_t* rows_dev, int64_t max_rows, int d, float eps,
                       hipStream_t stream, void* y16 = nullptr);
// the split-bf16 form's operand: y (nullable) fp32 rows; planes bf16 [rows, ld >= 3 d], a row = [hi | mid | lo] of the normed row
int launch_rmsnorm_planes(const float* x, const float* w, float* y, void* planes, int64_t ld, const int64_t* rows_dev, int64_t max_rows,
                          int d, float eps, hipStream_t stream, int f16x2 = 0);  // f16x2: rows [fp16 hi | fp16 (x - hi) * 2^11], ld >= 2 d
// same, output rounded to bf16 (RNE): the activation operand of a bf16-mode linear
int launch_rmsnorm_bf16(const float* x, const float* w, void* y_bf16, int64_t rows, int d, float eps, hipStream_t stream);
int launch_rmsnorm_bf16_dev(const float* x, const float* w, void* y_bf16, const int64_t* rows_dev, int64_t max_rows, int d,
                            float eps, hipStream_t stream);
// y = (x - mean) / sqrt(var + eps) * w + b   (torch.nn.LayerNorm; BERT / nn.TransformerDecoderLayer)
// optional addv [d]: y = LN(x + addv)  (the adaptor's constant single-key cross-attention output)
// f16x2_ld != 0: y16 receives plane rows [fp16 hi | fp16 (y - hi) * 2^11] of f16x2_ld >= 2 d elements (the fp16 x 2 split form's operand)
int launch_layernorm(const float* x, const float* w, const float* b, float* y, int64_t rows, int d, float eps,
                     const float* addv, hipStream_t stream, void* y16 = nullptr, int f16x2_ld = 0);
int launch_layernorm_dev(const float* x, const float* w, const float* b, float* y, const int64_t* rows_dev, int64_t max_rows,
                         int d, float eps, const float* addv, hipStream_t stream, void* y16 = nullptr, int f16x2_ld = 0);
// y = LN(LN(x; w1, b1) + addv; w2, b2) in one pass (bit-identical to the two launches); rows_dev may be null (= max_rows rows);
// returns 1 when d > 2048 (not served: run the two launches)
int launch_layernorm2(const float* x, const float* w1, const float* b1, const float* w2, const float* b2, const float* addv, float* y,
                      const int64_t* rows_dev, int64_t max_rows, int d, float eps, hipStream_t stream, void* y16 = nullptr);

}  // namespace gdr
