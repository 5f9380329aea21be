// The attention family's internal interface: the arguments and launchers that encoder.hip / bert.hip / decode.hip call, and the
// device helpers that the kernels of attention.hip (one-pass forms; the two MFMA self-attention kernels keep their bodies written out) and
// attention_long.hip (key-block walk) are written on — T5's
// relative-position bucket, the allowed-key term, the softmax over MFMA score fragments, the fp32 score tiles, the exact
// bf16 x 3 split of a probability and the context store, each defined once.
#pragma once
#include <math.h>

#include "common.h"

namespace gdr {

// T5 relative-position bucket of distance n = query_pos - key_pos >= 0 for n in [0,128); distances
// >= 128 saturate to the last bucket (reference modeling_t5.py:242-288, max_distance hard-coded 128).
struct BucketLut {
  uint8_t v[128];
};
// nb = buckets per direction (num_buckets/2 when bidirectional, num_buckets otherwise).
BucketLut make_bucket_lut(int nb, int max_distance);

struct AttnArgs {
  const float* q;  // row (b*q_bstride + i), head h at column h*dk
  const float* k;  // row (b*k_bstride + j)
  const float* v;
  float* out;      // row (b*o_bstride + i), head h at column h*dk
  void* out_bf16;  // when non-null the context is written here as bf16 (same indexing, ldo in elements) instead of `out`:
                   // it only feeds the next linear of the bf16 precision mode (every kernel form).
  int64_t ldq, ldk, ldv, ldo;          // row strides in floats
  int64_t q_bstride, k_bstride, o_bstride;  // rows per batch entry
  int B, H, dk, Lq, Lk;
  int q_pos0;                  // absolute position of query row 0 (decode with cache)
  float scale;                 // 1.0 for T5 (modeling_t5.py:384-386), hd^-0.5 for nn.MultiheadAttention
  const float* rel_bias;       // [num_buckets, H] or null
  int bidirectional, num_buckets;
  BucketLut lut;
  const int64_t* key_mask;     // int64 [B, Lk] (1 = attend) or null  -> adds (1-m)*-1e9
  int64_t mask_bstride;        // elements between batch entries of key_mask
  int causal;                  // key j allowed iff j <= q_pos0 + i  -> adds -1e9 otherwise (neg_inf: -inf)
  int causal_neg_inf;          // nn.Transformer masks use -inf (modeling_t5.py:1622-1627)
  // decode-time K/V sources (defaults: kv_rows = null, kv_group = 1)
  const int32_t* kv_rows;      // int32 [B, Lk]: absolute row of key j of batch entry b in k/v (beam-ancestor cache)
  int kv_group;                // batch entries sharing one K/V block: K/V batch index = b / kv_group (beams of a query)
  int q_same_pos;              // all Lq query rows of a batch entry sit at position q_pos0 (beam rows of one decode step)
  // packed (ragged) self-attention: batch entry b owns rows seq_off[b] .. seq_off[b] + seq_len[b] - 1 of q/k/v/out
  // (instead of b*bstride + i) and attends over its seq_len[b] keys; Lq = Lk = the longest possible sequence.  Only the
  // dk = 64 full self-attention forms read these: attention_mfma16_kernel, attention_mfma_bf16_kernel and, above 128 keys,
  // attention_long_f32_kernel / attention_long_bf16_kernel.
  const int32_t* seq_off;
  const int32_t* seq_len;
  int qkv_bf16;                // q, k, v point to bf16 data (ldq / ldk / ldv in bf16 elements): the qkv linear of the bf16
                               // precision mode emits them so; the same four d_kv = 64 self-attention kernels only
  const int64_t* b_count_dev;  // Lq = 1 decode form only, may be null: only batch entries b < *b_count_dev are computed
  // q left as split-K slabs by the projection in front (common.h SlabRef; the generic kernel and the key-block cross form): when
  // q_part != null the query element (row m, column n) is the sum over s < q_S of the slabs, in order, and `q` is not read
  const float* q_part;
  int q_S, q_tiles_n;
  // decode only, may be null: the generate call's "some query is still undecided" word (common.h StreamK::live); 0 = every
  // query is done (generation_utils.py:836-838), the launch exits at once — its output is never read
  const int32_t* live;
};
int launch_attention(const AttnArgs& a, hipStream_t stream);
// input tokens per sequence in every T5 entry point (encoder forms, generate): what launch_attention serves (ops.T5_MAX_LEN)
constexpr int T5_MAX_LEN = 512;
// attention_long.hip: d_kv = 64 full self-attention over 128 < Lk <= 512 keys (key-block walk, online softmax), fp32 or bf16 q / k / v,
// padded or packed layout; with rel_bias (the T5 encoder) fp32 only.  Reached through launch_attention only, which checks the form and
// opens the ProfScope.
int launch_attention_long(const AttnArgs& a, hipStream_t stream);
// the same walk for the Lq >= 1 beam rows of a decode step (q_same_pos) against 128 < Lk <= 512 encoder keys, d_kv = 64, fp32
int launch_attention_long_cross(const AttnArgs& a, hipStream_t stream);

// ------------------------------------------------------------------------------------------ shared arithmetic
// T5's bucket of n = query position - key position (modeling_t5.py:242-288) through the 128-entry table; the host table of
// gdr_t5_relative_bucket_table, which tests/test_host_logic.py pins against the reference, is this function too.
__host__ __device__ __forceinline__ int rel_bucket(const AttnArgs& a, int n) {
  int bucket = 0;
  if (a.bidirectional) {
    if (n < 0) {
      bucket = a.num_buckets >> 1;
      n = -n;
    }
  } else if (n < 0) {
    n = 0;
  }
  return bucket + a.lut.v[n < 127 ? n : 127];
}

// what a key that may not be attended adds to its score, once: the additive fp32 mask of modeling_utils.py:271-272, or nn.Transformer's -inf
__device__ __forceinline__ float masked_term(const AttnArgs& a) { return a.causal_neg_inf ? -INFINITY : -1e9f; }

// The additive term of key j (of K / V batch entry kb) for head h of a query at position i_abs: the position bias
// bias[bucket * bias_ld + h] (rel_bias itself, or a workgroup's LDS copy of its head's column), then one masked term when the key lies
// behind the causal edge or its mask word is 0 — (bias + mask) before the score, as the reference (modeling_t5.py:399-400).
__device__ __forceinline__ float key_term(const AttnArgs& a, const float* bias, int bias_ld, int h, int kb, int j, int i_abs) {
  float add = 0.f;
  if (a.rel_bias) add = bias[rel_bucket(a, i_abs - j) * bias_ld + h];
  bool allowed = true;
  if (a.causal) allowed = j <= i_abs;
  if (a.key_mask) allowed = allowed && (a.key_mask[(int64_t)kb * a.mask_bstride + j] != 0);
  if (!allowed) add += masked_term(a);
  return add;
}

// The context of four adjacent columns at element offset off: fp32 rows, or bf16 (RNE) for the next linear of the bf16 mode.
__device__ __forceinline__ void store_ctx4(const AttnArgs& a, int64_t off, float4 o) {
  if (a.out_bf16)
    *reinterpret_cast<uint2*>(static_cast<__bf16*>(a.out_bf16) + off) = pack_bf16x4(o.x, o.y, o.z, o.w);
  else
    *reinterpret_cast<float4*>(a.out + off) = o;
}

// ------------------------------------------------------------------------------------------ MFMA score fragments
// Every MFMA form computes S^T = K.Q^T in 16x16 tiles, so lane (c16 = lane & 15, q4 = lane >> 4) holds, in st[t][r], the score of
// key 16t + 4q4 + r for ONE query (c16 of its wave's tile): a query's row is spread over the four lanes of equal c16.
__device__ __forceinline__ float quad_max(float v) {
  v = fmaxf(v, __shfl_xor(v, 16));
  return fmaxf(v, __shfl_xor(v, 32));
}
__device__ __forceinline__ float quad_sum(float v) {
  v += __shfl_xor(v, 16);
  return v + __shfl_xor(v, 32);
}

// One-pass softmax over NT tiles: st[t][r] += add(t, r), then the probabilities ex(s - max) stay in st (unnormalised: the B operand of
// the P.V MFMAs as they stand) and 1 / sum is returned.
template <int NT, class Add, class Exp>
__device__ __forceinline__ float frag_softmax(f32x4_t (&st)[NT], Add add, Exp ex) {
  float mx = -INFINITY;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float s = st[t][r] + add(t, r);
      st[t][r] = s;
      mx = fmaxf(mx, s);
    }
  }
  mx = quad_max(mx);
  float sum = 0.f;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float p = ex(st[t][r] - mx);  // padded keys: exp(-inf) = 0
      st[t][r] = p;
      sum += p;
    }
  }
  return 1.0f / quad_sum(sum);
}

// fp32 S^T tiles on v_mfma_f32_16x16x4_f32, d_kv = 64: A = K rows (keys) of an LDS image with rows of 68 floats (conflict-free
// ds_read_b128), B = this lane's query fragments qv[jj] = Q[query c16][16jj + 4q4 .. +3]; the d index is permuted inside chunks of
// 16 (element s of the float4 read at d = 16jj + 4q4 is the operand of MFMA step s) identically on both operands.  Key rows past
// L - 1 read row L - 1; tiles past nt_live stay 0.
template <int NT>
__device__ __forceinline__ void score_tiles_f32(f32x4_t (&st)[NT], const float* Ks, const float4 (&qv)[4], int L, int nt_live, int c16,
                                                int q4) {
#pragma unroll
  for (int t = 0; t < NT; ++t) st[t] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int jj = 0; jj < 4; ++jj) {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      if (t >= nt_live) continue;
      const float4 kv = *reinterpret_cast<const float4*>(Ks + min(16 * t + c16, L - 1) * 68 + 4 * q4 + 16 * jj);
      st[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(kv.x, qv[jj].x, st[t], 0, 0, 0);
      st[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(kv.y, qv[jj].y, st[t], 0, 0, 0);
      st[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(kv.z, qv[jj].z, st[t], 0, 0, 0);
      st[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(kv.w, qv[jj].w, st[t], 0, 0, 0);
    }
  }
}

// ------------------------------------------------------------------------------------------ bf16 P.V
// A probability enters the bf16 P.V MFMAs split EXACTLY into three bf16 pieces p = hi + mid + lo (truncations of the successive
// remainders: 3 x 8 mantissa bits cover fp32's 24), so hi.V + mid.V + lo.V is the fp32 product p.v summed in fp32 — no new rounding.
__device__ __forceinline__ uint32_t bf16_trunc_bits(float x) { return __float_as_uint(x) & 0xffff0000u; }

// eight probabilities (the k-slots of one lane in a 32-key block) -> the three B operands
__device__ __forceinline__ void split_bf16x3(const float (&p)[8], uint4& ph, uint4& pm, uint4& pl) {
  uint32_t hi[8], mid[8], lo[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const uint32_t h1 = bf16_trunc_bits(p[e]);
    const float r1 = p[e] - __uint_as_float(h1);
    const uint32_t h2 = bf16_trunc_bits(r1);
    const float r2 = r1 - __uint_as_float(h2);
    hi[e] = h1 >> 16, mid[e] = h2 >> 16, lo[e] = bf16_trunc_bits(r2) >> 16;
  }
  ph = make_uint4(hi[0] | (hi[1] << 16), hi[2] | (hi[3] << 16), hi[4] | (hi[5] << 16), hi[6] | (hi[7] << 16));
  pm = make_uint4(mid[0] | (mid[1] << 16), mid[2] | (mid[3] << 16), mid[4] | (mid[5] << 16), mid[6] | (mid[7] << 16));
  pl = make_uint4(lo[0] | (lo[1] << 16), lo[2] | (lo[3] << 16), lo[4] | (lo[5] << 16), lo[6] | (lo[7] << 16));
}

}  // namespace gdr
