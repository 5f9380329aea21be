// Full self-attention for 128 < L <= 512 at d_kv = 64 (the doc tower at the reference's passage length, Data_process/NQ_dataset/bert/
// bert_NQ.sh:5 MAX_LEN=512).  The one-pass kernels of attention.hip keep the whole K and V of a (sequence, head) in LDS and give one wave
// to each 16-query tile: 2 * L * 68 * 4 B is 278 KB at L = 512.  Here a workgroup owns a block of ATTN_LONG_QB = 128 query rows of one
// (sequence, head) — 8 waves x 16 queries — and walks K / V from key 0 in blocks of ATTN_LONG_KB = 64 keys that are staged through a
// double-buffered LDS image, with an online softmax: per query row a running maximum m and a running sum l; when a block raises the
// maximum, the output accumulator and the running sum are multiplied by exp(m_old - m_new) exactly once, before the block's own
// probabilities (exponentiated against m_new) are added.  There is no deferred-rescale threshold: every block rescales.
//
// Lane layout is the one-pass kernels': S^T = K.Q^T, so a lane holds scores of ONE query (lane & 15; the four lanes lane >> 4 hold 4 of
// every 16 keys each), m / alpha are lane-local after two shuffles, and the probability registers are the B operand of the P.V MFMAs as
// they stand.  The running sum is kept per lane (its four lanes share alpha) and reduced once at the end.
//
// Ragged == padded bit for bit: both layouts walk the same 64-key blocks from key 0.  A masked key (mask 0, or past seq_len[b] in the
// packed layout) scores s + (-1e9) — the additive fp32 mask of modeling_utils.py:271-272, never -inf — and its probability
// exp(-1e9 - m) is exactly 0 next to any live key, so it adds exactly +0 to l and to every output element; a block of masked keys
// only leaves m unchanged, rescales by exp(0) = 1 and adds +0: skipping it (the packed layout skips blocks wholly past seq_len[b])
// changes no bit.  Blocks of masked keys IN FRONT of the first live key (a mask that is not a prefix of ones) are computed in both
// layouts alike and wiped by the first live block's alpha = exp(-1e9 - m) = 0.  A sequence whose mask is all zero keeps
// m ~ -1e9 and comes out as the reference's uniform average over all L keys.
//
// Staging: the next block's global loads are issued into registers before the current block's MFMAs and written to the other LDS
// buffer after them (one workgroup barrier per block); K / V rows past the sequence's end are read from its last row (finite values,
// probability 0).
#include "attention.h"

namespace gdr {

constexpr int ATTN_LONG_QB = 128;  // query rows per workgroup (8 waves x 16); ops.ATTN_LONG_QUERY_BLOCK states it for the tests
constexpr int ATTN_LONG_KB = 64;   // keys per staged block; ops.ATTN_LONG_KEY_BLOCK

// ---------------------------------------------------------------------------------------------------------------- fp32 q / k / v
// LDS: 2 buffers x (K[64][68] + V[64][68] + mask[64]) floats = 70 144 B (two workgroups per CU).  Row stride 68 floats: the
// per-lane ds_read_b128 of "my key's row" is conflict-free, as in attention_mfma16_kernel.
//
// Three forms of one body:
//   LONG_PLAIN     the doc tower: no position bias; the per-key cell of a block holds the additive mask.
//   LONG_T5_SELF   the T5 encoder: + rel_bias[bucket(k - q)][h].  The bias depends on k - q alone (positions local to the sequence in
//                  both layouts), so the workgroup builds its head's table over the 2 * 512 - 1 offsets once, RelT[(q - k) + 511]
//                  (4 KB behind the two buffers: 74 240 B, still two workgroups per CU), from the bucket table and rel_bias; a score
//                  is s + (RelT + mask), the one-pass kernels' and the reference's order (modeling_t5.py:399-400).
//   LONG_T5_CROSS  decode-time cross-attention: the Lq <= 256 beam rows of a query (all at decoder position q_pos0, q_same_pos) against
//                  the query's Lk encoder keys, K / V rows of batch entry b / kv_group.  The additive term of a key,
//                  cross_rel_bias[bucket(q_pos0 - j)][h] + mask, is the same for every row: it is staged with the block in the
//                  per-key cell, and the block loop is LONG_PLAIN's.  q rows come finished from memory or as the projection's split-K
//                  slabs (q_part), summed in the reduction kernel's order as attention_kernel does.  One row (step 0) is a tile too.
// Keys past the end inside the last block carry -inf in the two T5 forms (exactly probability 0 even when every real key is masked;
// key 0 of every visited block is real, so the running maximum stays finite); LONG_PLAIN keeps the -1e9 it shipped with.
enum { LONG_PLAIN = 0, LONG_T5_SELF = 1, LONG_T5_CROSS = 2 };
constexpr int ATTN_LONG_MAXL = 512;  // RelT spans the offsets of this many positions; launch_attention bounds Lk by it

template <int FORM>
__global__ __launch_bounds__(512) void attention_long_f32_kernel(const AttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int DK = 64, DS = DK + 4, KB = ATTN_LONG_KB, QB = ATTN_LONG_QB, BUF = 2 * KB * DS + KB;
  constexpr bool CROSS = FORM == LONG_T5_CROSS;
  if (CROSS && a.live && *a.live == 0) return;  // uniform: every query of the generate call is done
  const int b = blockIdx.x / a.H, h = blockIdx.x % a.H, tid = threadIdx.x;
  const int kvb = CROSS ? b / a.kv_group : b;                     // whose K / V rows and mask
  const int L = (!CROSS && a.seq_len) ? a.seq_len[b] : a.Lk;      // keys; ragged: this sequence's own length
  const int Lq = CROSS ? a.Lq : L;                                // query rows
  const int q0 = blockIdx.y * QB;
  if (q0 >= Lq) return;  // uniform: a query block past this sequence's end
  const bool packed = !CROSS && a.seq_off;
  const int64_t qrow0 = packed ? a.seq_off[b] : (int64_t)b * a.q_bstride;
  const int64_t krow0 = packed ? a.seq_off[b] : (int64_t)kvb * a.k_bstride;
  const int64_t orow0 = packed ? a.seq_off[b] : (int64_t)b * a.o_bstride;
  const int w = tid >> 6, lane = tid & 63, c16 = lane & 15, q4 = lane >> 4;
  const bool active = q0 + 16 * w < Lq;  // wave-uniform; an idle wave still stages and meets the barriers
  const int nkb = (L + KB - 1) / KB;     // key blocks wholly past the end are never visited

  // this wave's query fragments (B operand of S^T = K.Q^T): lane (c16, q4) holds Q[q0 + 16w + c16][16jj + 4q4 .. +3]
  float4 qv[DK / 16];
  {
    const int64_t qr = qrow0 + min(q0 + 16 * w + c16, Lq - 1);
    if (CROSS && a.q_part) {  // the projection's split-K slabs, summed in the reduction kernel's order
#pragma unroll
      for (int jj = 0; jj < DK / 16; ++jj) {
        const int n = h * DK + 16 * jj + 4 * q4;
        const float* p = a.q_part + ((qr >> 6) * a.q_tiles_n + (n >> 6)) * (int64_t)a.q_S * 4096 + (qr & 63) * 64 + (n & 63);
        float4 q = *reinterpret_cast<const float4*>(p);
        for (int s = 1; s < a.q_S; ++s) {
          const float4 u = *reinterpret_cast<const float4*>(p + (int64_t)s * 4096);
          q.x += u.x, q.y += u.y, q.z += u.z, q.w += u.w;
        }
        qv[jj] = q;
      }
    } else {
      const float* q32 = a.q + qr * a.ldq + h * DK + 4 * q4;
#pragma unroll
      for (int jj = 0; jj < DK / 16; ++jj) qv[jj] = *reinterpret_cast<const float4*>(q32 + 16 * jj);
    }
  }
  // staging registers of one key block: 64 keys x 16 float4 of K and of V over 512 threads, one mask word for the first 64
  float4 kst0, kst1, vst0, vst1;  // (separate registers, not arrays: arrays captured by the lambdas below end up in scratch)
  int64_t mk_raw = 1;
  float kbias = 0.f;  // LONG_T5_CROSS: the position bias of this thread's key
  const int sr = tid >> 4, sc = tid & 15;  // this thread's pieces: rows sr and sr + 32 of the block, float4 column sc
  auto load_block = [&](int kb) {
    const int64_t row0 = krow0 + min(kb * KB + sr, L - 1), row1 = krow0 + min(kb * KB + sr + 32, L - 1);
    kst0 = *reinterpret_cast<const float4*>(a.k + row0 * a.ldk + h * DK + 4 * sc);
    vst0 = *reinterpret_cast<const float4*>(a.v + row0 * a.ldv + h * DK + 4 * sc);
    kst1 = *reinterpret_cast<const float4*>(a.k + row1 * a.ldk + h * DK + 4 * sc);
    vst1 = *reinterpret_cast<const float4*>(a.v + row1 * a.ldv + h * DK + 4 * sc);
    mk_raw = 1;
    if (tid < KB && a.key_mask && kb * KB + tid < L) mk_raw = a.key_mask[(int64_t)kvb * a.mask_bstride + kb * KB + tid];
    if (CROSS && a.rel_bias && tid < KB && kb * KB + tid < L)
      kbias = a.rel_bias[rel_bucket(a, a.q_pos0 - (kb * KB + tid)) * a.H + h];
  };
  auto store_block = [&](int kb, float* buf) {
    *reinterpret_cast<float4*>(buf + sr * DS + 4 * sc) = kst0;
    *reinterpret_cast<float4*>(buf + KB * DS + sr * DS + 4 * sc) = vst0;
    *reinterpret_cast<float4*>(buf + (sr + 32) * DS + 4 * sc) = kst1;
    *reinterpret_cast<float4*>(buf + KB * DS + (sr + 32) * DS + 4 * sc) = vst1;
    if (FORM == LONG_PLAIN) {
      if (tid < KB) buf[2 * KB * DS + tid] = (kb * KB + tid < L && mk_raw != 0) ? 0.f : -1e9f;
    } else if (tid < KB) {  // (bias first, then one -1e9, as attention_cross_mfma16_kernel)
      buf[2 * KB * DS + tid] = kb * KB + tid < L ? (mk_raw != 0 ? kbias : kbias + -1e9f) : -INFINITY;
    }
  };
  load_block(0);
  store_block(0, smem);
  if (FORM == LONG_T5_SELF) {
    float* RelT = smem + 2 * BUF;  // RelT[(q - k) + 511]
    for (int c = tid; c < 2 * ATTN_LONG_MAXL - 1; c += 512)
      RelT[c] = a.rel_bias[rel_bucket(a, c - (ATTN_LONG_MAXL - 1)) * a.H + h];
  }
#pragma unroll
  for (int jj = 0; jj < DK / 16; ++jj) qv[jj].x *= a.scale, qv[jj].y *= a.scale, qv[jj].z *= a.scale, qv[jj].w *= a.scale;
  __syncthreads();

  float m = -INFINITY, l = 0.f;  // running maximum of this lane's query (equal in its four lanes); this lane's share of the running sum
  f32x4_t o[DK / 16];
#pragma unroll
  for (int dt = 0; dt < DK / 16; ++dt) o[dt] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

  for (int kb = 0; kb < nkb; ++kb) {
    float* cur = smem + (kb & 1) * BUF;
    const bool more = kb + 1 < nkb;
    if (more) load_block(kb + 1);  // in flight under this block's MFMAs
    // nothing above may sink below this line: the compiler otherwise moves every load next to its LDS store again
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("" ::: "memory");
    if (active) {
      const float* Ks = cur;
      const float* Vs = cur + KB * DS;
      const float* Mk = cur + 2 * KB * DS;
      f32x4_t st[KB / 16];
      score_tiles_f32<KB / 16>(st, Ks, qv, KB, KB / 16, c16, q4);  // every row of the staged block is a finite K row
      // additive mask, block maximum: this lane holds keys 16t + 4q4 + r of its query
      float bm = -INFINITY;
#pragma unroll
      for (int t = 0; t < KB / 16; ++t) {
        float4 mk = *reinterpret_cast<const float4*>(Mk + 16 * t + 4 * q4);
        if (FORM == LONG_T5_SELF) {  // (bias + mask) first, as the reference; key kb * KB + 16t + 4q4 + r sits r cells below
          const float* rb = smem + 2 * BUF + (q0 + 16 * w + c16) - (kb * KB + 16 * t + 4 * q4) + (ATTN_LONG_MAXL - 1);
          mk.x += rb[0], mk.y += rb[-1], mk.z += rb[-2], mk.w += rb[-3];
        }
        st[t][0] += mk.x, st[t][1] += mk.y, st[t][2] += mk.z, st[t][3] += mk.w;
        bm = fmaxf(bm, fmaxf(fmaxf(st[t][0], st[t][1]), fmaxf(st[t][2], st[t][3])));
      }
      bm = quad_max(bm);
      const float m_new = fmaxf(m, bm);          // finite: a masked key adds -1e9, and the -inf tail cells of the T5 forms follow real key 0 of the block
      const float alpha = __expf(m - m_new);     // first block: exp(-inf) = 0 over l = 0, o = 0
      m = m_new;
      float bs = 0.f;
#pragma unroll
      for (int t = 0; t < KB / 16; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float p = __expf(st[t][r] - m_new);
          st[t][r] = p;
          bs += p;
        }
      }
      l = l * alpha + bs;
      // O^T += V^T . P^T, four 16-wide d tiles: lane holds d = 16dt + 4q4 + 0..3 of its query
#pragma unroll
      for (int dt = 0; dt < DK / 16; ++dt) {
        o[dt][0] *= alpha, o[dt][1] *= alpha, o[dt][2] *= alpha, o[dt][3] *= alpha;
#pragma unroll
        for (int t = 0; t < KB / 16; ++t) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float vv = Vs[(16 * t + 4 * q4 + r) * DS + 16 * dt + c16];
            o[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(vv, st[t][r], o[dt], 0, 0, 0);
          }
        }
      }
    }
    if (more) store_block(kb + 1, smem + ((kb + 1) & 1) * BUF);  // that buffer was last read before the previous barrier
    __syncthreads();
  }
  if (!active) return;
  const float inv = 1.0f / quad_sum(l);
  const int i = q0 + 16 * w + c16;
  if (i < Lq) {
#pragma unroll
    for (int dt = 0; dt < DK / 16; ++dt)
      store_ctx4(a, (orow0 + i) * a.ldo + h * DK + 16 * dt + 4 * q4,
                 make_float4(o[dt][0] * inv, o[dt][1] * inv, o[dt][2] * inv, o[dt][3] * inv));
  }
}

// ---------------------------------------------------------------------------------------------------------------- bf16 q / k / v
// The twin of attention_mfma_bf16_kernel (packed layout, scale 1 folded into wqkv) with the same rounding points: bf16-MFMA scores
// accumulated in fp32, fp32 softmax, and the probabilities enter the P.V bf16 MFMAs split EXACTLY into three bf16 pieces
// (p = hi + mid + lo, truncations of the successive remainders), fp32 accumulate, bf16 output rows.  Because the split is exact, the
// running maximum of the online softmax adds no rounding point of its own.
// LDS: 2 buffers x (K[64][144 B] + V^T[64 d][152 B] + mask[64] floats) = 38 400 B.
__global__ __launch_bounds__(512) void attention_long_bf16_kernel(const AttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_b[];
  constexpr int DK = 64, KS = 144, VS = 152, KB = ATTN_LONG_KB, QB = ATTN_LONG_QB, BUF = KB * KS + DK * VS + KB * 4;
  static_assert(BUF % 16 == 0, "buffers stay 16-byte aligned");
  const int b = blockIdx.x / a.H, h = blockIdx.x % a.H, tid = threadIdx.x;
  const int L = a.seq_len ? a.seq_len[b] : a.Lk;
  const int q0 = blockIdx.y * QB;
  if (q0 >= L) return;
  const int64_t qrow0 = a.seq_off ? a.seq_off[b] : (int64_t)b * a.q_bstride;
  const int64_t krow0 = a.seq_off ? a.seq_off[b] : (int64_t)b * a.k_bstride;
  const int64_t orow0 = a.seq_off ? a.seq_off[b] : (int64_t)b * a.o_bstride;
  const __bf16* q16 = reinterpret_cast<const __bf16*>(a.q);
  const __bf16* k16 = reinterpret_cast<const __bf16*>(a.k);
  const __bf16* v16 = reinterpret_cast<const __bf16*>(a.v);
  const int w = tid >> 6, lane = tid & 63, c16 = lane & 15, q4 = lane >> 4;
  const bool active = q0 + 16 * w < L;
  const int nkb = (L + KB - 1) / KB;

  // query fragments (B operand of S^T): lane (c16, q4) holds Q[q0 + 16w + c16][32kk + 8q4 .. +7]
  uint4 qv[2];
  {
    const __bf16* qp = q16 + (qrow0 + min(q0 + 16 * w + c16, L - 1)) * a.ldq + h * DK + 8 * q4;
    qv[0] = *reinterpret_cast<const uint4*>(qp);
    qv[1] = *reinterpret_cast<const uint4*>(qp + 32);
  }
  // one key block: 64 keys x 8 sixteen-byte pieces of K and of V, one each per thread
  const int sr = tid >> 3, sc = tid & 7;
  uint4 kst, vst;
  int64_t mk_raw = 1;
  auto load_block = [&](int kb) {
    const int64_t row = krow0 + min(kb * KB + sr, L - 1);
    kst = *reinterpret_cast<const uint4*>(k16 + row * a.ldk + h * DK + 8 * sc);
    vst = *reinterpret_cast<const uint4*>(v16 + row * a.ldv + h * DK + 8 * sc);
    mk_raw = 1;
    if (tid < KB && a.key_mask && kb * KB + tid < L) mk_raw = a.key_mask[(int64_t)b * a.mask_bstride + kb * KB + tid];
  };
  auto store_block = [&](int kb, unsigned char* buf) {
    *reinterpret_cast<uint4*>(buf + sr * KS + 16 * sc) = kst;
    unsigned char* Vt = buf + KB * KS;  // V transposed: Vt[d][key of the block]; every cell is rewritten for every block
    const uint32_t wv[4] = {vst.x, vst.y, vst.z, vst.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      reinterpret_cast<uint16_t*>(Vt + (8 * sc + 2 * i) * VS)[sr] = (uint16_t)(wv[i] & 0xffffu);
      reinterpret_cast<uint16_t*>(Vt + (8 * sc + 2 * i + 1) * VS)[sr] = (uint16_t)(wv[i] >> 16);
    }
    if (tid < KB) reinterpret_cast<float*>(buf + KB * KS + DK * VS)[tid] = (kb * KB + tid < L && mk_raw != 0) ? 0.f : -1e9f;
  };
  load_block(0);
  store_block(0, smem_b);
  __syncthreads();

  float m = -INFINITY, l = 0.f;
  f32x4_t o[DK / 16];
#pragma unroll
  for (int dt = 0; dt < DK / 16; ++dt) o[dt] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

  for (int kb = 0; kb < nkb; ++kb) {
    unsigned char* cur = smem_b + (kb & 1) * BUF;
    const bool more = kb + 1 < nkb;
    if (more) load_block(kb + 1);
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("" ::: "memory");
    if (active) {
      const unsigned char* Ks = cur;
      const unsigned char* Vt = cur + KB * KS;
      const float* Mk = reinterpret_cast<const float*>(cur + KB * KS + DK * VS);
      f32x4_t st[KB / 16];
#pragma unroll
      for (int t = 0; t < KB / 16; ++t) {
        st[t] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
        const unsigned char* kr = Ks + (16 * t + c16) * KS + 16 * q4;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
          const uint4 kv = *reinterpret_cast<const uint4*>(kr + 64 * kk);
          st[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, kv), __builtin_bit_cast(bf16x8_t, qv[kk]), st[t], 0, 0, 0);
        }
      }
      float bm = -INFINITY;
#pragma unroll
      for (int t = 0; t < KB / 16; ++t) {
        const float4 mk = *reinterpret_cast<const float4*>(Mk + 16 * t + 4 * q4);
        st[t][0] += mk.x, st[t][1] += mk.y, st[t][2] += mk.z, st[t][3] += mk.w;
        bm = fmaxf(bm, fmaxf(fmaxf(st[t][0], st[t][1]), fmaxf(st[t][2], st[t][3])));
      }
      bm = quad_max(bm);
      const float m_new = fmaxf(m, bm);
      const float alpha = __expf(m - m_new);
      m = m_new;
      float bs = 0.f;
#pragma unroll
      for (int t = 0; t < KB / 16; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float p = __expf(st[t][r] - m_new);
          st[t][r] = p;
          bs += p;
        }
      }
      l = l * alpha + bs;
      // exact three-way split of every probability, packed as the B operand of its 32-key half block: slot e of lane-quarter q4 is
      // key 16 * (2u + e / 4) + 4 * q4 + e % 4 of the block
      uint4 ph[2], pm[2], pl[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        float p[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) p[e] = st[2 * u + (e >> 2)][e & 3];
        split_bf16x3(p, ph[u], pm[u], pl[u]);
      }
#pragma unroll
      for (int dt = 0; dt < DK / 16; ++dt) {
        o[dt][0] *= alpha, o[dt][1] *= alpha, o[dt][2] *= alpha, o[dt][3] *= alpha;
        const unsigned char* vr = Vt + (16 * dt + c16) * VS + 8 * q4;  // Vt[d][32u + 16 * (e / 4) + 4 * q4 + e % 4]
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const uint2 v0 = *reinterpret_cast<const uint2*>(vr + 64 * u);
          const uint2 v1 = *reinterpret_cast<const uint2*>(vr + 64 * u + 32);
          const bf16x8_t va = __builtin_bit_cast(bf16x8_t, make_uint4(v0.x, v0.y, v1.x, v1.y));
          o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(va, __builtin_bit_cast(bf16x8_t, ph[u]), o[dt], 0, 0, 0);
          o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(va, __builtin_bit_cast(bf16x8_t, pm[u]), o[dt], 0, 0, 0);
          o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(va, __builtin_bit_cast(bf16x8_t, pl[u]), o[dt], 0, 0, 0);
        }
      }
    }
    if (more) store_block(kb + 1, smem_b + ((kb + 1) & 1) * BUF);
    __syncthreads();
  }
  if (!active) return;
  const float inv = 1.0f / quad_sum(l);
  const int i = q0 + 16 * w + c16;
  if (i < L) {
#pragma unroll
    for (int dt = 0; dt < DK / 16; ++dt)
      store_ctx4(a, (orow0 + i) * a.ldo + h * DK + 16 * dt + 4 * q4,
                 make_float4(o[dt][0] * inv, o[dt][1] * inv, o[dt][2] * inv, o[dt][3] * inv));
  }
}

// d_kv = 64 full self-attention over 128 < Lk <= 512 keys; launch_attention has checked the form (no causal mask, Lq == Lk,
// q_pos0 == 0, own K / V rows) and opened the ProfScope.  With rel_bias: the T5 encoder's form, fp32 q / k / v only.
int launch_attention_long(const AttnArgs& a, hipStream_t stream) {
  static_assert(ATTN_LONG_MAXL >= ATTN_LONG_QB, "RelT index range");
  GDR_CHECK_ARG(a.Lk <= ATTN_LONG_MAXL, "attention: L=%d above the key-block form's %d", a.Lk, ATTN_LONG_MAXL);
  const dim3 grid((unsigned)(a.B * a.H), (unsigned)((a.Lk + ATTN_LONG_QB - 1) / ATTN_LONG_QB));
  if (a.rel_bias) {
    GDR_CHECK_ARG(!a.qkv_bf16, "attention: bf16 q/k/v with a position bias stop at 128 keys (L=%d): hand in fp32 q/k/v", a.Lk);
    const size_t lds = 2 * sizeof(float) * (size_t)(2 * ATTN_LONG_KB * 68 + ATTN_LONG_KB) + sizeof(float) * 2 * ATTN_LONG_MAXL;
    if (int rc__ = ensure_dyn_lds(reinterpret_cast<const void*>(attention_long_f32_kernel<LONG_T5_SELF>), 80 * 1024, "attention"))
      return rc__;
    hipLaunchKernelGGL(attention_long_f32_kernel<LONG_T5_SELF>, grid, dim3(512), lds, stream, a);
    GDR_CHECK_LAUNCH("attention_long_f32_kernel<T5 self>");
    return GDR_OK;
  }
  if (a.qkv_bf16) {
    GDR_CHECK_ARG(a.scale == 1.0f, "attention: bf16 q/k/v over L=%d > 128 keys need the scale folded into wqkv (scale=%g)", a.Lk,
                  (double)a.scale);
    const size_t lds = 2 * (size_t)(ATTN_LONG_KB * 144 + 64 * 152 + ATTN_LONG_KB * 4);
    if (int rc__ = ensure_dyn_lds(reinterpret_cast<const void*>(attention_long_bf16_kernel), 80 * 1024, "attention")) return rc__;
    hipLaunchKernelGGL(attention_long_bf16_kernel, grid, dim3(512), lds, stream, a);
    GDR_CHECK_LAUNCH("attention_long_bf16_kernel");
    return GDR_OK;
  }
  const size_t lds = 2 * sizeof(float) * (size_t)(2 * ATTN_LONG_KB * 68 + ATTN_LONG_KB);
  if (int rc__ = ensure_dyn_lds(reinterpret_cast<const void*>(attention_long_f32_kernel<LONG_PLAIN>), 80 * 1024, "attention")) return rc__;
  hipLaunchKernelGGL(attention_long_f32_kernel<LONG_PLAIN>, grid, dim3(512), lds, stream, a);
  GDR_CHECK_LAUNCH("attention_long_f32_kernel");
  return GDR_OK;
}

// d_kv = 64 beam rows x encoder keys over 128 < Lk <= 512 keys (LONG_T5_CROSS above); launch_attention has checked the form
// (q_same_pos, own K / V rows through kv_group, no causal mask, fp32, 16-byte rows) and opened the ProfScope.  Lq >= 1: a workgroup
// per 128 beam rows of a (query, head) stages the key blocks for its waves.
int launch_attention_long_cross(const AttnArgs& a, hipStream_t stream) {
  GDR_CHECK_ARG(a.Lk <= ATTN_LONG_MAXL, "attention: L=%d above the key-block form's %d", a.Lk, ATTN_LONG_MAXL);
  const dim3 grid((unsigned)(a.B * a.H), (unsigned)((a.Lq + ATTN_LONG_QB - 1) / ATTN_LONG_QB));
  const size_t lds = 2 * sizeof(float) * (size_t)(2 * ATTN_LONG_KB * 68 + ATTN_LONG_KB);
  if (int rc__ = ensure_dyn_lds(reinterpret_cast<const void*>(attention_long_f32_kernel<LONG_T5_CROSS>), 80 * 1024, "attention"))
    return rc__;
  hipLaunchKernelGGL(attention_long_f32_kernel<LONG_T5_CROSS>, grid, dim3(512), lds, stream, a);
  GDR_CHECK_LAUNCH("attention_long_f32_kernel<T5 cross>");
  return GDR_OK;
}

}  // namespace gdr
