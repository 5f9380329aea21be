// Host-side scaffolding shared by the two encoder towers (encoder.hip: T5, bert.hip: BERT / DPR).  The towers have one block body per
// precision form, written out; what stands around a body — the pack plan's place in the workspace, the stream-K scratch, the
// self-attention arguments, the wrapper of the LDS-DMA linear, the way out of a packed forward, the checks of a call — is here, once.
// Plain structs and functions: nothing here launches a kernel that the forward calling it did not launch at the same point before.
#pragma once
#include "attention.h"
#include "layers.h"

namespace gdr {

// ---- pack plan (launch_pack_plan): the live rows of a padded batch, front to back ------------------------------------------------
struct PackPlan {
  int32_t *seq_len, *seq_off, *row_src;  // [B] live rows of a sequence, [B + 1] its first packed row, [B * L] packed row -> b * L + position
  int64_t* rows_dev;                     // [1] live rows of the batch: the device-side row count of every packed launch
};
struct PackPlanWs {  // byte offsets in a workspace
  size_t seq_len, seq_off, row_src, rows_dev, end;
};
static inline PackPlanWs pack_plan_ws(int B, int L, size_t at) {
  PackPlanWs p{};
  size_t o = at;
  p.seq_len = o, o += align_up((size_t)B * 4, 256);
  p.seq_off = o, o += align_up((size_t)(B + 1) * 4, 256);
  p.row_src = o, o += align_up((size_t)B * L * 4, 256);
  p.rows_dev = o, o += 256;
  p.end = o;
  return p;
}
static inline PackPlan carve_pack_plan(char* base, const PackPlanWs& p) {
  return {reinterpret_cast<int32_t*>(base + p.seq_len), reinterpret_cast<int32_t*>(base + p.seq_off),
          reinterpret_cast<int32_t*>(base + p.row_src), reinterpret_cast<int64_t*>(base + p.rows_dev)};
}
static inline int launch_pack_plan(const int64_t* mask, int B, int L, const PackPlan& p, hipStream_t stream) {
  return launch_pack_plan(mask, B, L, p.seq_len, p.seq_off, p.row_src, p.rows_dev, stream);
}

// ---- stream-K scratch at the head of a workspace's GEMM scratch region (which serves the split-K forms too: a launch uses one or the
// other); flags zeroed once per call
static inline int tower_streamk(char* region, StreamK* sk, const char* who, hipStream_t stream) {
  sk->part = reinterpret_cast<float*>(region);
  sk->flag = reinterpret_cast<int32_t*>(region + STREAMK_PART_BYTES);
  sk->epoch = 0;
  if (hipMemsetAsync(sk->flag, 0, 512 * sizeof(int32_t), stream) != hipSuccess) {
    set_error("%s: memset of the stream-K flags failed", who);
    return GDR_EHIP;
  }
  return GDR_OK;
}

// ---- encoder self-attention: q, k, v side by side in rows of `ld` elements, the context in rows of H * dk, L tokens per sequence,
// the key mask.  As built: padded layout, scale 1, no position bias, no operand — the setters below say what a forward adds.
static inline AttnArgs self_attn_args(int B, int H, int dk, int L, int64_t ld, const int64_t* mask) {
  AttnArgs at{};
  at.ldq = at.ldk = at.ldv = ld, at.ldo = H * dk;
  at.q_bstride = at.k_bstride = at.o_bstride = L;
  at.B = B, at.H = H, at.dk = dk, at.Lq = L, at.Lk = L;
  at.q_pos0 = 0, at.scale = 1.0f;
  at.rel_bias = nullptr, at.bidirectional = 1, at.num_buckets = 0;
  at.key_mask = mask, at.mask_bstride = L, at.causal = 0, at.causal_neg_inf = 0;
  at.kv_rows = nullptr, at.kv_group = 1;
  return at;
}
static inline void attn_f32(AttnArgs& at, const float* qkv, float* ctx) {  // fp32 q | k | v rows, fp32 context
  at.q = qkv, at.k = qkv + at.ldo, at.v = qkv + 2 * at.ldo, at.out = ctx;
}
static inline void attn_qkv_bf16(AttnArgs& at, const void* qkv) {  // the qkv linear left bf16 q | k | v rows (ld in bf16 elements)
  const __bf16* q16 = static_cast<const __bf16*>(qkv);
  at.q = reinterpret_cast<const float*>(q16), at.k = reinterpret_cast<const float*>(q16 + at.ldo);
  at.v = reinterpret_cast<const float*>(q16 + 2 * at.ldo), at.qkv_bf16 = 1;
}
static inline void attn_ctx_bf16(AttnArgs& at, void* ctx16) { at.out_bf16 = ctx16; }  // the context leaves as bf16 (`out` is not written)
static inline void attn_packed(AttnArgs& at, const PackPlan& p) { at.seq_off = p.seq_off, at.seq_len = p.seq_len; }
static inline void attn_t5_bias(AttnArgs& at, const float* rel_bias, const GdrT5Dims& dm) {  // bucketed relative bias (layer 0's table)
  at.rel_bias = rel_bias, at.num_buckets = dm.rel_buckets;
  at.lut = make_bucket_lut(dm.rel_buckets / 2, dm.rel_max_distance);
}
static inline void attn_scale(AttnArgs& at, float scale) { at.scale = scale; }  // BERT: 1 / sqrt(head width)

// ---- the LDS-DMA linear (gemm_bf16.hip) as the towers call it: dense operand rows, the residual and the output in rows of ldc.
// terms 0: bf16 operands [rows, K]; 6 / 3 / 2: split form, K is K0 and a row of A / W holds the planes (split_row_elems).
// out_mode 0 fp32 / 1 bf16 / 2 bf16 planes / 3 fp16 planes.  md: the device-side row count or null; the profiler is told the live rows.
struct GldsLinear {
  const char* who;
  int64_t live_rows_hint;
  int terms;
  hipStream_t stream;
};
static inline int linear_glds(const GldsLinear& g, const void* A, const float* W, void* C, int64_t ldc, int64_t rows, const int64_t* md,
                              int N, int K, int act, const float* bias, const float* residual, int out_mode) {
  const int ld = g.terms ? split_row_elems(K, g.terms == 2) : K;
  ProfScope prof(PROF_LINEAR, 2.0 * (double)(md && g.live_rows_hint >= 0 ? g.live_rows_hint : rows) * (double)N * (double)K, g.stream);
  const int rc = launch_linear_bf16_glds(A, ld, W, ld, static_cast<float*>(C), ldc, rows, N, K, bias != nullptr, residual != nullptr, act, bias,
                                         residual, ldc, out_mode, g.stream, md, g.terms);
  if (rc > 0) {
    set_error("%s: shape not served by the LDS-DMA linear", g.who);
    return GDR_EINVAL;
  }
  return rc;
}

// ---- the way out of a packed forward: the CLS rows of `src` into out_pooled and / or the packed rows back into the [B, L, d] layout
// (PAD rows zero); either output may be null
static inline int unpack_rows(const float* src, const PackPlan& p, int B, int64_t M, int d, float* out_pooled, float* out_hidden,
                              const char* who, hipStream_t stream) {
  if (out_pooled) GDR_TRY(launch_gather_rows(src, p.seq_off, B, d, out_pooled, stream));
  if (out_hidden) {
    if (hipMemsetAsync(out_hidden, 0, (size_t)M * d * sizeof(float), stream) != hipSuccess) {
      set_error("%s: memset failed", who);
      return GDR_EHIP;
    }
    GDR_TRY(launch_scatter_rows(src, p.row_src, p.rows_dev, M, d, out_hidden, stream));
  }
  return GDR_OK;
}

// ---- the checks of a call, in the order every entry point has kept them (the first failing check names the error).  ptrs_ok: the
// caller's own pointer list (the forms differ in what may be null).  A form's own shape rule stands between the two calls.
static inline int check_t5_call(const char* who, bool ptrs_ok, const GdrT5EncoderWeights* w, int B, int L, bool dims4) {
  GDR_CHECK_ARG(ptrs_ok, "%s: null pointer", who);
  const GdrT5Dims& dm = w->dims;
  GDR_CHECK_ARG(B > 0 && L > 0 && L <= T5_MAX_LEN, "%s: B=%d L=%d (L must be in [1,%d])", who, B, L, T5_MAX_LEN);
  GDR_CHECK_ARG(!dims4 || (dm.d_model % 4 == 0 && dm.d_kv % 4 == 0 && dm.d_ff % 4 == 0), "%s: dims must be multiples of 4", who);
  GDR_CHECK_ARG(w->embed && w->rel_bias && w->final_ln && w->layers, "%s: null weight pointer", who);
  return GDR_OK;
}
static inline int check_bert_call(const char* who, bool ptrs_ok, const GdrBertWeights* w, int B, int L) {
  GDR_CHECK_ARG(ptrs_ok, "%s: null pointer", who);
  GDR_CHECK_ARG(B > 0 && L > 0 && L <= 512 && L <= w->max_pos, "%s: B=%d L=%d (L must be <= min(512, max_pos = %d))", who, B, L, w->max_pos);
  const int d = w->d_model, H = w->num_heads;
  GDR_CHECK_ARG(d % 4 == 0 && H > 0 && d % H == 0 && (d / H) % 4 == 0 && w->d_ff % 4 == 0, "%s: unsupported dims", who);
  GDR_CHECK_ARG(w->word_emb && w->pos_emb && w->type_emb && w->emb_ln_w && w->emb_ln_b && w->layers, "%s: null weight", who);
  return GDR_OK;
}
static inline int check_workspace(const char* who, const void* workspace, size_t workspace_bytes, size_t required) {
  if (workspace_bytes < required) {
    set_error("%s: workspace %zu < required %zu", who, workspace_bytes, required);
    return GDR_ENOSPC;
  }
  GDR_CHECK_ARG(((uintptr_t)workspace & 255) == 0, "%s: workspace must be 256-byte aligned", who);
  return GDR_OK;
}

}  // namespace gdr
