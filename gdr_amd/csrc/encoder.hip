// T5 encoder forward on gfx950 — replaces `T5Stack.forward` of the reference
// (GDR_model/transformers/modeling_t5.py:685-821, blocks :498-584, eval mode: dropout = identity).
//
// Per layer (pre-norm, T5 v1.0):   h += o(attn(qkv(rms(h))))    ;    h += wo(relu(wi(rms(h))))
//   rms           layers.hip  rmsnorm_kernel                                  (modeling_t5.py:164-171)
//   qkv / o / wi / wo   gemm_f32.hip on v_mfma_f32_32x32x2_f32 (persistent form at encoder batch sizes); q,k,v fused into
//                 one [3*inner,d] GEMM,
//                 residual add and ReLU fused into the GEMM epilogues        (:360-364,:413,:182-185,:199)
//   attn          attention.hip  attention_mfma16_kernel (d_kv = 64: S^T = K·Q^T and O^T = V^T·P^T on v_mfma_f32_16x16x4_f32, one
//                 wave per 16-query tile; above 128 tokens attention_long.hip's key-block form) or attention_kernel (any d_kv): QKᵀ (no 1/sqrt(d)) + bucketed relative bias +
//                 pad mask (1-m)*-1e9 + fp32 softmax + PV                           (:384-413, :290-314)
// The position bias is never materialised as a [B,H,L,L] tensor: the kernel re-derives it from the
// [buckets,H] table (layer 0's, shared by all layers as in :790-795).
//
// Layout of this file.  Five forwards, each with its block body written out: t5_encoder_impl (padded fp32, and the padded bf16 mode
// with its fused form), ragged_f32_blocks / ragged_bf16_blocks (packed; ragged_impl in front of them does the checks, the two-chain
// hand-off, the pack plan and the padded fallback) and ragged_split_impl (packed, split-form linears).  What stands around a body —
// pack plan, stream-K scratch, attention arguments, the LDS-DMA linear's wrapper, the packed exit, the call checks — is tower.h's,
// shared with bert.hip; the workspace layouts (EncWs, RagWs) and their typed views (carve_enc, carve_rag) are below.
#include <algorithm>
#include <mutex>
#include <vector>

#include "tower.h"

namespace gdr {

constexpr size_t ENC_SPLITK_BYTES = (size_t)112 << 20;  // <= 384 tail tiles x 4 splits x 64 KiB + slack; the same region
                                                        // serves as the stream-K hand-off scratch (a launch uses one or the other)
static_assert(STREAMK_BYTES <= ENC_SPLITK_BYTES, "stream-K scratch must fit the split-K region");
constexpr bool ENC_LAST_Q_CLS_DEFAULT = true;  // GDR_ENC_LAST_Q_CLS when unset (DESIGN 4 "Token table": the A/B that decided it)

struct EncWs {
  size_t off_h, off_nx, off_qkv, off_ctx, off_ff, off_splitk, off_bf, total;
};
struct EncBuf {
  float *h, *nx, *qkv, *ctx, *ff;
  char* splitk;  // split-K slabs / stream-K scratch (tower_streamk; StreamK::part is its first byte)
  void* abf;     // bf16 copy of a GEMM's A operand (the bf16 layouts only)
};
static EncBuf carve_enc(char* base, const EncWs& ws) {
  return {reinterpret_cast<float*>(base + ws.off_h),   reinterpret_cast<float*>(base + ws.off_nx), reinterpret_cast<float*>(base + ws.off_qkv),
          reinterpret_cast<float*>(base + ws.off_ctx), reinterpret_cast<float*>(base + ws.off_ff), base + ws.off_splitk,
          base + ws.off_bf};
}

static EncWs enc_ws(const GdrT5Dims& dm, int64_t M, bool bf16 = false) {
  EncWs w{};
  const size_t inner = (size_t)dm.num_heads * dm.d_kv;
  size_t o = 0;
  w.off_h = o, o += align_up((size_t)M * dm.d_model * 4, 256);
  w.off_nx = o, o += align_up((size_t)M * dm.d_model * 4, 256);
  w.off_qkv = o, o += align_up((size_t)M * 3 * inner * 4, 256);
  w.off_ctx = o, o += align_up((size_t)M * inner * 4, 256);
  w.off_ff = o, o += align_up((size_t)M * dm.d_ff * 4, 256);
  w.off_splitk = o, o += ENC_SPLITK_BYTES;  // small batches: split-K partial slabs (gemm_f32.hip)
  w.off_bf = o;
  if (bf16) o += align_up((size_t)M * (dm.d_ff > dm.d_model ? dm.d_ff : dm.d_model) * 2, 256);  // bf16 copy of a GEMM's A operand
  w.total = o;
  return w;
}

}  // namespace gdr

extern "C" size_t gdr_t5_encoder_workspace_bytes(const GdrT5Dims* dims, int B, int L) {
  if (!dims || B <= 0 || L <= 0) return 0;
  return gdr::enc_ws(*dims, (int64_t)B * L).total;
}

namespace gdr {
// bf16 precision mode, fused form: every contraction length a multiple of 64, so the LDS-DMA linear serves all four linears of a block
static bool t5_fused16(const GdrT5EncoderWeights& w) {
  const GdrT5Dims& dm = w.dims;
  return dm.d_model % 64 == 0 && (dm.num_heads * dm.d_kv) % 64 == 0 && dm.d_ff % 64 == 0 && (((uintptr_t)w.layers[0].wqkv) & 15) == 0;
}

static int t5_encoder_impl(const GdrT5EncoderWeights* w, const int64_t* ids, const int64_t* mask, int B, int L,
                           float* out_hidden, float* out_pooled, void* workspace, size_t workspace_bytes, bool bf16,
                           hipStream_t stream) {
  if (B == 0) return GDR_OK;  // empty batch
  GDR_TRY(check_t5_call("t5_encoder", w && ids && out_hidden && workspace, w, B, L, true));
  const GdrT5Dims& dm = w->dims;
  const int64_t M = (int64_t)B * L;
  const EncWs ws = enc_ws(dm, M, bf16);
  GDR_CHECK_ARG(!bf16 || (dm.d_model % 8 == 0 && dm.d_ff % 8 == 0 && (dm.num_heads * dm.d_kv) % 8 == 0),
                "t5_encoder_bf16: dims must be multiples of 8");
  GDR_TRY(check_workspace("t5_encoder", workspace, workspace_bytes, ws.total));
  const EncBuf e = carve_enc(static_cast<char*>(workspace), ws);
  float *h = e.h, *nx = e.nx, *qkv = e.qkv, *ctx = e.ctx, *ff = e.ff;
  void* abf = e.abf;
  StreamK sk{};
  if (!bf16) GDR_TRY(tower_streamk(e.splitk, &sk, "t5_encoder", stream));
  // one linear: fp32 as is; in bf16 mode the activation operand is rounded to bf16 into `abf` first (the weights were
  // rounded once by the caller) and the GEMM runs on v_mfma_f32_32x32x16_bf16 with fp32 accumulate / epilogue / output
  auto linear = [&](const float* A, int64_t lda, const float* W, float* C, int64_t ldc, int N, int K, int epi,
                    const float* residual) -> int {
    if (!bf16)
      return launch_linear_f32_ws(A, lda, W, K, C, ldc, M, N, K, epi, nullptr, residual, ldc, sk.part, ENC_SPLITK_BYTES, stream, &sk);
    GDR_CHECK_ARG(lda == K, "t5_encoder_bf16: operand must be dense");
    int rc_ = launch_cast_f32_bf16(A, abf, M * (int64_t)K, stream);
    if (rc_) return rc_;
    return launch_linear_bf16(abf, K, W, K, C, ldc, M, N, K, epi, nullptr, residual, ldc, stream);
  };
  const int d = dm.d_model, H = dm.num_heads, dk = dm.d_kv, inner = H * dk;

  int rc = launch_embed(w->embed, ids, M, d, dm.vocab_size, h, stream);  // modeling_t5.py:725
  if (rc) return rc;

  // bf16 mode, fused form: the producers write the bf16 operand of the next linear directly — RMSNorm, the attention context
  // and the ReLU epilogue of wi — instead of fp32 + a cast pass.  Rounding points are the same as in the cast form.
  const bool fused16 = bf16 && t5_fused16(*w);
  // d_kv = 64 (the MFMA attention form): q, k, v leave the linear as bf16 and are widened inside the attention kernel
  const bool qkv16 = fused16 && dk == 64 && L <= 128;
  AttnArgs at = self_attn_args(B, H, dk, L, 3 * inner, mask);
  attn_f32(at, qkv, ctx), attn_t5_bias(at, w->rel_bias, dm);
  if (qkv16) attn_qkv_bf16(at, qkv);
  if (fused16) attn_ctx_bf16(at, abf);  // ctx as bf16 [M, inner] (nx is dead)

  const GldsLinear glds{"t5_encoder_bf16", -1, 0, stream};
  auto lin16 = [&](const void* A, const float* W, float* C, int64_t ldc, int N, int K, int act, const float* residual,
                   int out_bf16) -> int { return linear_glds(glds, A, W, C, ldc, M, nullptr, N, K, act, nullptr, residual, out_bf16); };
  for (int i = 0; i < dm.num_layers; ++i) {
    const GdrT5EncLayer& ly = w->layers[i];
    GDR_CHECK_ARG(ly.ln_attn && ly.wqkv && ly.wo && ly.ln_ff && ly.wi && ly.wo_ff, "t5_encoder: layer %d null weight", i);
    if (fused16) {
      if ((rc = launch_rmsnorm_bf16(h, ly.ln_attn, abf, M, d, dm.eps, stream))) return rc;
      if ((rc = lin16(abf, ly.wqkv, qkv, 3 * inner, 3 * inner, d, 0, nullptr, qkv16 ? 1 : 0))) return rc;
      if ((rc = launch_attention(at, stream))) return rc;
      if ((rc = lin16(abf, ly.wo, h, d, d, inner, 0, h, 0))) return rc;
      if ((rc = launch_rmsnorm_bf16(h, ly.ln_ff, abf, M, d, dm.eps, stream))) return rc;
      if ((rc = lin16(abf, ly.wi, ff, dm.d_ff, dm.d_ff, d, 1, nullptr, 1))) return rc;  // relu, bf16 out (in the fp32 ff buffer)
      if ((rc = lin16(ff, ly.wo_ff, h, d, d, dm.d_ff, 0, h, 0))) return rc;
      continue;
    }
    if ((rc = launch_rmsnorm(h, ly.ln_attn, nx, M, d, dm.eps, nullptr, 1, stream))) return rc;
    if ((rc = linear(nx, d, ly.wqkv, qkv, 3 * inner, 3 * inner, d, GDR_EPI_NONE, nullptr))) return rc;
    if ((rc = launch_attention(at, stream))) return rc;
    if ((rc = linear(ctx, inner, ly.wo, h, d, d, inner, GDR_EPI_RESIDUAL, h))) return rc;
    if ((rc = launch_rmsnorm(h, ly.ln_ff, nx, M, d, dm.eps, nullptr, 1, stream))) return rc;
    if ((rc = linear(nx, d, ly.wi, ff, dm.d_ff, dm.d_ff, d, GDR_EPI_RELU, nullptr))) return rc;
    if ((rc = linear(ff, dm.d_ff, ly.wo_ff, h, d, d, dm.d_ff, GDR_EPI_RESIDUAL, h))) return rc;
  }
  // final_layer_norm (:803) + CLS pool h[:,0] (main_models.py:102-109)
  return launch_rmsnorm(h, w->final_ln, out_hidden, M, d, dm.eps, out_pooled, L, stream);
}
}  // namespace gdr

extern "C" int gdr_t5_encoder_forward(const GdrT5EncoderWeights* w, const int64_t* ids, const int64_t* mask, int B,
                                      int L, float* out_hidden, float* out_pooled, void* workspace,
                                      size_t workspace_bytes, void* stream_) {
  return gdr::t5_encoder_impl(w, ids, mask, B, L, out_hidden, out_pooled, workspace, workspace_bytes, false,
                              static_cast<hipStream_t>(stream_));
}

// ------------------------------------------------------------------------------------------------ ragged form
// The same forward over the token rows that can influence the requested outputs (include/gdr_hip.h):
//   * PAD rows are never computed: the live rows of the batch are packed front to back (launch_pack_plan), every linear /
//     norm / residual runs over the packed rows, attention works per sequence on its own length.  A row's arithmetic is
//     unchanged — GEMM rows are independent and keep their k order, a PAD key contributes exp(-1e9 - max) = 0 to a live
//     query's softmax in the padded form and is simply absent here — so live rows are BIT-IDENTICAL to the padded form.
//   * pooled-only calls (out_hidden == NULL: config C2, EncoderModel.encode_query) stop computing non-CLS rows after the
//     last layer's attention: its o / wi / wo and the final norm run on the B CLS rows alone.
// The row count is a device-side value (the mask lives on the device): grids are sized for B*L and kernels read the count,
// so the call stays free of host synchronisation.
namespace gdr {
struct RagWs {  // behind an EncWs (bf16 layout): the pack plan, then the CLS rows of a pooled-only call's last block
  PackPlanWs plan;
  size_t ctx_cls, h_cls, nx_cls, ff_cls, total;
};
struct RagBuf {
  PackPlan plan;
  float *ctx_cls, *h_cls, *nx_cls, *ff_cls;  // [B, inner], [B, d], [B, d], [B, d_ff]; the bf16 mode keeps bf16 rows in all but h_cls
};
static RagWs rag_ws(const GdrT5Dims& dm, int B, int L, size_t base) {
  RagWs r{};
  const size_t inner = (size_t)dm.num_heads * dm.d_kv;
  r.plan = pack_plan_ws(B, L, base);
  size_t o = r.plan.end;
  r.ctx_cls = o, o += align_up((size_t)B * inner * 4, 256);
  r.h_cls = o, o += align_up((size_t)B * dm.d_model * 4, 256);
  r.nx_cls = o, o += align_up((size_t)B * dm.d_model * 4, 256);
  r.ff_cls = o, o += align_up((size_t)B * dm.d_ff * 4, 256);
  r.total = o;
  return r;
}
static RagBuf carve_rag(char* base, const RagWs& r) {
  return {carve_pack_plan(base, r.plan), reinterpret_cast<float*>(base + r.ctx_cls), reinterpret_cast<float*>(base + r.h_cls),
          reinterpret_cast<float*>(base + r.nx_cls), reinterpret_cast<float*>(base + r.ff_cls)};
}
// The packed form needs the d_kv = 64 attention kernel.  ragged_packs: a 128x128 tile grid that fills the chip without
// split-K (the narrowest linear has N = d_model) — the un-split forms, with the pooled-only tail on the CLS rows.
// ragged_packs_small (r03): smaller batches (C3's 64-query encoder pass).  The padded form runs those on the split-K /
// stream-K forms of launch_linear_f32_ws, chosen from B*L alone; the packed form takes the SAME forms with the live row
// count on the device, so kept rows are still bit-identical — only the pooled-only tail is not taken (its un-split
// kernels would sum in another order than the padded form's split ones).
static bool ragged_packs(const GdrT5Dims& dm, int B, int L) {
  const int64_t tiles = (((int64_t)B * L + 127) / 128) * ((dm.d_model + 127) / 128);
  return dm.d_kv == 64 && tiles >= 192 && dm.d_model % 32 == 0 && dm.d_ff % 32 == 0 && (dm.num_heads * dm.d_kv) % 32 == 0;
}
static bool ragged_packs_small(const GdrT5Dims& dm, int B, int L) {
  return dm.d_kv == 64 && (int64_t)B * L >= 256 && dm.d_model % 32 == 0 && dm.d_ff % 32 == 0 && (dm.num_heads * dm.d_kv) % 32 == 0;
}

// ---- two chains (GDR_ENC_CHAINS=2; DESIGN 4 "Two encoder chains") ------------------------------------------------------
// A pooled-only fp32 call whose two halves [0, B/2) and [B/2, B) both satisfy ragged_packs runs as two independent packed
// forwards — sequences do not interact — each on its own slice of ids / mask / out_pooled and its own workspace (its own pack
// plan and stream-K scratch): chain A on the caller's stream, chain B on a leased side stream forked from and joined to
// the caller's stream by events, so the caller sees one stream-ordered call (and a capture of it stays legal).  While one
// chain is in a norm, an attention, a GEMM's ramp or its hand-off, the other holds the matrix pipes.
// Co-residency: every persistent / stream-K linear of a chain is capped at ENC_CHAIN_GRID workgroups, so a call never has
// more than 2 x 256 = 512 of them in flight — the chip's slots (256 CUs x 2): a stream-K workgroup's predecessor is
// resident or becomes so as soon as a short non-GEMM kernel retires, never behind the other chain's GEMM.
// A row's bits do not depend on the chain count: every whole-K form gives the same bits and the CLS tail is un-split.
constexpr int ENC_CHAIN_GRID = 256;
constexpr int ENC_CHAINS_DEFAULT = 2;  // GDR_ENC_CHAINS when unset (DESIGN 4 "Two encoder chains": the A/B that decided it)
// Chain B starts behind this many of chain A's block-0 linears (0..3).  Started together the chains reach every boundary
// together and the step is slower than one chain; behind A's o projection (1) they stay half a block apart.  Measured
// 0 / 1 / 2 / 3: +0.5 % / -2.0 % / -1.9 % / +0.8 % of the C2 step (profiles/r21_enc_chains_stagger.txt).
constexpr int ENC_CHAIN_STAGGER_DEFAULT = 1;
struct EncChain {
  int grid_cap;          // workgroups of the chain's persistent / stream-K linears
  hipEvent_t after;      // recorded on the chain's stream behind its `after_linears`-th batch linear; null: none
  int after_linears;
};
static bool enc_chains_eligible(const GdrT5Dims& dm, int B, int L) {  // B/2 is the smaller half
  return B >= 2 && dm.num_layers >= 2 && ragged_packs(dm, B / 2, L);
}
static size_t ragged_one_chain_bytes(const GdrT5Dims& dm, int B, int L) {  // a multiple of 256
  return rag_ws(dm, B, L, enc_ws(dm, (int64_t)B * L, true).total).total;
}
static size_t ragged_bytes(const GdrT5Dims& dm, int B, int L) {
  const size_t one = ragged_one_chain_bytes(dm, B, L);
  if (!enc_chains_eligible(dm, B, L)) return one;
  const size_t two = ragged_one_chain_bytes(dm, B / 2, L) + ragged_one_chain_bytes(dm, B - B / 2, L);
  return two > one ? two : one;
}

struct EncSide {
  hipStream_t s = nullptr;
  hipEvent_t fork = nullptr, stagger = nullptr, join = nullptr;
  int dev = -1;
};
static std::mutex g_enc_side_mu;
static std::vector<EncSide*> g_enc_side_free;
// leased per call from a per-device pool, as decode.hip's side streams: created once, reused, never shared by two calls
static EncSide* enc_side_acquire() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  {
    std::lock_guard<std::mutex> lock(g_enc_side_mu);
    for (size_t i = 0; i < g_enc_side_free.size(); ++i)
      if (g_enc_side_free[i]->dev == dev) {
        EncSide* x = g_enc_side_free[i];
        g_enc_side_free.erase(g_enc_side_free.begin() + i);
        return x;
      }
  }
  EncSide* x = new EncSide();
  x->dev = dev;
  if (hipStreamCreateWithFlags(&x->s, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&x->fork, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&x->stagger, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&x->join, hipEventDisableTiming) != hipSuccess) {
    (void)hipGetLastError();
    delete x;  // the caller runs one chain
    return nullptr;
  }
  return x;
}
static void enc_side_release(EncSide* x) {  // when the call has finished enqueueing: the stream is in-order
  std::lock_guard<std::mutex> lock(g_enc_side_mu);
  g_enc_side_free.push_back(x);
}

static int ragged_impl(const GdrT5EncoderWeights* w, const int64_t* ids, const int64_t* mask, int B, int L, float* out_hidden,
                       float* out_pooled, int64_t live_rows_hint, void* workspace, size_t workspace_bytes, bool bf16,
                       hipStream_t stream, const EncChain* chain = nullptr);

static int ragged_two_chains(const GdrT5EncoderWeights* w, const int64_t* ids, const int64_t* mask, int B, int L, float* out_pooled,
                             int64_t live_rows_hint, char* base, int stagger, EncSide* side, hipStream_t stream) {
  const GdrT5Dims& dm = w->dims;
  const int BA = B / 2, BB = B - BA;
  const size_t bytes_a = ragged_one_chain_bytes(dm, BA, L), bytes_b = ragged_one_chain_bytes(dm, BB, L);
  const int64_t hint_a = live_rows_hint >= 0 ? live_rows_hint / 2 : -1;  // a tuning input only
  const int64_t hint_b = live_rows_hint >= 0 ? live_rows_hint - hint_a : -1;
  if (hipEventRecord(side->fork, stream) != hipSuccess || hipStreamWaitEvent(side->s, side->fork, 0) != hipSuccess) {
    set_error("t5_encoder_ragged: fork to the side stream failed");
    return GDR_EHIP;
  }
  const EncChain ca{ENC_CHAIN_GRID, stagger > 0 ? side->stagger : nullptr, stagger};
  const EncChain cb{ENC_CHAIN_GRID, nullptr, 0};
  int rc = ragged_impl(w, ids, mask, BA, L, nullptr, out_pooled, hint_a, base, bytes_a, false, stream, &ca);
  if (rc == GDR_OK && stagger > 0 && hipStreamWaitEvent(side->s, side->stagger, 0) != hipSuccess) {
    set_error("t5_encoder_ragged: wait on the stagger event failed");
    rc = GDR_EHIP;
  }
  if (rc == GDR_OK)
    rc = ragged_impl(w, ids + (size_t)BA * L, mask + (size_t)BA * L, BB, L, nullptr, out_pooled + (size_t)BA * dm.d_model, hint_b,
                     base + bytes_a, bytes_b, false, side->s, &cb);
  // the join is enqueued whatever happened above: the side stream must not stay forked (a capture would be left open)
  if (hipEventRecord(side->join, side->s) != hipSuccess || hipStreamWaitEvent(stream, side->join, 0) != hipSuccess) {
    if (rc == GDR_OK) set_error("t5_encoder_ragged: join of the side stream failed");
    return rc ? rc : GDR_EHIP;
  }
  return rc;
}
}  // namespace gdr

extern "C" size_t gdr_t5_encoder_ragged_workspace_bytes(const GdrT5Dims* dims, int B, int L) {
  if (!dims || B <= 0 || L <= 0) return 0;
  return gdr::ragged_bytes(*dims, B, L);  // serves both precisions and both chain counts
}

namespace gdr {
// ---- packed form of the bf16 precision mode: the producers write the bf16 operand of the next linear (RMSNorm, the attention
//      context, the ReLU epilogue of wi); same rounding points as gdr_t5_encoder_forward_bf16, rows independent.  The CLS buffers
//      of `r` hold bf16 rows here (all but h_cls).
static int ragged_bf16_blocks(const GdrT5EncoderWeights* w, const int64_t* ids, const int64_t* mask, int B, int L, float* out_hidden,
                              float* out_pooled, int64_t live_rows_hint, const EncBuf& e, const RagBuf& r, hipStream_t stream) {
  const GdrT5Dims& dm = w->dims;
  const int64_t M = (int64_t)B * L;
  const int d = dm.d_model, H = dm.num_heads, dk = dm.d_kv, inner = H * dk;
  float *h = e.h, *nx = e.nx, *qkv = e.qkv, *ff = e.ff, *h_cls = r.h_cls;
  void *abf = e.abf, *ctx_cls16 = r.ctx_cls, *nx_cls16 = r.nx_cls, *ff_cls16 = r.ff_cls;
  const int32_t* seq_off = r.plan.seq_off;
  const int64_t* rows_dev = r.plan.rows_dev;
  int rc;
  const GldsLinear glds{"t5_encoder_ragged_bf16", live_rows_hint, 0, stream};
  auto lin16 = [&](const void* A, const float* W, void* C, int64_t ldc, int64_t rows, const int64_t* md, int N, int K, int act,
                   const float* residual, int out_bf16) -> int {
    return linear_glds(glds, A, W, C, ldc, rows, md, N, K, act, nullptr, residual, out_bf16);
  };
  if ((rc = launch_embed_packed(w->embed, ids, r.plan.row_src, rows_dev, M, d, dm.vocab_size, h, stream))) return rc;
  // the packed form always runs a d_kv = 64 MFMA attention: up to 128 tokens on bf16 q / k / v; above, the key-block form with
  // position bias is fp32 (as the padded form above): the qkv linear stores fp32 and the context still leaves as bf16
  const bool qkv16 = L <= 128;
  AttnArgs at = self_attn_args(B, H, dk, L, 3 * inner, mask);
  if (qkv16)
    attn_qkv_bf16(at, qkv);
  else
    attn_f32(at, qkv, nullptr);
  attn_ctx_bf16(at, abf), attn_t5_bias(at, w->rel_bias, dm), attn_packed(at, r.plan);
  const bool pooled_only = out_hidden == nullptr;
  for (int i = 0; i < dm.num_layers; ++i) {
    const GdrT5EncLayer& ly = w->layers[i];
    GDR_CHECK_ARG(ly.ln_attn && ly.wqkv && ly.wo && ly.ln_ff && ly.wi && ly.wo_ff, "t5_encoder_ragged: layer %d null weight", i);
    if ((rc = launch_rmsnorm_bf16_dev(h, ly.ln_attn, abf, rows_dev, M, d, dm.eps, stream))) return rc;
    if ((rc = lin16(abf, ly.wqkv, qkv, 3 * inner, M, rows_dev, 3 * inner, d, 0, nullptr, qkv16 ? 1 : 0))) return rc;  // q,k,v: bf16 up to 128 tokens, fp32 above
    if ((rc = launch_attention(at, stream))) return rc;  // ctx -> abf as bf16 [rows, inner]
    if (pooled_only && i == dm.num_layers - 1) {
      // bf16 rows are inner/2 (d/2, d_ff/2) floats wide for the row mover
      if ((rc = launch_gather_rows(static_cast<const float*>(abf), seq_off, B, inner / 2, static_cast<float*>(ctx_cls16), stream)))
        return rc;
      if ((rc = launch_gather_rows(h, seq_off, B, d, h_cls, stream))) return rc;
      if ((rc = lin16(ctx_cls16, ly.wo, h_cls, d, B, nullptr, d, inner, 0, h_cls, 0))) return rc;
      if ((rc = launch_rmsnorm_bf16(h_cls, ly.ln_ff, nx_cls16, B, d, dm.eps, stream))) return rc;
      if ((rc = lin16(nx_cls16, ly.wi, ff_cls16, dm.d_ff, B, nullptr, dm.d_ff, d, 1, nullptr, 1))) return rc;
      if ((rc = lin16(ff_cls16, ly.wo_ff, h_cls, d, B, nullptr, d, dm.d_ff, 0, h_cls, 0))) return rc;
      return launch_rmsnorm(h_cls, w->final_ln, out_pooled, B, d, dm.eps, nullptr, 1, stream);
    }
    if ((rc = lin16(abf, ly.wo, h, d, M, rows_dev, d, inner, 0, h, 0))) return rc;
    if ((rc = launch_rmsnorm_bf16_dev(h, ly.ln_ff, abf, rows_dev, M, d, dm.eps, stream))) return rc;
    if ((rc = lin16(abf, ly.wi, ff, dm.d_ff, M, rows_dev, dm.d_ff, d, 1, nullptr, 1))) return rc;  // relu, bf16 out (in the ff buffer)
    if ((rc = lin16(ff, ly.wo_ff, h, d, M, rows_dev, d, dm.d_ff, 0, h, 0))) return rc;
  }
  if ((rc = launch_rmsnorm_dev(h, w->final_ln, nx, rows_dev, M, d, dm.eps, stream))) return rc;
  return unpack_rows(nx, r.plan, B, M, d, out_pooled, out_hidden, "t5_encoder_ragged", stream);
}

// ---- packed fp32 form.  big: the un-split forms (ragged_packs), with the token table, the last block's q on the CLS rows and the
//      pooled-only tail; otherwise (ragged_packs_small) the forms the padded forward picks for B*L rows, over the live rows only.
static int ragged_f32_blocks(const GdrT5EncoderWeights* w, const int64_t* ids, const int64_t* mask, int B, int L, float* out_hidden,
                             float* out_pooled, int64_t live_rows_hint, const EncBuf& e, const RagBuf& r, bool big, const EncChain* chain,
                             hipStream_t stream) {
  const GdrT5Dims& dm = w->dims;
  const int64_t M = (int64_t)B * L;
  const int d = dm.d_model, H = dm.num_heads, dk = dm.d_kv, inner = H * dk;
  float *h = e.h, *nx = e.nx, *qkv = e.qkv, *ctx = e.ctx, *ff = e.ff;
  float *ctx_cls = r.ctx_cls, *h_cls = r.h_cls, *nx_cls = r.nx_cls, *ff_cls = r.ff_cls;
  const int32_t *seq_off = r.plan.seq_off, *row_src = r.plan.row_src;
  const int64_t* rows_dev = r.plan.rows_dev;
  int rc;
  StreamK sk{};
  if ((rc = tower_streamk(e.splitk, &sk, "t5_encoder", stream))) return rc;
  int batch_linears = 0;  // two-chain form: chain A raises chain B's start event behind one of its first linears
  auto linear = [&](const float* A, int64_t lda, const float* W, float* C, int64_t ldc, int N, int K, int epi,
                    const float* residual) -> int {
    if (!big)  // the forms the padded forward picks for B*L rows (split-K / stream-K), over the live rows only
      return launch_linear_f32_ws(A, lda, W, K, C, ldc, M, N, K, epi, nullptr, residual, ldc, sk.part, ENC_SPLITK_BYTES, stream, &sk,
                                  rows_dev, live_rows_hint);
    GDR_TRY(launch_linear_f32_dev(A, lda, W, K, C, ldc, M, rows_dev, N, K, epi, nullptr, residual, ldc, live_rows_hint, stream, &sk,
                                  chain ? chain->grid_cap : 0));
    if (chain && chain->after && ++batch_linears == chain->after_linears && hipEventRecord(chain->after, stream) != hipSuccess) {
      set_error("t5_encoder_ragged: event record behind a linear failed");
      return GDR_EHIP;
    }
    return GDR_OK;
  };
  // Token table (un-split forms only): block 0's q/k/v depend on the token id alone — no position embedding, a per-row norm,
  // independent GEMM rows — so the caller may hand them in as a [vocab, 3*inner] table made with the same norm and the same
  // un-split linear (same k order: the bits of the launch it replaces).  One gather by ids[row_src[row]], with the embedding's
  // clamp, fills h and qkv; block 0's norm and qkv linear are not launched.  Rows of qkv past the live count stay unwritten
  // and unread (attention clamps to a sequence's last row).
  const float* qkv0 = big ? w->qkv0_table : nullptr;
  GDR_CHECK_ARG(!qkv0 || (((uintptr_t)qkv0) & 15) == 0, "t5_encoder_ragged: qkv0_table must be 16-byte aligned");
  if (qkv0)
    rc = launch_embed_packed2(w->embed, qkv0, ids, row_src, rows_dev, M, d, 3 * inner, dm.vocab_size, h, qkv, stream);
  else
    rc = launch_embed_packed(w->embed, ids, row_src, rows_dev, M, d, dm.vocab_size, h, stream);
  if (rc) return rc;

  AttnArgs at = self_attn_args(B, H, dk, L, 3 * inner, mask);
  attn_f32(at, qkv, ctx), attn_t5_bias(at, w->rel_bias, dm), attn_packed(at, r.plan);

  const bool pooled_only = out_hidden == nullptr && big;
  // exact A/B knob: 0 = the last block's q for every live row (one qkv launch)
  static const bool last_q_cls_on = env_flag("GDR_ENC_LAST_Q_CLS", ENC_LAST_Q_CLS_DEFAULT);
  for (int i = 0; i < dm.num_layers; ++i) {
    const GdrT5EncLayer& ly = w->layers[i];
    GDR_CHECK_ARG(ly.ln_attn && ly.wqkv && ly.wo && ly.ln_ff && ly.wi && ly.wo_ff, "t5_encoder_ragged: layer %d null weight", i);
    if (i == 0 && qkv0) {
      // q, k, v came with the embedding gather
    } else if (pooled_only && i == dm.num_layers - 1 && last_q_cls_on) {
      // only the CLS queries' context is read below: k and v over every live row, q for the B CLS rows alone.  The other q rows
      // keep what an earlier block left (or what the workspace held): each attention lane computes one query, and only ctx rows
      // seq_off[b] are gathered afterwards.  Un-split kernel for the B rows, as in the tail below: the full launch's bits.
      if ((rc = launch_rmsnorm_dev(h, ly.ln_attn, nx, rows_dev, M, d, dm.eps, stream))) return rc;
      if ((rc = linear(nx, d, ly.wqkv + (size_t)inner * d, qkv + inner, 3 * inner, 2 * inner, d, GDR_EPI_NONE, nullptr))) return rc;
      if ((rc = launch_gather_rows(nx, seq_off, B, d, nx_cls, stream))) return rc;
      if ((rc = launch_linear_f32(nx_cls, d, ly.wqkv, d, ctx_cls, inner, B, inner, d, GDR_EPI_NONE, nullptr, nullptr, 0, stream)))
        return rc;
      if ((rc = launch_scatter_rows_strided(ctx_cls, seq_off, B, inner, qkv, 3 * inner, stream))) return rc;
    } else {
      if ((rc = launch_rmsnorm_dev(h, ly.ln_attn, nx, rows_dev, M, d, dm.eps, stream))) return rc;
      if ((rc = linear(nx, d, ly.wqkv, qkv, 3 * inner, 3 * inner, d, GDR_EPI_NONE, nullptr))) return rc;
    }
    if ((rc = launch_attention(at, stream))) return rc;
    if (pooled_only && i == dm.num_layers - 1) {
      // only h[:,0] leaves this call: the rest of the block on the B CLS rows (packed row seq_off[b]); unsplit kernels,
      // so the k order — and with it every bit of the result — is that of the full-batch GEMMs
      if ((rc = launch_gather_rows(ctx, seq_off, B, inner, ctx_cls, stream))) return rc;
      if ((rc = launch_gather_rows(h, seq_off, B, d, h_cls, stream))) return rc;
      if ((rc = launch_linear_f32(ctx_cls, inner, ly.wo, inner, h_cls, d, B, d, inner, GDR_EPI_RESIDUAL, nullptr, h_cls, d, stream)))
        return rc;
      if ((rc = launch_rmsnorm(h_cls, ly.ln_ff, nx_cls, B, d, dm.eps, nullptr, 1, stream))) return rc;
      if ((rc = launch_linear_f32(nx_cls, d, ly.wi, d, ff_cls, dm.d_ff, B, dm.d_ff, d, GDR_EPI_RELU, nullptr, nullptr, 0, stream)))
        return rc;
      if ((rc = launch_linear_f32(ff_cls, dm.d_ff, ly.wo_ff, dm.d_ff, h_cls, d, B, d, dm.d_ff, GDR_EPI_RESIDUAL, nullptr, h_cls, d,
                                  stream)))
        return rc;
      return launch_rmsnorm(h_cls, w->final_ln, out_pooled, B, d, dm.eps, nullptr, 1, stream);
    }
    if ((rc = linear(ctx, inner, ly.wo, h, d, d, inner, GDR_EPI_RESIDUAL, h))) return rc;
    if ((rc = launch_rmsnorm_dev(h, ly.ln_ff, nx, rows_dev, M, d, dm.eps, stream))) return rc;
    if ((rc = linear(nx, d, ly.wi, ff, dm.d_ff, dm.d_ff, d, GDR_EPI_RELU, nullptr))) return rc;
    if ((rc = linear(ff, dm.d_ff, ly.wo_ff, h, d, d, dm.d_ff, GDR_EPI_RESIDUAL, h))) return rc;
  }
  // final_layer_norm over the live rows, then back into the [B,L,d] layout (PAD rows zero) and / or the CLS pool
  if ((rc = launch_rmsnorm_dev(h, w->final_ln, nx, rows_dev, M, d, dm.eps, stream))) return rc;
  return unpack_rows(nx, r.plan, B, M, d, out_pooled, out_hidden, "t5_encoder_ragged", stream);
}

// the packed entry points: checks, the two-chain hand-off, the pack plan, then the block sequence of the form that serves the call
static int ragged_impl(const GdrT5EncoderWeights* w, const int64_t* ids, const int64_t* mask, int B, int L, float* out_hidden,
                       float* out_pooled, int64_t live_rows_hint, void* workspace, size_t workspace_bytes, bool bf16,
                       hipStream_t stream, const EncChain* chain) {
  if (B == 0) return GDR_OK;
  GDR_TRY(check_t5_call("t5_encoder_ragged", w && ids && mask && workspace && (out_hidden || out_pooled), w, B, L, true));
  const GdrT5Dims& dm = w->dims;
  const EncWs ws = enc_ws(dm, (int64_t)B * L, true);
  const RagWs rw = rag_ws(dm, B, L, ws.total);
  // a chain's slice; a call: the documented size
  GDR_TRY(check_workspace("t5_encoder_ragged", workspace, workspace_bytes, chain ? rw.total : ragged_bytes(dm, B, L)));
  char* base = static_cast<char*>(workspace);
  if (!chain && !bf16 && !out_hidden && enc_chains_eligible(dm, B, L)) {
    // exact A/B knob: 1 = one chain, 2 = two half-batch chains in flight
    static const int chains = env_int("GDR_ENC_CHAINS", ENC_CHAINS_DEFAULT);
    // lab knob: chain B starts behind this many of chain A's linears; block 0 of a chain has three batch linears at least (o, wi, wo)
    static const int stagger = std::max(0, std::min(3, env_int("GDR_ENC_CHAIN_STAGGER", ENC_CHAIN_STAGGER_DEFAULT)));
    if (chains == 2) {
      if (EncSide* side = enc_side_acquire()) {
        const int rc2 = ragged_two_chains(w, ids, mask, B, L, out_pooled, live_rows_hint, base, stagger, side, stream);
        enc_side_release(side);
        return rc2;
      }
    }
  }
  const EncBuf e = carve_enc(base, ws);
  const RagBuf r = carve_rag(base, rw);
  GDR_TRY(launch_pack_plan(mask, B, L, r.plan, stream));
  const bool big = ragged_packs(dm, B, L);
  const bool small = !big && !bf16 && ragged_packs_small(dm, B, L);
  // bf16 precision mode: the packed form exists for the fused producer chain only
  if ((!big && !small) || (bf16 && !t5_fused16(*w))) {
    // small problem / other head size: the padded forward, then the rows that the packed form would not have computed
    // are zeroed so that the output contract does not depend on which form ran
    float* full = out_hidden ? out_hidden : e.qkv;  // qkv is dead when the final norm runs
    GDR_TRY(t5_encoder_impl(w, ids, mask, B, L, full, out_pooled, workspace, ws.total, bf16, stream));
    return out_hidden ? launch_zero_dead_rows(out_hidden, r.plan.seq_len, B, L, dm.d_model, stream) : GDR_OK;
  }
  if (bf16) return ragged_bf16_blocks(w, ids, mask, B, L, out_hidden, out_pooled, live_rows_hint, e, r, stream);
  return ragged_f32_blocks(w, ids, mask, B, L, out_hidden, out_pooled, live_rows_hint, e, r, big, chain, stream);
}
}  // namespace gdr

// ------------------------------------------------------------------------------------------------ split form (r06, exploratory)
// The ragged forward with every linear in the split-bf16 form (gemm_bf16.hip: fp32 operands carried as three bf16 planes, the six
// leading products on the bf16 MFMA path, fp32 accumulate — the fp32 linear's error against float64, not its bits).  Everything
// else — embedding, T5LayerNorm, attention (fp32 MFMA), residual stream, CLS tail — is the fp32 path's.  The linear weights of `w`
// point to plane-form bf16 rows [N, gdr_split_row_elems(K)]; activations are split by their producers' followers
// (split_f32_bf16x3_kernel) into one plane buffer.  Beside gdr_t5_encoder_forward_ragged, never instead of it.
namespace gdr {
// two plane buffers: one for the d_model / inner wide operands (normed rows, attention context), one for the d_ff wide ReLU output,
// which the wi GEMM's epilogue writes while it still reads the first
static size_t split_ws_a_bytes(const GdrT5Dims& dm, int64_t M) {  // sized for the bf16 x 3 form (the fp16 x 2 rows are shorter)
  const int inner = dm.num_heads * dm.d_kv;
  int ld = split_row_elems(dm.d_model);
  if (split_row_elems(inner) > ld) ld = split_row_elems(inner);
  return align_up((size_t)M * ld * 2, 256);
}
static size_t split_ws_bytes(const GdrT5Dims& dm, int64_t M) {
  return split_ws_a_bytes(dm, M) + align_up((size_t)M * split_row_elems(dm.d_ff) * 2, 256);
}

static int ragged_split_impl(const GdrT5EncoderWeights* w, const int64_t* ids, const int64_t* mask, int B, int L, float* out_hidden,
                             float* out_pooled, int64_t live_rows_hint, int terms, void* workspace, size_t workspace_bytes,
                             hipStream_t stream) {
  if (B == 0) return GDR_OK;
  GDR_CHECK_ARG(terms == 6 || terms == 3 || terms == 2, "t5_encoder_split: terms must be 6 or 3 (bf16 planes) or 2 (fp16 x 2)");
  const int f16 = terms == 2 ? 1 : 0;
  GDR_TRY(check_t5_call("t5_encoder_split", w && ids && mask && workspace && (out_hidden || out_pooled), w, B, L, false));
  const GdrT5Dims& dm = w->dims;
  const int d = dm.d_model, H = dm.num_heads, dk = dm.d_kv, inner = H * dk, dff = dm.d_ff;
  GDR_CHECK_ARG(dk == 64 && d % 64 == 0 && inner % 64 == 0 && dff % 64 == 0,
                "t5_encoder_split: needs d_kv = 64 and d_model, inner, d_ff multiples of 64 (the packed attention and the LDS-DMA linear)");
  const int64_t M = (int64_t)B * L;
  const EncWs ws = enc_ws(dm, M, true);
  const RagWs rw = rag_ws(dm, B, L, ws.total);
  const size_t planes_off = rw.total, total = planes_off + split_ws_bytes(dm, M);
  GDR_TRY(check_workspace("t5_encoder_split", workspace, workspace_bytes, total));
  char* base = static_cast<char*>(workspace);
  const EncBuf e = carve_enc(base, ws);
  const RagBuf r = carve_rag(base, rw);
  int rc;
  if ((rc = launch_pack_plan(mask, B, L, r.plan, stream))) return rc;
  float *h = e.h, *nx = e.nx, *qkv = e.qkv, *ctx = e.ctx, *ff = e.ff;
  float *ctx_cls = r.ctx_cls, *h_cls = r.h_cls, *nx_cls = r.nx_cls, *ff_cls = r.ff_cls;
  const int32_t* seq_off = r.plan.seq_off;
  const int64_t* rows_dev = r.plan.rows_dev;
  void* planes = base + planes_off;                                  // d_model / inner wide operands
  void* planes_ff = base + planes_off + split_ws_a_bytes(dm, M);     // the d_ff wide ReLU output of wi
  // A/B knob: 0 = every operand split by a launch of its own (split_f32_bf16x3_kernel)
  static const bool fuse_on = env_flag("GDR_SPLIT_FUSE", true);
  // the split GEMM over plane rows P [rows, split_row_elems(K)]; out_planes: the output leaves as plane rows (row stride ldc elements)
  const GldsLinear glds{"t5_encoder_split", live_rows_hint, terms, stream};
  auto gemm = [&](const void* P, const float* W, void* C, int64_t ldc, int64_t rows, const int64_t* md, int N, int K, int act,
                  const float* residual, int out_planes) -> int {
    return linear_glds(glds, P, W, C, ldc, rows, md, N, K, act, nullptr, residual, out_planes ? (f16 ? 3 : 2) : 0);
  };
  // one linear over `rows` fp32 rows (md: their device-side count, or null): split the operand into planes, then the split GEMM
  auto linear = [&](const float* A, const float* W, float* C, int64_t ldc, int64_t rows, const int64_t* md, int N, int K, int act,
                    const float* residual) -> int {
    void* P = K == dff ? planes_ff : planes;
    if (int rc_ = launch_split_f32_bf16x3(A, K, P, split_row_elems(K, f16), rows, K, md, stream, f16)) return rc_;
    return gemm(P, W, C, ldc, rows, md, N, K, act, residual, 0);
  };
  // from 8 192 rows the norms write the operand planes themselves; the wi GEMM's plane epilogue lives in the 256-row tile kernel only,
  // which the launcher picks by the VIRTUAL contraction length (6 K0 / 3 K0 >= 2 048: not at d_model = 512 with 3 terms or fp16 x 2) —
  // asked here with the launcher's own predicate; where it says no, wi stores fp32 and a split launch makes wo_ff's planes
  const bool fuse = fuse_on && M >= 8192;
  const bool fuse_wi = fuse && linear_bf16_tile_form(M, dff, d, 0, f16 ? 3 : 2, terms) >= 192;
  const int ld_d = split_row_elems(d, f16), ld_ff = split_row_elems(dff, f16);
  if ((rc = launch_embed_packed(w->embed, ids, r.plan.row_src, rows_dev, M, d, dm.vocab_size, h, stream))) return rc;
  AttnArgs at = self_attn_args(B, H, dk, L, 3 * inner, mask);
  attn_f32(at, qkv, ctx), attn_t5_bias(at, w->rel_bias, dm), attn_packed(at, r.plan);
  const bool pooled_only = out_hidden == nullptr;
  for (int i = 0; i < dm.num_layers; ++i) {
    const GdrT5EncLayer& ly = w->layers[i];
    GDR_CHECK_ARG(ly.ln_attn && ly.wqkv && ly.wo && ly.ln_ff && ly.wi && ly.wo_ff, "t5_encoder_split: layer %d null weight", i);
    if (fuse) {  // the norm writes the operand's planes itself (no fp32 copy, no split launch)
      if ((rc = launch_rmsnorm_planes(h, ly.ln_attn, nullptr, planes, ld_d, rows_dev, M, d, dm.eps, stream, f16))) return rc;
      if ((rc = gemm(planes, ly.wqkv, qkv, 3 * inner, M, rows_dev, 3 * inner, d, 0, nullptr, 0))) return rc;
    } else {
      if ((rc = launch_rmsnorm_dev(h, ly.ln_attn, nx, rows_dev, M, d, dm.eps, stream))) return rc;
      if ((rc = linear(nx, ly.wqkv, qkv, 3 * inner, M, rows_dev, 3 * inner, d, 0, nullptr))) return rc;
    }
    if ((rc = launch_attention(at, stream))) return rc;
    if (pooled_only && i == dm.num_layers - 1) {
      if ((rc = launch_gather_rows(ctx, seq_off, B, inner, ctx_cls, stream))) return rc;
      if ((rc = launch_gather_rows(h, seq_off, B, d, h_cls, stream))) return rc;
      if ((rc = linear(ctx_cls, ly.wo, h_cls, d, B, nullptr, d, inner, 0, h_cls))) return rc;
      if ((rc = launch_rmsnorm(h_cls, ly.ln_ff, nx_cls, B, d, dm.eps, nullptr, 1, stream))) return rc;
      if ((rc = linear(nx_cls, ly.wi, ff_cls, dff, B, nullptr, dff, d, 1, nullptr))) return rc;
      if ((rc = linear(ff_cls, ly.wo_ff, h_cls, d, B, nullptr, d, dff, 0, h_cls))) return rc;
      return launch_rmsnorm(h_cls, w->final_ln, out_pooled, B, d, dm.eps, nullptr, 1, stream);
    }
    if ((rc = linear(ctx, ly.wo, h, d, M, rows_dev, d, inner, 0, h))) return rc;
    if (fuse_wi) {  // norm -> planes; wi's ReLU epilogue writes the planes of wo_ff's operand
      if ((rc = launch_rmsnorm_planes(h, ly.ln_ff, nullptr, planes, ld_d, rows_dev, M, d, dm.eps, stream, f16))) return rc;
      if ((rc = gemm(planes, ly.wi, planes_ff, ld_ff, M, rows_dev, dff, d, 1, nullptr, 1))) return rc;
      if ((rc = gemm(planes_ff, ly.wo_ff, h, d, M, rows_dev, d, dff, 0, h, 0))) return rc;
    } else if (fuse) {  // norm -> planes; wi stores fp32 (no plane epilogue at this virtual K), then the split launch for wo_ff
      if ((rc = launch_rmsnorm_planes(h, ly.ln_ff, nullptr, planes, ld_d, rows_dev, M, d, dm.eps, stream, f16))) return rc;
      if ((rc = gemm(planes, ly.wi, ff, dff, M, rows_dev, dff, d, 1, nullptr, 0))) return rc;
      if ((rc = linear(ff, ly.wo_ff, h, d, M, rows_dev, d, dff, 0, h))) return rc;
    } else {
      if ((rc = launch_rmsnorm_dev(h, ly.ln_ff, nx, rows_dev, M, d, dm.eps, stream))) return rc;
      if ((rc = linear(nx, ly.wi, ff, dff, M, rows_dev, dff, d, 1, nullptr))) return rc;
      if ((rc = linear(ff, ly.wo_ff, h, d, M, rows_dev, d, dff, 0, h))) return rc;
    }
  }
  if ((rc = launch_rmsnorm_dev(h, w->final_ln, nx, rows_dev, M, d, dm.eps, stream))) return rc;
  return unpack_rows(nx, r.plan, B, M, d, out_pooled, out_hidden, "t5_encoder_split", stream);
}
}  // namespace gdr

extern "C" size_t gdr_t5_encoder_split_workspace_bytes(const GdrT5Dims* dims, int B, int L) {
  if (!dims || B <= 0 || L <= 0) return 0;
  const int64_t M = (int64_t)B * L;
  return gdr::rag_ws(*dims, B, L, gdr::enc_ws(*dims, M, true).total).total + gdr::split_ws_bytes(*dims, M);
}

extern "C" int gdr_t5_encoder_forward_ragged_split(const GdrT5EncoderWeights* w, const int64_t* ids, const int64_t* mask, int B, int L,
                                                   float* out_hidden, float* out_pooled, int64_t live_rows_hint, int terms,
                                                   void* workspace, size_t workspace_bytes, void* stream_) {
  return gdr::ragged_split_impl(w, ids, mask, B, L, out_hidden, out_pooled, live_rows_hint, terms, workspace, workspace_bytes,
                                static_cast<hipStream_t>(stream_));
}

extern "C" int gdr_t5_encoder_forward_ragged(const GdrT5EncoderWeights* w, const int64_t* ids, const int64_t* mask, int B,
                                             int L, float* out_hidden, float* out_pooled, int64_t live_rows_hint,
                                             void* workspace, size_t workspace_bytes, void* stream_) {
  return gdr::ragged_impl(w, ids, mask, B, L, out_hidden, out_pooled, live_rows_hint, workspace, workspace_bytes, false,
                          static_cast<hipStream_t>(stream_));
}

extern "C" int gdr_t5_encoder_forward_ragged_bf16(const GdrT5EncoderWeights* w, const int64_t* ids, const int64_t* mask, int B,
                                                  int L, float* out_hidden, float* out_pooled, int64_t live_rows_hint,
                                                  void* workspace, size_t workspace_bytes, void* stream_) {
  return gdr::ragged_impl(w, ids, mask, B, L, out_hidden, out_pooled, live_rows_hint, workspace, workspace_bytes, true,
                          static_cast<hipStream_t>(stream_));
}

extern "C" size_t gdr_t5_encoder_bf16_workspace_bytes(const GdrT5Dims* dims, int B, int L) {
  if (!dims || B <= 0 || L <= 0) return 0;
  return gdr::enc_ws(*dims, (int64_t)B * L, true).total;
}

extern "C" int gdr_t5_encoder_forward_bf16(const GdrT5EncoderWeights* w, const int64_t* ids, const int64_t* mask, int B,
                                           int L, float* out_hidden, float* out_pooled, void* workspace,
                                           size_t workspace_bytes, void* stream_) {
  return gdr::t5_encoder_impl(w, ids, mask, B, L, out_hidden, out_pooled, workspace, workspace_bytes, true,
                              static_cast<hipStream_t>(stream_));
}
