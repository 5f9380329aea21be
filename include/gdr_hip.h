/*
 * gdr_hip.h — C ABI of libgdr_hip.so, the MI355X (gfx950) implementation of GDR's inference hot path.
 *
 * The reference (ypw0102/GDR) has no FFI: its boundary is the Python call surface of
 * GDR_model/main_models.py / GDR_model/transformers.  gdr_amd/modeling.py keeps
 * that surface (generate(), get_encoder(), encode_query(), compute_similarity()) and binds the entry
 * points below with ctypes (gdr_amd/_ffi.py); INTEGRATION.md shows the stub a reference maintainer
 * would add.  Each entry point names the reference call site it replaces.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (tensor.data_ptr()); outputs are
 *     pre-allocated by the caller; the library allocates nothing — scratch comes from the caller's
 *     workspace, sized by the matching *_workspace_bytes();
 *   - `stream` is a hipStream_t passed as void* (0 = default stream); calls are asynchronous on it and
 *     contain no host synchronisation (hipGraph-capturable);
 *   - return 0 on success, a negative GDR_E* code otherwise; gdr_last_error() gives the thread-local
 *     message; no exceptions cross the ABI.  Re-entrant from several host threads and for several devices in one
 *     process (the device current in the calling thread is the one used): the only process-wide state is the
 *     thread-local message, a mutex-guarded (kernel, device) table of raised dynamic-LDS limits, a mutex-guarded pool
 *     of per-device side streams that gdr_t5_generate leases per call, and the opt-in profiler below (single-threaded);
 *   - row-major fp32 unless stated; ids int64 where the reference uses LongTensor inputs, int32 for
 *     doc ids produced on device.
 */
#ifndef GDR_HIP_H
#define GDR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GDR_OK 0
#define GDR_EINVAL (-1)   /* bad argument (shape, alignment, null pointer) */
#define GDR_ENOSPC (-2)   /* workspace too small */
#define GDR_EHIP (-3)     /* HIP runtime error at launch, or a device-side failure of an EARLIER launch (see stream-K below) */

const char* gdr_last_error(void);
int gdr_abi_version(void);
/* Kernel launches this library has enqueued in this process so far (every entry point, every stream): a monitoring counter —
 * bench.py reports launches per generate() call from it. */
int64_t gdr_launch_count(void);

/* Opt-in launch profiler used by bench.py for the roofline line: while enabled, every launch of the dense
 * kernels is bracketed by a hipEvent pair recorded on the stream it is launched on.  Process-global, not
 * thread-safe, off by default (then no event is created or recorded).  gdr_prof_collect synchronises,
 * fills three host arrays of length 8 indexed by kernel class {0 linear GEMM, 1 sim sample GEMM,
 * 2 sim filter GEMM} with {launch count, total ms, total flops}, and disables the profiler again.
 * total ms of a class is the length of the UNION of its launches' [start, stop] intervals on one time axis, not the sum
 * of their durations: launches that overlap (the two chains of gdr_t5_encoder_forward_ragged, two batches in flight on
 * two streams) share the chip, and summing them would count that time twice.  Without overlap the two are equal. */
int gdr_prof_enable(int max_events);
int gdr_prof_collect(int64_t* launches, double* total_ms, double* total_work);
/* Sampling: while the gate is 0 an enabled profiler records nothing (and costs nothing).  Two hipEventRecord packets per launch are
 * not free — around every dense launch of the C2 step they took 2.4 % of its throughput (28.69 k against 28.02 k q/s, r05) —, so
 * bench.py opens the gate for every 4th step of its timed region only.  The gate is open after gdr_prof_enable. */
void gdr_prof_gate(int on);

/* ------------------------------------------------------------------------------------------------
 * Dense linear:  C[M,N] = epilogue(A[M,K] · W[N,K]^T)      (nn.Linear layout, both K-contiguous)
 * replaces every `nn.Linear` / `torch.matmul` call site on the path:
 *   transformers/modeling_t5.py:360-364,413 (q/k/v/o), :182-185 (wi/ReLU/wo), :1634 (adaptor_linear),
 *   dense.py:21-23 (pooler), torch nn.TransformerDecoderLayer linears (modeling_t5.py:1241-1244).
 * fp32 in / fp32 accumulate on v_mfma_f32_32x32x2_f32 (bit-identical to a k-ordered fmaf chain).
 * K % 4 == 0; lda/ldw/ldc in elements, multiples of 4.  `residual` may alias C.
 * ---------------------------------------------------------------------------------------------- */
enum {
  GDR_EPI_NONE = 0,
  GDR_EPI_RESIDUAL = 1,       /* C = acc + residual                     (h + dropout(y), modeling_t5.py:199,452) */
  GDR_EPI_RELU = 2,           /* C = max(acc, 0)                        (modeling_t5.py:183)                      */
  GDR_EPI_BIAS = 3,           /* C = acc + bias[n]                                                                */
  GDR_EPI_BIAS_RELU = 4,      /* C = max(acc + bias[n], 0)              (TransformerDecoderLayer linear1)         */
  GDR_EPI_BIAS_RESIDUAL = 5,  /* C = acc + bias[n] + residual                                                     */
  GDR_EPI_BIAS_GELU = 6       /* C = gelu_erf(acc + bias[n])            (BERT intermediate, modeling_bert.py)     */
};
int gdr_linear_f32(const float* A, int64_t lda, const float* W, int64_t ldw, float* C, int64_t ldc,
                   int64_t M, int N, int K, int epilogue, const float* bias, const float* residual,
                   int64_t ldr, void* stream);
/* Same, with a scratch buffer: when the 128x128 tile grid cannot fill the 256 CUs (decode-time linears with
 * M = batch*beams rows) the K dimension is split into partial slabs [S][M][N] in `workspace` and reduced in fixed
 * order (deterministic) by a second kernel that applies the epilogue.  workspace may be NULL (= gdr_linear_f32).
 * A workspace of at least 33 558 528 bytes (512 x 64 KiB + 4 KiB) also serves grids of more than 256 tiles: the last
 * tiles of a launch are then dealt by K-step ranges with an exact accumulator hand-off between workgroups (bit-identical
 * to whole tiles, DESIGN.md §4 "stream-K tail") instead of leaving CUs idle in a partial last round of tiles.
 * Co-residency: that form launches at most 512 workgroups (2 per CU) and a workgroup waits for its predecessor's
 * accumulators, so all of them must become resident while the launch runs — true on an otherwise idle or normally shared
 * GPU.  If another kernel keeps a predecessor off the chip for seconds, the waiting workgroup stops waiting, the launch
 * finishes with INVALID output, and the next linear launched through this library returns GDR_EHIP once (no trap, no hang);
 * the same holds for the encoder / decode entry points, which use this form internally. */
int gdr_linear_f32_splitk(const float* A, int64_t lda, const float* W, int64_t ldw, float* C, int64_t ldc,
                          int64_t M, int N, int K, int epilogue, const float* bias, const float* residual,
                          int64_t ldr, void* workspace, size_t workspace_bytes, void* stream);

/* Which kernel form a DENSE launch (lda = ldw = K) of gdr_linear_f32 (workspace_bytes = 0) or gdr_linear_f32_splitk gets (host-only, no
 * GPU work; for tests and profiles, like gdr_linear_bf16_tile_form below); 0 = a shape the linear refuses. */
#define GDR_F32_FORM_TILES 1         /* one 128x128 tile per workgroup                                          */
#define GDR_F32_FORM_PERSISTENT 2    /* more than 512 tiles: 512 workgroups walk the tiles                      */
#define GDR_F32_FORM_SMALL 3         /* 64x64 tiles (few rows), whole K                                         */
#define GDR_F32_FORM_SMALL_SPLITK 4  /* 64x64 tiles, K slabs in the workspace + fixed-order reduction           */
#define GDR_F32_FORM_SPLITK 5        /* 128x128 tiles, K slabs in the workspace + fixed-order reduction         */
#define GDR_F32_FORM_STREAMK_256 6   /* 256 < tiles <= 512: stream-K on 256 workgroups                          */
#define GDR_F32_FORM_STREAMK_TAIL 7  /* more than 512 tiles: whole-tile rounds, then the stream-K tail          */
int gdr_linear_f32_form(int64_t M, int N, int K, size_t workspace_bytes);

/* bf16 operands (A [M,K], W [N,K] bf16, round-to-nearest-even of the fp32 tensors), fp32 accumulate, epilogue and output:
 * the linear of the opt-in bf16 precision mode (BASELINE config C5; the reference itself runs precision=32).  K, lda,
 * ldw multiples of 8.  K % 64 == 0 takes the LDS-DMA kernel (gemm_bf16.hip), other K the generic core. */
int gdr_linear_bf16(const void* A, int64_t lda, const void* W, int64_t ldw, float* C, int64_t ldc, int64_t M, int N,
                    int K, int epilogue, const float* bias, const float* residual, int64_t ldr, void* stream);
/* EXPLORATORY (r06), beside the fp32 linear, never instead of it: fp32 operands carried as three bf16 planes — x = hi + mid + lo, hi =
 * bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid) (gdr_split_f32_bf16x3: fp32 [rows, K] -> bf16 [rows, ld_out >= 3K], a row = [hi | mid | lo | pad]) —
 * and a linear that keeps the six leading products hi.hi + hi.mid + mid.hi + hi.lo + lo.hi + mid.mid on the bf16 MFMA path, fp32 accumulate
 * (the call sites of gdr_linear_f32: modeling_t5.py:360-364,413,182-185).  24 significand bits are carried: the error against float64 is
 * that of the strict-fp32 MFMA linear (tools/exp_split_bf16.py), the bits are not.  A3 [M, lda >= 3K], W3 [N, ldw >= 3K] bf16; K % 64 == 0. */
int gdr_split_row_elems(int K, int terms);   /* row length (elements) of a plane-form operand: 3 K (terms 6 / 3) or 2 K (terms 2), rounded up to 64 */
int gdr_split_f32_bf16x3(const float* in, void* out_planes, int64_t rows, int K, int64_t ld_out, void* stream);
/* fp16 x 2 planes (terms = 2 below): a row = [hi | lo'] with hi = fp16(x), lo' = fp16((x - hi) * 2^11) — 22 significand bits; the linear
 * computes hi.hi + 2^-11 (hi.lo' + lo'.hi) on v_mfma_f32_16x16x32_f16 (three K-blocks, the two cross blocks first, scaled, then hi.hi).
 * |x| must stay below fp16's 65 504 (normed activations, ReLU outputs and weights of the path do; a residual stream would not). */
int gdr_split_f32_f16x2(const float* in, void* out_planes, int64_t rows, int K, int64_t ld_out, void* stream);
/* terms = 6: the form above.  terms = 2: the fp16 x 2 form (A3 / W3 rows [hi | lo'], lda / ldw >= 2 K, K % 128 == 0).  terms = 3: hi.hi + hi.mid + mid.hi only — 16 significand bits, NARROWER than fp32 (error ~3e-5 of mean |c|
 * against fp32's ~8e-6 on the encoder's shapes), half the MFMA work: a measured knob, reported as such, never called fp32. */
int gdr_linear_split_bf16(const void* A3, int64_t lda, const void* W3, int64_t ldw, float* C, int64_t ldc, int64_t M, int N, int K,
                          int terms, int epilogue, const float* bias, const float* residual, int64_t ldr, void* stream);
/* Which tile form gdr_linear_bf16 gives a well-aligned [M,K] x [N,K] launch (host-only, no GPU work; for tests and profiles):
 * 64 / 128 = the 128-column kernel with 64- / 128-row tiles, 192 / 256 = the 256-row tile of that width, 0 = generic core. */
int gdr_linear_bf16_tile_form(int64_t M, int N, int K, int epilogue);

/* T5LayerNorm (modeling_t5.py:164-171): y = w * (x / sqrt(mean(x^2) + eps)) per row, fp32 — the norm every T5 block of the
 * path applies, as an operator of its own.  The quotient is the IEEE division's, bit for bit (the kernels divide a row by its
 * one denominator with a correctly rounded reciprocal and one exact-residual correction per element).  x, y fp32 [rows, d],
 * d % 4 == 0; y may alias x. */
int gdr_t5_layer_norm(const float* x, const float* w, float* y, int64_t rows, int d, float eps, void* stream);

/* y[r] = x[r] / max(||x[r]||_2, eps) — `torch.nn.functional.normalize(rep, dim=-1)` of DensePooler (dense.py:24-25;
 * torch's eps is 1e-12).  x, y fp32 [rows, d]; y may alias x. */
int gdr_l2_normalize(const float* x, float* y, int64_t rows, int d, float eps, void* stream);

/* ------------------------------------------------------------------------------------------------
 * T5 encoder forward — replaces `model.get_encoder()(input_ids, attention_mask=, return_dict=True)
 * .last_hidden_state` (transformers/modeling_t5.py:685-821; called at generation_utils.py:410-411).
 * Weights: pointer table built once from the reference state_dict; wqkv is the
 * row-concatenation [q;k;v] of the three [inner,d] projection matrices.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  int32_t vocab_size, d_model, d_kv, d_ff, num_heads, num_layers;
  int32_t rel_buckets, rel_max_distance;
  float eps;
} GdrT5Dims;

typedef struct {
  const float* ln_attn;   /* [d]            block.i.layer.0.layer_norm.weight              */
  const float* wqkv;      /* [3*inner, d]   layer.0.SelfAttention.{q,k,v}.weight row-concat */
  const float* wo;        /* [d, inner]     layer.0.SelfAttention.o.weight                 */
  const float* ln_ff;     /* [d]            layer.1.layer_norm.weight                      */
  const float* wi;        /* [d_ff, d]      layer.1.DenseReluDense.wi.weight               */
  const float* wo_ff;     /* [d, d_ff]      layer.1.DenseReluDense.wo.weight               */
} GdrT5EncLayer;

typedef struct {
  GdrT5Dims dims;
  const float* embed;       /* [vocab, d]     shared.weight                                          */
  const float* rel_bias;    /* [buckets, H]   encoder.block.0...relative_attention_bias.weight       */
  const float* final_ln;    /* [d]            encoder.final_layer_norm.weight                        */
  const GdrT5EncLayer* layers;  /* host array of num_layers entries (device pointers inside)        */
  const float* qkv0_table;  /* optional [vocab_size, 3*inner] fp32, NULL = compute: row id holds block 0's q/k/v of token id,
                             * rmsnorm(embed[id], layers[0].ln_attn) x layers[0].wqkv^T as gdr_t5_layer_norm + gdr_linear_f32
                             * give it.  Read by gdr_t5_encoder_forward_ragged alone (see there); a snapshot of the weights. */
} GdrT5EncoderWeights;

size_t gdr_t5_encoder_workspace_bytes(const GdrT5Dims* dims, int B, int L);
/* ids/mask int64[B,L]; out_hidden fp32[B,L,d]; optional out_pooled fp32[B,d] = hidden[:,0]
 * (CLS pool, main_models.py:102-109 / dense.py:39,50) or NULL.
 * 1 <= L <= 512 in every T5 encoder form below (the reference's T5Stack takes any length; --max_input_length is a free flag).  Up to
 * 128 tokens the one-pass attention kernels serve every head width; above, d_kv = 64 takes the key-block kernel with T5's relative
 * position bias (csrc/attention_long.hip, padded and packed layout, fp32 q / k / v in every precision mode: the bf16 mode keeps
 * q, k, v in fp32 there), another head width the generic kernel while the K / V rows of one (sequence, head) fit in LDS (d_kv = 16 at
 * L = 512 does; d_kv = 128 does not: GDR_EINVAL naming d_kv and L). */
int gdr_t5_encoder_forward(const GdrT5EncoderWeights* w, const int64_t* ids, const int64_t* mask, int B, int L,
                           float* out_hidden, float* out_pooled, void* workspace, size_t workspace_bytes,
                           void* stream);

/* Ragged form of the same forward: only the token rows that can reach the requested outputs are computed.
 *   - PAD rows are dropped: a sequence whose mask row is a non-empty prefix of ones (right padding, what the reference's
 *     tokenizer emits) keeps its first sum(mask) positions; any other mask row (empty, holes, left padding) keeps all L
 *     positions and its mask, so every case the reference handles is still handled.  Kept rows are bit-identical to
 *     gdr_t5_encoder_forward (GEMM rows are independent; a PAD key adds exp(-1e9 - max) = 0 to a live query's softmax).
 *   - out_hidden (may be NULL): kept rows exact, dropped rows ZERO — they are not the reference's values there, which is
 *     why model.get_encoder() / gdr_t5_encoder_forward stay the exact default; the decode path (cross-attention masks
 *     those keys) and the CLS pool never read them.
 *   - out_pooled (may be NULL; one of the two must be given) = hidden[:,0].  With out_hidden == NULL the last block's
 *     o / wi / wo and the final norm run on the B CLS rows only.
 *   - the live-row count is derived from the mask ON THE DEVICE; kernels read it, the call never synchronises.
 *     live_rows_hint: that count if the host happens to know it, else -1 — a TUNING input: the launcher picks between
 *     kernel forms that are bit-identical to one another (whole tiles, the stream-K tail, the 256-workgroup launch) by the
 *     tile count it implies, and the opt-in profiler (gdr_prof_*) prices flops with it; a wrong or absent hint can cost
 *     speed, never a bit of the result.
 * Batches of fewer than 256 token rows, or d_kv != 64, run the padded form internally (same outputs); below 4 096 token
 * rows the packed form runs on the split-K / stream-K kernel forms the padded forward picks for the same B*L (kept rows
 * still bit-identical) and the pooled-only shortcut of the last block is not taken.
 * From 192 tiles of 128 x 128 over B*L x d_model (the form with the pooled-only shortcut) two more pieces of work that the
 * result does not need are left out, both exact:
 *   - w->qkv0_table != NULL: block 0's q/k/v are a function of the token id alone (T5 adds no position embedding, the norm is
 *     per row, GEMM rows are independent), so they are gathered from the table by the id that also picks the embedding row —
 *     one launch for both — instead of a norm and a [rows, 3*inner, d_model] linear per call.  Smaller batches, the padded
 *     form, the bf16 mode and the split form never read the field.
 *   - pooled-only, last block (GDR_ENC_LAST_Q_CLS, see README): k and v over every live row, q for the B CLS rows alone
 *     (gather, un-split linear, scatter into the q columns); the other q rows are stale and feed attention lanes whose
 *     output nothing reads.
 * Two chains (GDR_ENC_CHAINS=1|2, read once per process; default 2): a pooled-only fp32 call (out_hidden == NULL) whose halves
 * [0, B/2) and [B/2, B) each reach those 192 tiles, with at least two layers, runs the halves as two independent forwards, the
 * first on `stream`, the second on a library-owned side stream forked from and joined to `stream` by events before the call
 * returns: the caller sees one stream-ordered call, and a stream capture of it stays legal.  Every persistent / stream-K linear
 * of a chain is launched on 256 workgroups, so the call never has more than 512 of them in flight (the co-residency the
 * stream-K hand-off assumes).  Same bits as one chain.  Calls with out_hidden, the bf16 and split forms and the padded form
 * always run one chain.
 * Workspace size rule: S1(B) = the one-chain layout for B sequences (activations for B*L rows, one split-K / stream-K region,
 * the pack plan and the CLS tail's rows).  gdr_t5_encoder_ragged_workspace_bytes = S1(B) when the halves do not qualify, else
 * max(S1(B), S1(B/2) + S1(B - B/2)): each chain owns a whole layout — its own stream-K hand-off scratch, flags and epoch
 * included — which adds about one split-K region (112 MiB) to S1(B).  The size does not depend on the knob. */
size_t gdr_t5_encoder_ragged_workspace_bytes(const GdrT5Dims* dims, int B, int L);
int gdr_t5_encoder_forward_ragged(const GdrT5EncoderWeights* w, const int64_t* ids, const int64_t* mask, int B, int L,
                                  float* out_hidden, float* out_pooled, int64_t live_rows_hint, void* workspace,
                                  size_t workspace_bytes, void* stream);

/* The ragged form in the bf16 precision mode below (weights as for gdr_t5_encoder_forward_bf16): same contract, kept rows
 * bit-identical to gdr_t5_encoder_forward_bf16.  The packed kernels serve the fused bf16 chain (d_model, inner and d_ff
 * multiples of 64); other shapes run the padded bf16 form internally.  gdr_t5_encoder_ragged_workspace_bytes serves both. */
int gdr_t5_encoder_forward_ragged_bf16(const GdrT5EncoderWeights* w, const int64_t* ids, const int64_t* mask, int B, int L,
                                       float* out_hidden, float* out_pooled, int64_t live_rows_hint, void* workspace,
                                       size_t workspace_bytes, void* stream);
/* EXPLORATORY (r06), beside gdr_t5_encoder_forward_ragged, never instead of it: the ragged forward with every linear in the split-bf16
 * form of gdr_linear_split_bf16 (24 significand bits carried through bf16 MFMAs; the fp32 linear's error, not its bits); embedding,
 * T5LayerNorm, attention and the residual stream are the fp32 path's.  The linear weight pointers of `w` (wqkv, wo, wi, wo_ff) point
 * to plane-form bf16 rows [N, gdr_split_row_elems(K)] made by gdr_split_f32_bf16x3.  Needs d_kv = 64 and d_model, inner, d_ff
 * multiples of 64.  Hidden states within 2e-4 of the reference golden like the fp32 path (tests/test_gpu_parity.py). */
size_t gdr_t5_encoder_split_workspace_bytes(const GdrT5Dims* dims, int B, int L);
int gdr_t5_encoder_forward_ragged_split(const GdrT5EncoderWeights* w, const int64_t* ids, const int64_t* mask, int B, int L,
                                        float* out_hidden, float* out_pooled, int64_t live_rows_hint, int terms, void* workspace,
                                        size_t workspace_bytes, void* stream);   /* terms: 6 / 3 (weights as bf16 planes) or 2 (weights as fp16 x 2 rows), as gdr_linear_split_bf16 */

/* bf16 precision mode (BASELINE config C5): the SAME structs, but the four linear weights of every layer (wqkv, wo, wi,
 * wo_ff) point to bf16 [N,K] matrices (round-to-nearest-even of the fp32 checkpoint, e.g. gdr_cast_f32_bf16); the
 * `const float*` field type is nominal for them.  Each linear rounds its activation operand to bf16 and accumulates in
 * fp32; with d_kv = 64 (the MFMA attention form) and L <= 128 the qkv linear also EMITS q, k, v as bf16 — QK^T and PV take those
 * rounded operands, accumulate in fp32, softmax in fp32; embedding, norms, the residual stream and both outputs stay fp32.  The
 * reference has no such mode (it runs precision=32, main.py:61,91): parity is against the fp32 path within bf16
 * tolerance and against the oracle's bf16 emulation (oracle/t5_ref.py bf16_linears). */
size_t gdr_t5_encoder_bf16_workspace_bytes(const GdrT5Dims* dims, int B, int L);
int gdr_t5_encoder_forward_bf16(const GdrT5EncoderWeights* w, const int64_t* ids, const int64_t* mask, int B, int L,
                                float* out_hidden, float* out_pooled, void* workspace, size_t workspace_bytes,
                                void* stream);

/* ------------------------------------------------------------------------------------------------
 * Corpus similarity + top-k, fused: never materialises the [B,N] score matrix.
 * replaces `compute_similarity` (dense.py:53-54, encoder.py:128-129: q @ p.T) followed by
 * `Tensor.topk(k, largest=True, sorted=True)` (as at main_models.py:1625).
 *   Q fp32[B,d], D fp32[N,d] (the resident corpus shard) -> out_val fp32[B,k] descending,
 *   out_idx int32[B,k] = row in D + idx_offset (idx_offset + N <= 2^31 - 1, else GDR_EINVAL: the largest id is 2^31 - 2).
 *   Ties: higher score first, then lower id.  Scores are ordered by the IEEE
 *   total order of their fp32 bit patterns (the kernels' sort keys), which differs from comparison by value in ONE place:
 *   +0.0 ranks above -0.0 whatever the ids.  The same holds for gdr_sim_topk_bf16 / _prefilter, gdr_topk_merge,
 *   gdr_topk_merge_packed and gdr_rerank_topk*; a NaN score is not ordered (inputs are finite).
 *   status (device int32[B], may be NULL): status[q] = 1 if query q's candidate list overflowed — only possible on
 *   degenerate data (tens of thousands of docs tied at / above the sampled threshold, e.g. duplicated embeddings);
 *   its result is then the top-k of a subset.  Re-running those queries with GDR_SIM_EXHAUSTIVE (every score kept,
 *   workspace B*N*8 bytes) is exact for any input.  The C entry point never synchronises, so the re-run is the
 *   caller's job: gdr_amd.ops.sim_topk does it by default (exact_on_overflow=True: one status read-back per call);
 *   latency-critical callers pass exact_on_overflow=False and receive the device status tensor instead.
 * d % 4 == 0, 1 <= k <= 8192, k <= N (gdr_sim_topk_bf16 likewise; gdr_sim_topk_prefilter stops at k <= 1024).  Up to k = 1024 the first
 *   wave of the select's workgroup sorts the list; from 1025 on the same radix passes pick the k keys and the whole workgroup sorts
 *   them in one LDS sort of 2048 .. 8192 keys — the same list by the same rule, one workgroup per query either way.
 *   Workspace (gdr_sim_topk_workspace_bytes): a candidate list of 8 bytes per entry and query, sample block + 4 x the expected
 *   survivors + 4096, beside 132 bytes per query.  At N = 320 000: k = 1024 -> sample stride 17, 92 288 entries, 360.6 MiB at 512 queries;
 *   k = 8192 -> sample stride 6, 253 952 entries: 77.5 MiB at 40 queries, 992 MiB at 512.  The answer is the largest list of any
 *   k' <= k (one call's list dips by 1 - 2 % where a larger k lowers the sample stride by one, and shrinks where the whole corpus
 *   becomes the sample), so it never shrinks when k grows: a buffer sized for the deepest k of a caller serves its shallower ones.
 *   gdr_sim_topk_prefilter_workspace_bytes is never below it (plus its bf16 queries and bands).
 * GDR_SIM_LIVE_MASK (gdr_sim_topk, gdr_sim_topk_bf16): the top-k over the LIVE rows of D only.  The first
 *   M = align_up(4 * ceil(N / 32), 256) bytes of `workspace` are then an INPUT the caller writes before the call: a bitmap, bit r % 32 of
 *   int32 word r / 32 set = row r of D is live; bits past N in the last word are ignored.  The library only reads that region, its own
 *   scratch starts behind it, and gdr_sim_topk_workspace_bytes(.., flags | GDR_SIM_LIVE_MASK) = the unflagged size + M (a smaller
 *   workspace is GDR_ENOSPC before any launch).  Scores, tie rule, ids (row + idx_offset) and the status contract are those of the
 *   unflagged call — the list equals the unflagged call over the matrix of the live rows, ids mapped back; with fewer than k live rows
 *   the tail of a list is -inf / -1.  A dead row's score is still computed: the mask is applied to the candidate lists between the
 *   passes (three small launches more).  When fewer than k rows of the sampled tiles are live the sample gives no threshold; the
 *   filter pass then keeps every row and the list either holds the whole corpus (exact) or overflows: status[q] = 1, and the re-run is
 *   GDR_SIM_EXHAUSTIVE | GDR_SIM_LIVE_MASK.  With the flag clear nothing changes: layout, launches and results are as before.
 *   gdr_sim_topk_prefilter takes no flags and stays UNMASKED: a masked search over such a corpus is gdr_sim_topk's (the same fp32
 *   answer by that entry point's own contract), or gdr_sim_topk_prefilter_masked's (gdr_hip_prefilter_mask.h, included below: the same
 *   answer through the bf16 pre-filter, for the live mask and for per-query bitmaps).
 * GDR_SIM_QUERY_MASK (gdr_sim_topk, gdr_sim_topk_bf16): a row filter PER QUERY.  The first B * M bytes of `workspace` (M as above) are
 *   then the caller's input: B bitmaps in GDR_SIM_LIVE_MASK's format, bitmap q at byte q * M; bit r % 32 of its int32 word r / 32 set =
 *   row r of D may be returned for query q.  Bits past N and the padding up to M are ignored, the library only reads the region, its
 *   scratch starts behind it, and gdr_sim_topk_workspace_bytes(.., flags | GDR_SIM_QUERY_MASK) = the size for `flags` + B * M (a smaller
 *   workspace is GDR_ENOSPC before any launch).  Row q of the result is the top-k over the rows bitmap q allows: scores, tie rule and
 *   ids are those of the unflagged call, the tail of a list with fewer than k allowed rows is -inf / -1, status[q] speaks for query q
 *   alone.  It is GDR_SIM_LIVE_MASK's sequence with bitmap q read for list q, and the count of allowed sample rows taken per query:
 *   a query with fewer than k of them loses its own threshold only.  Both flags in one call are GDR_EINVAL (two layouts; the size asked for the pair is 0): AND the live
 *   rows into the per-query bitmaps and pass this flag alone.  GDR_SIM_EXHAUSTIVE and GDR_SIM_NO_STREAM combine with it as with the live mask.
 *   NARROW FILTERS: a disallowed row that reaches the threshold still takes a slot of the candidate list until the second mask pass
 *   drops it, and the list holds 4 x the survivors expected of an unfiltered query.  A query whose filter keeps a small fraction of
 *   the rows therefore overflows: status[q] = 1.  Such a query is served by GDR_SIM_ROW_GATHER below, which scores its allowed rows
 *   only; the re-run with GDR_SIM_EXHAUSTIVE | GDR_SIM_QUERY_MASK stays exact for every filter and is a second pass over the corpus.
 *   Measured at N = 320 000, d = 768, k = 100 with independent random filters (tools/bench_query_mask.py,
 *   profiles/r22_query_mask_bench.jsonl): no query of 512 overflows with 50 % of the rows kept, 1 with 30 %, 33 with 25 %, 313 with
 *   20 %, 509 with 15 %, all with 10 % — overflow begins where a filter keeps less than about 30 % of the rows and is the rule below
 *   20 %.  The fraction moves with the plan (k, N): it is where k N / (f n_sample) passes the list's 4 k N / n_sample + 4096 slots.
 * GDR_SIM_ROW_GATHER (with GDR_SIM_QUERY_MASK; gdr_sim_topk, gdr_sim_topk_bf16): the mode for NARROW filters.  Input: GDR_SIM_QUERY_MASK's
 *   B bitmaps at the head of `workspace` (bitmap q at byte q * M, bits past N and the padding ignored, only read).  Bitmap q is
 *   compacted into its allowed row ids in ascending order (popcounts, a scan, ordered placement: no atomics), only those rows are
 *   read and scored (a wave per 4 rows, 16 bytes per lane, fp32 fmaf chain in ascending column order; a bf16 corpus is widened
 *   exactly), and keys (score, row) are sorted: row q of the result is the top-k over the rows bitmap q allows, higher score first in
 *   the total order of the fp32 bits, then the lower id; ids = row + idx_offset; a -inf / -1 tail where fewer than k rows are allowed,
 *   the empty bitmap included.  The score of (query, row) depends on the two vectors and d alone.
 *   Capacity: GDR_SIM_GATHER_CHUNKS(c) in bits 8..16 of flags sets cap = 4096 c rows per query, c in 1 .. 256, 0 reads as 2.  A query
 *   that allows more than cap rows gets status[q] = 1 and the top-k of its FIRST cap allowed rows in ascending row order (deterministic;
 *   the top-k of a subset, as every status 1): re-run it with a larger c or with GDR_SIM_EXHAUSTIVE | GDR_SIM_QUERY_MASK.  No other
 *   query is affected.  c <= 2: one LDS sort per query, any k <= min(N, 8192).  c > 2: chunks of 4096 list positions keep their first k
 *   and merge rounds join them (k <= 1024, as the long rerank) — the same list bit for bit.
 *   gdr_sim_topk_workspace_bytes(.., flags) = B * M + the gather layout for (B, cap, k): row ids and scores [B][cap], counts, the scan
 *   scratch and, for c > 2, two partial-list buffers; it does not depend on N or d and never shrinks when c or k grows.  A smaller
 *   workspace is GDR_ENOSPC.  GDR_EINVAL before any launch: the flag without GDR_SIM_QUERY_MASK, with GDR_SIM_LIVE_MASK or with
 *   GDR_SIM_EXHAUSTIVE, a chunk field above 256 or without the flag, k > 1024 with c > 2 (the size asked for any of them is 0).
 *   GDR_SIM_NO_STREAM is accepted and means nothing: no GEMM core runs.  Stream-ordered and capturable, no host synchronisation.
 *   Measured at N = 320 000, d = 768, k = 100 (tools/bench_query_gather.py, profiles/r23_query_gather_bench.jsonl): 512 fp32 queries that
 *   keep 3 200 rows each take 0.87 ms here against 15.4 ms for the dense masked call with its exhaustive re-run; the mode wins at 512 and
 *   32 queries, fp32 and bf16, up to 32 768 rows per query and loses at 65 536 (gdr_amd.ops.GATHER_MAX_ROWS = 32768 routes by that).
 *   With bit 16 and bits 8..16 of flags clear, every layout, launch and result is what it was.
 * ---------------------------------------------------------------------------------------------- */
#define GDR_SIM_EXHAUSTIVE 1
#define GDR_SIM_NO_STREAM 2   /* force the tiled GEMM core even at B <= 32 (A/B testing of the latency-mode kernel) */
#define GDR_SIM_LIVE_MASK 4   /* workspace starts with a live-row bitmap; rank the live rows only */
#define GDR_SIM_QUERY_MASK 8  /* workspace starts with one row bitmap per query; rank query q's allowed rows only */
#define GDR_SIM_ROW_GATHER 16                 /* with GDR_SIM_QUERY_MASK: score only the rows bitmap q allows */
#define GDR_SIM_GATHER_CHUNKS(c) ((c) << 8)   /* bits 8..16 of flags: per-query list capacity in chunks of 4096 rows, 1..256; 0 = 2 */
size_t gdr_sim_topk_workspace_bytes(int B, int64_t N, int d, int k, int flags);
int gdr_sim_topk(const float* Q, int B, const float* D, int64_t N, int d, int k, int32_t idx_offset,
                 float* out_val, int32_t* out_idx, int32_t* status, int flags, void* workspace,
                 size_t workspace_bytes, void* stream);

/* bf16 corpus / bf16 queries, fp32 accumulate on v_mfma_f32_32x32x16_bf16 (BASELINE config C5: 1M x 768 bf16).
 * Q, D are bf16 (uint16 bit patterns) [B,d] / [N,d]; d % 8 == 0 and d*2 % 128 == 0 is the fast path.  Scores and the
 * top-k semantics are those of gdr_sim_topk applied to the bf16-rounded inputs (products of bf16 values are exact in
 * fp32; only the summation order differs from a CPU fp32 matmul of the same rounded inputs). */
int gdr_sim_topk_bf16(const void* Q, int B, const void* D, int64_t N, int d, int k, int32_t idx_offset,
                      float* out_val, int32_t* out_idx, int32_t* status, int flags, void* workspace,
                      size_t workspace_bytes, void* stream);
/* The same fp32 result through a bf16 PRE-FILTER (r05; replaces the same call site, dense.py:53-54 + topk as at main_models.py:1625):
 * the corpus-wide pass runs on the bf16 MFMA path over D_bf16 (= gdr_cast_f32_bf16(D), resident beside D), and only the docs whose
 * bf16-operand score lies within 2*eps_q of the k-th largest one are scored in fp32 (from D) and ranked exactly — with
 *     eps_q = ||q|| * dnorm_max * (2^-7 + 2^-16 + d * 2^-22)   >=   |bf16-operand score - fp32 score|   for every doc,
 * that band provably contains the fp32 top-k including every doc tied at the cut (derivation: csrc/sim_topk.hip), so out_val / out_idx
 * are the top-k of the fp32 scores for every input, ties as in gdr_sim_topk (higher score, then lower id); the values are fp32 dot
 * products of the same operands in another summation order.  dnorm_max: the largest ||D[r]||_2 (sqrt of gdr_row_norm2_max's result).
 * status as in gdr_sim_topk (1 = an overflowed list: re-run that query with gdr_sim_topk).  d % 8 == 0, d <= 1024, 1 <= k <= 1024 (the
 * tail sorts 4k band keys in one workgroup's LDS and rescores them in fp32; a deeper list is gdr_sim_topk's: the same answer).
 * The workspace depends on d beyond the bf16 queries it holds: the filter pass keeps every doc above the sample threshold MINUS 2 eps_q,
 * and 2 eps_q measured in deviations of a query's scores grows like sqrt(d), so the candidate list is sized for that lowered threshold
 * (never smaller than gdr_sim_topk's list for the same B, N, k; non-decreasing in d, and in k: the answer is the largest layout of any
 * k' <= k, as gdr_sim_topk_workspace_bytes').  The sizing is an expectation for scores that are
 * roughly Gaussian and row norms within 1.25 of their rms; other corpora are served by the status contract above. */
size_t gdr_sim_topk_prefilter_workspace_bytes(int B, int64_t N, int d, int k);
int gdr_sim_topk_prefilter(const float* Q, int B, const float* D, const void* D_bf16, float dnorm_max, int64_t N, int d, int k,
                           int32_t idx_offset, float* out_val, int32_t* out_idx, int32_t* status, void* workspace,
                           size_t workspace_bytes, void* stream);
/* out_dev[0] = max over rows of ||D[r]||_2^2 (device float; the call zeroes it first).  d % 4 == 0. */
int gdr_row_norm2_max(const float* D, int64_t N, int d, float* out_dev, void* stream);
/* fp32 -> bf16, round-to-nearest-even (v_cvt_pk_bf16_f32), n % 4 == 0. */
int gdr_cast_f32_bf16(const float* in, void* out_bf16, int64_t n, void* stream);

/* Merge of per-shard top-k lists after the RCCL all-gather (no reference analogue):
 * vals/idx [G,B,k] (shard-major) -> [B,k], 1 <= k <= 8192, any G with G * k < 2^31; same tie rule (higher score in total order — +0.0 above -0.0 —, then lower id), so
 * every rank computes identical output. */
int gdr_topk_merge(const float* vals, const int32_t* idx, int G, int B, int k, float* out_val, int32_t* out_idx,
                   void* stream);
/* The wire form of a per-shard result, so that the exchange is ONE collective: per query row k+1 entries of
 * 8 bytes, entry j < k = {fp32 score, int32 id}, entry k = {0, status[q]} (status may be NULL = 0).
 * gdr_topk_pack writes pairs[B, k+1]; gdr_topk_merge_packed merges pairs[G, B, k+1] (shard-major, as an all-gather /
 * all-to-all lays them out) into out_val/out_idx [B,k] with gdr_topk_merge's tie rule and, when out_status is given,
 * out_status[q] = 1 if any shard flagged query q (its list was the top-k of a subset, see gdr_sim_topk).  1 <= k <= 8192 in both. */
int gdr_topk_pack(const float* vals, const int32_t* idx, const int32_t* status, int B, int k, void* pairs, void* stream);
int gdr_topk_merge_packed(const void* pairs, int G, int B, int k, float* out_val, int32_t* out_idx,
                          int32_t* out_status, void* stream);

/* ------------------------------------------------------------------------------------------------
 * In-cluster rerank — replaces main_models.py:1574-1637, block-diagonal only.
 *   q fp32[B,d]; D fp32[N,d]; beam_scores fp32[B,R] (length-penalised); candidate lists in one of two layouts:
 *     cand_stride == 0: cand_offsets int32[B*R+1], ONE CSR over the decoded clusters (query-major, beam order) into
 *                       cand_ids int32[...] — the reference's concatenation (main_models.py:1441-1443);
 *     cand_stride  > 0: a block per query — cand_offsets int32[B][R+1] relative to the block ([b][0] = 0), cand_ids
 *                       int32[B][cand_stride]: what gdr_cluster_candidates emits and what ranks exchange (fixed size);
 *   alphas fp32[A]; out_val fp32[B,A,k], out_idx int32[B,A,k] (doc ids; -1 / -inf padding when a
 *   query has fewer than k candidates — the reference raises there).  func: 0 tanh, 1 sigmoid.
 *   max_cand: upper bound of any query's candidate count (num beams x largest cluster; 1 <= max_cand <= 2^20) — sizes the
 *   score scratch and the sort; candidates past it are ignored.  The CSR may live on the device only
 *   (gdr_cluster_candidates below): nothing here needs its contents on the host.  Two regimes, same result bit for bit:
 *     max_cand <= 8192: ONE sort of the query's list in LDS per (alpha, query); any k.
 *     max_cand  > 8192: the list is sorted in chunks of 4096 positions, the chunks' first k are merged in rounds of up to
 *                       8192 / k lists (the order is total: the top-k of a list is the top-k of its pieces' top-k).
 *                       Needs k <= 1024; a larger k, or max_cand > 2^20, is GDR_EINVAL before anything is launched.
 *   GDR_RERANK_CHUNKED takes the second form whatever max_cand is (same k <= 1024 rule): the exact A/B switch, set by
 *   nothing in the product.
 *   Row-sharded corpus (GDR mode): D points to rows [doc_lo, doc_hi) of the corpus; candidates outside
 *   the range are skipped.  Unsharded: doc_lo = 0, doc_hi = N.  With GDR_RERANK_POSITIONS out_idx holds the candidate's
 *   POSITION in its query's list (0-based) instead of the doc id: merging the per-shard lists by "higher score, then
 *   lower position" (gdr_topk_merge_packed over B*A rows) reproduces the unsharded list bit for bit, because a
 *   candidate's score does not depend on which shard computed it.
 *   workspace: gdr_rerank_workspace_bytes(B, max_cand) — the score scratch [B][max_cand] for max_cand <= 8192; above,
 *   also the partial lists of 8 alphas at k = 1024 (more alphas run in groups of 8, one after the other on the stream),
 *   so the size serves any A and any legal k.  Non-decreasing in both arguments.  A call with GDR_RERANK_CHUNKED at
 *   max_cand <= 8192 needs the partial lists too: size it with gdr_rerank_workspace_bytes(B, max(max_cand, 8193)); a
 *   smaller workspace is GDR_ENOSPC, the message states the required size.
 * ---------------------------------------------------------------------------------------------- */
#define GDR_RERANK_POSITIONS 1
#define GDR_RERANK_CHUNKED 2
/* GDR_RERANK_ROW_QUERIES: q is fp32[B*R, d], one query vector per (query, segment): a candidate of segment j of query b is
 * scored against q[b*R + j] — the reference's doc_similarity_all[i][cluster i's columns] of the decoder-side stage-2 forms
 * (main_models.py:1588-1594), where every decoded hypothesis brings its own vector.  Only the dot pass differs (a candidate finds
 * its segment among the query's R + 1 offsets); the beam softmax, the keys, both selects, both layouts, the bf16 corpus, doc
 * ranges and the other flags are untouched, and R equal rows per query give the one-vector call's result bit for bit.  The
 * value is 8: 4 stays an unknown flag (GDR_EINVAL), as it has been refused since the flags argument exists. */
#define GDR_RERANK_ROW_QUERIES 8
size_t gdr_rerank_workspace_bytes(int B, int max_cand);
int gdr_rerank_topk(const float* q, const float* D, int d, const int32_t* cand_offsets, const int32_t* cand_ids,
                    const float* beam_scores, int B, int R, const float* alphas, int A, int k, int func,
                    float* out_val, int32_t* out_idx, int max_cand, int cand_stride, int32_t doc_lo, int32_t doc_hi,
                    int flags, void* workspace, size_t workspace_bytes, void* stream);
/* The same over a bf16 corpus (BASELINE config C5: 1M x 768 bf16): rows are gathered as bf16 and widened (exact), the dot
 * product is the same fp32 fmaf chain against the fp32 query, same keys, same order — i.e. gdr_rerank_topk applied to the
 * bf16-rounded corpus.  The corpus is never up-cast as a whole. */
int gdr_rerank_topk_bf16(const float* q, const void* D_bf16, int d, const int32_t* cand_offsets, const int32_t* cand_ids,
                         const float* beam_scores, int B, int R, const float* alphas, int A, int k, int func,
                         float* out_val, int32_t* out_idx, int max_cand, int cand_stride, int32_t doc_lo, int32_t doc_hi,
                         int flags, void* workspace, size_t workspace_bytes, void* stream);

/* Decoded docid rows -> clusters -> candidate CSR on the device — replaces `decode_token` + the `id_mapping` dict lookup +
 * the candidate concatenation of main_models.py:1398,1441-1443 (the reference walks Python strings per beam).
 * decode_token (main_models.py:322-346) drops START, cuts at the first EOS and prints token - (i*V + 2) per position; a row
 * WITHOUT EOS is printed whole, START included.  That string is a one-to-one image of the token body, so
 * `id_mapping[string]` is an exact-match lookup of the body: `keys[c]` holds cluster c's body tokens (the tokens whose
 * decode is the cluster's name), `slots` an open-addressing table (linear probing) over gdr_cluster_key_hash(body).
 * A body that matches no cluster gives an empty segment, as the reference's KeyError path does.
 *   out_ids int64[B*R, max_length] = gdr_t5_generate's out_ids (untrimmed);
 *   cluster_of int32[B*R] (out: cluster index or -1); cand_offsets int32[B][R+1] and cand_ids int32[B][cand_stride] (out):
 *   the per-query block layout of gdr_rerank_topk — members in cluster order, beams in order = the reference's
 *   concatenation order within a query; entries past cand_stride are dropped (size it num_beams * largest cluster). */
typedef struct {
  int32_t n_clusters;
  int32_t key_len;          /* ints per stored body (>= the longest body) */
  int32_t table_size;       /* power of two > n_clusters */
  const int32_t* slots;     /* device int32 [table_size]: cluster index or -1 */
  const int32_t* keys;      /* device int32 [n_clusters, key_len] */
  const int32_t* key_lens;  /* device int32 [n_clusters] */
  const int32_t* offsets;   /* device int32 [n_clusters + 1]  CSR of the member doc ids */
  const int32_t* members;   /* device int32 [N] */
} GdrClusterIndex;
uint64_t gdr_cluster_key_hash(const int32_t* tokens_host, int len);   /* host routine, the hash the device lookup uses */
int gdr_cluster_candidates(const GdrClusterIndex* ci, const int64_t* out_ids, int B, int R, int max_length,
                           int32_t* cluster_of, int32_t* cand_offsets, int32_t* cand_ids, int cand_stride, void* stream);

/* Corpus expansion — replaces tree_embedding_calculate + tree_embedding_insert (main_models.py:154-179, 268-295, called at
 * :877-889): new documents join the cluster with the nearest centroid without retraining the generative model.
 *
 * Centroids: centroids fp32[n_clusters, d], counts int32[n_clusters] from D fp32[N, d] and the member CSR
 *   (offsets int32[n_clusters+1] into members int32[n_members]).  With every cluster's members ASCENDING (the order in which
 *   the reference's TreeBuilder attaches them) the centroid is bit-identical to the reference's
 *   sum([emb[i] for i in members]) / len(members): sequential fp32 adds starting from 0, then one correctly rounded fp32
 *   division.  An empty cluster gets count 0 and a zero row.  Member ids outside [0, N) contribute nothing (validate them on
 *   the host).  d % 4 == 0, d <= 4096; D and out_centroids 16-byte aligned; N, n_members < 2^31.
 *
 * Assignment is gdr_sim_topk with k = 1 over the compacted matrix of the non-empty centroids (ties: higher score, then the
 *   lower cluster index).
 *
 * Insert: the member CSR (offsets, members: n_old ids) plus n_new documents new_ids int32[n_new] (ASCENDING) with their
 *   targets new_target int32[n_new] -> out_offsets int32[n_clusters+1], out_members int32[n_old+n_new]: every cluster keeps
 *   its members in their order, followed by the documents it received in ascending id order.  target_map int32[n_map]
 *   (may be NULL, n_map = 0) maps a target to its cluster index (the compact index of the assignment -> cluster).
 *   out_max (device int32[1]) = the largest cluster after the insertion, or -1 if a target was out of range or the old
 *   offsets were inconsistent (offsets[0] != 0, offsets[n_clusters] != n_old, a negative segment): the output is then
 *   invalid.  Deterministic (the result does not depend on atomic order); O(n_old + n_new) while no cluster receives more than
 *   4,096 documents, plus one ordered pass over the n_new inputs for each cluster that does; n_old + n_new < 2^31.
 *   workspace: gdr_cluster_insert_workspace_bytes(n_clusters) bytes.
 *
 * Remove is a mode of the same call, selected by new_target == NULL with new_ids != NULL and n_new > 0: new_ids
 *   int32[n_new] (STRICTLY ASCENDING) are the doc ids to take out of the member CSR.  target_map must be NULL and n_map 0
 *   (GDR_EINVAL otherwise).  The segments of the CSR may hold their members in any order.  Every cluster keeps its surviving
 *   members in their order; a cluster that loses all of them becomes an empty segment; an id that is a member of no cluster
 *   is ignored.  out_members still has room for n_old entries: the first out_offsets[n_clusters] are written, the rest of the
 *   buffer is left untouched, and n_old - out_offsets[n_clusters] ids were removed.  out_max = the largest cluster afterwards,
 *   or -1 under the "old offsets inconsistent" conditions above (the output is then invalid).  Integers only, no atomics: the
 *   result is a function of the inputs alone.  Same workspace; O(n_old log n_new), one wave per cluster (one huge cluster
 *   serialises on one wave, as the copy of the insert mode does); n_old < 2^31. */
int gdr_cluster_centroids(const float* D, int64_t N, int d, const int32_t* offsets, const int32_t* members, int64_t n_members,
                          int n_clusters, float* out_centroids, int32_t* out_counts, void* stream);
size_t gdr_cluster_insert_workspace_bytes(int n_clusters);
int gdr_cluster_insert(const int32_t* offsets, const int32_t* members, int n_clusters, int64_t n_old, const int32_t* new_ids,
                       const int32_t* new_target, int n_new, const int32_t* target_map, int n_map, int32_t* out_offsets,
                       int32_t* out_members, int32_t* out_max, void* workspace, size_t workspace_bytes, void* stream);

/* The exchange row of the SHARDED in-cluster rerank (gdr_amd/dist.py ShardedIndex.rerank_own; the arithmetic being sharded
 * is main_models.py:1434-1462,1574-1637, the per-GPU layout follows Data_process/NQ_dataset/bert/bert_NQ.sh:5-12): per query
 * ONE int32 row  wire[b] = { q fp32[d] | beam_scores fp32[R] | cand_offsets int32[R+1] | cand_ids int32[cand_stride] },
 * so that every rank's queries + candidate blocks travel in ONE fixed-size all-gather.  gdr_rerank_wire_pack builds
 * wire[B][d + 2R + 1 + cand_stride]; gdr_rerank_wire_unpack splits the gathered rows back into the four contiguous arrays
 * gdr_rerank_topk reads; gdr_rerank_positions_to_ids maps the merged candidate POSITIONS (GDR_RERANK_POSITIONS lists after
 * gdr_topk_merge_packed) of query b = i / per_query back to doc ids through the query's own candidate block
 * (position < 0, the "fewer than k candidates" padding, stays -1). */
int gdr_rerank_wire_pack(const float* q, const float* beam_scores, const int32_t* cand_offsets, const int32_t* cand_ids,
                         int B, int d, int R, int cand_stride, int32_t* wire, void* stream);
int gdr_rerank_wire_unpack(const int32_t* wire, int B, int d, int R, int cand_stride, float* q, float* beam_scores,
                           int32_t* cand_offsets, int32_t* cand_ids, void* stream);
int gdr_rerank_positions_to_ids(const int32_t* pos, const int32_t* cand_ids, int B, int per_query, int cand_stride,
                                int32_t* out_ids, void* stream);

/* Device-side faults that do not abort the process.  The stream-K form of the linear GEMM hands raw accumulators from one
 * workgroup to the next behind a bounded spin; if that spin ever runs out (the launch's workgroups were not co-resident)
 * the launch completes with INVALID output and raises a sticky, process-wide fault word.  While it is raised every
 * stream-K launch fails with GDR_EHIP; gdr_device_fault_pending() returns 1 (message in gdr_last_error()) so that a
 * caller can check it wherever it synchronises with the device before trusting a result; gdr_device_fault_clear()
 * acknowledges it.  Nothing clears it implicitly.  gdr_device_fault_inject_for_tests() raises it by hand (host only). */
int gdr_device_fault_pending(void);
void gdr_device_fault_clear(void);
void gdr_device_fault_inject_for_tests(void);

/* Hierarchical k-means docid construction: one Lloyd round over every open node of a tree level — the device form
 * of the reference's Data_process/NQ_dataset/kmeans/kmeans.py.  The state of a level is a CSR over nodes: rows int32[n_rows] (doc
 * ids, ASCENDING inside every node), node_offsets int32[n_nodes+1] (node_offsets[0] = 0, node_offsets[n_nodes] = n_rows), and a
 * centroid table fp32[n_nodes*k, d].  Both calls take a work list work int32[n_work, 2] = (node, first row position): every
 * tile of gdr_kmeans_assign_tile() / gdr_kmeans_partition_tile() rows of every node to process, nodes ascending and the tiles of
 * a node ascending and contiguous.  An item that names no node, or a position outside its node (for the partition: one that is
 * not a multiple of the tile past the node's start) touches nothing and sets bit 2 of out_status (device int32[1]).
 *
 * Assign: for every listed row position p: out_labels[p] = argmax_j (x . c_j - 0.5 |c_j|^2) over the k centroids of p's node,
 *   ties to the lower j, out_score[p] = that maximum (fp32; |x - c|^2 = |x|^2 - 2 score), out_changed[node] = how many labels of
 *   the node differ from prev_labels (NULL: all of them).  Exact fp32 products (v_mfma_f32_32x32x2_f32); a row's dot product is ONE
 *   fma chain in a fixed column order, so its bits do not depend on the tile, the other nodes of the call or the launch.  A row id
 *   outside [0, N) reads as a zero row.  d % 4 == 0, d <= 4096, 2 <= k <= 64, N and n_rows < 2^31; D, centroids 16-byte aligned.
 *   workspace: gdr_kmeans_assign_workspace_bytes(n_nodes, k).
 *
 * Partition: stable segmented counting sort of each listed node's rows by label -> out_rows int32[n_rows] and
 *   out_child_offsets int32[n_nodes*k+1]: child j of node s holds out_rows[out_child_offsets[s*k+j] : out_child_offsets[s*k+j+1]],
 *   ascending again (stable + ascending input) — the member order gdr_cluster_centroids wants (the update step is that call over
 *   this CSR) and the next level's state.  No ticket atomics: label counts per tile by ballot, one exclusive scan, ordered
 *   placement.  Every node must be non-empty and listed (a node that is not keeps -1 in its child offsets).  A label outside
 *   [0, k) sets bit 1 of out_status and its row is dropped.  workspace: gdr_kmeans_partition_workspace_bytes(n_work, k).
 *
 * Update: gdr_kmeans_centroids — member means over the child CSR as a FIXED-SHAPE two-stage sum: a child's members are cut into
 *   chunks of 256 counted from the child's own start, each chunk is summed member after member in fp32, the chunk sums are added
 *   in chunk order, then one correctly rounded division.  Deterministic, a function of the child's member list alone, and for a
 *   child of <= 256 members bit-identical to gdr_cluster_centroids (which stays the update of record for the expansion: one
 *   sequential chain per cluster; here a 10,000-member child would make every Lloyd round wait for that chain).  An empty child
 *   gets count 0 and a zero row.  workspace: gdr_kmeans_centroids_workspace_bytes(n_rows, d), 16-byte aligned. */
int gdr_kmeans_assign_tile(void);
int gdr_kmeans_partition_tile(void);
size_t gdr_kmeans_assign_workspace_bytes(int n_nodes, int k);
int gdr_kmeans_assign(const float* D, int64_t N, int d, const int32_t* rows, int64_t n_rows, const int32_t* node_offsets,
                      int n_nodes, const float* centroids, int k, const int32_t* work, int n_work, const int32_t* prev_labels,
                      int32_t* out_labels, float* out_score, int32_t* out_changed, int32_t* out_status, void* workspace,
                      size_t workspace_bytes, void* stream);
size_t gdr_kmeans_partition_workspace_bytes(int n_work, int k);
int gdr_kmeans_partition(const int32_t* rows, const int32_t* labels, int64_t n_rows, const int32_t* node_offsets, int n_nodes,
                         int k, const int32_t* work, int n_work, int32_t* out_rows, int32_t* out_child_offsets,
                         int32_t* out_status, void* workspace, size_t workspace_bytes, void* stream);
size_t gdr_kmeans_centroids_workspace_bytes(int64_t n_rows, int d);
int gdr_kmeans_centroids(const float* D, int64_t N, int d, const int32_t* child_offsets, const int32_t* rows, int64_t n_rows,
                         int n_children, float* out_centroids, int32_t* out_counts, void* workspace, size_t workspace_bytes,
                         void* stream);

/* T5 relative-position buckets (transformers/modeling_t5.py:242-288) for relative_position =
 * key_pos - query_pos, written to a HOST int32[qlen*klen] table; the attention kernels use the same
 * host routine, so tests pin it bit-exact against the reference. */
int gdr_t5_relative_bucket_table(int bidirectional, int num_buckets, int max_distance, int qlen, int klen,
                                 int32_t* out_host);

/* ------------------------------------------------------------------------------------------------
 * Doc tower — replaces `EncoderModel.forward(passage=...)` (main_models.py:79-89) = DPRContextEncoder
 * (transformers/modeling_dpr.py:146-191) over BertModel (transformers/modeling_bert.py); pooled = hidden[:,0].
 * Producer of the corpus matrix D (Data_process/NQ_dataset/bert/bert.py:69-71).  L <= min(512, max_pos) in all four entry points
 * (the reference's corpus embedder runs at MAX_LEN=512, bert_NQ.sh:5).  Up to 128 tokens the one-pass attention kernels serve every
 * head width; above, head width 64 takes the key-block kernels (online softmax; same results in the padded and the ragged form, bit
 * for bit) and another head width the generic kernel while K and V of one head fit in 160 KB of LDS (d_kv = 16 at L = 512 does,
 * d_kv = 128 does not: GDR_EINVAL naming d_kv and L).
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  const float *wqkv, *bqkv;      /* [3d,d],[3d]  attention.self.{query,key,value} row-concat   */
  const float *wo, *bo;          /* attention.output.dense                                       */
  const float *ln1_w, *ln1_b;    /* attention.output.LayerNorm                                   */
  const float *wi, *bi;          /* intermediate.dense (GeLU, erf form)                          */
  const float *wo2, *bo2;        /* output.dense                                                 */
  const float *ln2_w, *ln2_b;    /* output.LayerNorm                                             */
} GdrBertLayer;

typedef struct {
  int32_t vocab_size, d_model, num_heads, d_ff, num_layers, max_pos, type_vocab;
  float eps;
  const float *word_emb, *pos_emb, *type_emb, *emb_ln_w, *emb_ln_b;
  const GdrBertLayer* layers;    /* host array [num_layers] */
} GdrBertWeights;

size_t gdr_bert_encoder_workspace_bytes(const GdrBertWeights* w, int B, int L);
/* ids/mask int64[B,L], token_type_ids int64[B,L] or NULL (zeros); out_hidden fp32[B,L,d] and/or out_pooled fp32[B,d]. */
int gdr_bert_encoder_forward(const GdrBertWeights* w, const int64_t* ids, const int64_t* mask,
                             const int64_t* token_type_ids, int B, int L, float* out_hidden, float* out_pooled,
                             void* workspace, size_t workspace_bytes, void* stream);
/* The same forward over the token rows that can reach the requested outputs (r06; the T5 side's gdr_t5_encoder_forward_ragged for the
 * doc tower).  The reference pads a batch of passages to its longest member (Data_process/NQ_dataset/bert/bert.py:69-71) and computes
 * every position (modeling_bert.py:210-285); PAD keys carry weight exp(-1e9 - max) = 0 and PAD rows never reach
 * pooled = sequence_output[:, 0] (modeling_dpr.py:178-181).  Here the live rows are packed, attention runs per sequence on its own
 * length, and a pooled-only call (out_hidden == NULL) carries only the CLS rows through the last block.  Kept rows are BIT-IDENTICAL to
 * gdr_bert_encoder_forward; PAD rows of out_hidden are zero.  Masks that are not a prefix of ones keep all their positions.
 * live_rows_hint: the number of kept rows if the caller knows it (-1 otherwise) — prices the profiler's flops, never a result input.
 * Small batches / head widths other than 64 run the padded forward (same results). */
size_t gdr_bert_encoder_ragged_workspace_bytes(const GdrBertWeights* w, int B, int L);
int gdr_bert_encoder_forward_ragged(const GdrBertWeights* w, const int64_t* ids, const int64_t* mask,
                                    const int64_t* token_type_ids, int B, int L, float* out_hidden, float* out_pooled,
                                    int64_t live_rows_hint, void* workspace, size_t workspace_bytes, void* stream);
/* ... in the bf16 precision mode (BASELINE config C5 keeps its corpus in bf16; the reference itself runs precision = 32): every linear
 * weight pointer of `w` (wqkv, wo, wi, wo2) points to bf16 data (RNE of the fp32 tensor, gdr_cast_f32_bf16), biases / LayerNorm /
 * embeddings stay fp32; bf16 operands, fp32 accumulate, fp32 residual stream and norms; q, k, v are emitted as bf16 for the bf16-MFMA
 * attention.  The attention's 1/sqrt(dh) must be FOLDED INTO THE q ROWS of wqkv and bqkv by the caller (dh = 64: the factor 1/8 is a
 * power of two, the fold is exact).  Needs head width 64 and d_model, d_ff multiples of 64.  Same workspace size. */
int gdr_bert_encoder_forward_ragged_bf16(const GdrBertWeights* w, const int64_t* ids, const int64_t* mask,
                                         const int64_t* token_type_ids, int B, int L, float* out_hidden, float* out_pooled,
                                         int64_t live_rows_hint, void* workspace, size_t workspace_bytes, void* stream);
/* EXPLORATORY (r06), beside gdr_bert_encoder_forward_ragged: every linear in the fp16 x 2 split form of gdr_linear_split_bf16 (terms = 2:
 * fp32 operands carried as [fp16 hi | fp16 (x - hi) * 2^11], fp32-level error on the fp16 MFMA path); embeddings, LayerNorm, attention,
 * GeLU and the residual stream are the fp32 path's.  The linear weight pointers of `w` point to fp16 plane rows [N, 2 K]
 * (gdr_split_f32_f16x2); biases stay fp32.  Needs head width 64 and d_model, d_ff multiples of 128.  Same workspace size. */
int gdr_bert_encoder_forward_ragged_split(const GdrBertWeights* w, const int64_t* ids, const int64_t* mask,
                                          const int64_t* token_type_ids, int B, int L, float* out_hidden, float* out_pooled,
                                          int64_t live_rows_hint, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Docid beam decode — replaces `_generate_beam_search` (transformers/generation_utils.py:629-921, with
 * `BeamHypotheses` :1052-1099) driving `T5ForConditionalGeneration.forward`'s decode branch
 * (transformers/modeling_t5.py:1529-1646) as GDR calls it (main_models.py:1380-1397): greedy beams,
 * early_stopping=False, use_cache=False semantics, positional vocabulary mask.
 *
 * Device-resident: no host synchronisation between steps (the reference syncs per candidate via .item()).
 * Same arithmetic, restructured: K/V caches addressed through a beam-ancestor table instead of
 * recomputing the whole prefix every step; cross-attention K/V projected once per query instead of once per
 * beam row per step; the adaptor's single-key cross-attention folded into a per-layer constant; the
 * adaptor_linear head evaluated for the last position and its V+1 unmasked columns only.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  const float* ln_self;   /* [d]           decoder.block.i.layer.0.layer_norm.weight              */
  const float* wqkv;      /* [3*inner, d]  layer.0.SelfAttention.{q,k,v}.weight row-concat        */
  const float* wo;        /* [d, inner]    layer.0.SelfAttention.o.weight                         */
  const float* ln_cross;  /* [d]           layer.1.layer_norm.weight                              */
  const float* wq_c;      /* [inner, d]    layer.1.EncDecAttention.q.weight                       */
  const float* wkv_c;     /* [2*inner, d]  layer.1.EncDecAttention.{k,v}.weight row-concat        */
  const float* wo_c;      /* [d, inner]    layer.1.EncDecAttention.o.weight                       */
  const float* ln_ff;     /* [d]           layer.2.layer_norm.weight                              */
  const float* wi;        /* [d_ff, d]     layer.2.DenseReluDense.wi.weight                       */
  const float* wo_ff;     /* [d, d_ff]     layer.2.DenseReluDense.wo.weight                       */
} GdrT5DecLayer;

typedef struct {          /* one torch.nn.TransformerDecoderLayer (post-LN, ReLU), modeling_t5.py:1241-1244 */
  const float *in_w, *in_b;        /* self_attn.in_proj_{weight[3d,d],bias[3d]}                              */
  const float *out_w, *out_b;      /* self_attn.out_proj                                                    */
  const float *ln1_w, *ln1_b;
  const float* cross_const;        /* [d] = multihead_attn.out_proj(v_proj(adaptor_embeddings)): a single-key
                                      softmax is exactly 1, so the cross-attention output is this constant  */
  const float *ln2_w, *ln2_b;
  const float *lin1_w, *lin1_b;    /* [aff,d],[aff] */
  const float *lin2_w, *lin2_b;    /* [d,aff],[d]   */
  const float *ln3_w, *ln3_b;
} GdrAdaptorLayer;

/* Two forms of the docid head, chosen by the weights themselves:
 *   adaptor head  adaptor_layers > 0 with alayers and head_w set: the "efficient adaptor" of --adaptor_decode 1 --adaptor_efficient 1
 *                 (modeling_t5.py:1615-1639): logits = h * d^-0.5 . (adaptor_linear(adaptor(prefix)) + lm_head).
 *   plain head    adaptor_layers == 0 && alayers == NULL && head_w == NULL: the adaptor-free model of --adaptor_decode 0
 *                 --adaptor_efficient 0 (no adaptor is built, modeling_t5.py:1245-1249): logits = lm_head(h * d^-0.5) (:1640-1641).
 *                 head_e is still required; adaptor_nhead / adaptor_ff / adaptor_eps are ignored.
 * Any mixture (layers > 0 with a NULL alayers or head_w; layers == 0 with either of them set) is GDR_EINVAL naming the field. */
typedef struct {
  GdrT5Dims dims;                  /* num_layers = num_decoder_layers; vocab_size = decode_vocab_size (Vd) */
  int32_t out_vocab;               /* V  (--output_vocab_size / --kary)                                     */
  int32_t max_out_len;             /* --max_output_length; Vd = V*max_out_len + 2                           */
  int32_t adaptor_layers, adaptor_nhead, adaptor_ff;
  float adaptor_eps;
  const float* dec_embed;          /* [Vd, d]   decode_embeddings.weight (= decoder.embed_tokens = lm_head) */
  const float* self_rel_bias;      /* [buckets,H] decoder.block.0.layer.0.SelfAttention.relative_attention_bias */
  const float* cross_rel_bias;     /* [buckets,H] decoder.block.0.layer.1.EncDecAttention.relative_attention_bias */
  const float* final_ln;           /* [d]       decoder.final_layer_norm.weight                              */
  const GdrT5DecLayer* layers;     /* host array [num_layers]                                                */
  const GdrAdaptorLayer* alayers;  /* host array [adaptor_layers]; NULL for the plain head                   */
  /* head slices: position p in [0, max_out_len-1), local column c in [0, V] (c < V: token p*V+2+c; c == V: EOS=1)
   *   head_w[p][c][i][k] = adaptor_linear.weight[i*Vd + token(p,c), k]      (modeling_t5.py:1634-1636)
   *   head_e[p][c][i]    = lm_head.weight[token(p,c), i]                                                    */
  const float* head_w;             /* [(max_out_len-1), V+1, d, d]; NULL for the plain head */
  const float* head_e;             /* [(max_out_len-1), V+1, d]    */
} GdrT5DecoderWeights;

/* Optional trie constraint = the NCI semantics of the reference's earlier, un-imported generation_utils_previous.py:
 * 714-729 (`--tree 1`; the shipped generation_utils.py has the block commented out): after log_softmax,
 * -inf on every token that is not a child of the trie node reached by the beam's prefix (trie = TreeBuilder of
 * main_models.py:112-151 over the docids); a prefix that left the tree may only emit EOS.  Flattened for the device:
 * child[node*V + c] = next node (or -1) for digit c at the node's depth, eos_ok[node] = 1 if EOS is a child;
 * node 0 is the root.  Pass NULL for the shipped behaviour (positional vocabulary mask only). */
typedef struct {
  const int32_t* child;   /* device int32 [n_nodes, V] */
  const int32_t* eos_ok;  /* device int32 [n_nodes]    */
  int32_t n_nodes;
  int32_t V;              /* digits per level the table was built for; must equal the head's out_vocab (checked) */
} GdrTrie;

/* Prefix table (optional, exact): the adaptor chain and the head matrix W = adaptor_linear(adaptor(prefix))[V+1 columns] +
 * lm_head depend only on the decoded TOKEN PREFIX, never on the query (modeling_t5.py:1618-1639:
 * decode_embeddings(decoder_input_ids) -> adaptor(memory = adaptor_embeddings) -> adaptor_linear).  For every node of the
 * corpus' docid trie (nodes in BREADTH-FIRST order, root = 0; the first n_table nodes = all nodes of depth < n_levels) the
 * table holds, per adaptor layer, the in_proj output (q,k,v) of the node's position and the finished head matrix.  With
 * it, gdr_t5_generate reads W[node] for a beam row whose prefix is a table node; rows whose prefix left the trie (or is
 * deeper than the table) are compacted on the device and run the adaptor + head GEMM for themselves, attending over
 * ancestors' K/V taken from the table or computed earlier in the call.  Built once per (weights, corpus): a pure function
 * of those two, nothing query-dependent is ever stored.  Size: n_table * (adaptor_layers*3*d + (V+1)*d) floats
 * (320k-doc corpus, t5-base: 27 598 nodes, 3.6 GB). */
typedef struct {
  const int32_t* child;   /* device int32 [n_nodes, V]: the trie, as GdrTrie.child                                   */
  int32_t n_nodes, V;
  int32_t n_table;        /* nodes with entries: the first n_table nodes (breadth-first order)                       */
  const float* kv;        /* device [adaptor_layers][n_table][3*d]                                                   */
  const float* W;         /* device [n_table][V+1][d]   (adaptor_linear slice + lm_head rows of the node's position) */
  int32_t complete_levels; /* c >= 1: every one of the V^s prefixes of length s is a table node for all s < c (level 0 = the
                            * root always is).  A beam row of decode step s sits on a prefix of length s, so at steps s < c
                            * no row can miss and gdr_t5_generate does not enqueue the miss-row chain at all (1 = step 0 only;
                            * a value larger than the truth gives WRONG logits for the rows that do miss)                    */
} GdrPrefixTable;

/* Plain-head weights have no table: gdr_t5_prefix_table_workspace_bytes answers 0 and the builders GDR_EINVAL. */
size_t gdr_t5_prefix_table_workspace_bytes(const GdrT5DecoderWeights* w, int max_level_nodes);
/* level_off: HOST int32 [n_levels+1], node range of each depth (level 0 = the root alone);
 * node_tok: device int64 [n_table], the token that leads to the node (root: START = 0);
 * node_anc: device int32, level after level, for each node of depth s its s+1 ancestors root..self (node ids);
 * kv, W: the table storage (device), filled by this call.  n_levels <= max_output_length - 1. */
int gdr_t5_prefix_table_build(const GdrT5DecoderWeights* w, int n_levels, const int32_t* level_off, const int64_t* node_tok,
                              const int32_t* node_anc, float* kv, float* W, void* workspace, size_t workspace_bytes,
                              void* stream);

size_t gdr_t5_generate_workspace_bytes(const GdrT5DecoderWeights* w, int B, int L, int num_beams, int max_length);
/* enc_hidden fp32[B,L,d] (NOT beam-expanded), enc_mask int64[B,L], 1 <= L <= 512 (both modes).  Over more than 128 encoder keys the
 * cross-attention of d_kv = 64 is the key-block kernel of csrc/attention_long.hip (beam rows as 16-row MFMA tiles, 64-key blocks,
 * online softmax; also step 0's single row per query); another head width takes the generic kernel while K / V fit in LDS, else
 * GDR_EINVAL naming d_kv and L.
 * out_ids int64[B*nret, max_length] (hypothesis tokens incl. START, then EOS if it fits, then PAD),
 * out_len int32[B*nret] (= len(hyp), EOS excluded), out_scores fp64[B*nret] (sum_logprobs / len^length_penalty,
 * computed in double like the reference's Python floats).  Optional trace (NULL to skip):
 * step_scores fp32[max_length-1, B, 2R], step_tokens int32[...] = the per-step topk(2R) (generation_utils.py:775).
 * 2 <= num_beams <= 1024 (what the stage behind it takes: gdr_rerank_topk / gdr_cluster_candidates), num_beams * (V+1) <= 131072
 * candidates per query and step, num_return_sequences <= num_beams, max_length <= max_out_len (<= 32).
 *   The top-2*num_beams of a step: ONE sort of the query's candidates in LDS while num_beams * (V+1) <= 8192; above, chunks of
 *   4096 candidate positions are sorted on their own and their first 2*num_beams merged in rounds of up to 8192 / (2*num_beams)
 *   lists — the same list bit for bit (distinct keys: the top of a list is the top of its pieces' tops).  The environment switch
 *   GDR_DECODE_BEAM_CHUNKED=1 (read once per process; an exact A/B knob, nothing in the product sets it) takes the chunked form
 *   at every size; gdr_t5_generate_workspace_bytes / gdr_beam_search_table_workspace_bytes account for it (the chunked form adds
 *   its partial lists; a call that stays in the one-sort form needs what it always needed).
 *   A query's hypothesis heap (num_beams + 1 entries of max_length tokens) and, at the end, its open beam rows live in one
 *   workgroup's LDS (160 KiB): roughly num_beams * (8 * max_length + 32) bytes.  1024 beams fit up to max_length = 13, 512 beams
 *   up to 32; a combination that does not fit is refused with GDR_EINVAL naming num_beams and max_length before any launch.
 * num_beams == 1 selects the reference's non-beam branch instead (_generate_no_beam_search, generation_utils.py:553-627), the call
 * its generate() makes by default: one row per query, next token = argmax of the step's logits over the whole decode vocabulary
 * (of the logits, not a log-softmax; equal maxima: the lowest token id as torch.argmax on the CPU gives, so EOS = 1 wins a tie
 * against any digit token; masked columns are exactly -1e9 and never win), PAD after a row's EOS, the loop ends when every row has
 * emitted EOS (the same early exit as below; the step reported is width - 1) or at max_length.  The decoder chain, adaptor chain,
 * head, prefix table and both cross-attention forms are the beam path's launches over B rows; the select and bookkeeping are one
 * launch per step.  Contract:
 *   num_return_sequences must be 1 (the reference asserts it, :341-346); trie, step_scores and step_tokens must be NULL (the
 *   constraint and the top-2R trace exist for the beam search only) — any violation is GDR_EINVAL naming the argument, before any
 *   launch; length_penalty is accepted and unused; prefix_table is allowed;
 *   out_ids int64[B, max_length] = START, the tokens, then PAD after EOS; out_len int32[B] = the reference's sent_lengths: START
 *   and EOS both count, max_length for a row that never emitted EOS (so generate()'s result is out_ids[:, :max(out_len)]);
 *   out_scores[b] = 0.0 (the reference keeps none);
 *   gdr_t5_generate_workspace_bytes(w, B, L, 1, max_length) is what this form needs: the beam form's layout at one row per query,
 *   non-zero and never more than the answer for num_beams = 2.
 * gdr_beam_search_table has no such form: it keeps refusing num_beams = 1.
 * Plain-head weights (see GdrT5DecoderWeights): the decoder chain is the one above; no adaptor chain is enqueued and nothing is forked
 * to or joined from the side stream per step (the side stream still projects the cross-attention K/V at step 0); the head of a step
 * is ONE launch, head_plain_kernel — logits[r][c] = sum_i (h[r][i] * d^-0.5) * head_e[s][c][i] over the V+1 live columns, per (row,
 * column) in the adaptor head's order with a zero head matrix, so an adaptor model whose adaptor_linear is zero gives the same bits;
 * fp32 in both precision modes — followed by the unchanged beam / greedy step.  Beams 2 .. 1024 (chunked select), num_beams == 1,
 * the trie constraint, the trace, the early exit and its counters, L up to 512 and stream capture all apply.  prefix_table must be
 * NULL (GDR_EINVAL naming it: the table stores adaptor results, and lm_head alone has nothing query-independent to store).
 * gdr_t5_generate_workspace_bytes leaves out the adaptor K/V cache, the adaptor activations and the rows x (V+1) x d head-matrix
 * buffer for such weights.
 *
 * Score mode — out_len == NULL: the decoder runs over GIVEN docid rows instead of searching for them (teacher forcing; the forward
 * the reference's validation step makes with decoder_input_ids = outs, main_models.py:1467-1571).  Contract:
 *   rows = B * num_beams with 1 <= num_beams <= 1024 rows per query (row b*num_beams + r belongs to query b); neither the
 *   hypothesis-heap LDS limit nor the num_beams * (V+1) candidate limit applies (no heap, no select);
 *   num_return_sequences must equal num_beams; trie, prefix_table and step_tokens must be NULL; length_penalty > 0; max_length in
 *   [2, max_out_len] — any violation is GDR_EINVAL naming the argument, before any launch;
 *   out_ids int64[rows, max_length] is an INPUT that is only read: rows as a search with nret == num_beams writes them (START,
 *   tokens, EOS, then PAD);
 *   out_scores fp64[rows] = what the search reports for that hypothesis: sum_t log_softmax(logits_t)[ids[t+1]] / len^length_penalty
 *   over the positions before the row's first EOS (the EOS' own log-probability included), len = the EOS position, max_length
 *   for a row without EOS; logits_t are the V+1 live columns of position t, and a token that is no live column of its position
 *   counts as the masked logit, exactly -1e9; the sum is accumulated in fp32 in position order, as the search accumulates it;
 *   step_scores (optional) fp32[max_length + 2][rows][d_model], an output: planes 0 .. max_length-1 the decoder's last hidden state
 *   of each position (after final_layer_norm; zero behind a row's first EOS), plane max_length the hidden state AT the first EOS
 *   (a zero row without one), plane max_length + 1 the mean over t = 0 and every t >= 1 with ids[t] != PAD (summed ascending in
 *   fp32, one division by the count);
 *   workspace: gdr_t5_generate_workspace_bytes(w, B, L, num_beams, max_length) serves the mode.
 * All max_length positions run (one more than a search; the head is not run behind the last), every row keeps cache slots of its
 * own, there is no early exit and no host synchronisation; stream capture, both precision modes and both head forms apply. */
int gdr_t5_generate(const GdrT5DecoderWeights* w, const float* enc_hidden, const int64_t* enc_mask, int B, int L,
                    int num_beams, int max_length, double length_penalty, int num_return_sequences,
                    const GdrTrie* trie, const GdrPrefixTable* prefix_table /* NULL: compute every row */, int64_t* out_ids,
                    int32_t* out_len, double* out_scores, float* step_scores, int32_t* step_tokens, void* workspace,
                    size_t workspace_bytes, void* stream);

/* bf16 precision mode of the decode path (BASELINE config C5; the reference itself runs precision=32, main.py:61,91): the
 * SAME structs, but every linear weight — GdrT5DecLayer.{wqkv, wo, wq_c, wkv_c, wo_c, wi, wo_ff},
 * GdrAdaptorLayer.{in_w, out_w, lin1_w, lin2_w} and head_w — points to bf16 data (round-to-nearest-even of the fp32
 * checkpoint); the `const float*` field type is nominal for them.  Each linear rounds its activation operand to bf16 and
 * accumulates in fp32; embeddings, norms, attention, biases, the residual stream, the head dot product (h · W), log-softmax
 * and all beam arithmetic stay fp32, hypothesis scores fp64.  A prefix table for this mode is built by the _bf16 builder
 * (same rounding points as the in-call computation); its storage stays fp32.  Parity: against the oracle's emulation of
 * exactly these rounding points (oracle/t5_ref.py bf16_linears) and within bf16 tolerance of the fp32 path.
 * Workspace: gdr_t5_generate_workspace_bytes / gdr_t5_prefix_table_workspace_bytes serve both modes. */
int gdr_t5_generate_bf16(const GdrT5DecoderWeights* w, const float* enc_hidden, const int64_t* enc_mask, int B, int L,
                         int num_beams, int max_length, double length_penalty, int num_return_sequences,
                         const GdrTrie* trie, const GdrPrefixTable* prefix_table, int64_t* out_ids, int32_t* out_len,
                         double* out_scores, float* step_scores, int32_t* step_tokens, void* workspace,
                         size_t workspace_bytes, void* stream);
/* Early exit of the step loop — `if all(done): break`, generation_utils.py:836-838, without a host synchronisation.  When the
 * last query of a call becomes done (BeamHypotheses.is_done, :827-829) the beam bookkeeping kernel (a) clears a device word
 * that the 64x64-tile linears and the miss-row chain of every step already enqueued look at — they exit at once — and
 * (b) stores the call's epoch in host-mapped memory, which the host reads before it enqueues the next step and then stops.
 * The steps that still run change nothing (done queries only pad, :786-794): outputs are bit-identical to running all
 * max_length - 1 steps.  Not taken while the per-step trace is requested; under graph capture only (a) applies.  Random
 * weights never finish early; a trained model does after the docid's length + 1 steps, a trie-constrained call always does.
 * Returns how many generate calls of this process left their loop on the host side (monitoring / tests). */
int64_t gdr_t5_generate_early_exits(void);
/* The device half of the same exit, observable: the decode step (cur_len, 1-based) at which the LAST query of the most recent
 * gdr_t5_generate call of this process became done, written by the beam bookkeeping kernel into host-mapped memory; 0 when
 * that call ran to max_length without every query finishing (or ran with the per-step trace).  Read it after the call's
 * stream has been synchronised.  Deterministic (unlike the host-side counter above, which races with the GPU by design) —
 * for STRICTLY SERIAL calls only: "the most recent call" is the most recently STARTED one of the process, so with several calls
 * in flight (GDRRetriever.validation_steps at depth >= 2, several host threads) or after a call that took no epoch (per-step trace
 * requested) it reports another call's step, or 0.  A monitoring / test hook, not part of the result. */
int gdr_t5_generate_last_done_step(void);
int gdr_t5_prefix_table_build_bf16(const GdrT5DecoderWeights* w, int n_levels, const int32_t* level_off,
                                   const int64_t* node_tok, const int32_t* node_anc, float* kv, float* W, void* workspace,
                                   size_t workspace_bytes, void* stream);

/* The same device beam search driven by a logit table instead of the model (teacher forcing):
 * logits(prefix) = table[b, pos, last_token, :] (fp32 [B, max_length, Vd, Vd]) with the positional mask.
 * Exercises EOS / early-done / eviction paths that random weights never reach.  num_beams, num_beams * (out_vocab+1) and
 * max_length obey gdr_t5_generate's rules (the chunked select and GDR_DECODE_BEAM_CHUNKED included). */
size_t gdr_beam_search_table_workspace_bytes(int B, int num_beams, int max_length, int out_vocab);
int gdr_beam_search_table(const float* table, int B, int out_vocab, int num_beams, int max_length,
                          double length_penalty, int num_return_sequences, const GdrTrie* trie, int64_t* out_ids,
                          int32_t* out_len, double* out_scores, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

/* The pre-filtered search over live rows / per-query filters and the row-wise upkeep of the bf16 image: declared in a header of their own. */
#include "gdr_hip_prefilter_mask.h"
/* Compacting a live corpus (the plan, the row mover, the id and row-bitmap remaps): declared in a header of their own. */
#include "gdr_hip_compact.h"
/* k-means++ seeding of the hierarchical docid build (one greedy step over every node of a level): declared in a header of its own. */
#include "gdr_hip_kmeans_seed.h"

#endif /* GDR_HIP_H */
