// Docid decode on gfx950, the model step — device-resident replacement of the forward that the reference's generate() hot loop drives
// (T5ForConditionalGeneration.forward's decode branch, transformers/modeling_t5.py:1529-1646).  The loop's own bookkeeping — the
// beam search and the greedy decode of generation_utils.py — is beam.hip: a step here ends with the logits in BeamBufs::logits and
// starts from the tokens (cur_tok) and ancestor rows (kv_rows) that beam.hip left.
//
// What changes relative to the reference (arithmetic per produced number is the same):
//   * use_cache=False recomputes the whole prefix every step; here every layer's K/V rows are written once per
//     position into a [Tmax][rows][3*width] cache and beams reach their ancestors' rows through an int32 table
//     (`kv_rows`) that the beam-update kernel rewrites each step — no cache reordering copies, no recompute.
//   * cross-attention K/V are projected once per QUERY (beams share them: kv_group = num_beams) instead of once
//     per beam row per step (generation_utils.py:459-461 expands the encoder states to B*beams rows).
//   * the adaptor's cross-attention over a single learned key (modeling_t5.py:1628-1631) is the constant
//     out_proj(v_proj(adaptor_embeddings)) — softmax over one key is exactly 1 — precomputed at load time.
//   * the adaptor_linear head (modeling_t5.py:1634-1639: [R*t,768]x[768,768*302] + a [R,t,768,302] broadcast add)
//     is evaluated for the last position and its V+1 unmasked columns only: one GEMM against a re-laid weight
//     slice [V+1][d][d] and a fused dot kernel; masked columns are exactly -1e9 either way.
//   * the adaptor chain and the head matrix W = adaptor_linear(adaptor(prefix)) + lm_head depend on the TOKEN PREFIX
//     only, never on the query (modeling_t5.py:1618-1639): with a GdrPrefixTable — built once from the weights and the
//     corpus' docid trie (gdr_t5_prefix_table_build) — a row whose prefix is a trie node reads its head matrix (and,
//     for its descendants, its adaptor K/V) from the table; only rows whose prefix left the trie are compacted and run
//     through the adaptor + head GEMM (device-side row count, no host round trip).
#include <math.h>

#include <atomic>
#include <mutex>
#include <vector>

#include "attention.h"
#include "beam.h"
#include "layers.h"
#include "scan.h"

namespace gdr {

constexpr size_t SPLITK_WS_BYTES = (size_t)48 << 20;  // <= 640 partial 128x128 tiles + slack
static_assert(STREAMK_BYTES <= SPLITK_WS_BYTES, "stream-K scratch must fit the split-K region");

// logits[r][c] = sum_i (h[r][i] * d^-0.5) * (A[r][c*d + i] + E[c][i])      (modeling_t5.py:1575-1576,1637-1639)
__global__ __launch_bounds__(256) void head_logits_kernel(const float* __restrict__ h, const float* __restrict__ A,
                                                          const float* __restrict__ E, int rows, int V1, int d,
                                                          float scale, float* __restrict__ logits,
                                                          const int32_t* __restrict__ live) {
  const int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (item >= (int64_t)rows * V1) return;
  if (live && *live == 0) return;  // every query is done: these logits are never ranked
  const int r = (int)(item / V1), c = (int)(item % V1), lane = threadIdx.x & 63;
  const float4* h4 = reinterpret_cast<const float4*>(h + (size_t)r * d);
  const float4* a4 = reinterpret_cast<const float4*>(A + ((size_t)r * V1 + c) * d);
  const float4* e4 = reinterpret_cast<const float4*>(E + (size_t)c * d);
  float acc = 0.f;
  for (int i = lane; i < d / 4; i += 64) {
    const float4 hv = h4[i], av = a4[i], ev = e4[i];
    acc = fmaf(hv.x * scale, av.x + ev.x, acc);
    acc = fmaf(hv.y * scale, av.y + ev.y, acc);
    acc = fmaf(hv.z * scale, av.z + ev.z, acc);
    acc = fmaf(hv.w * scale, av.w + ev.w, acc);
  }
  acc = wave_sum(acc);
  if (lane == 0) logits[item] = acc;
}

// The head of a model WITHOUT the adaptor (GdrT5DecoderWeights' plain form; modeling_t5.py:1640-1641 lm_head(sequence_output)):
//   logits[r][c] = sum_i (h[r][i] * d^-0.5) * E[c][i]
// Per (row, column) this is head_logits_kernel's arithmetic with A == 0 — lane l walks the float4 pieces l, l + 64, ... in .x .y .z .w
// order, then wave_sum; 0 + e == e exactly — so an adaptor model whose adaptor_linear is zero gives the same bits.  A wave serves one
// row: it reads (and scales) the row once, NP pieces per lane in registers (d / 4 <= 64 * NP; NP = 0: any width, the row is read again
// for every column), and loops over the V + 1 columns; lane c % 64 keeps column c's sum and every 64 columns are stored in one go.
template <int NP>
__global__ __launch_bounds__(256) void head_plain_kernel(const float* __restrict__ h, const float* __restrict__ E, int rows, int V1,
                                                         int d, float scale, float* __restrict__ logits,
                                                         const int32_t* __restrict__ live) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  if (live && *live == 0) return;  // every query is done: these logits are never ranked
  const int lane = threadIdx.x & 63, n4 = d >> 2;
  const float4* h4 = reinterpret_cast<const float4*>(h + (size_t)r * d);
  float4 hs[NP > 0 ? NP : 1];
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    const int i = lane + 64 * k;
    const float4 hv = i < n4 ? h4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    hs[k] = make_float4(hv.x * scale, hv.y * scale, hv.z * scale, hv.w * scale);
  }
  float* out = logits + (size_t)r * V1;
  float mine = 0.f;
  for (int c = 0; c < V1; ++c) {
    const float4* e4 = reinterpret_cast<const float4*>(E + (size_t)c * d);
    float acc = 0.f;
    if (NP > 0) {
#pragma unroll
      for (int k = 0; k < NP; ++k) {
        const int i = lane + 64 * k;
        if (i < n4) {
          const float4 ev = e4[i];
          acc = fmaf(hs[k].x, ev.x, acc);
          acc = fmaf(hs[k].y, ev.y, acc);
          acc = fmaf(hs[k].z, ev.z, acc);
          acc = fmaf(hs[k].w, ev.w, acc);
        }
      }
    } else {
      for (int i = lane; i < n4; i += 64) {
        const float4 hv = h4[i], ev = e4[i];
        acc = fmaf(hv.x * scale, ev.x, acc);
        acc = fmaf(hv.y * scale, ev.y, acc);
        acc = fmaf(hv.z * scale, ev.z, acc);
        acc = fmaf(hv.w * scale, ev.w, acc);
      }
    }
    acc = wave_sum(acc);
    if ((c & 63) == lane) mine = acc;
    if ((c & 63) == 63 || c + 1 == V1) {
      const int c0 = c & ~63;
      if (c0 + lane <= c) out[c0 + lane] = mine;
    }
  }
}

static int launch_head_plain(const float* h, const float* E, int rows, int V1, int d, float* logits, const int32_t* live,
                             hipStream_t stream) {
  const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
  const float scale = 1.0f / sqrtf((float)d);
  const int n4 = d / 4;
#define GDR_HEAD_PLAIN(NP) hipLaunchKernelGGL(head_plain_kernel<NP>, grid, block, 0, stream, h, E, rows, V1, d, scale, logits, live)
  if (n4 <= 64) GDR_HEAD_PLAIN(1);
  else if (n4 <= 128) GDR_HEAD_PLAIN(2);
  else if (n4 <= 192) GDR_HEAD_PLAIN(3);
  else if (n4 <= 256) GDR_HEAD_PLAIN(4);
  else GDR_HEAD_PLAIN(0);
#undef GDR_HEAD_PLAIN
  GDR_CHECK_LAUNCH("head_plain_kernel");
  return GDR_OK;
}

// Prefix-table form of the same dot: a row whose prefix is a table node reads its finished head matrix
// W[node][c][i] = A + E (built at load); any other row reads the A computed this step for its compacted slot.
__global__ __launch_bounds__(256) void head_logits_table_kernel(const float* __restrict__ h, const float* __restrict__ A_c,
                                                                const float* __restrict__ E, const float* __restrict__ tabW,
                                                                const int32_t* __restrict__ node,
                                                                const int32_t* __restrict__ miss_index, int n_table,
                                                                int rows, int V1, int d, float scale,
                                                                float* __restrict__ logits, const int32_t* __restrict__ live,
                                                                const float* __restrict__ partial = nullptr) {
  const int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (item >= (int64_t)rows * V1) return;
  if (live && *live == 0) return;  // every query is done: these logits are never ranked
  const int r = (int)(item / V1), c = (int)(item % V1), lane = threadIdx.x & 63;
  const float4* h4 = reinterpret_cast<const float4*>(h + (size_t)r * d);
  const int mi = miss_index[r];
  float acc = 0.f;
  if (mi < 0) {
    const float4* w4 = reinterpret_cast<const float4*>(tabW + ((size_t)node[r] * V1 + c) * d);
    for (int i = lane; i < d / 4; i += 64) {
      const float4 hv = h4[i], wv = w4[i];
      acc = fmaf(hv.x * scale, wv.x, acc);
      acc = fmaf(hv.y * scale, wv.y, acc);
      acc = fmaf(hv.z * scale, wv.z, acc);
      acc = fmaf(hv.w * scale, wv.w, acc);
    }
  } else if (partial) {
    // the head GEMM's epilogue already took the dot (launch_linear_bf16_headdot): d / 64 partial sums per (row, c), added in a fixed tree
    const int slots = d >> 6;
    if (lane < slots) acc = partial[((size_t)mi * V1 + c) * slots + lane];
  } else {
    const float4* a4 = reinterpret_cast<const float4*>(A_c + ((size_t)mi * V1 + c) * d);
    const float4* e4 = reinterpret_cast<const float4*>(E + (size_t)c * d);
    for (int i = lane; i < d / 4; i += 64) {
      const float4 hv = h4[i], av = a4[i], ev = e4[i];
      acc = fmaf(hv.x * scale, av.x + ev.x, acc);
      acc = fmaf(hv.y * scale, av.y + ev.y, acc);
      acc = fmaf(hv.z * scale, av.z + ev.z, acc);
      acc = fmaf(hv.w * scale, av.w + ev.w, acc);
    }
  }
  acc = wave_sum(acc);
  if (lane == 0) logits[item] = acc;
  (void)n_table;
}

// Prefix-table mode, once per step (one workgroup): which rows have a table entry for their prefix?  The others are
// compacted in ascending row order (deterministic) together with their ancestor rows; *n_miss is what every kernel of
// the adaptor chain reads as its row count.
__global__ __launch_bounds__(1024) void prefix_plan_kernel(BeamBufs bb, int rows, int stride, int cur, int n_table) {
  // A thread owns ceil(rows / 1024) CONSECUTIVE rows: it counts its misses, one scan over the 1024 counts gives every thread the
  // number of misses before its first row, and it numbers its own misses from there — ascending row order, one pass.  (Through
  // round 3 the workgroup walked the rows 1 024 at a time with three barriers per chunk: 470 us at 20 480 rows, at the head of
  // the adaptor chain of every step.)
  __shared__ int wsum[16];
  const int tid = threadIdx.x;
  const int per = (rows + 1023) >> 10;
  const int r0 = tid * per, r1 = min(rows, r0 + per);
  int cnt = 0;
  for (int r = r0; r < r1; ++r) {
    const int nd = bb.node[cur][r];
    cnt += (nd >= 0 && nd < n_table) ? 0 : 1;
  }
  int total;
  int pos = block_scan_once<1024>(cnt, wsum, &total);
  for (int r = r0; r < r1; ++r) {
    const int nd = bb.node[cur][r];
    const bool miss = !(nd >= 0 && nd < n_table);
    bb.miss_index[r] = miss ? pos : -1;
    if (miss) bb.miss_rows[pos++] = r;
  }
  // every query done (beam_update_kernel): the miss rows' adaptor chain and head GEMM of this step run on zero rows; the
  // index arrays stay as computed, so whoever still reads them (the head lookup of a step nobody consumes) stays in bounds
  if (tid == 0) *bb.n_miss = *bb.live ? total : 0;
  (void)stride;
}

// kv_rows_c[i][p] = kv_rows[miss_rows[i]][p]; hit rows: the table's (q,k,v) of the node -> this step's slot of every
// adaptor layer's cache, so that a descendant that later leaves the trie finds its ancestors' K/V where it looks.
__global__ __launch_bounds__(256) void prefix_fill_kernel(BeamBufs bb, int rows, int stride, int cur,
                                                          const float* __restrict__ tab_kv, int64_t tab_layer_stride,
                                                          float* __restrict__ acache_slot, int64_t cache_layer_stride,
                                                          int n_layers, int d3) {
  const int r = blockIdx.x;
  if (bb.live_gate && *bb.live_gate == 0) return;  // every query is done: nobody will look for ancestors in this step's slots
  const int mi = bb.miss_index[r];
  if (mi >= 0) {
    for (int p = threadIdx.x; p < stride; p += 256) bb.kv_rows_c[(size_t)mi * stride + p] = bb.kv_rows[(size_t)r * stride + p];
    return;
  }
  const int nd = bb.node[cur][r];
  const int n4 = d3 >> 2;
  for (int l = 0; l < n_layers; ++l) {
    const float4* src = reinterpret_cast<const float4*>(tab_kv + l * tab_layer_stride + (size_t)nd * d3);
    float4* dst = reinterpret_cast<float4*>(acache_slot + l * cache_layer_stride + (size_t)r * d3);
    for (int c = threadIdx.x; c < n4; c += 256) dst[c] = src[c];
  }
}

// xd[r] = table[tok[r]] and nx[r] = T5LayerNorm(xd[r]; w) in one launch: the embedding of a decode step and the first norm
// of the decoder stack (modeling_t5.py:725, :164-171), arithmetic of rmsnorm_kernel (layers.hip).  One wave per row.
__global__ __launch_bounds__(256) void embed_rmsnorm_kernel(const float* __restrict__ table, const int64_t* __restrict__ tok,
                                                            int rows, int d4, int vocab, const float* __restrict__ w, float eps,
                                                            float* __restrict__ xd, float* __restrict__ nx,
                                                            const int32_t* __restrict__ live) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  if (live && *live == 0) return;  // every query is done (beam_update_kernel): this step's rows are never read
  const int lane = threadIdx.x & 63;
  int64_t id = tok[row];
  id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
  const float4* src = reinterpret_cast<const float4*>(table) + id * d4;
  float4* xr = reinterpret_cast<float4*>(xd) + (int64_t)row * d4;
  float ss = 0.f;
  for (int c = lane; c < d4; c += 64) {
    const float4 v = src[c];
    xr[c] = v;
    ss += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
  }
  ss = wave_sum(ss);
  const RowDivisor over(sqrtf(ss / (float)(d4 * 4) + eps));  // x / denom, bit for bit (common.h)
  float4* yr = reinterpret_cast<float4*>(nx) + (int64_t)row * d4;
  const float4* wr = reinterpret_cast<const float4*>(w);
  for (int c = lane; c < d4; c += 64) {
    const float4 v = src[c], g = wr[c];
    yr[c] = make_float4(g.x * over(v.x), g.y * over(v.y), g.z * over(v.z), g.w * over(v.w));
  }
}

// out[i] = table[tok[rows_map[i]]] for i < *n_dev
__global__ __launch_bounds__(256) void embed_rows_kernel(const float* __restrict__ table, const int64_t* __restrict__ tok,
                                                         const int32_t* __restrict__ rows_map,
                                                         const int64_t* __restrict__ n_dev, int d4, int vocab,
                                                         float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= *n_dev) return;
  int64_t id = tok[rows_map[i]];
  id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
  const float4* src = reinterpret_cast<const float4*>(table) + id * d4;
  float4* dst = reinterpret_cast<float4*>(out) + i * d4;
  for (int c = threadIdx.x & 63; c < d4; c += 64) dst[c] = src[c];
}

// slot[rows_map[i]][c0 ..] = src[i][c0 ..] (rows of n4 float4, columns from c0 on), i < *n_dev: the compacted (k, v) of this
// step into the cache slot — the q third of a row stays in the compacted buffer, where this step's attention reads it; nobody
// reads q from the cache in the prefix-table mode (descendants need their ancestors' K / V only)
__global__ __launch_bounds__(256) void scatter_slot_kernel(const float* __restrict__ src, const int32_t* __restrict__ rows_map,
                                                           const int64_t* __restrict__ n_dev, int n4, int c0,
                                                           float* __restrict__ slot) {
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= *n_dev) return;
  const float4* s4 = reinterpret_cast<const float4*>(src) + i * n4;
  float4* d4 = reinterpret_cast<float4*>(slot) + (int64_t)rows_map[i] * n4;
  for (int c = c0 + (threadIdx.x & 63); c < n4; c += 64) d4[c] = s4[c];
}

// The adaptor chain (decode_embeddings -> 4 post-LN layers) and the T5 decoder stack of one step are independent until
// the head consumes both, and each of their kernels fills only part of the chip at decode batch sizes: they run
// concurrently, the adaptor on a side stream forked / joined with events (graph-capturable pattern).  Side streams are
// leased per CALL from a per-device pool (created on first use on the device that is current in the calling thread), so
// concurrent gdr_t5_generate calls from several host threads or on several devices never share one.
// `if all(done): break` (generation_utils.py:836-838) without a host sync: beam_update_kernel stores the call's epoch into a
// host-mapped word when the last query becomes done, and the host looks at that word before it enqueues the next step.  The
// host runs ahead of the GPU by less than a step's worth of launches at decode batch sizes, so a call whose beams all finish
// at step s enqueues at most a step or two more (which change nothing: done queries only pad, :786-794) instead of all
// max_length - 1.  Random weights (bench.py) never finish early; a trained model does after the docid's length + 1 steps, and so
// does every trie-constrained call.  64 words used round-robin by epoch: a stale store from the call 64 epochs ago cannot match.
static int32_t* done_words() {
  static int32_t* words = [] {
    int32_t* h = nullptr;
    // words 0..63: the epoch words; words 64..127: the decode step (cur_len) at which word i's call saw its last query finish
    if (hipHostMalloc(reinterpret_cast<void**>(&h), 128 * sizeof(int32_t), hipHostMallocPortable | hipHostMallocMapped | hipHostMallocCoherent) !=
        hipSuccess) {
      (void)hipGetLastError();
      return static_cast<int32_t*>(nullptr);
    }
    for (int i = 0; i < 128; ++i) h[i] = 0;
    return h;
  }();
  return words;
}
static std::atomic<int32_t> g_done_epoch{0};
static std::atomic<int64_t> g_early_exits{0};
constexpr int SIDE_MAX_LAYERS = 48;
struct SideStream {
  hipStream_t s = nullptr;
  hipEvent_t fork = nullptr, join = nullptr;
  hipEvent_t ckv[SIDE_MAX_LAYERS] = {};  // "cross-attention K/V of layer l are projected" (gdr_t5_generate, before step 0)
  int dev = -1;
};
static std::mutex g_side_mu;
static std::vector<SideStream*> g_side_free;

static SideStream* side_stream_acquire() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  {
    std::lock_guard<std::mutex> lock(g_side_mu);
    for (size_t i = 0; i < g_side_free.size(); ++i)
      if (g_side_free[i]->dev == dev) {
        SideStream* x = g_side_free[i];
        g_side_free.erase(g_side_free.begin() + i);
        return x;
      }
  }
  SideStream* x = new SideStream();
  x->dev = dev;
  if (hipStreamCreateWithFlags(&x->s, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&x->fork, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&x->join, hipEventDisableTiming) != hipSuccess) {
    delete x;  // the caller falls back to running the adaptor chain on the main stream
    return nullptr;
  }
  for (int l = 0; l < SIDE_MAX_LAYERS; ++l)
    if (hipEventCreateWithFlags(&x->ckv[l], hipEventDisableTiming) != hipSuccess) {
      delete x;
      return nullptr;
    }
  return x;
}
// A lease ends when the call has finished ENQUEUEING: the stream is in-order, so the next lessee's work simply queues
// behind what is still in flight, and a wait already enqueued on `join` keeps the event state it captured.
struct SideLease {
  SideStream* ss = nullptr;
  void acquire() { ss = side_stream_acquire(); }
  ~SideLease() {
    if (!ss) return;
    std::lock_guard<std::mutex> lock(g_side_mu);
    g_side_free.push_back(ss);
  }
};
// `waiter` goes on only after what `producer` holds now: the fork / join of the two streams
static int stream_after(hipStream_t waiter, hipEvent_t event, hipStream_t producer, const char* what) {
  if (hipEventRecord(event, producer) != hipSuccess || hipStreamWaitEvent(waiter, event, 0) != hipSuccess) {
    set_error("%s", what);
    return GDR_EHIP;
  }
  return GDR_OK;
}
// A/B knob of the fused consumers (0 = every linear writes its output and its consumer runs as a launch of its own): the fp32 norm
// behind a split-K linear (dec_linear_norm) and the bf16 head GEMM's dot epilogue (GenCall::head)
static bool fuse_norm_on() {
  static const bool on = env_flag("GDR_DECODE_FUSE_NORM", true);
  return on;
}

// One linear of the decode path.  fp32: the split-K / small-tile launcher (device-side row count when m_dev is given).
// bf16 precision mode (BASELINE config C5): W points to bf16 data, the activation operand is rounded to bf16 into `abf`
// (RNE) and the GEMM accumulates in fp32; bias / residual / output stay fp32.
// bf16 mode: the norm that produced a linear's fp32 operand also left it rounded to bf16 (`buf`), so the linear needs no cast
// launch of its own — `src` says which fp32 buffer the image belongs to; anything else is cast as before.  One per chain
// (stream); whoever rewrites a normed buffer by other means resets `src`.
struct Bf16Image {
  const float* src = nullptr;
  void* buf = nullptr;
};

static int dec_linear(bool bf16, void* abf, const float* A, int64_t lda, const float* W, int64_t ldw, float* C, int64_t ldc,
                      int64_t M, const int64_t* m_dev, int N, int K, int epi, const float* bias, const float* res, int64_t ldr,
                      float* skw, hipStream_t st, StreamK* sk = nullptr, const Bf16Image* img = nullptr) {
  if (!bf16)
    return m_dev ? launch_linear_f32_ws_dev(A, lda, W, ldw, C, ldc, M, m_dev, N, K, epi, bias, res, ldr, skw, SPLITK_WS_BYTES, st, sk)
                 : launch_linear_f32_ws(A, lda, W, ldw, C, ldc, M, N, K, epi, bias, res, ldr, skw, SPLITK_WS_BYTES, st, sk);
  if (M == 0) return GDR_OK;
  GDR_CHECK_ARG(lda == K && K % 8 == 0, "decode(bf16): the activation operand must be dense with K %% 8 == 0");
  if (img && img->buf && img->src == A)  // the producing norm already wrote this operand's bf16 image
    return launch_linear_bf16(img->buf, K, W, ldw, C, ldc, M, N, K, epi, bias, res, ldr, st, m_dev);
  if (int rc = launch_cast_f32_bf16(A, abf, M * (int64_t)K, st)) return rc;
  return launch_linear_bf16(abf, K, W, ldw, C, ldc, M, N, K, epi, bias, res, ldr, st, m_dev);
}
// bf16 mode: a linear whose output feeds nothing but the next linear (wi -> wo_ff, linear1 -> linear2) emits it as bf16 straight
// from the GEMM epilogue — no fp32 copy is written and the consumer needs no cast launch (the rounding is the cast kernel's RNE of
// the same fp32 value: results are bit-identical).  out->buf receives the rows, out->src is set to `C` (the fp32 buffer the
// consumer names as its operand).  Returns 1 when the LDS-DMA kernel does not serve the shape (the caller runs the fp32 form).
static int dec_linear_out16(void* abf, const float* A, int64_t lda, const float* W, int64_t ldw, const float* C, int64_t ldc,
                            int64_t M, const int64_t* m_dev, int N, int K, int epi, const float* bias, hipStream_t st,
                            const Bf16Image* img, Bf16Image* out) {
  if (!out || !out->buf || lda != K || K % 64 != 0 || ldc != N) return 1;
  if (M == 0) return GDR_OK;
  const bool nb = epi == GDR_EPI_BIAS || epi == GDR_EPI_BIAS_RELU;
  const int act = (epi == GDR_EPI_RELU || epi == GDR_EPI_BIAS_RELU) ? 1 : 0;
  if (epi == GDR_EPI_RESIDUAL || epi == GDR_EPI_BIAS_RESIDUAL || epi == GDR_EPI_BIAS_GELU || (nb && !bias)) return 1;
  const void* a16 = abf;
  if (img && img->buf && img->src == A) {
    a16 = img->buf;
  } else if (int rc = launch_cast_f32_bf16(A, abf, M * (int64_t)K, st)) {
    return rc;
  }
  ProfScope prof(PROF_LINEAR, 2.0 * (double)M * (double)N * (double)K, st);
  const int rc = launch_linear_bf16_glds(a16, K, W, ldw, static_cast<float*>(out->buf), ldc, M, N, K, nb, 0, act, bias, nullptr, 0, 1, st,
                                         m_dev);
  if (rc == 0) out->src = C;
  return rc;
}
// A linear whose output rows are whole model rows, followed by the norm that always comes next on the decode path:
// C = epilogue(A·W^T), ne.Y = norm(C).  fp32 with split-K: the reduction kernel applies the norm while it holds the
// finished row (one launch instead of two or three); otherwise the linear and the norm kernels run one after another.
static int dec_linear_norm(bool bf16, void* abf, const float* A, int64_t lda, const float* W, int64_t ldw, float* C, int64_t ldc,
                           int64_t M, const int64_t* m_dev, int N, int K, int epi, const float* bias, const float* res,
                           int64_t ldr, float* skw, hipStream_t st, const NormEpilogue& ne, StreamK* sk = nullptr,
                           Bf16Image* img = nullptr, const Bf16Image* a_img = nullptr) {
  // img: receives the bf16 image of the norm's output; a_img (optional): where THIS linear's operand already lies as bf16
  // (an attention context or a ReLU output emitted as bf16 by its producer) — otherwise img is looked at for the operand too
  if (M == 0) return GDR_OK;
  const int64_t tiles = ((M + 127) / 128) * ((N + 127) / 128);
  // measured in round 2: 1 x 100 beams 8.62 -> 8.36 ms, 16 x 10 beams 9.88 -> 9.55, 64 x 10 beams 18.00 -> 17.60
  if (fuse_norm_on() && !bf16 && tiles < 192 && M <= 1536 && K % 32 == 0 && K / 32 >= 4 && ldc == N && ne.ldy == N) {
    const bool nb = epi == GDR_EPI_BIAS || epi == GDR_EPI_BIAS_RELU || epi == GDR_EPI_BIAS_RESIDUAL;
    const bool nr = epi == GDR_EPI_RESIDUAL || epi == GDR_EPI_BIAS_RESIDUAL;
    const int act = (epi == GDR_EPI_RELU || epi == GDR_EPI_BIAS_RELU) ? 1 : 0;
    GDR_CHECK_ARG(epi != GDR_EPI_BIAS_GELU && (!nb || bias) && (!nr || res), "decode: bad epilogue for a fused norm");
    const int rc = launch_linear_f32_small(A, lda, W, ldw, C, ldc, M, N, K, nb, nr, act, bias, res, ldr, skw, SPLITK_WS_BYTES, st,
                                           m_dev, &ne, nullptr, sk ? sk->live : nullptr);
    if (rc <= 0) return rc;
  }
  if (int rc = dec_linear(bf16, abf, A, lda, W, ldw, C, ldc, M, m_dev, N, K, epi, bias, res, ldr, skw, st, sk, a_img ? a_img : img))
    return rc;
  // bf16 mode: the last norm of this call also leaves its output rounded to bf16 for the linear that reads it next
  void* y16 = (bf16 && img && img->buf && ne.ldy == N) ? img->buf : nullptr;
  if (img) img->src = y16 ? ne.Y : nullptr;
  if (ne.kind == 1) {
    if (y16 && ne.y16_only)  // nobody reads these rows as fp32 (bf16 mode: every consumer is a linear): write the bf16 image alone
      return m_dev ? launch_rmsnorm_bf16_dev(C, ne.w1, y16, m_dev, M, N, ne.eps, st) : launch_rmsnorm_bf16(C, ne.w1, y16, M, N, ne.eps, st);
    return m_dev ? launch_rmsnorm_dev(C, ne.w1, ne.Y, m_dev, M, N, ne.eps, st, y16)
                 : launch_rmsnorm(C, ne.w1, ne.Y, M, N, ne.eps, nullptr, 1, st, y16);
  }
  if (ne.kind == 3) {  // norm1 -> + addv -> norm2 with the row held in registers (one launch, no intermediate pass)
    const int rc2 = launch_layernorm2(C, ne.w1, ne.b1, ne.w2, ne.b2, ne.addv, ne.Y, m_dev, M, N, ne.eps, st, y16);
    if (rc2 <= 0) return rc2;
  }
  // LayerNorm(s): the second one reads the first one's output through Y
  float* y1 = ne.kind == 3 ? C : ne.Y;  // kind 3: norm1 may overwrite C (the pre-norm rows are not needed again)
  if (int rc = m_dev ? launch_layernorm_dev(C, ne.w1, ne.b1, y1, m_dev, M, N, ne.eps, nullptr, st, ne.kind == 3 ? nullptr : y16)
                     : launch_layernorm(C, ne.w1, ne.b1, y1, M, N, ne.eps, nullptr, st, ne.kind == 3 ? nullptr : y16))
    return rc;
  if (ne.kind == 3)
    return m_dev ? launch_layernorm_dev(y1, ne.w2, ne.b2, ne.Y, m_dev, M, N, ne.eps, ne.addv, st, y16)
                 : launch_layernorm(y1, ne.w2, ne.b2, ne.Y, M, N, ne.eps, ne.addv, st, y16);
  return GDR_OK;
}
// element offset into a linear weight (fp32 or bf16 storage)
static const float* w_at(const float* W, size_t elems, bool bf16) {
  return reinterpret_cast<const float*>(reinterpret_cast<const char*>(W) + elems * (bf16 ? 2 : 4));
}

// One chain of decode linears: a stream with the scratch that only launches on that stream may touch — the bf16 mode's rounded
// operand (abf), the split-K region (skw) with its stream-K hand-off (sk) and the bf16 image of the chain's last normed rows (img).
// m_dev: device-side row count, or null for all M rows.
struct DecChain {
  bool bf16;
  void* abf;
  float* skw;
  hipStream_t st;
  StreamK* sk;
  Bf16Image* img;
  int linear(const float* A, int64_t lda, const float* W, int64_t ldw, float* C, int64_t ldc, int64_t M, const int64_t* m_dev, int N,
             int K, int epi, const float* bias, const float* res, int64_t ldr) const {
    return dec_linear(bf16, abf, A, lda, W, ldw, C, ldc, M, m_dev, N, K, epi, bias, res, ldr, skw, st, sk, img);
  }
  int linear_norm(const float* A, int64_t lda, const float* W, int64_t ldw, float* C, int64_t ldc, int64_t M, const int64_t* m_dev,
                  int N, int K, int epi, const float* bias, const float* res, int64_t ldr, const NormEpilogue& ne,
                  const Bf16Image* a_img = nullptr) const {
    return dec_linear_norm(bf16, abf, A, lda, W, ldw, C, ldc, M, m_dev, N, K, epi, bias, res, ldr, skw, st, ne, sk, img, a_img);
  }
  // a linear that feeds nothing but the next linear: bf16 mode emits `out` (dec_linear_out16) when the LDS-DMA kernel serves the
  // shape; otherwise, and in the fp32 mode, the fp32 form writes C and `out` names nothing
  int linear_for_linear(const float* A, int64_t lda, const float* W, int64_t ldw, float* C, int64_t ldc, int64_t M, const int64_t* m_dev,
                        int N, int K, int epi, const float* bias, Bf16Image* out) const {
    const int r16 = bf16 ? dec_linear_out16(abf, A, lda, W, ldw, C, ldc, M, m_dev, N, K, epi, bias, st, img, out) : 1;
    if (r16 != 1) return r16 < 0 ? r16 : GDR_OK;
    out->src = nullptr;
    return linear(A, lda, W, ldw, C, ldc, M, m_dev, N, K, epi, bias, nullptr, 0);
  }
};

// Self-attention of a decode step: one query row per batch entry against its Lk ancestors (itself last) in a [rows][3*width] cache
// of (q | k | v) rows, key j of entry b at cache row kv_rows[b][j].  The caller sets the output (and b_count_dev / live).
static AttnArgs ancestor_attn(const float* q, const float* cache, int width, int heads, int B, int Lk, const int32_t* kv_rows,
                              float scale, const float* rel_bias, int buckets, const BucketLut& lut, int causal_neg_inf) {
  AttnArgs at{};
  at.q = q, at.k = cache + width, at.v = cache + 2 * width;
  at.ldq = at.ldk = at.ldv = 3 * width, at.ldo = width;
  at.q_bstride = 1, at.k_bstride = 0, at.o_bstride = 1;
  at.B = B, at.H = heads, at.dk = width / heads, at.Lq = 1, at.Lk = Lk, at.q_pos0 = Lk - 1, at.scale = scale;
  at.rel_bias = rel_bias, at.bidirectional = 0, at.num_buckets = buckets, at.lut = lut;
  at.key_mask = nullptr, at.mask_bstride = 0, at.causal = 1, at.causal_neg_inf = causal_neg_inf;
  at.kv_rows = kv_rows, at.kv_group = 1;
  return at;
}

// ------------------------------------------------------------------------------------------ model workspace
// The plain form of GdrT5DecoderWeights (include/gdr_hip.h): no adaptor, the head is lm_head's rows alone.
static bool plain_head(const GdrT5DecoderWeights& w) { return w.adaptor_layers == 0 && !w.alayers && !w.head_w; }

struct GenBufs {
  BeamBufs bb;
  float *dcache, *acache, *crosskv, *xd, *xa, *nx, *ctx, *qc, *ff, *tmp, *A, *hl, *skw, *ctx2, *ff2, *skw2, *qkv_c;
  void *abf, *abf2, *img1, *img2, *c16a, *c16b, *f16a, *f16b;
};

// a region of a workspace laid out at offset `o`: counted always, and with `dst` its pointer is filed in dst->field
#define CARVE(dst, field, bytes)                                                      \
  do {                                                                                \
    const size_t at__ = carve(o, bytes);                                              \
    if (dst) dst->field = reinterpret_cast<decltype(dst->field)>(base + at__);        \
  } while (0)

// Bytes of gdr_t5_generate's workspace; with `base` (and g) the regions' pointers are filled in (the shape of beam_layout).
static size_t gen_layout(const GdrT5DecoderWeights& w, const BeamDims& bd, int L, char* base, GenBufs* g) {
  // plain head: no adaptor chain — its K/V cache, its activations and their bf16 images, and the head-matrix buffer A take no
  // bytes (adaptor_ff is ignored); the side stream's split-K region and bf16 operand stay, the cross K/V projections use them
  const bool plain = plain_head(w);
  const size_t ad = plain ? 0 : 1, aff = plain ? 0 : (size_t)w.adaptor_ff;
  const GdrT5Dims& dm = w.dims;
  const size_t rows = (size_t)bd.B * bd.R, d = dm.d_model, inner = (size_t)dm.num_heads * dm.d_kv;
  const size_t tmax = bd.maxlen, wide = inner > d ? inner : d;
  const size_t ffw = (size_t)dm.d_ff > aff ? (size_t)dm.d_ff : aff;
  const size_t abf_main = rows * ffw > (size_t)bd.B * L * d ? rows * ffw : (size_t)bd.B * L * d;
  size_t o = 0;
  const size_t beam_at = carve(o, beam_layout(bd, nullptr, nullptr));
  if (g) beam_layout(bd, base + beam_at, &g->bb);
  CARVE(g, dcache, 4 * (size_t)dm.num_layers * tmax * rows * 3 * inner);
  CARVE(g, acache, ad * 4 * (size_t)w.adaptor_layers * tmax * rows * 3 * d);
  CARVE(g, crosskv, 4 * (size_t)dm.num_layers * bd.B * L * 2 * inner);
  CARVE(g, xd, 4 * rows * d);
  CARVE(g, xa, ad * 4 * rows * d);
  CARVE(g, nx, 4 * rows * d);
  CARVE(g, ctx, 4 * rows * wide);
  CARVE(g, qc, 4 * rows * inner);
  CARVE(g, ff, 4 * rows * ffw);
  CARVE(g, tmp, ad * 4 * rows * d);
  CARVE(g, A, ad * 4 * rows * (size_t)(bd.V + 1) * d);
  CARVE(g, hl, 4 * rows * d);
  CARVE(g, skw, SPLITK_WS_BYTES);
  CARVE(g, ctx2, ad * 4 * rows * d);      // adaptor chain runs on a side stream: own scratch
  CARVE(g, ff2, 4 * rows * aff);
  CARVE(g, skw2, SPLITK_WS_BYTES);
  CARVE(g, qkv_c, ad * 4 * rows * 3 * d);  // prefix-table mode: (q,k,v) of the compacted rows
  CARVE(g, abf, 2 * abf_main);            // bf16 mode: the rounded activation operand of a linear (main stream)
  CARVE(g, abf2, 2 * abf_main);           //            ... of the side stream (adaptor chain, cross K/V projections)
  CARVE(g, img1, 2 * rows * d);           // bf16 mode: the bf16 image of the last normed rows of either chain (Bf16Image)
  CARVE(g, img2, ad * 2 * rows * d);
  CARVE(g, c16a, 2 * rows * wide);        // bf16 mode: attention contexts / ReLU outputs emitted as bf16 by their
  CARVE(g, c16b, ad * 2 * rows * d);      // producers (a: decoder chain, b: adaptor chain) — the operand of
  CARVE(g, f16a, 2 * rows * ffw);         // the linear behind them, which then needs no cast launch
  CARVE(g, f16b, 2 * rows * aff);
  return o;
}

// bf16 mode from ~1 000 beam rows on: the head GEMM waits for the decoder stack and takes the dot with its hidden state in its own
// epilogue (launch_linear_bf16_headdot) instead of writing rows x (V+1) x d floats for head_logits to read back (1.46 GB per step at
// 15 360 rows).  At these sizes both chains fill the chip, so the adaptor chain gives up nothing by ending one GEMM earlier
// (generate() 512 x 30 beams 44.5 -> 41.8 ms, 2 048 x 10 62.4 -> 58.9, 256 x 10 14.43 -> 14.15, 64 x 30 12.64 -> 12.5; below
// HEAD_DOT_ROWS the GEMM stays on the adaptor chain, beside the decoder stack).  Same products, another fp32 summation tree.
constexpr int HEAD_DOT_ROWS = 1024;

// One gdr_t5_generate call: its arguments, what they imply, and the pieces of the step loop (generate_impl puts them in order).
// The chains point at the call's own StreamK / Bf16Image members: a GenCall is built in place and never copied.
struct GenCall {
  const GdrT5DecoderWeights* w;  // the arguments, as gdr_t5_generate names them
  const float* enc_hidden;
  const int64_t* enc_mask;
  int B, L, num_beams, max_length;
  const GdrPrefixTable* ptab;
  int64_t* out_ids;
  int32_t* out_len;
  double* out_scores;
  float* step_scores;
  int32_t* step_tokens;
  void* workspace;
  size_t workspace_bytes;
  bool bf16;
  hipStream_t stream;
  bool forced, greedy, plain;  // set by validate() / lay_out()
  BeamDims bd;
  GenBufs g;
  int d, H, dk, inner, rows, V1, aH, ahd, aff;
  size_t dslab, aslab, dlayer, alayer, ckv_layer;  // one position of one decoder / adaptor layer's cache; a layer's cache, cross K/V
  bool dedup0, slab_q_on, ckv_side;  // set by begin()
  Bf16Image img1, img2, c16a, c16b, f16a, f16b;
  StreamK sk1, sk2;
  int32_t *done_word, my_epoch;
  SideLease lease;
  hipStream_t as;       // adaptor stream: the leased side stream, or the caller's
  DecChain main, side;  // the two chains of linears: the decoder stack on the caller's stream, the adaptor on `as`
  BucketLut lut_uni, lut_bi;
  int cur;  // index of the current seq / node buffer: flips every step

  int validate(double length_penalty, int num_return_sequences, const GdrTrie* trie) {
    // out_len == NULL selects the score mode: out_ids holds GIVEN rows (read, never written), out_scores receives the score the search
    // reports for each of them and step_scores, when given, the decoder's last hidden states (forced_step_kernel's planes).  There is
    // nothing to search or constrain, and one row's tokens say nothing about a prefix-table node
    GDR_CHECK_ARG(w && enc_hidden && enc_mask && out_ids && out_scores && workspace, "generate: null pointer");
    forced = out_len == nullptr;
    if (forced) {
      GDR_CHECK_ARG(!trie, "generate(score mode, out_len=NULL): trie must be NULL (the rows are given, nothing is constrained)");
      GDR_CHECK_ARG(!ptab, "generate(score mode, out_len=NULL): prefix_table must be NULL");
      GDR_CHECK_ARG(!step_tokens,
                    "generate(score mode, out_len=NULL): step_tokens must be NULL (step_scores receives the hidden states; there is no top-2R trace)");
    }
    const GdrT5Dims& dm = w->dims;
    // num_beams = 1 is the reference's non-beam branch (greedy_step_kernel): one sequence per query, and neither the trie constraint nor
    // the top-2R trace, which exist for the beam search only — refused here, before anything behind those pointers is looked at
    greedy = !forced && num_beams == 1;
    if (greedy) {
      GDR_CHECK_ARG(num_return_sequences == 1, "generate: num_return_sequences=%d must be 1 at num_beams=1 (greedy decoding gives one sequence per query)",
                    num_return_sequences);
      GDR_CHECK_ARG(!trie, "generate: trie must be NULL at num_beams=1 (the constraint belongs to the beam search)");
      GDR_CHECK_ARG(!step_scores, "generate: step_scores must be NULL at num_beams=1 (the top-2R trace belongs to the beam search)");
      GDR_CHECK_ARG(!step_tokens, "generate: step_tokens must be NULL at num_beams=1 (the top-2R trace belongs to the beam search)");
    }
    // the head: either the adaptor (layers > 0 with alayers and head_w) or the plain form (none of the three) — never a mixture
    GDR_CHECK_ARG(w->adaptor_layers >= 0, "generate: adaptor_layers=%d must be >= 0", w->adaptor_layers);
    GDR_CHECK_ARG(w->adaptor_layers == 0 || w->alayers, "generate: alayers is NULL at adaptor_layers=%d", w->adaptor_layers);
    GDR_CHECK_ARG(w->adaptor_layers == 0 || w->head_w, "generate: head_w is NULL at adaptor_layers=%d", w->adaptor_layers);
    GDR_CHECK_ARG(w->adaptor_layers > 0 || !w->alayers, "generate: alayers must be NULL at adaptor_layers=0 (the plain lm_head form)");
    GDR_CHECK_ARG(w->adaptor_layers > 0 || !w->head_w, "generate: head_w must be NULL at adaptor_layers=0 (the plain lm_head form)");
    plain = plain_head(*w);
    GDR_CHECK_ARG(!plain || !ptab,
                  "generate: prefix_table must be NULL with plain-head weights (the table stores adaptor results; lm_head alone has "
                  "nothing query-independent to store)");
    GDR_CHECK_ARG(!trie || (trie->child && trie->eos_ok && trie->n_nodes > 0), "generate: bad trie");
    GDR_CHECK_ARG(!trie || trie->V == w->out_vocab, "generate: trie built for V=%d but the head has output_vocab_size=%d",
                  trie ? trie->V : 0, w->out_vocab);
    GDR_CHECK_ARG(!ptab || (ptab->child && ptab->kv && ptab->W && ptab->n_nodes > 0 && ptab->n_table > 0 &&
                            ptab->n_table <= ptab->n_nodes && ptab->V == w->out_vocab),
                  "generate: bad prefix table (V=%d, head output_vocab_size=%d)", ptab ? ptab->V : 0, w->out_vocab);
    GDR_CHECK_ARG(!ptab || !trie || (trie->child == ptab->child && trie->n_nodes == ptab->n_nodes),
                  "generate: the trie constraint and the prefix table must be built over the same trie arrays");
    GDR_CHECK_ARG(!ptab || (dm.d_model % 32 == 0 && w->adaptor_ff % 32 == 0), "generate: prefix-table mode needs d %% 32 == 0");
    if (ptab && ptab->complete_levels > 1) {
      // complete_levels = c claims that levels 0 .. c-1 of the table hold ALL V^s prefixes of their length: at steps s < c the
      // miss-row chain is not even enqueued, so an overstated c would read head rows nobody computed.  It can be checked
      // against the table's own size: sum_{s<c} V^s nodes must fit in n_table, and no level lies beyond the decode length.
      GDR_CHECK_ARG(ptab->complete_levels <= w->max_out_len - 1, "generate: prefix table complete_levels=%d exceeds the %d decode steps",
                    ptab->complete_levels, w->max_out_len - 1);
      int64_t need = 0, pw = 1;
      for (int s = 0; s < ptab->complete_levels; ++s) {
        need += pw;
        pw *= ptab->V;
        if (need > ptab->n_table) break;
      }
      GDR_CHECK_ARG(need <= ptab->n_table, "generate: prefix table claims %d complete levels (>= %lld nodes) but holds %d nodes",
                    ptab->complete_levels, (long long)need, ptab->n_table);
    }
    bd = BeamDims{B, num_beams, w->out_vocab, dm.vocab_size, max_length, num_return_sequences, length_penalty,
                  trie ? trie->child : (ptab ? ptab->child : nullptr), trie ? trie->eos_ok : nullptr,
                  trie ? trie->n_nodes : (ptab ? ptab->n_nodes : 0)};
    GDR_TRY(forced ? check_forced_dims(bd, max_length) : greedy ? check_greedy_dims(bd, max_length) : check_beam_dims(bd, max_length));
    GDR_CHECK_ARG(L >= 1 && L <= T5_MAX_LEN, "generate: L=%d must be in [1,%d]", L, T5_MAX_LEN);
    GDR_CHECK_ARG(max_length <= w->max_out_len, "generate: max_length=%d > max_output_length=%d of the head", max_length,
                  w->max_out_len);
    GDR_CHECK_ARG(dm.d_model % 4 == 0 && dm.d_kv % 4 == 0, "generate: unsupported dims");
    // the adaptor's head width; the plain form ignores adaptor_nhead / adaptor_ff / adaptor_eps
    GDR_CHECK_ARG(plain || (w->adaptor_nhead > 0 && dm.d_model % w->adaptor_nhead == 0 && (dm.d_model / w->adaptor_nhead) % 4 == 0),
                  "generate: unsupported dims");
    GDR_CHECK_ARG(w->dec_embed && w->self_rel_bias && w->cross_rel_bias && w->final_ln && w->layers && w->head_e,
                  "generate: null weight pointer");
    return GDR_OK;
  }

  // the workspace checks (behind validate(), in the order they always had) and the sizes every piece uses
  int lay_out() {
    const GdrT5Dims& dm = w->dims;
    const size_t need = gen_layout(*w, bd, L, nullptr, nullptr);
    if (workspace_bytes < need) {
      set_error("generate: workspace %zu < required %zu", workspace_bytes, need);
      return GDR_ENOSPC;
    }
    GDR_CHECK_ARG(((uintptr_t)workspace & 255) == 0, "generate: workspace must be 256-byte aligned");
    gen_layout(*w, bd, L, static_cast<char*>(workspace), &g);
    GDR_CHECK_ARG(!bf16 || (dm.d_model % 8 == 0 && dm.d_ff % 8 == 0 && (dm.num_heads * dm.d_kv) % 8 == 0 && (plain || w->adaptor_ff % 8 == 0)),
                  "generate(bf16): dims must be multiples of 8");
    d = dm.d_model, H = dm.num_heads, dk = dm.d_kv, inner = H * dk;
    rows = B * num_beams, V1 = bd.V + 1;
    aH = w->adaptor_nhead, ahd = plain ? 0 : d / aH, aff = w->adaptor_ff;
    dslab = (size_t)rows * 3 * inner, aslab = (size_t)rows * 3 * d;
    dlayer = (size_t)max_length * dslab, alayer = (size_t)max_length * aslab;
    ckv_layer = (size_t)B * L * 2 * inner;
    return GDR_OK;
  }

  // the bookkeeping's first launch, the stream-K flags, the early exit's words, the side stream and the two chains
  int begin() {
    static const bool dedup0_on = env_flag("GDR_DECODE_DEDUP0", true);     // exact A/B knob: 0 = run step 0 on all B*R (identical) beam rows
    static const bool early_on = env_flag("GDR_DECODE_EARLY_EXIT", true);  // A/B knob: 0 = always run all max_length - 1 steps
    static const bool slab_q = env_flag("GDR_DECODE_SLAB_Q", true);        // A/B knob: 0 = reduce the cross-attention q projection in its own launch
    dedup0 = dedup0_on && !forced, slab_q_on = slab_q;  // score mode: the rows of a query differ from position 1 on and keep a slot each
    BeamBufs& bb = g.bb;
    GDR_TRY(forced   ? forced_begin(bb, bd, out_ids, stream)
            : greedy ? greedy_begin(bb, bd, out_ids, out_len, out_scores, stream)
                     : beam_begin(bb, bd, stream, dedup0));
    // stream-K hand-off scratch of the two chains' big linears (gemm_f32.hip) inside their split-K regions — a launch uses one
    // or the other; both flag blocks are zeroed here, on the caller's stream, before the adaptor stream is first forked
    sk1 = StreamK{g.skw, reinterpret_cast<int32_t*>(reinterpret_cast<char*>(g.skw) + STREAMK_PART_BYTES), 0};
    sk2 = StreamK{g.skw2, reinterpret_cast<int32_t*>(reinterpret_cast<char*>(g.skw2) + STREAMK_PART_BYTES), 0};
    if (hipMemsetAsync(sk1.flag, 0, 512 * sizeof(int32_t), stream) != hipSuccess ||
        hipMemsetAsync(sk2.flag, 0, 512 * sizeof(int32_t), stream) != hipSuccess) {
      set_error("generate: memset of the stream-K flags failed");
      return GDR_EHIP;
    }
    // early exit (see done_words): not while a caller wants the per-step trace — its rows of the steps not run would be undefined
    done_word = nullptr, my_epoch = 0;
    if (early_on && !forced && !step_scores && !step_tokens) {  // score mode: every position of every row is wanted
      if (int32_t* words = done_words()) {
        my_epoch = g_done_epoch.fetch_add(1) + 1;  // never 0
        done_word = words + (my_epoch & 63);
        bb.all_done_host = done_word, bb.done_epoch = my_epoch;  // travels with every beam_update launch
      }
      sk1.live = sk2.live = bb.live;  // the device-side half: steps already enqueued when the last query finishes skip their work
      bb.live_gate = bb.live;         // ... and so do their attention, reduction, head and beam bookkeeping launches
    }
    lease.acquire();
    as = lease.ss ? lease.ss->s : stream;
    Bf16Image* const im[6] = {&img1, &img2, &c16a, &c16b, &f16a, &f16b};
    void* const im_buf[6] = {g.img1, g.img2, g.c16a, g.c16b, g.f16a, g.f16b};
    for (int i = 0; i < 6; ++i) *im[i] = Bf16Image{nullptr, bf16 ? im_buf[i] : nullptr};
    main = DecChain{bf16, g.abf, g.skw, stream, &sk1, &img1};  // each chain with scratch of its own
    side = DecChain{bf16, g.abf2, g.skw2, as, &sk2, &img2};
    lut_uni = make_bucket_lut(w->dims.rel_buckets, w->dims.rel_max_distance);
    lut_bi = make_bucket_lut(w->dims.rel_buckets / 2, w->dims.rel_max_distance);
    cur = 0;
    return GDR_OK;
  }

  // cross-attention K/V once per query and layer (modeling_t5.py:365-368 recomputes them per beam row per step).  They
  // depend on the encoder states only: with a side stream they are projected THERE (the adaptor chain's scratch), layer by
  // layer, while the main stream already runs step 0 — a chain of small latency-bound kernels over one row per query that
  // leaves most of the chip idle — and layer l's cross-attention of step 0 waits for layer l's event.
  int cross_kv() {
    ckv_side = lease.ss && w->dims.num_layers <= SIDE_MAX_LAYERS;
    if (ckv_side) GDR_TRY(stream_after(as, lease.ss->fork, stream, "generate: fork to the side stream failed"));
    const DecChain early{bf16, g.abf2, g.skw2, as, &sk2, nullptr};  // the side chain before its first norm: no bf16 image yet
    const DecChain& chain = ckv_side ? early : main;
    for (int l = 0; l < w->dims.num_layers; ++l) {
      GDR_TRY(chain.linear(enc_hidden, d, w->layers[l].wkv_c, d, g.crosskv + l * ckv_layer, 2 * inner, (int64_t)B * L, nullptr, 2 * inner, d,
                           GDR_EPI_NONE, nullptr, nullptr, 0));
      if (ckv_side && hipEventRecord(lease.ss->ckv[l], as) != hipSuccess) {
        set_error("generate: event record on the side stream failed");
        return GDR_EHIP;
      }
    }
    return GDR_OK;
  }

  // `if all(done): break` (generation_utils.py:836-838): the word beam_update_kernel / greedy_step_kernel store the call's epoch into
  bool all_done(int s) const { return done_word && s > 0 && __atomic_load_n(done_word, __ATOMIC_RELAXED) == my_epoch; }

  // Step 0: the R beam rows of a query hold the same START token and the same encoder states, so their decoder /
  // adaptor / head outputs are identical rows (generation_utils.py:437-442 expands the encoder states, :663-668 starts
  // every beam but the first at -1e9): one row per query is computed (row b of the step-0 cache slots; every row's
  // ancestor at position 0 is b, beam_init_kernel) and beam_topk_kernel reads the query's logits for all of its beams.
  bool one_row_per_query(int s) const { return s == 0 && dedup0; }
  int rows_at(int s) const { return one_row_per_query(s) ? B : rows; }
  int beams_at(int s) const { return one_row_per_query(s) ? 1 : num_beams; }
  // prefix-table mode, steps at which every possible prefix is a table node (step 0: the root; deeper while the trie's
  // levels are complete, GdrPrefixTable.complete_levels): the adaptor chain and the head GEMM would run over zero rows
  // (34 launches per step that exit at once — 0.2 ms of the side queue and, at one query x 100 beams, of the host's time)
  bool adaptor_idle(int s) const { return ptab != nullptr && s < (ptab->complete_levels > 1 ? ptab->complete_levels : 1); }
  bool fuse_head(int s) const {
    return bf16 && ptab && !adaptor_idle(s) && fuse_norm_on() && rows_at(s) >= HEAD_DOT_ROWS && d % 128 == 0;
  }
  const float* head_w(int s) const { return w_at(w->head_w, (size_t)s * V1 * d * d, bf16); }

  // the decoder's normed rows `nx` feed linears only; in the bf16 mode those read the bf16 image, so the fp32 copy is not written
  // (the final norm's rows `hl` go into the fp32 head dot: kept)
  NormEpilogue rms(const float* wgt, float* y) const {
    return NormEpilogue{1, wgt, nullptr, nullptr, nullptr, nullptr, w->dims.eps, y, (int64_t)d, (bf16 && y != g.hl) ? 1 : 0};
  }
  NormEpilogue ln(const float* w1, const float* b1, float* y) const {
    return NormEpilogue{2, w1, b1, nullptr, nullptr, nullptr, w->adaptor_eps, y, (int64_t)d};
  }
  NormEpilogue ln2(const GdrAdaptorLayer& al, float* y) const {  // norm1 -> + cross_const -> norm2
    return NormEpilogue{3, al.ln1_w, al.ln1_b, al.ln2_w, al.ln2_b, al.cross_const, w->adaptor_eps, y, (int64_t)d};
  }
  // the bf16-mode attention kernels write the context's bf16 image only (d_kv % 4 == 0 rows of 8-byte pieces)
  void ctx_to(AttnArgs& at, Bf16Image& im, float* fp32_ctx) const {
    if (bf16 && im.buf) at.out = nullptr, at.out_bf16 = im.buf, im.src = fp32_ctx;
    else at.out = fp32_ctx;
    at.live = g.bb.live_gate;  // a step behind the last query's end: the attention launch exits at once
  }

  // the decoder's input rows with the first norm of its stack; the adaptor chain starts beside it, its input rows on `as`
  // (adaptor = false: a position with no head behind it, the score mode's last — the decoder stack alone)
  int embed_and_fork(int s, bool adaptor = true) {
    const BeamBufs& bb = g.bb;
    const int rows_s = rows_at(s);
    img1.src = img2.src = nullptr;  // the embedding kernels rewrite nx / xa without a bf16 image
    hipLaunchKernelGGL(embed_rmsnorm_kernel, dim3((unsigned)((rows_s + 3) / 4)), dim3(256), 0, stream, w->dec_embed, bb.cur_tok, rows_s,
                       d / 4, w->dims.vocab_size, w->layers[0].ln_self, w->dims.eps, g.xd, g.nx, sk1.live);
    GDR_CHECK_LAUNCH("embed_rmsnorm_kernel");
    if (!adaptor) return GDR_OK;
    // plain head: no second chain — nothing is forked or joined per step (the cross K/V projections are joined through
    // their own per-layer events at step 0)
    if (lease.ss && !plain) GDR_TRY(stream_after(as, lease.ss->fork, stream, "generate: fork to the adaptor stream failed"));
    if (!ptab && !plain) GDR_TRY(launch_embed(w->dec_embed, bb.cur_tok, rows_s, d, w->dims.vocab_size, g.xa, as));
    if (!ptab) return GDR_OK;
    // ---------------- prefix-table mode: rows whose prefix is a table node take everything from the table; the rest
    // are compacted (row count *bb.n_miss lives on the device) and run the same chain + the head GEMM on `as`
    hipLaunchKernelGGL(prefix_plan_kernel, dim3(1), dim3(1024), 0, as, bb, rows_s, s + 1, cur, ptab->n_table);
    GDR_CHECK_LAUNCH("prefix_plan_kernel");
    hipLaunchKernelGGL(prefix_fill_kernel, dim3(rows_s), dim3(256), 0, as, bb, rows_s, s + 1, cur, ptab->kv,
                       (int64_t)ptab->n_table * 3 * d, g.acache + s * aslab, (int64_t)alayer, w->adaptor_layers, 3 * d);
    GDR_CHECK_LAUNCH("prefix_fill_kernel");
    if (!adaptor_idle(s)) {  // idle steps: every row sits on a table node, nothing is compacted
      hipLaunchKernelGGL(embed_rows_kernel, dim3((unsigned)((rows_s + 3) / 4)), dim3(256), 0, as, w->dec_embed, bb.cur_tok,
                         bb.miss_rows, bb.n_miss, d / 4, w->dims.vocab_size, g.xa);
      GDR_CHECK_LAUNCH("embed_rows_kernel");
    }
    return GDR_OK;
  }

  // ---------------- adaptor: post-LN nn.TransformerDecoder over decode_embeddings(ids) (modeling_t5.py:1615-1633)
  int ad_layer(int l, int s) {
    const BeamBufs& bb = g.bb;
    const GdrAdaptorLayer& al = w->alayers[l];
    const int rows_s = rows_at(s);
    const bool tab = ptab != nullptr;  // the compacted rows: (q,k,v) into qkv_c and from there to their cache slots; *n_miss rows
    float *xa = g.xa, *tmp = g.tmp, *ff2 = g.ff2;
    float* cache = g.acache + l * alayer;
    float* slot = cache + s * aslab;
    float* qkv = tab ? g.qkv_c : slot;
    const int64_t* m_dev = tab ? bb.n_miss : nullptr;
    GDR_TRY(side.linear(xa, d, al.in_w, d, qkv, 3 * d, rows_s, m_dev, 3 * d, d, GDR_EPI_BIAS, al.in_b, nullptr, 0));
    if (tab) {
      hipLaunchKernelGGL(scatter_slot_kernel, dim3((unsigned)((rows_s + 3) / 4)), dim3(256), 0, as, g.qkv_c, bb.miss_rows, bb.n_miss,
                         3 * d / 4, d / 4, slot);
      GDR_CHECK_LAUNCH("scatter_slot_kernel");
    }
    AttnArgs at = ancestor_attn(qkv, cache, d, aH, rows_s, s + 1, tab ? bb.kv_rows_c : bb.kv_rows, 1.0f / sqrtf((float)ahd), nullptr, 0,
                                lut_uni, 1);
    at.b_count_dev = m_dev;
    ctx_to(at, c16b, g.ctx2);
    GDR_TRY(launch_attention(at, as));
    // tmp = norm2(norm1(out_proj(ctx) + xa) + cross_const); xa = norm3(lin2(relu(lin1(tmp))) + tmp)
    GDR_TRY(side.linear_norm(g.ctx2, d, al.out_w, d, tmp, d, rows_s, m_dev, d, d, GDR_EPI_BIAS_RESIDUAL, al.out_b, xa, d, ln2(al, tmp),
                             &c16b));
    GDR_TRY(side.linear_for_linear(tmp, d, al.lin1_w, d, ff2, aff, rows_s, m_dev, aff, d, GDR_EPI_BIAS_RELU, al.lin1_b, &f16b));
    return side.linear_norm(ff2, aff, al.lin2_w, aff, xa, d, rows_s, m_dev, d, aff, GDR_EPI_BIAS_RESIDUAL, al.lin2_b, tmp, d,
                            ln(al.ln3_w, al.ln3_b, xa), &f16b);
  }

  // ---------------- T5 decoder stack (modeling_t5.py:498-584, 685-821)
  int dec_layer(int l, int s) {
    const GdrT5Dims& dm = w->dims;
    const GdrT5DecLayer& ly = w->layers[l];
    const int rows_s = rows_at(s), R_s = beams_at(s);
    float *xd = g.xd, *nx = g.nx, *ctx = g.ctx, *qc = g.qc, *ff = g.ff;
    float* cache = g.dcache + l * dlayer;
    float* slot = cache + s * dslab;
    // every later RMS norm rides on the reduction of the residual linear in front of it (dec_linear_norm)
    // (the first block's norm rides on the embedding launch: embed_rmsnorm_kernel)
    GDR_TRY(main.linear(nx, d, ly.wqkv, d, slot, 3 * inner, rows_s, nullptr, 3 * inner, d, GDR_EPI_NONE, nullptr, nullptr, 0));
    AttnArgs at = ancestor_attn(slot, cache, inner, H, rows_s, s + 1, g.bb.kv_rows, 1.0f, w->self_rel_bias, dm.rel_buckets, lut_uni, 0);
    ctx_to(at, c16a, ctx);
    GDR_TRY(launch_attention(at, stream));
    GDR_TRY(main.linear_norm(ctx, inner, ly.wo, inner, xd, d, rows_s, nullptr, d, inner, GDR_EPI_RESIDUAL, nullptr, xd, d,
                             rms(ly.ln_cross, nx), &c16a));
    // cross attention over the encoder states of the row's query
    // the q projection's split-K slabs go to the attention kernel un-reduced (it sums them while it stages the beam rows'
    // queries): one dependent launch less per layer and step
    SlabRef qsl{nullptr, 1, 0};
    bool q_from_slabs = false;
    if (slab_q_on && !bf16 && R_s > 1 /* the Lq = 1 kernel of the de-duplicated step 0 takes finished q rows */ &&
        ((rows_s + 127) / 128) * ((inner + 127) / 128) < 192 && rows_s <= 1536 && d % 32 == 0 && d / 32 >= 4) {
      const int rc_ = launch_linear_f32_small(nx, d, ly.wq_c, d, qc, inner, rows_s, inner, d, 0, 0, 0, nullptr, nullptr, 0, g.skw,
                                              SPLITK_WS_BYTES, stream, nullptr, nullptr, &qsl, sk1.live);
      if (rc_ < 0) return rc_;
      q_from_slabs = rc_ == 0;
    }
    if (!q_from_slabs) GDR_TRY(main.linear(nx, d, ly.wq_c, d, qc, inner, rows_s, nullptr, inner, d, GDR_EPI_NONE, nullptr, nullptr, 0));
    AttnArgs ca{};
    const float* ckv = g.crosskv + l * ckv_layer;
    // the R beam rows of a query are consecutive and share its K/V: one workgroup per (query, head) stages K/V
    // once and serves all R rows (they all sit at decoder position s)
    ca.q = qc, ca.k = ckv, ca.v = ckv + inner;
    ctx_to(ca, c16a, ctx);
    ca.ldq = inner, ca.ldk = ca.ldv = 2 * inner, ca.ldo = inner;
    ca.q_bstride = R_s, ca.k_bstride = L, ca.o_bstride = R_s;
    ca.B = B, ca.H = H, ca.dk = dk, ca.Lq = R_s, ca.Lk = L, ca.q_pos0 = s, ca.scale = 1.0f, ca.q_same_pos = 1;
    ca.rel_bias = w->cross_rel_bias, ca.bidirectional = 1, ca.num_buckets = dm.rel_buckets, ca.lut = lut_bi;
    ca.key_mask = enc_mask, ca.mask_bstride = L, ca.causal = 0, ca.causal_neg_inf = 0;
    ca.kv_rows = nullptr, ca.kv_group = 1;
    if (q_from_slabs && qsl.S > 1) ca.q_part = qsl.part, ca.q_S = qsl.S, ca.q_tiles_n = qsl.tiles_n;
    if (s == 0 && ckv_side && hipStreamWaitEvent(stream, lease.ss->ckv[l], 0) != hipSuccess) {
      set_error("generate: wait for the cross K/V of layer %d failed", l);
      return GDR_EHIP;
    }
    GDR_TRY(launch_attention(ca, stream));
    GDR_TRY(main.linear_norm(ctx, inner, ly.wo_c, inner, xd, d, rows_s, nullptr, d, inner, GDR_EPI_RESIDUAL, nullptr, xd, d,
                             rms(ly.ln_ff, nx), &c16a));
    const bool last = l + 1 == dm.num_layers;  // the norm behind the block: the next block's first, or final_layer_norm
    GDR_TRY(main.linear_for_linear(nx, d, ly.wi, d, ff, dm.d_ff, rows_s, nullptr, dm.d_ff, d, GDR_EPI_RELU, nullptr, &f16a));
    return main.linear_norm(ff, dm.d_ff, ly.wo_ff, dm.d_ff, xd, d, rows_s, nullptr, d, dm.d_ff, GDR_EPI_RESIDUAL, nullptr, xd, d,
                            rms(last ? w->final_ln : w->layers[l + 1].ln_self, last ? g.hl : nx), &f16a);
  }

  // the adaptor chain's end: the head GEMM of the compacted rows belongs to it (it needs nothing from the decoder stack) unless the
  // head takes the dot in that GEMM's epilogue (fuse_head)
  int join(int s) {
    if (ptab && !adaptor_idle(s) && !fuse_head(s))
      GDR_TRY(side.linear(g.xa, d, head_w(s), d, g.A, (int64_t)V1 * d, rows_at(s), g.bb.n_miss, V1 * d, d, GDR_EPI_NONE, nullptr, nullptr, 0));
    if (lease.ss && !plain) GDR_TRY(stream_after(stream, lease.ss->join, as, "generate: adaptor stream join failed"));
    return GDR_OK;
  }

  // ---------------- head: last position, unmasked columns only (modeling_t5.py:1634-1646)
  int head(int s) {
    const BeamBufs& bb = g.bb;
    const int rows_s = rows_at(s);
    float *xa = g.xa, *A = g.A, *hl = g.hl;
    const float* he = w->head_e + (size_t)s * V1 * d;
    const float scale = 1.0f / sqrtf((float)d);
    const int64_t items = (int64_t)rows_s * V1;
    if (plain)  // lm_head(sequence_output) alone (modeling_t5.py:1640-1641): one launch, fp32 in both modes
      return launch_head_plain(hl, he, rows_s, V1, d, bb.logits, bb.live_gate, stream);
    if (!ptab) {
      GDR_TRY(main.linear(xa, d, head_w(s), d, A, (int64_t)V1 * d, rows_s, nullptr, V1 * d, d, GDR_EPI_NONE, nullptr, nullptr, 0));
      hipLaunchKernelGGL(head_logits_kernel, dim3((unsigned)((items + 3) / 4)), dim3(256), 0, stream, hl, A, he, rows_s, V1, d, scale,
                         bb.logits, bb.live_gate);
      GDR_CHECK_LAUNCH("head_logits_kernel");
      return GDR_OK;
    }
    const float* partial = nullptr;
    if (fuse_head(s)) {
      const void* a16 = (img2.buf && img2.src == xa) ? img2.buf : nullptr;  // the last adaptor norm's bf16 image of xa
      if (!a16) {
        GDR_TRY(launch_cast_f32_bf16(xa, g.abf2, (int64_t)rows_s * d, stream));
        a16 = g.abf2;
      }
      const int rc_ = launch_linear_bf16_headdot(a16, d, head_w(s), d, rows_s, bb.n_miss, V1 * d, d, hl, d, bb.miss_rows, he, d, scale, A, stream);
      if (rc_ < 0) return rc_;
      if (rc_ == 0) {
        partial = A;
      } else {  // shape not served: the plain form, now behind the join — the side chain's scratch, the caller's stream
        DecChain joined = side;
        joined.st = stream;
        GDR_TRY(joined.linear(xa, d, head_w(s), d, A, (int64_t)V1 * d, rows_s, bb.n_miss, V1 * d, d, GDR_EPI_NONE, nullptr, nullptr, 0));
      }
    }
    hipLaunchKernelGGL(head_logits_table_kernel, dim3((unsigned)((items + 3) / 4)), dim3(256), 0, stream, hl, A, he, ptab->W, bb.node[cur],
                       bb.miss_index, ptab->n_table, rows_s, V1, d, scale, bb.logits, bb.live_gate, partial);
    GDR_CHECK_LAUNCH("head_logits_table_kernel");
    return GDR_OK;
  }

  // the step's select and bookkeeping (beam.hip); the seq / node buffers flip
  int select(int s) {
    const int c = cur;
    cur ^= 1;
    return greedy ? greedy_step(g.bb, bd, s, c, out_ids, out_len, stream)
                  : beam_step(g.bb, bd, s, c, step_scores, step_tokens, stream, one_row_per_query(s));
  }
  int end() const {  // greedy_step_kernel wrote out_ids / out_len as it went
    return greedy ? GDR_OK : beam_end(g.bb, bd, max_length, cur, out_ids, out_len, out_scores, stream);
  }

  // ---------------- score mode: the step loop over GIVEN rows.  The pieces above as they are, with the identity ancestor table and the
  // rows' own tokens that forced_step_kernel leaves where the select would; all max_length positions run (one more than a search:
  // the hidden state of the last one is wanted, the caches hold max_length positions), and the last has no head — head_e ends at
  // max_out_len - 1 slices and nothing follows that position.  No early exit, no epoch, no hypothesis heap.
  int score_given_rows() {
    for (int s = 0; s < max_length; ++s) {
      const bool headed = s + 1 < max_length;
      GDR_TRY(embed_and_fork(s, headed));
      for (int l = 0; l < w->dims.num_layers || (headed && l < w->adaptor_layers); ++l) {
        if (l < w->dims.num_layers) GDR_TRY(dec_layer(l, s));
        if (headed && l < w->adaptor_layers) GDR_TRY(ad_layer(l, s));
      }
      if (headed) {
        GDR_TRY(join(s));
        GDR_TRY(head(s));
      }
      GDR_TRY(forced_step(g.bb, bd, s, out_ids, g.hl, d, step_scores, stream));
    }
    return forced_end(g.bb, bd, out_ids, d, step_scores, out_scores, stream);
  }
};

}  // namespace gdr

extern "C" size_t gdr_t5_generate_workspace_bytes(const GdrT5DecoderWeights* w, int B, int L, int num_beams,
                                                  int max_length) {
  if (!w || B <= 0 || L <= 0 || num_beams <= 0 || max_length < 2) return 0;
  (void)gdr::done_words();  // pinned host words of the early exit: allocated here, never inside a caller's stream capture
  gdr::BeamDims bd{B, num_beams, w->out_vocab, w->dims.vocab_size, max_length, num_beams, 1.0, nullptr, nullptr, 0};
  return gdr::gen_layout(*w, bd, L, nullptr, nullptr);
}

namespace gdr {
static int generate_impl(const GdrT5DecoderWeights* w, const float* enc_hidden, const int64_t* enc_mask, int B, int L,
                         int num_beams, int max_length, double length_penalty, int num_return_sequences,
                         const GdrTrie* trie, const GdrPrefixTable* ptab, int64_t* out_ids, int32_t* out_len,
                         double* out_scores, float* step_scores, int32_t* step_tokens, void* workspace,
                         size_t workspace_bytes, bool bf16, hipStream_t stream) {
  GenCall c{w,       enc_hidden,  enc_mask,    B,         L,    num_beams, max_length, ptab, out_ids, out_len, out_scores,
            step_scores, step_tokens, workspace, workspace_bytes, bf16, stream};
  GDR_TRY(c.validate(length_penalty, num_return_sequences, trie));
  GDR_TRY(c.lay_out());
  GDR_TRY(c.begin());
  GDR_TRY(c.cross_kv());
  if (c.forced) return c.score_given_rows();
  for (int s = 0; s + 1 < max_length; ++s) {  // position s, cur_len = s + 1 (generation_utils.py:676)
    if (c.all_done(s)) {
      g_early_exits.fetch_add(1);
      break;
    }
    GDR_TRY(c.embed_and_fork(s));
    // The two chains are enqueued layer by layer in turn: a host thread that first enqueued the whole adaptor chain left
    // the main stream idle for as long as those ~55 launches take to issue (measured: a fifth of a 100-beam step).
    for (int l = 0; l < w->dims.num_layers || l < w->adaptor_layers; ++l) {
      if (l < w->dims.num_layers) GDR_TRY(c.dec_layer(l, s));
      if (l < w->adaptor_layers && !c.adaptor_idle(s)) GDR_TRY(c.ad_layer(l, s));
    }
    GDR_TRY(c.join(s));
    GDR_TRY(c.head(s));
    GDR_TRY(c.select(s));
  }
  return c.end();
}
}  // namespace gdr

extern "C" int64_t gdr_t5_generate_early_exits(void) { return gdr::g_early_exits.load(); }

extern "C" int gdr_t5_generate_last_done_step(void) {
  int32_t* words = gdr::done_words();
  const int32_t e = gdr::g_done_epoch.load();
  if (!words || e == 0) return 0;
  return __atomic_load_n(words + (e & 63), __ATOMIC_ACQUIRE) == e ? __atomic_load_n(words + 64 + (e & 63), __ATOMIC_RELAXED) : 0;
}

extern "C" int gdr_t5_generate(const GdrT5DecoderWeights* w, const float* enc_hidden, const int64_t* enc_mask, int B,
                               int L, int num_beams, int max_length, double length_penalty,
                               int num_return_sequences, const GdrTrie* trie, const GdrPrefixTable* ptab,
                               int64_t* out_ids, int32_t* out_len, double* out_scores, float* step_scores,
                               int32_t* step_tokens, void* workspace, size_t workspace_bytes, void* stream_) {
  return gdr::generate_impl(w, enc_hidden, enc_mask, B, L, num_beams, max_length, length_penalty, num_return_sequences, trie,
                            ptab, out_ids, out_len, out_scores, step_scores, step_tokens, workspace, workspace_bytes, false,
                            static_cast<hipStream_t>(stream_));
}

extern "C" int gdr_t5_generate_bf16(const GdrT5DecoderWeights* w, const float* enc_hidden, const int64_t* enc_mask, int B,
                                    int L, int num_beams, int max_length, double length_penalty,
                                    int num_return_sequences, const GdrTrie* trie, const GdrPrefixTable* ptab,
                                    int64_t* out_ids, int32_t* out_len, double* out_scores, float* step_scores,
                                    int32_t* step_tokens, void* workspace, size_t workspace_bytes, void* stream_) {
  return gdr::generate_impl(w, enc_hidden, enc_mask, B, L, num_beams, max_length, length_penalty, num_return_sequences, trie,
                            ptab, out_ids, out_len, out_scores, step_scores, step_tokens, workspace, workspace_bytes, true,
                            static_cast<hipStream_t>(stream_));
}

// ------------------------------------------------------------------------------------------------ prefix table build
// Level by level over the trie (nodes in breadth-first order, so a level is a contiguous row range and the GEMMs write
// straight into the table): the adaptor chain of every node of depth s attends over the node's ancestors, whose (q,k,v)
// rows of every layer are already in the table; the head GEMM with the level's slice of adaptor_linear and lm_head as
// bias gives W[node] = A + E.  Same arithmetic as the in-call chain of gdr_t5_generate, at corpus scale.
namespace gdr {
struct TabBufs {
  float *xa, *tmp, *ctx, *ff, *skw;
  void* abf;
};
static size_t tab_layout(const GdrT5DecoderWeights& w, int max_level_nodes, char* base, TabBufs* t) {
  const size_t n = (size_t)max_level_nodes, d = w.dims.d_model;
  size_t o = 0;
  CARVE(t, xa, 4 * n * d);
  CARVE(t, tmp, 4 * n * d);
  CARVE(t, ctx, 4 * n * d);
  CARVE(t, ff, 4 * n * (size_t)w.adaptor_ff);
  CARVE(t, skw, SPLITK_WS_BYTES);
  CARVE(t, abf, 2 * n * (size_t)(w.adaptor_ff > (int)d ? w.adaptor_ff : (int)d));
  return o;
}
#undef CARVE
}  // namespace gdr

extern "C" size_t gdr_t5_prefix_table_workspace_bytes(const GdrT5DecoderWeights* w, int max_level_nodes) {
  if (!w || max_level_nodes <= 0 || gdr::plain_head(*w)) return 0;  // plain head: there is no table to build
  return gdr::tab_layout(*w, max_level_nodes, nullptr, nullptr);
}

namespace gdr {
static int table_build_impl(const GdrT5DecoderWeights* w, int n_levels, const int32_t* level_off, const int64_t* node_tok,
                            const int32_t* node_anc, float* kv, float* W, void* workspace, size_t workspace_bytes, bool bf16,
                            hipStream_t stream) {
  GDR_CHECK_ARG(w, "prefix_table_build: null pointer");
  GDR_CHECK_ARG(!plain_head(*w), "prefix_table_build: plain-head weights (adaptor_layers=0) have no adaptor results to store");
  GDR_CHECK_ARG(w->adaptor_layers > 0 && w->alayers && w->head_w && w->head_e && w->adaptor_nhead > 0,
                "prefix_table_build: adaptor_layers / alayers / head_w / head_e do not describe an adaptor head");
  GDR_CHECK_ARG(level_off && node_tok && node_anc && kv && W && workspace, "prefix_table_build: null pointer");
  const GdrT5Dims& dm = w->dims;
  GDR_CHECK_ARG(n_levels >= 1 && n_levels <= w->max_out_len - 1 && n_levels <= MAXLEN_CAP,
                "prefix_table_build: n_levels=%d must be in [1, max_output_length - 1 = %d]", n_levels, w->max_out_len - 1);
  GDR_CHECK_ARG(level_off[0] == 0 && level_off[1] == 1, "prefix_table_build: level 0 must be the root alone");
  const int d = dm.d_model, V1 = w->out_vocab + 1, aH = w->adaptor_nhead, ahd = d / aH, aff = w->adaptor_ff;
  GDR_CHECK_ARG(d % 4 == 0 && d % aH == 0 && ahd % 4 == 0, "prefix_table_build: unsupported dims");
  int max_n = 0;
  for (int s = 0; s < n_levels; ++s) {
    GDR_CHECK_ARG(level_off[s + 1] > level_off[s], "prefix_table_build: empty level %d", s);
    max_n = level_off[s + 1] - level_off[s] > max_n ? level_off[s + 1] - level_off[s] : max_n;
  }
  const size_t need = tab_layout(*w, max_n, nullptr, nullptr);
  if (workspace_bytes < need) {
    set_error("prefix_table_build: workspace %zu < required %zu", workspace_bytes, need);
    return GDR_ENOSPC;
  }
  GDR_CHECK_ARG(((uintptr_t)workspace & 255) == 0, "prefix_table_build: workspace must be 256-byte aligned");
  TabBufs t;
  tab_layout(*w, max_n, static_cast<char*>(workspace), &t);
  float *xa = t.xa, *tmp = t.tmp, *ctx = t.ctx, *ff = t.ff;
  const int64_t n_table = level_off[n_levels];
  const size_t layer_stride = (size_t)n_table * 3 * d;
  const BucketLut lut = make_bucket_lut(dm.rel_buckets, dm.rel_max_distance);
  const DecChain chain{bf16, t.abf, t.skw, stream, nullptr, nullptr};
  size_t anc_off = 0;  // level s block of node_anc: [n_s][s + 1]
  for (int s = 0; s < n_levels; ++s) {
    const int lo = level_off[s], n = level_off[s + 1] - lo;
    GDR_TRY(launch_embed(w->dec_embed, node_tok + lo, n, d, dm.vocab_size, xa, stream));
    for (int l = 0; l < w->adaptor_layers; ++l) {
      const GdrAdaptorLayer& al = w->alayers[l];
      float* tab = kv + l * layer_stride;       // [n_table][3d] of this layer
      float* slot = tab + (size_t)lo * 3 * d;   // this level's rows
      GDR_TRY(chain.linear(xa, d, al.in_w, d, slot, 3 * d, n, nullptr, 3 * d, d, GDR_EPI_BIAS, al.in_b, nullptr, 0));
      AttnArgs at = ancestor_attn(slot, tab, d, aH, n, s + 1, node_anc + anc_off, 1.0f / sqrtf((float)ahd), nullptr, 0, lut, 1);
      at.out = ctx;
      GDR_TRY(launch_attention(at, stream));
      GDR_TRY(chain.linear(ctx, d, al.out_w, d, tmp, d, n, nullptr, d, d, GDR_EPI_BIAS_RESIDUAL, al.out_b, xa, d));
      GDR_TRY(launch_layernorm(tmp, al.ln1_w, al.ln1_b, xa, n, d, w->adaptor_eps, nullptr, stream));
      GDR_TRY(launch_layernorm(xa, al.ln2_w, al.ln2_b, tmp, n, d, w->adaptor_eps, al.cross_const, stream));
      GDR_TRY(chain.linear(tmp, d, al.lin1_w, d, ff, aff, n, nullptr, aff, d, GDR_EPI_BIAS_RELU, al.lin1_b, nullptr, 0));
      GDR_TRY(chain.linear(ff, aff, al.lin2_w, aff, xa, d, n, nullptr, d, aff, GDR_EPI_BIAS_RESIDUAL, al.lin2_b, tmp, d));
      GDR_TRY(launch_layernorm(xa, al.ln3_w, al.ln3_b, xa, n, d, w->adaptor_eps, nullptr, stream));
    }
    // W[node][c][i] = sum_k xa[node][k] * head_w[s][c][i][k] + head_e[s][c][i]      (modeling_t5.py:1634-1639)
    GDR_TRY(chain.linear(xa, d, w_at(w->head_w, (size_t)s * V1 * d * d, bf16), d, W + (size_t)lo * V1 * d, (int64_t)V1 * d, n, nullptr, V1 * d,
                       d, GDR_EPI_BIAS, w->head_e + (size_t)s * V1 * d, nullptr, 0));
    anc_off += (size_t)n * (s + 1);
  }
  return GDR_OK;
}
}  // namespace gdr

extern "C" int gdr_t5_prefix_table_build(const GdrT5DecoderWeights* w, int n_levels, const int32_t* level_off,
                                         const int64_t* node_tok, const int32_t* node_anc, float* kv, float* W,
                                         void* workspace, size_t workspace_bytes, void* stream_) {
  return gdr::table_build_impl(w, n_levels, level_off, node_tok, node_anc, kv, W, workspace, workspace_bytes, false,
                               static_cast<hipStream_t>(stream_));
}

extern "C" int gdr_t5_prefix_table_build_bf16(const GdrT5DecoderWeights* w, int n_levels, const int32_t* level_off,
                                              const int64_t* node_tok, const int32_t* node_anc, float* kv, float* W,
                                              void* workspace, size_t workspace_bytes, void* stream_) {
  return gdr::table_build_impl(w, n_levels, level_off, node_tok, node_anc, kv, W, workspace, workspace_bytes, true,
                               static_cast<hipStream_t>(stream_));
}
