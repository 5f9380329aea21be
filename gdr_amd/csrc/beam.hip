// Docid beam search and greedy decode on gfx950 — the device-resident bookkeeping of the reference's generate() loops
// (GDR_model/transformers/generation_utils.py:629-921 + BeamHypotheses :1052-1099; num_beams = 1: _generate_no_beam_search :553-627).
// Nothing here knows a model: a step finds its unmasked-column logits in BeamBufs::logits (decode.hip's model step, or
// table_logits_kernel for gdr_beam_search_table) and leaves the next step's input tokens in cur_tok and, for the model's K/V caches,
// the ancestor rows in kv_rows.
//   * beam bookkeeping (top-2R, EOS handling, BeamHypotheses.add/is_done, finalisation) runs in three small
//     kernels per step with no host round trip; the reference syncs per candidate through .item().
//   * beams reach their ancestors' cache rows through an int32 table (`kv_rows`) that the beam-update kernel rewrites each step —
//     no cache reordering copies.
#include <math.h>

#include "beam.h"
#include "select.h"

namespace gdr {

// ---- the top-2R select of a step: one LDS sort per query while its R*(V+1) candidates fit SEL_SORT_MAX keys, above that (or
// with GDR_DECODE_BEAM_CHUNKED=1, an exact A/B knob nothing in the product sets) chunks of SEL_CHUNK candidate positions are
// sorted on their own and their first 2R keys merged — the same list bit for bit (beam_chunk_kernel, select.h's merge rounds).
constexpr int BEAM_MAX_CAND = 1 << 17; // num_beams * (V+1): 1024 beams up to V = 127; flat indices stay far inside 32 bits
constexpr int BEAM_LDS_LIMIT = 160 * 1024;  // LDS of a CU = the most one workgroup may hold (static + dynamic)
static_assert(2 * GDR_MAX_BEAMS <= SEL_MAX_KEEP, "select.h's merge rounds are sized for lists of up to SEL_MAX_KEEP keys");

static bool beam_chunked_forced() {
  static const bool on = env_flag("GDR_DECODE_BEAM_CHUNKED", false);
  return on;
}
static bool beam_chunked(int R, int V) { return beam_chunked_forced() || (int64_t)R * (V + 1) > SEL_SORT_MAX; }
static int beam_chunks(int R, int V) { return (int)(((int64_t)R * (V + 1) + SEL_CHUNK - 1) / SEL_CHUNK); }

size_t beam_layout(const BeamDims& bd, char* base, BeamBufs* bb) {
  const size_t rows = (size_t)bd.B * bd.R, ml = bd.maxlen, V1 = bd.V + 1;
  size_t o = 0;
#define CARVE(field, type, count)                                       \
  do {                                                                  \
    const size_t at__ = carve(o, sizeof(type) * (count));               \
    if (bb) bb->field = reinterpret_cast<type*>(base + at__);           \
  } while (0)
  CARVE(seq[0], int32_t, rows * ml);
  CARVE(seq[1], int32_t, rows * ml);
  CARVE(beam_scores, float, rows);
  CARVE(cur_tok, int64_t, rows);
  CARVE(parent, int32_t, rows);
  CARVE(anc[0], int32_t, rows * ml);
  CARVE(anc[1], int32_t, rows * ml);
  CARVE(kv_rows, int32_t, rows * ml);
  CARVE(node[0], int32_t, rows);
  CARVE(node[1], int32_t, rows);
  CARVE(miss_rows, int32_t, rows);
  CARVE(miss_index, int32_t, rows);
  CARVE(kv_rows_c, int32_t, rows * ml);
  CARVE(n_miss, int64_t, 1);
  CARVE(logits, float, rows * V1);
  CARVE(cand_score, float, (size_t)bd.B * 2 * bd.R);
  CARVE(cand_idx, int32_t, (size_t)bd.B * 2 * bd.R);
  CARVE(hyp_score, double, (size_t)bd.B * (bd.R + 1));
  CARVE(hyp_len, int32_t, (size_t)bd.B * (bd.R + 1));
  CARVE(hyp_tok, int32_t, (size_t)bd.B * (bd.R + 1) * ml);
  CARVE(hyp_seq, int32_t, (size_t)bd.B * (bd.R + 1));
  CARVE(hyp_next, int32_t, bd.B);
  CARVE(hyp_cnt, int32_t, bd.B);
  CARVE(hyp_worst, double, bd.B);
  CARVE(done, int32_t, bd.B);
  CARVE(n_done, int32_t, 1);
  CARVE(live, int32_t, 1);
  // the chunked select's scratch: nothing (zero bytes, the offsets above unchanged) for a call that stays in the one-sort form
  const bool chunked = beam_chunked(bd.R, bd.V);
  // a merge workgroup sorts `fan` partial lists of 2R keys: >= 4 for every accepted R (the size functions take any R)
  const size_t lists = chunked ? (size_t)beam_chunks(bd.R, bd.V) : 0, fan = sel_merge_fan(2 * bd.R);
  CARVE(lse, float, chunked ? rows * 2 : 0);
  CARVE(part[0], unsigned long long, (size_t)bd.B * lists * 2 * bd.R);
  CARVE(part[1], unsigned long long, (size_t)bd.B * ((lists + fan - 1) / fan) * 2 * bd.R);
#undef CARVE
  return o;
}

// ------------------------------------------------------------------------------------------ kernels
__global__ void beam_init_kernel(BeamBufs bb, BeamDims bd, int dedup0) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  const int rows = bd.B * bd.R;
  if (r < rows) {
    bb.seq[0][(size_t)r * bd.maxlen] = START_ID;
    bb.beam_scores[r] = (r % bd.R == 0) ? 0.f : -1e9f;  // generation_utils.py:663-668
    bb.cur_tok[r] = START_ID;
    bb.parent[r] = r;
    // dedup0: step 0 computes ONE row per query (identical beam rows), filed as row b of the position-0 cache slots
    bb.anc[0][(size_t)r * bd.maxlen] = dedup0 ? r / bd.R : r;
    bb.kv_rows[r] = r;  // step 0: stride 1, position 0 (dedup0: the first B entries serve the B computed rows)
    bb.node[0][r] = 0;  // trie root
  }
  if (r < bd.B) {
    bb.hyp_cnt[r] = 0;
    bb.hyp_next[r] = 0;
    bb.hyp_worst[r] = 1e9;  // :1062
    bb.done[r] = 0;
  }
  if (r == 0) *bb.n_done = 0, *bb.live = 1;
}

// Teacher forcing: logits[r][c] = table[b][pos][last_token][token(pos,c)]
__global__ void table_logits_kernel(const float* __restrict__ table, const int64_t* __restrict__ cur_tok, int rows,
                                    int R, int V, int Vd, int maxlen, int pos, float* __restrict__ logits) {
  const int item = blockIdx.x * blockDim.x + threadIdx.x;
  const int V1 = V + 1;
  if (item >= rows * V1) return;
  const int r = item / V1, c = item % V1, b = r / R;
  const int tok = c < V ? pos * V + 2 + c : EOS_ID;
  logits[item] = table[(((size_t)b * maxlen + pos) * Vd + (size_t)cur_tok[r]) * Vd + tok];
}

// The first `keep` = 2R of a query's sorted keys -> cand_score / cand_idx [B][2R] and, when wanted, the step's trace.  What the one-sort
// select and the last merge round of the chunked one (select.h sel_merge_kernel; its lane is the query) both end with.
struct BeamEmit {
  const int32_t* live_gate;
  float* cand_score;
  int32_t* cand_idx;
  float* step_scores;
  int32_t* step_tokens;
  __device__ bool skip() const { return live_gate && *live_gate == 0; }  // every query is done, nothing is ranked any more
  __device__ void operator()(int b, const unsigned long long* keys, int /*npad*/, int keep) const {
    const int nthr = blockDim.x;
    for (int i = threadIdx.x; i < keep; i += nthr) {
      const float s = sel_score(keys[i]);
      const int32_t flat = (int32_t)sel_low(keys[i]);
      cand_score[(size_t)b * keep + i] = s;
      cand_idx[(size_t)b * keep + i] = flat;
      if (step_scores) {
        step_scores[(size_t)b * keep + i] = s;
        step_tokens[(size_t)b * keep + i] = flat;
      }
    }
  }
};

// Per query: log_softmax of every beam's row (masked columns contribute exp(-1e9 - max) = 0 exactly), add the
// beam score, take the 2R best of the R*(V+1) unmasked candidates, sorted (generation_utils.py:698,766-775).
__global__ __launch_bounds__(1024) void beam_topk_kernel(BeamBufs bb, BeamDims bd, int pos, int npad, int cur, int bcast,
                                                        float* __restrict__ step_scores,
                                                        int32_t* __restrict__ step_tokens) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long keys[];  // [npad]
  if (bb.live_gate && *bb.live_gate == 0) return;  // uniform: every query is done, nothing is ranked any more
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int R = bd.R, V1 = bd.V + 1, nthr = blockDim.x, nwaves = blockDim.x >> 6;
  float* lse_max = reinterpret_cast<float*>(keys + npad);  // [R]
  float* lse_log = lse_max + R;                            // [R]
  float* lg_s = lse_log + R;                               // [R*V1] this query's logits, staged once (coalesced)
  const int ncand = R * V1;
  // bcast (step 0 with one computed row per query): logits holds [B][V1], every beam of the query reads row b
  for (int e = tid; e < ncand; e += nthr) lg_s[e] = bcast ? bb.logits[(size_t)b * V1 + e % V1] : bb.logits[(size_t)b * ncand + e];
  __syncthreads();
  for (int j = wave; j < R; j += nwaves) {
    const float* lg = lg_s + j * V1;
    float mx = -INFINITY;
    for (int c = lane; c < V1; c += 64) mx = fmaxf(mx, lg[c]);
    mx = wave_max(mx);
    float sm = 0.f;
    for (int c = lane; c < V1; c += 64) sm += expf(lg[c] - mx);
    sm = wave_sum(sm);
    if (lane == 0) {
      lse_max[j] = mx;
      lse_log[j] = logf(sm);
    }
  }
  __syncthreads();
  for (int e = tid; e < npad; e += nthr) {
    unsigned long long key = 0ull;
    if (e < ncand) {
      const int j = e / V1, c = e - j * V1;
      const float logp = (lg_s[e] - lse_max[j]) - lse_log[j];
      float s = logp + bb.beam_scores[(size_t)b * R + j];
      if (bd.trie_eos) {  // scores += mask(-inf on tokens that are not children of the prefix' node)
        const int nd = bb.node[cur][(size_t)b * R + j];
        const bool ok = c < bd.V ? (nd >= 0 && bd.trie_child[(size_t)nd * bd.V + c] >= 0) : (nd < 0 || bd.trie_eos[nd] != 0);
        if (!ok) s = -INFINITY;
      }
      const int tok = c < bd.V ? pos * bd.V + 2 + c : EOS_ID;
      const uint32_t flat = (uint32_t)(j * bd.Vd + tok);
      key = sel_pack(s, flat);
    }
    keys[e] = key;
  }
  __syncthreads();
  // Bitonic sort, descending.  A wave owns a block of epw consecutive keys: every stage whose compare-exchange pairs stay
  // inside a block (2*stride <= epw) needs no workgroup barrier — LDS operations of one wave execute in order — so of the
  // 78 stages of a 4096-key sort (100 beams) only the 10 with stride >= 256 cost a barrier pair.  The kernel takes 49 us
  // per step at 100 beams (rocprofv3); keeping the keys in registers (4 per lane: in-thread swaps, 64-bit shuffles inside a
  // wave, LDS only across waves) was built and measured no faster (54 us) — 8 ds_bpermute per shuffle stage cost what the
  // LDS round trip of a stage costs.
  const int epw = npad / nwaves;
  if (epw >= 2 * R && nwaves > 1) {
    // Only the 2R best of the npad keys are wanted and a wave's block holds at least that many: every wave sorts its own
    // block (descending, no workgroup barrier), then blocks are merged pairwise keeping the better half — for A and B
    // sorted descending, max(A[i], B[epw-1-i]) is a bitonic sequence holding the epw largest of both, which log2(epw)
    // wave-local stages sort — until block 0 holds the top epw of all.  log2(nwaves) + 1 workgroup barriers where the full
    // network below takes a barrier pair on each of its 10 wide stages: 49 -> (measured) us per step at 100 beams.
    unsigned long long* blk = keys + wave * epw;
    for (int size = 2; size <= epw; size <<= 1) {
      for (int stride = size >> 1; stride > 0; stride >>= 1) {
        for (int q = lane; q < (epw >> 1); q += 64) sel_cmpx(blk, q, stride, size);
        wave_sync();
      }
    }
    for (int nb = nwaves; nb > 1; nb >>= 1) {
      __syncthreads();
      if (wave < (nb >> 1)) {
        const unsigned long long* other = keys + (wave + (nb >> 1)) * epw;
        for (int q = lane; q < epw; q += 64) {
          const unsigned long long x = blk[q], y = other[epw - 1 - q];
          blk[q] = x > y ? x : y;
        }
        wave_sync();
        for (int stride = epw >> 1; stride > 0; stride >>= 1) {
          for (int q = lane; q < (epw >> 1); q += 64) sel_cmpx(blk, q, stride, 0);
          wave_sync();
        }
      }
    }
  } else {
    bitonic_stages(keys, npad, nthr);
  }
  __syncthreads();
  BeamEmit{nullptr, bb.cand_score, bb.cand_idx, step_scores, step_tokens}(b, keys, npad, 2 * R);  // the gate was taken above: only the write-out
}

// ---- the chunked select (R*(V+1) > SEL_SORT_MAX candidates per query, or forced) ---------------------------------------------
// Three kinds of launches leave in cand_score / cand_idx (and the trace) what beam_topk_kernel leaves, bit for bit:
//   beam_norm_kernel   every beam row's max and log-sum-exp — a wave per row with beam_topk_kernel's lane assignment and order, so
//                      the log-probabilities get the same bits;
//   beam_chunk_kernel  a workgroup per (chunk of SEL_CHUNK candidate positions, query) builds beam_topk_kernel's keys for its
//                      positions (key 0 past the query's last candidate), sorts them and files its first 2R;
//   sel_merge_kernel   (select.h) a workgroup per (group of lists, query) sorts the group's keys and files the first 2R; the round
//                      that is left with one list per query writes the result instead (BeamEmit).
// The keys are distinct (the flat index is the low word), so their order is total: the first 2R of the whole list are the first 2R
// of the chunks' first 2R, whatever the grouping.  No atomics, nothing depends on the order workgroups run in.

__global__ __launch_bounds__(256) void beam_norm_kernel(BeamBufs bb, BeamDims bd, int bcast) {
  if (bb.live_gate && *bb.live_gate == 0) return;
  const int b = blockIdx.x, lane = threadIdx.x & 63, V1 = bd.V + 1;
  const int j = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (j >= bd.R) return;
  const float* lg = bb.logits + (bcast ? (size_t)b * V1 : ((size_t)b * bd.R + j) * V1);
  float mx = -INFINITY;
  for (int c = lane; c < V1; c += 64) mx = fmaxf(mx, lg[c]);
  mx = wave_max(mx);
  float sm = 0.f;
  for (int c = lane; c < V1; c += 64) sm += expf(lg[c] - mx);
  sm = wave_sum(sm);
  if (lane == 0) {
    bb.lse[((size_t)b * bd.R + j) * 2] = mx;
    bb.lse[((size_t)b * bd.R + j) * 2 + 1] = logf(sm);
  }
}

__global__ __launch_bounds__(1024) void beam_chunk_kernel(BeamBufs bb, BeamDims bd, int pos, int cur, int bcast, int nchunks) {
  __shared__ __attribute__((aligned(16))) unsigned long long keys[SEL_CHUNK];
  if (bb.live_gate && *bb.live_gate == 0) return;
  const int b = blockIdx.x, ch = blockIdx.y, tid = threadIdx.x;
  const int R = bd.R, V1 = bd.V + 1, ncand = R * V1, keep = 2 * R;
  for (int i = tid; i < SEL_CHUNK; i += 1024) {
    const int e = ch * SEL_CHUNK + i;
    unsigned long long key = 0ull;
    if (e < ncand) {
      const int j = e / V1, c = e - j * V1;
      const float lgt = bcast ? bb.logits[(size_t)b * V1 + c] : bb.logits[(size_t)b * ncand + e];
      const float* nrm = bb.lse + ((size_t)b * R + j) * 2;
      const float logp = (lgt - nrm[0]) - nrm[1];
      float s = logp + bb.beam_scores[(size_t)b * R + j];
      if (bd.trie_eos) {
        const int nd = bb.node[cur][(size_t)b * R + j];
        const bool ok = c < bd.V ? (nd >= 0 && bd.trie_child[(size_t)nd * bd.V + c] >= 0) : (nd < 0 || bd.trie_eos[nd] != 0);
        if (!ok) s = -INFINITY;
      }
      const int tok = c < bd.V ? pos * bd.V + 2 + c : EOS_ID;
      const uint32_t flat = (uint32_t)(j * bd.Vd + tok);
      key = sel_pack(s, flat);
    }
    keys[i] = key;
  }
  __syncthreads();
  bitonic_desc(keys, SEL_CHUNK, 1024);
  unsigned long long* dst = bb.part[0] + ((size_t)b * nchunks + ch) * keep;
  for (int i = tid; i < keep; i += 1024) dst[i] = keys[i];
}

// ---- BeamHypotheses of one query, held in LDS by the single wave that serves the query -------------------------------
// The reference keeps `self.beams` as a Python list (generation_utils.py:1052-1099): add() appends, an over-full list
// drops its worst entry with `del` (order of the rest kept), the final pick is a stable sort by score popped from the
// end.  Only the RELATIVE list order of surviving entries is ever observed (tie-breaks), so each entry carries its
// insertion number and the storage order is free: a delete moves the last entry into the hole.
// The hypothesis-heap helpers below are executed by ONE wave (the first wave of the block): LDS operations of a wave
// execute in order, so a wave-level barrier (plus fences for the compiler) is all the synchronisation they need.
struct HypLds {
  double* sc;   // [R+1]
  int32_t* ln;  // [R+1]
  int32_t* sq;  // [R+1]
  int32_t* tk;  // [R+1][ml]
  int n, next;
  double worst;
};
__host__ __device__ static size_t hyp_lds_bytes(int R, int ml) { return (size_t)(R + 1) * (8 + 4 + 4 + 4 * (size_t)ml) + 8; }

__device__ __forceinline__ void hyp_load(HypLds& H, char* smem, const BeamBufs& bb, const BeamDims& bd, int b, int lane) {
  const int cap = bd.R + 1, ml = bd.maxlen;
  H.sc = reinterpret_cast<double*>(smem);
  H.ln = reinterpret_cast<int32_t*>(H.sc + cap);
  H.sq = H.ln + cap;
  H.tk = H.sq + cap;
  H.n = bb.hyp_cnt[b], H.next = bb.hyp_next[b], H.worst = bb.hyp_worst[b];
  for (int i = lane; i < H.n; i += 64) {
    H.sc[i] = bb.hyp_score[(size_t)b * cap + i];
    H.ln[i] = bb.hyp_len[(size_t)b * cap + i];
    H.sq[i] = bb.hyp_seq[(size_t)b * cap + i];
  }
  for (int e = lane; e < H.n * ml; e += 64) H.tk[e] = bb.hyp_tok[(size_t)b * cap * ml + e];
  wave_sync();
}

// the same view of the LDS arrays for waves that do not take part in the load (beam_finalize_kernel)
__device__ __forceinline__ void hyp_load_ptrs(HypLds& H, char* smem, const BeamBufs& bb, const BeamDims& bd, int b) {
  const int cap = bd.R + 1;
  H.sc = reinterpret_cast<double*>(smem);
  H.ln = reinterpret_cast<int32_t*>(H.sc + cap);
  H.sq = H.ln + cap;
  H.tk = H.sq + cap;
  H.n = bb.hyp_cnt[b], H.next = bb.hyp_next[b], H.worst = bb.hyp_worst[b];
}

__device__ __forceinline__ void hyp_store(const HypLds& H, const BeamBufs& bb, const BeamDims& bd, int b, int lane) {
  const int cap = bd.R + 1, ml = bd.maxlen;
  wave_sync();
  for (int i = lane; i < H.n; i += 64) {
    bb.hyp_score[(size_t)b * cap + i] = H.sc[i];
    bb.hyp_len[(size_t)b * cap + i] = H.ln[i];
    bb.hyp_seq[(size_t)b * cap + i] = H.sq[i];
  }
  for (int e = lane; e < H.n * ml; e += 64) bb.hyp_tok[(size_t)b * cap * ml + e] = H.tk[e];
  if (lane == 0) bb.hyp_cnt[b] = H.n, bb.hyp_next[b] = H.next, bb.hyp_worst[b] = H.worst;
}

// BeamHypotheses.add (generation_utils.py:1070-1084); Python-float arithmetic = double.  Called by all 64 lanes of the
// query's wave with uniform arguments.
// `len_pow` = pow(len, length_penalty), computed once by the caller (every add of one launch has the same length).
__device__ __forceinline__ void hyp_add(HypLds& H, const BeamDims& bd, const int32_t* toks, int len, double sum_logp, int lane, double len_pow) {
  const int ml = bd.maxlen;
  const double score = sum_logp / len_pow;
  if (!(H.n < bd.R || score > H.worst)) return;
  if (lane == 0) H.sc[H.n] = score, H.ln[H.n] = len, H.sq[H.n] = H.next;
  for (int t = lane; t < len; t += 64) H.tk[(size_t)H.n * ml + t] = toks[t];
  ++H.n, ++H.next;
  wave_sync();
  if (H.n > bd.R) {
    // sorted([(s, idx)])[0] is removed (lowest score, then lowest list index = lowest insertion number);
    // [1] gives the new worst score
    double bs = INFINITY;
    int bq = 0x7fffffff, bi = -1;
    for (int i = lane; i < H.n; i += 64) {
      const double v = H.sc[i];
      const int q = H.sq[i];
      if (v < bs || (v == bs && q < bq)) bs = v, bq = q, bi = i;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const double os = __shfl_xor(bs, off);
      const int oq = __shfl_xor(bq, off), oi = __shfl_xor(bi, off);
      if (os < bs || (os == bs && oq < bq)) bs = os, bq = oq, bi = oi;
    }
    const int lo = bi;
    double second = INFINITY;
    for (int i = lane; i < H.n; i += 64)
      if (i != lo && H.sc[i] < second) second = H.sc[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) second = fmin(second, __shfl_xor(second, off));
    const int last = H.n - 1;
    if (lo != last) {
      if (lane == 0) H.sc[lo] = H.sc[last], H.ln[lo] = H.ln[last], H.sq[lo] = H.sq[last];
      for (int t = lane; t < ml; t += 64) H.tk[(size_t)lo * ml + t] = H.tk[(size_t)last * ml + t];
    }
    --H.n;
    H.worst = second;
    wave_sync();
  } else {
    H.worst = score < H.worst ? score : H.worst;
  }
}

// The ancestor table of a query's R rows for the position about to be processed (pos = cur_len: the new rows have length
// cur_len + 1): position p < pos is inherited from the row's parent, position pos is the row itself.  Runs at the end of
// beam_update_kernel (the parents were written by this workgroup: visible after its barrier) — a launch of its own in round 2.
__device__ __forceinline__ void anc_update_query(const BeamBufs& bb, const BeamDims& bd, int b, int pos, int cur, int tid) {
  __syncthreads();
  const int R = bd.R, ml = bd.maxlen, stride = pos + 1, rows = bd.B * R;
  for (int e = tid; e < R * stride; e += 256) {
    const int j = e / stride, p = e - j * stride, r = b * R + j;
    const int a = p < pos ? bb.anc[cur][(size_t)bb.parent[r] * ml + p] : r;
    bb.anc[cur ^ 1][(size_t)r * ml + p] = a;
    bb.kv_rows[(size_t)r * stride + p] = p * rows + a;
  }
}

// The host loop of generation_utils.py:783-850, one workgroup of four waves per query.  What that loop decides is fixed
// by the ranked candidate list alone: the next beams are the first R non-EOS candidates, and the EOS candidates that are
// offered to the hypothesis heap are those of rank < R that come before the R-th non-EOS one — so the non-EOS ranks are
// found with ballots / popcounts, and only the (few) EOS candidates walk the heap one after another, in rank order, on the
// first wave.  All four waves then fill the rows.  cur = index of the current seq buffer.
__global__ __launch_bounds__(256) void beam_update_kernel(BeamBufs bb, BeamDims bd, int cur_len, int cur) {
  extern __shared__ __attribute__((aligned(16))) char bsm[];
  __shared__ int n_sh;
  // every query was done BEFORE this step (the word is only cleared by a previous launch of this kernel): the step would pad
  // every entry (:786-794) and nothing reads the padding — beam_finalize takes done queries from their hypothesis heaps
  if (bb.live_gate && *bb.live_gate == 0) return;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int R = bd.R, ml = bd.maxlen;
  const int32_t* seq_c = bb.seq[cur];
  int32_t* seq_n = bb.seq[cur ^ 1];
  if (bb.done[b]) {  // :786-794 padded batch entry
    for (int j = tid; j < R; j += 256) {
      const int row = b * R + j;
      bb.beam_scores[row] = 0.f;
      bb.cur_tok[row] = PAD_ID;
      bb.parent[row] = b * R;
      bb.node[cur ^ 1][row] = -1;
    }
    for (int e = tid; e < R * (cur_len + 1); e += 256) {
      const int j = e / (cur_len + 1), t = e - j * (cur_len + 1);
      seq_n[(size_t)(b * R + j) * ml + t] = t < cur_len ? seq_c[(size_t)(b * R) * ml + t] : PAD_ID;
    }
    anc_update_query(bb, bd, b, cur_len, cur, tid);
    return;
  }
  int32_t* sel = reinterpret_cast<int32_t*>(bsm + ((hyp_lds_bytes(R, ml) + 15) & ~(size_t)15));  // [R] chosen candidate ranks
  int32_t* ci = sel + R;                               // [2R] ranked candidates, staged once
  float* cs = reinterpret_cast<float*>(ci + 2 * R);    // [2R]
  for (int e = tid; e < 2 * R; e += 256) {
    ci[e] = bb.cand_idx[(size_t)b * 2 * R + e];
    cs[e] = bb.cand_score[(size_t)b * 2 * R + e];
  }
  __syncthreads();
  if (wave == 0) {
    HypLds H;
    hyp_load(H, bsm, bb, bd, b, lane);
    // pass 1: rank of the j-th non-EOS candidate -> sel[j]; `end` = one past the rank at which the R-th one is taken
    int n = 0, end = 2 * R;
    for (int base = 0; base < 2 * R && n < R; base += 64) {
      const int rank = base + lane;
      const bool live = rank < 2 * R && (ci[rank] % bd.Vd) != EOS_ID;
      const unsigned long long m = __ballot(live);
      const int before = n + __popcll(m & ((1ull << lane) - 1ull));
      if (live && before < R) sel[before] = rank;
      const int tot = n + __popcll(m);
      if (tot >= R) {  // the R-th non-EOS candidate sits in this chunk: find its rank
        const unsigned long long hit = __ballot(live && before == R - 1);
        end = base + (int)__ffsll((long long)hit);
      }
      n = tot < R ? tot : R;
    }
    // pass 2: EOS candidates of rank < min(R, end) enter the heap, in rank order (:811-817)
    bool touched = false;
    const double len_pow = pow((double)cur_len, bd.lp);
    const int lim = end < R ? end : R;
    for (int base = 0; base < lim; base += 64) {
      const int rank = base + lane;
      unsigned long long m = __ballot(rank < lim && (ci[rank] % bd.Vd) == EOS_ID);
      while (m) {
        const int rk = base + (int)__ffsll((long long)m) - 1;
        m &= m - 1;
        hyp_add(H, bd, seq_c + (size_t)(b * R + ci[rk] / bd.Vd) * ml, cur_len, (double)cs[rk], lane, len_pow);
        touched = true;
      }
    }
    if (touched) hyp_store(H, bb, bd, b, lane);
    // :827-829  is_done(best_sum_logprobs = next_scores[b].max(), cur_len)
    if (lane == 0) {
      n_sh = n;
      if (H.n >= R) {
        const double cur_score = (double)cs[0] / len_pow;
        if (H.worst >= cur_score) {
          bb.done[b] = 1;  // set once: a done query takes the early return at the top from now on
          // generation_utils.py:836-838 `if all(done): break` — the host polls this word between steps (generate_impl)
          if (atomicAdd(bb.n_done, 1) + 1 == bd.B) {
            *bb.live = 0;  // the steps already enqueued skip their linears (StreamK::live) and their miss-row chain
            if (bb.all_done_host) {
              __hip_atomic_store(bb.all_done_host + 64, cur_len, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);  // the step it happened at
              // release: a host that sees the epoch also sees the step word stored just above
              __hip_atomic_store(bb.all_done_host, bb.done_epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            }
          }
        }
      }
    }
  }
  __syncthreads();
  const int n = n_sh;
  for (int j = tid; j < n; j += 256) {
    const int rank = sel[j];
    const int flat = ci[rank];
    const int beam = flat / bd.Vd, tok = flat % bd.Vd;
    const int eff = b * R + beam, row = b * R + j;
    bb.beam_scores[row] = cs[rank];
    bb.cur_tok[row] = tok;
    bb.parent[row] = eff;
    if (bd.trie_child) {
      const int nd = bb.node[cur][eff], c = tok - ((cur_len - 1) * bd.V + 2);
      int nx = (nd >= 0 && c >= 0 && c < bd.V) ? bd.trie_child[(size_t)nd * bd.V + c] : -1;
      if (nx >= bd.trie_nodes) nx = -1;  // a malformed table must not send later lookups out of bounds
      bb.node[cur ^ 1][row] = nx;
    }
  }
  for (int e = tid; e < n * (cur_len + 1); e += 256) {
    const int j = e / (cur_len + 1), t = e - j * (cur_len + 1);
    const int flat = ci[sel[j]];
    const int beam = flat / bd.Vd, tok = flat % bd.Vd;
    seq_n[(size_t)(b * R + j) * ml + t] = t < cur_len ? seq_c[(size_t)(b * R + beam) * ml + t] : tok;
  }
  anc_update_query(bb, bd, b, cur_len, cur, tid);
}

// :862-919 finalise open beams, pick the nret best per query, lay out tokens / EOS / PAD.  One workgroup of four waves per query.
// The R open beams of a query that is not done enter its hypothesis heap one after another in the reference (:863-883).  What that
// sequence leaves behind is decided by the scores alone except inside ONE tie group: with v = the R-th largest score over the old
// entries and the R new ones, every entry above v survives (when it is offered the full heap holds something smaller, and nothing
// can evict it), nothing below v does (a full heap's minimum never decreases), and when the entries equal to v all fit they all
// survive — the heap ends with R entries and they are the only candidates left.  So the survivors are found by counting (R^2
// compares spread over 256 lanes instead of R dependent heap updates of one wave: 165 us at 100 beams); only when the tie group AT
// v is cut by the capacity — equal double-precision scores of different hypotheses — the admission / eviction order matters
// (strict `>` against the worst score, the oldest of the worst evicted) and the original one-by-one walk runs.  The insertion numbers
// only ever decide the relative order of equal scores: new entry j takes next + j (offer order).
__global__ __launch_bounds__(256) void beam_finalize_kernel(BeamBufs bb, BeamDims bd, int final_len, int cur, int max_length,
                                                            int64_t* out_ids, int32_t* out_len, double* out_scores) {
  extern __shared__ __attribute__((aligned(16))) char bsm[];
  __shared__ int n_fin, cut_tie, n_keep;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int R = bd.R, ml = bd.maxlen;
  HypLds H;
  if (wave == 0) hyp_load(H, bsm, bb, bd, b, lane);
  else hyp_load_ptrs(H, bsm, bb, bd, b);
  int32_t* order = reinterpret_cast<int32_t*>(bsm + ((hyp_lds_bytes(R, ml) + 15) & ~(size_t)15));  // [nret] entry of rank j
  int32_t* rows_s = order + bd.nret;                         // [R][ml] the open beams' rows
  float* sc_s = reinterpret_cast<float*>(rows_s + R * ml);   // [R]
  double* all_sc = reinterpret_cast<double*>((reinterpret_cast<uintptr_t>(sc_s + R) + 7) & ~(uintptr_t)7);  // [2R + 1] old entries' scores, then the new ones'
  int32_t* keep = reinterpret_cast<int32_t*>(all_sc + 2 * R + 1);  // [2R + 1] slot of a surviving entry, -1 otherwise
  if (tid == 0) n_fin = H.n, cut_tie = 0, n_keep = 0;
  __syncthreads();
  const bool open = !bb.done[b];  // uniform
  if (open) {
    // the rows are staged in LDS first: read one by one from device memory, every add paid a dependent round trip
    for (int e = tid; e < R * ml; e += 256) rows_s[e] = bb.seq[cur][(size_t)b * R * ml + e];
    for (int j = tid; j < R; j += 256) sc_s[j] = bb.beam_scores[b * R + j];
    __syncthreads();
    const double len_pow = pow((double)final_len, bd.lp);
    const int n0 = H.n, T = n0 + R;
    for (int i = tid; i < T; i += 256) all_sc[i] = i < n0 ? H.sc[i] : (double)sc_s[i - n0] / len_pow;
    __syncthreads();
    // survivors by counting; a cut tie group is flagged
    for (int i = tid; i < T; i += 256) {
      const double v = all_sc[i];
      int gt = 0, eq = 0;
      for (int j = 0; j < T; ++j) {
        const double w = all_sc[j];
        gt += w > v ? 1 : 0, eq += w == v ? 1 : 0;
      }
      const bool in = gt + eq <= R;               // the whole group of equal scores fits
      if (!in && gt < R && eq > 1) cut_tie = 1;   // the group at the boundary is cut and holds several entries (benign race: all store 1)
      // a cut group of ONE entry cannot exist (gt < R and eq == 1 means gt + eq <= R)
      keep[i] = in ? 1 : 0;
    }
    __syncthreads();
    if (cut_tie) {
      if (wave == 0) {  // the reference's walk, one add after another
        for (int j = 0; j < R; ++j) hyp_add(H, bd, rows_s + j * ml, final_len, (double)sc_s[j], lane, len_pow);
        if (lane == 0) n_fin = H.n;
      }
    } else {
      // compact the survivors into the heap arrays: old entries first (their relative storage order is free), then new ones;
      // old entries that do not survive leave holes that surviving NEW entries fill
      if (wave == 0) {
        // slots: survivors are numbered in index order by ballot prefix sums
        int base = 0;
        for (int i0 = 0; i0 < T; i0 += 64) {
          const int i = i0 + lane;
          const bool kp = i < T && keep[i] != 0;
          const unsigned long long m = __ballot(kp);
          if (i < T) keep[i] = kp ? base + __popcll(m & ((1ull << lane) - 1ull)) : -1;
          base += __popcll(m);
        }
        if (lane == 0) n_fin = base;
      }
      __syncthreads();
      // Move in two steps through registers-free staging: scores / lengths / insertion numbers / tokens of survivors are first
      // gathered into the tail region (rows_s is reused as scratch for tokens is not possible — it is the source), so the old entries
      // are moved in ascending slot order by one wave (slot <= index: a survivor never moves up), then new entries are written.
      if (wave == 0) {
        for (int i = 0; i < n0; ++i) {  // uniform loop; slot <= i, so the source of a later move is never overwritten earlier
          const int sl = keep[i];
          if (sl >= 0 && sl != i) {
            if (lane == 0) H.sc[sl] = H.sc[i], H.ln[sl] = H.ln[i], H.sq[sl] = H.sq[i];
            for (int t = lane; t < ml; t += 64) H.tk[(size_t)sl * ml + t] = H.tk[(size_t)i * ml + t];
            wave_sync();
          }
        }
      }
      __syncthreads();
      for (int j = wave; j < R; j += 4) {  // a wave per new entry
        const int sl = keep[n0 + j];
        if (sl < 0) continue;
        if (lane == 0) H.sc[sl] = all_sc[n0 + j], H.ln[sl] = final_len, H.sq[sl] = H.next + j;
        for (int t = lane; t < final_len; t += 64) H.tk[(size_t)sl * ml + t] = rows_s[j * ml + t];
      }
    }
  }
  __syncthreads();
  // sorted(beams, key=score) is stable ascending and pop() takes the last: highest score first, among equal scores the
  // later list entry first.  rank(i) = number of entries that precede i in that order.
  const int n = n_fin;
  for (int i = tid; i < n; i += 256) {
    const double v = H.sc[i];
    const int q = H.sq[i];
    int rank = 0;
    for (int j = 0; j < n; ++j) {
      const double w = H.sc[j];
      rank += (w > v || (w == v && H.sq[j] > q)) ? 1 : 0;
    }
    if (rank < bd.nret) order[rank] = i;
  }
  __syncthreads();
  for (int j = tid; j < bd.nret; j += 256) {
    const size_t o = (size_t)b * bd.nret + j;
    // fewer hypotheses than requested cannot happen when V^depth >= R (the reference would raise)
    out_len[o] = j < n ? H.ln[order[j]] : 0;
    out_scores[o] = j < n ? H.sc[order[j]] : -INFINITY;
  }
  for (int e = tid; e < bd.nret * max_length; e += 256) {
    const int j = e / max_length, t = e - j * max_length;
    int64_t v = PAD_ID;
    if (j < n) {
      const int best = order[j], len = H.ln[best];
      if (t < len) v = H.tk[(size_t)best * ml + t];
      else if (t == len) v = EOS_ID;  // :915-916 (len < max_length)
    }
    out_ids[((size_t)b * bd.nret + j) * max_length + t] = v;
  }
}

// ---- num_beams = 1: the reference's _generate_no_beam_search (generation_utils.py:553-627) --------------------------------------
// One row per query and no hypotheses: `unfinished` is !done[b], `sent_len` is out_len[b], and the tokens go straight into out_ids.
// greedy_init_kernel leaves out_ids = START, PAD, PAD, ... and out_len = max_length, so a finished row — and a step the early exit
// never runs — has nothing left to write: padding is what is already there.
__global__ void greedy_init_kernel(BeamBufs bb, BeamDims bd, int64_t* __restrict__ out_ids, int32_t* __restrict__ out_len,
                                   double* __restrict__ out_scores) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < bd.B) {
    bb.cur_tok[b] = START_ID;
    bb.kv_rows[b] = b;      // step 0: stride 1, position 0
    bb.node[0][b] = 0;      // trie root (prefix-table mode)
    bb.done[b] = 0;         // :553 unfinished_sents = 1
    out_len[b] = bd.maxlen; // :554 sent_lengths = max_length
    out_scores[b] = 0.0;    // the reference keeps no score
    for (int t = 0; t < bd.maxlen; ++t) out_ids[(size_t)b * bd.maxlen + t] = t == 0 ? START_ID : PAD_ID;
  }
  if (b == 0) *bb.n_done = 0, *bb.live = 1;
}

// One decode step's select and bookkeeping at num_beams = 1, a wave per query (:596-619).  next = argmax over the full decode
// vocabulary: the V+1 live columns are ranked here, every other column is exactly -1e9 after select_valid_embedding and loses to
// any logit a model produces.  torch.argmax takes the LOWEST token id among equal maxima; EOS (token 1) sits in the LAST live
// column, so lanes compare (logit, token id) pairs, never columns.  pos = the position just computed (cur_len = pos + 1 before the
// token is added); the cache row of position p of query b is p*B + b at every step, so the step only re-lays kv_rows for the next
// stride.
__global__ __launch_bounds__(256) void greedy_step_kernel(BeamBufs bb, BeamDims bd, int pos, int cur, int64_t* __restrict__ out_ids,
                                                          int32_t* __restrict__ out_len) {
  // every query finished at an earlier step: nothing reads what this step would write (see beam_update_kernel)
  if (bb.live_gate && *bb.live_gate == 0) return;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (b >= bd.B) return;
  const int V = bd.V, V1 = V + 1, stride = pos + 2;
  for (int p = lane; p < stride; p += 64) bb.kv_rows[(size_t)b * stride + p] = p * bd.B + b;
  if (bb.done[b]) {  // :601 a finished row adds PAD — already in out_ids — and feeds PAD to the next step
    if (lane == 0) {
      bb.cur_tok[b] = PAD_ID;
      bb.node[cur ^ 1][b] = -1;
    }
    return;
  }
  const float* lg = bb.logits + (size_t)b * V1;
  float best = -INFINITY;
  int btok = INT32_MAX;
  for (int c = lane; c < V1; c += 64) {
    const float v = lg[c];
    const int tok = c < V ? pos * V + 2 + c : EOS_ID;
    if (v > best || (v == best && tok < btok)) best = v, btok = tok;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {  // the pairs are totally ordered: after the butterfly every lane holds the same one
    const float ov = __shfl_xor(best, o);
    const int ot = __shfl_xor(btok, o);
    if (ov > best || (ov == best && ot < btok)) best = ov, btok = ot;
  }
  if (lane != 0) return;
  if (btok == INT32_MAX) btok = EOS_ID;  // a row of NaNs ranks nothing: end it rather than index the tables with a non-token
  bb.cur_tok[b] = btok;
  out_ids[(size_t)b * bd.maxlen + pos + 1] = btok;
  if (bd.trie_child) {
    const int nd = bb.node[cur][b], c = btok - (pos * V + 2);
    int nx = (nd >= 0 && c >= 0 && c < V) ? bd.trie_child[(size_t)nd * V + c] : -1;
    if (nx >= bd.trie_nodes) nx = -1;  // a malformed table must not send later lookups out of bounds
    bb.node[cur ^ 1][b] = nx;
  }
  if (btok != EOS_ID) return;
  out_len[b] = pos + 2;  // :613 sent_lengths = cur_len after the increment: START and EOS both count
  bb.done[b] = 1;        // :615
  if (atomicAdd(bb.n_done, 1) + 1 == bd.B) {  // :618-619 `if unfinished_sents.max() == 0: break` — the words beam_update_kernel raises
    *bb.live = 0;
    if (bb.all_done_host) {
      __hip_atomic_store(bb.all_done_host + 64, pos + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __hip_atomic_store(bb.all_done_host, bb.done_epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

// ---- given tokens: gdr_t5_generate's score mode (out_len == NULL) ----------------------------------------------------------------
// Nothing is searched: row r of `ids` [rows][maxlen] is START, tokens, then EOS, then PAD, as beam_finalize_kernel lays a hypothesis
// out, and the call reports the score the search gives that hypothesis.  Every row keeps its own cache slots (the ancestor of row r
// at position p is row r), the step's input token is the row's own, and what the select does in a search is one wave per row here:
// the log-softmax of the row's V + 1 live logits — beam_topk_kernel's / beam_norm_kernel's lane assignment and order, so the
// log-probabilities get the same bits — read off at the forced token and added to the row's sum in fp32, as the search adds it to
// beam_scores.  maxlen <= MAXLEN_CAP < 64: lane t of the wave looks at the row's token t.
__device__ __forceinline__ int forced_first_eos(const int64_t* __restrict__ row, int ml, int lane) {
  const unsigned long long m = __ballot(lane >= 1 && lane < ml && row[lane] == EOS_ID);
  return m ? (int)__ffsll((long long)m) - 1 : ml;  // ml: the row never ends
}

__global__ void forced_init_kernel(BeamBufs bb, BeamDims bd, const int64_t* __restrict__ ids) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < bd.B * bd.R) {
    bb.beam_scores[r] = 0.f;
    bb.cur_tok[r] = ids[(size_t)r * bd.maxlen];
    bb.kv_rows[r] = r;  // step 0: stride 1, position 0
  }
  if (r == 0) *bb.n_done = 0, *bb.live = 1;
}

// After position `pos` of every row.  planes (optional) [maxlen + 2][rows][d]: plane t < maxlen the last hidden state of position t
// (zero behind the row's first EOS), plane maxlen the one AT the first EOS (zero for a row without), plane maxlen + 1 the sum over
// t = 0 and every t >= 1 with ids[t] != PAD, ascending in fp32 (forced_finish_kernel divides it by the count).
__global__ __launch_bounds__(256) void forced_step_kernel(BeamBufs bb, BeamDims bd, int pos, const int64_t* __restrict__ ids,
                                                          const float* __restrict__ hl, int d4, float* __restrict__ planes) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int rows = bd.B * bd.R, ml = bd.maxlen, V = bd.V, V1 = V + 1;
  if (r >= rows) return;
  const int64_t* row = ids + (size_t)r * ml;
  const int eos = forced_first_eos(row, ml, lane);
  if (pos + 1 < ml && pos < eos) {  // the token behind this position counts: up to and including the first EOS
    const float* lg = bb.logits + (size_t)r * V1;
    float mx = -INFINITY;
    for (int c = lane; c < V1; c += 64) mx = fmaxf(mx, lg[c]);
    mx = wave_max(mx);
    float sm = 0.f;
    for (int c = lane; c < V1; c += 64) sm += expf(lg[c] - mx);
    sm = wave_sum(sm);
    // column V is EOS' alone: the first digit token of the NEXT position, pos * V + 2 + V, is no live column of this one.  A token
    // that is no live column of this position holds the masked logit (select_valid_embedding: exactly -1e9)
    const int64_t tok = row[pos + 1], digit = tok - ((int64_t)pos * V + 2);
    const int64_t c = tok == EOS_ID ? V : ((digit >= 0 && digit < V) ? digit : -1);
    const float lgt = c >= 0 ? lg[c] : -1e9f;
    const float logp = (lgt - mx) - logf(sm);
    if (lane == 0) bb.beam_scores[r] = logp + bb.beam_scores[r];
  }
  if (planes) {
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4* h = reinterpret_cast<const float4*>(hl) + (size_t)r * d4;
    float4* p4 = reinterpret_cast<float4*>(planes);
    float4* tr = p4 + ((size_t)pos * rows + r) * d4;
    float4* at_eos = p4 + ((size_t)ml * rows + r) * d4;
    float4* mean = p4 + ((size_t)(ml + 1) * rows + r) * d4;
    const bool counted = pos == 0 || row[pos] != PAD_ID;
    for (int c = lane; c < d4; c += 64) {
      const float4 v = h[c];
      tr[c] = pos <= eos ? v : zero;
      if (pos == 0) {
        at_eos[c] = zero;  // eos >= 1: the step that reaches it writes over this
        mean[c] = v;
      } else {
        if (pos == eos) at_eos[c] = v;
        if (counted) {
          const float4 m = mean[c];
          mean[c] = make_float4(m.x + v.x, m.y + v.y, m.z + v.z, m.w + v.w);
        }
      }
    }
  }
  if (pos + 1 < ml) {  // the next position's input token and key list: the row's own slots of positions 0 .. pos + 1
    const int stride = pos + 2;
    if (lane == 0) bb.cur_tok[r] = row[pos + 1];
    if (lane < stride) bb.kv_rows[(size_t)r * stride + lane] = lane * rows + r;
  }
}

// score = sum / len^length_penalty in double (hyp_add, beam_finalize_kernel): len = the EOS position, maxlen for a row without
__global__ __launch_bounds__(256) void forced_finish_kernel(BeamBufs bb, BeamDims bd, const int64_t* __restrict__ ids, int d4,
                                                            float* __restrict__ planes, double* __restrict__ out_scores) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int rows = bd.B * bd.R, ml = bd.maxlen;
  if (r >= rows) return;
  const int64_t* row = ids + (size_t)r * ml;
  const int eos = forced_first_eos(row, ml, lane);
  if (lane == 0) out_scores[r] = (double)bb.beam_scores[r] / pow((double)eos, bd.lp);
  if (!planes) return;
  const float n = (float)(1 + __popcll(__ballot(lane >= 1 && lane < ml && row[lane] != PAD_ID)));
  float4* mean = reinterpret_cast<float4*>(planes) + ((size_t)(ml + 1) * rows + r) * d4;
  for (int c = lane; c < d4; c += 64) {
    const float4 m = mean[c];
    mean[c] = make_float4(m.x / n, m.y / n, m.z / n, m.w / n);
  }
}

// ------------------------------------------------------------------------------------------ driver pieces
// dynamic LDS of the two kernels that hold a query's hypothesis heap
static size_t beam_update_lds(const BeamDims& bd) {
  return ((hyp_lds_bytes(bd.R, bd.maxlen) + 15) & ~(size_t)15) + (size_t)bd.R * 4 + (size_t)bd.R * 16;
}
static size_t beam_finalize_lds(const BeamDims& bd) {
  return ((hyp_lds_bytes(bd.R, bd.maxlen) + 15) & ~(size_t)15) + (size_t)bd.nret * 4 +
         (size_t)bd.R * bd.maxlen * 4 + (size_t)(bd.R + 2) * 4 +   // + the staged beam rows and scores
         (size_t)(2 * bd.R + 2) * 12 + 16;                         // + all scores (double) and survivor slots
}

int check_beam_dims(const BeamDims& bd, int max_length) {
  GDR_CHECK_ARG(bd.B > 0 && bd.R >= 2 && bd.R <= GDR_MAX_BEAMS, "beam: B=%d num_beams=%d (need 2..%d)", bd.B, bd.R, GDR_MAX_BEAMS);
  GDR_CHECK_ARG(bd.nret >= 1 && bd.nret <= bd.R, "beam: num_return_sequences=%d must be in [1,num_beams]", bd.nret);
  GDR_CHECK_ARG(max_length >= 2 && max_length <= MAXLEN_CAP, "beam: max_length=%d must be in [2,%d]", max_length,
                MAXLEN_CAP);
  GDR_CHECK_ARG(bd.V >= 1 && bd.Vd >= bd.V * (max_length - 1) + 2, "beam: decode vocab %d too small for V=%d, max_length=%d",
                bd.Vd, bd.V, max_length);
  GDR_CHECK_ARG((int64_t)bd.R * (bd.V + 1) <= BEAM_MAX_CAND, "beam: num_beams*(V+1)=%lld exceeds the %d candidates per query of the select",
                (long long)bd.R * (bd.V + 1), BEAM_MAX_CAND);
  GDR_CHECK_ARG(bd.lp > 0.0, "beam: length_penalty must be > 0");
  // the hypothesis heap of a query (R+1 entries of max_length tokens) lives in one workgroup's LDS, beside the finalisation's staged
  // beam rows: 64 bytes are left for the kernels' static words
  const size_t heap = beam_update_lds(bd) > beam_finalize_lds(bd) ? beam_update_lds(bd) : beam_finalize_lds(bd);
  GDR_CHECK_ARG(heap + 64 <= (size_t)BEAM_LDS_LIMIT,
                "beam: num_beams=%d at max_length=%d needs %zu B of LDS for a query's hypothesis heap (limit %d): fewer beams or a shorter max_length",
                bd.R, max_length, heap + 64, BEAM_LDS_LIMIT);
  return GDR_OK;
}

// num_beams = 1 (gdr_t5_generate only: gdr_beam_search_table keeps check_beam_dims' range).  No candidate list and no hypothesis
// heap, so none of the select's or the LDS limits apply; length_penalty is accepted and unused, as in the reference.
int check_greedy_dims(const BeamDims& bd, int max_length) {
  GDR_CHECK_ARG(bd.B > 0, "generate: B=%d must be positive", bd.B);
  GDR_CHECK_ARG(max_length >= 2 && max_length <= MAXLEN_CAP, "generate: max_length=%d must be in [2,%d]", max_length, MAXLEN_CAP);
  GDR_CHECK_ARG(bd.V >= 1 && bd.Vd >= bd.V * (max_length - 1) + 2, "generate: decode vocab %d too small for V=%d, max_length=%d",
                bd.Vd, bd.V, max_length);
  return GDR_OK;
}

// The score mode of gdr_t5_generate: any 1 .. GDR_MAX_BEAMS rows per query — no candidate list and no hypothesis heap, so neither the
// select's nor the LDS limit applies.  Every row is reported: num_return_sequences = num_beams.
int check_forced_dims(const BeamDims& bd, int max_length) {
  GDR_CHECK_ARG(bd.B > 0, "generate(score mode, out_len=NULL): B=%d must be positive", bd.B);
  GDR_CHECK_ARG(bd.R >= 1 && bd.R <= GDR_MAX_BEAMS, "generate(score mode, out_len=NULL): num_beams=%d rows per query must be in [1,%d]", bd.R,
                GDR_MAX_BEAMS);
  GDR_CHECK_ARG(bd.nret == bd.R, "generate(score mode, out_len=NULL): num_return_sequences=%d must equal num_beams=%d (every given row is scored)",
                bd.nret, bd.R);
  GDR_CHECK_ARG(max_length >= 2 && max_length <= MAXLEN_CAP, "generate(score mode, out_len=NULL): max_length=%d must be in [2,%d]", max_length,
                MAXLEN_CAP);
  GDR_CHECK_ARG(bd.V >= 1 && bd.Vd >= bd.V * (max_length - 1) + 2, "generate(score mode, out_len=NULL): decode vocab %d too small for V=%d, max_length=%d",
                bd.Vd, bd.V, max_length);
  GDR_CHECK_ARG(bd.lp > 0.0, "generate(score mode, out_len=NULL): length_penalty must be > 0");
  return GDR_OK;
}

int forced_begin(const BeamBufs& bb, const BeamDims& bd, const int64_t* ids, hipStream_t stream) {
  const int rows = bd.B * bd.R;
  hipLaunchKernelGGL(forced_init_kernel, dim3((rows + 255) / 256), dim3(256), 0, stream, bb, bd, ids);
  GDR_CHECK_LAUNCH("forced_init_kernel");
  return GDR_OK;
}

int forced_step(const BeamBufs& bb, const BeamDims& bd, int pos, const int64_t* ids, const float* hl, int d, float* planes,
                hipStream_t stream) {
  const int rows = bd.B * bd.R;
  hipLaunchKernelGGL(forced_step_kernel, dim3((rows + 3) / 4), dim3(256), 0, stream, bb, bd, pos, ids, hl, d / 4, planes);
  GDR_CHECK_LAUNCH("forced_step_kernel");
  return GDR_OK;
}

int forced_end(const BeamBufs& bb, const BeamDims& bd, const int64_t* ids, int d, float* planes, double* out_scores, hipStream_t stream) {
  const int rows = bd.B * bd.R;
  hipLaunchKernelGGL(forced_finish_kernel, dim3((rows + 3) / 4), dim3(256), 0, stream, bb, bd, ids, d / 4, planes, out_scores);
  GDR_CHECK_LAUNCH("forced_finish_kernel");
  return GDR_OK;
}

int greedy_begin(const BeamBufs& bb, const BeamDims& bd, int64_t* out_ids, int32_t* out_len, double* out_scores, hipStream_t stream) {
  hipLaunchKernelGGL(greedy_init_kernel, dim3((bd.B + 255) / 256), dim3(256), 0, stream, bb, bd, out_ids, out_len, out_scores);
  GDR_CHECK_LAUNCH("greedy_init_kernel");
  return GDR_OK;
}

// One decode step's select and bookkeeping at num_beams = 1 after bb.logits holds the step's unmasked-column logits.
int greedy_step(const BeamBufs& bb, const BeamDims& bd, int pos, int cur, int64_t* out_ids, int32_t* out_len, hipStream_t stream) {
  hipLaunchKernelGGL(greedy_step_kernel, dim3((bd.B + 3) / 4), dim3(256), 0, stream, bb, bd, pos, cur, out_ids, out_len);
  GDR_CHECK_LAUNCH("greedy_step_kernel");
  return GDR_OK;
}

// One decode step's beam machinery after bb.logits holds the step's unmasked-column logits.
int beam_step(const BeamBufs& bb, const BeamDims& bd, int pos, int cur, float* step_scores, int32_t* step_tokens, hipStream_t stream,
              bool bcast) {
  const size_t tr = (size_t)pos * bd.B * 2 * bd.R;
  float* tr_s = step_scores ? step_scores + tr : nullptr;
  int32_t* tr_t = step_tokens ? step_tokens + tr : nullptr;
  if (!beam_chunked(bd.R, bd.V)) {
    const int npad = sel_pow2(bd.R * (bd.V + 1));
    const size_t lds = (size_t)npad * 8 + (size_t)bd.R * 8 + (size_t)bd.R * (bd.V + 1) * 4;
    hipLaunchKernelGGL(beam_topk_kernel, dim3(bd.B), dim3(npad >= 2048 ? 1024 : 256), lds, stream, bb, bd, pos, npad, cur,
                       bcast ? 1 : 0, tr_s, tr_t);
    GDR_CHECK_LAUNCH("beam_topk_kernel");
  } else {
    const int nchunks = beam_chunks(bd.R, bd.V);
    hipLaunchKernelGGL(beam_norm_kernel, dim3(bd.B, (bd.R + 3) / 4), dim3(256), 0, stream, bb, bd, bcast ? 1 : 0);
    GDR_CHECK_LAUNCH("beam_norm_kernel");
    hipLaunchKernelGGL(beam_chunk_kernel, dim3(bd.B, nchunks), dim3(1024), 0, stream, bb, bd, pos, cur, bcast ? 1 : 0, nchunks);
    GDR_CHECK_LAUNCH("beam_chunk_kernel");
    // at most 3 rounds: 32 chunks, 4 lists per workgroup at 1024 beams
    const BeamEmit emit{bb.live_gate, bb.cand_score, bb.cand_idx, tr_s, tr_t};
    if (int rc__ = sel_merge_rounds(bb.part, nchunks, 2 * bd.R, bd.B, 1, emit, "sel_merge_kernel<beam>", stream)) return rc__;
  }
  const size_t hyp_lds = beam_update_lds(bd);
  hipLaunchKernelGGL(beam_update_kernel, dim3(bd.B), dim3(256), hyp_lds, stream, bb, bd, pos + 1, cur);
  GDR_CHECK_LAUNCH("beam_update_kernel");
  return GDR_OK;  // the ancestor table of the next position is rebuilt at the end of beam_update_kernel
}

int beam_begin(const BeamBufs& bb, const BeamDims& bd, hipStream_t stream, bool dedup0) {
  const int rows = bd.B * bd.R;
  // 1024 beams: the one-sort form's keys + staged logits reach 104 KiB (7 columns), a query's hypothesis heap whatever
  // check_beam_dims lets through
  if (int rc__ = ensure_dyn_lds(reinterpret_cast<const void*>(beam_topk_kernel), BEAM_LDS_LIMIT, "beam")) return rc__;
  if (int rc__ = ensure_dyn_lds(reinterpret_cast<const void*>(beam_update_kernel), BEAM_LDS_LIMIT - 64, "beam")) return rc__;
  if (int rc__ = ensure_dyn_lds(reinterpret_cast<const void*>(beam_finalize_kernel), BEAM_LDS_LIMIT - 64, "beam")) return rc__;
  if (int rc__ = ensure_dyn_lds(reinterpret_cast<const void*>(sel_merge_kernel<BeamEmit>), SEL_SORT_MAX * 8, "beam")) return rc__;
  hipLaunchKernelGGL(beam_init_kernel, dim3((rows + 255) / 256), dim3(256), 0, stream, bb, bd, dedup0 ? 1 : 0);
  GDR_CHECK_LAUNCH("beam_init_kernel");
  return GDR_OK;
}

int beam_end(const BeamBufs& bb, const BeamDims& bd, int max_length, int cur, int64_t* out_ids, int32_t* out_len, double* out_scores,
             hipStream_t stream) {
  const size_t hyp_lds = beam_finalize_lds(bd);
  hipLaunchKernelGGL(beam_finalize_kernel, dim3(bd.B), dim3(256), hyp_lds, stream, bb, bd, max_length, cur, max_length, out_ids,
                     out_len, out_scores);
  GDR_CHECK_LAUNCH("beam_finalize_kernel");
  return GDR_OK;
}

}  // namespace gdr

extern "C" size_t gdr_beam_search_table_workspace_bytes(int B, int num_beams, int max_length, int out_vocab) {
  if (B <= 0 || num_beams <= 0 || max_length < 2) return 0;
  gdr::BeamDims bd{B, num_beams, out_vocab, out_vocab * max_length + 2, max_length, num_beams, 1.0, nullptr, nullptr, 0};
  return gdr::beam_layout(bd, nullptr, nullptr);
}

extern "C" int gdr_beam_search_table(const float* table, int B, int out_vocab, int num_beams, int max_length,
                                     double length_penalty, int num_return_sequences, const GdrTrie* trie,
                                     int64_t* out_ids, int32_t* out_len, double* out_scores, void* workspace,
                                     size_t workspace_bytes, void* stream_) {
  using namespace gdr;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  GDR_CHECK_ARG(table && out_ids && out_len && out_scores && workspace, "beam_search_table: null pointer");
  BeamDims bd{B, num_beams, out_vocab, out_vocab * max_length + 2, max_length, num_return_sequences, length_penalty,
              trie ? trie->child : nullptr, trie ? trie->eos_ok : nullptr, trie ? trie->n_nodes : 0};
  GDR_CHECK_ARG(!trie || (trie->child && trie->eos_ok && trie->n_nodes > 0), "beam_search_table: bad trie");
  GDR_CHECK_ARG(!trie || trie->V == out_vocab, "beam_search_table: trie built for V=%d but out_vocab=%d",
                trie ? trie->V : 0, out_vocab);
  int rc = check_beam_dims(bd, max_length);
  if (rc) return rc;
  const size_t need = beam_layout(bd, nullptr, nullptr);
  if (workspace_bytes < need) {
    set_error("beam_search_table: workspace %zu < required %zu", workspace_bytes, need);
    return GDR_ENOSPC;
  }
  BeamBufs bb{};
  beam_layout(bd, static_cast<char*>(workspace), &bb);
  if ((rc = beam_begin(bb, bd, stream))) return rc;
  const int rows = B * num_beams, V1 = out_vocab + 1;
  int cur = 0;
  for (int s = 0; s + 1 < max_length; ++s) {
    const int n = rows * V1;
    hipLaunchKernelGGL(table_logits_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, table, bb.cur_tok, rows,
                       num_beams, out_vocab, bd.Vd, max_length, s, bb.logits);
    GDR_CHECK_LAUNCH("table_logits_kernel");
    if ((rc = beam_step(bb, bd, s, cur, nullptr, nullptr, stream))) return rc;
    cur ^= 1;
  }
  return beam_end(bb, bd, max_length, cur, out_ids, out_len, out_scores, stream);
}
