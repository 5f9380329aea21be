// Fused corpus similarity + top-k for gfx950 (include/gdr_hip.h: gdr_sim_topk, gdr_topk_merge).
//
// Replaces `scores = q_reps @ p_reps.T` (reference GDR_model/dense.py:53-54, encoder.py:128-129)
// followed by `scores.topk(k, largest=True, sorted=True)` (as at main_models.py:1625) without ever
// writing the [B,N] score matrix:
//
//   1. SAMPLE   the GEMM core (gemm_f32.hip) runs over every `stride`-th 128-doc tile of the corpus and
//               stores those scores into per-query candidate lists  cand[q][0 .. n_slots).
//   2. THRESH   one workgroup per query radix-selects the k-th largest sample score thr[q].  The k-th
//               largest over ANY subset of the docs is a lower bound of the k-th largest over all of
//               them, so `score >= thr[q]` can never reject a true top-k doc (ties included).
//   3. FILTER   the GEMM core runs over the remaining tiles; its epilogue compares the accumulators
//               (a lane owns one query: docs sit in the row role) against thr and appends the few
//               survivors (expected k*N/n_sample per query) with one returning atomic each.
//   4. SELECT   one workgroup per query radix-selects the exact k largest 64-bit keys
//               (orderable(score) << 32 | ~doc) — distinct keys, so ties resolve as "higher score, then
//               lower doc id" — then bitonic-sorts them in LDS and writes values + ids.
//
// n_sample ≈ sqrt(k·N) balances list length against survivors.  Small corpora take steps 1, 2, 4 only.
//
// Steps 1 - 3, with the row mask of GDR_SIM_LIVE_MASK / GDR_SIM_QUERY_MASK between them, are written once: run_candidate_passes.
// gdr_sim_topk[_bf16] (sim_topk_impl) puts step 4 behind it; the bf16 pre-filter (prefilter_impl) puts the query prep in front and its
// rescoring tail behind.  The bitmaps at the head of a workspace are described once too (MaskHead), as are the argument checks
// (check_search_args), the "largest plan up to k" of the workspace questions (largest_plan_up_to) and the select launch (launch_select).
#include <stdlib.h>

#include <map>
#include <mutex>
#include <tuple>

#include "scan.h"
#include "select.h"

namespace gdr {

constexpr int TILE = 128;
constexpr int SEL_THREADS = 256;

struct SimPlan {
  int64_t tiles_m;
  int stride;          // sample tiles: index % stride == 0
  int64_t n_sample_tiles;
  int64_t n_slots;     // n_sample_tiles * TILE
  int64_t cap;         // candidate list capacity per query (multiple of TILE)
  size_t off_val, off_idx, off_cnt, off_thr, off_part, total;
};

// survivors: by how much the filter pass's threshold admits more docs than the k-th largest sample score would (1 = that score
// itself; the pre-filter lowers it by 2 eps_q, see prefilter_survivor_factor).
// base: bytes in front of the plan's own scratch (GDR_SIM_LIVE_MASK: the caller's row bitmap, live_mask_bytes; GDR_SIM_QUERY_MASK:
// one such bitmap per query, B of them) — every offset and the total move by it; 0 for every other call.
static SimPlan make_plan(int B, int64_t N, int k, bool exhaustive, double survivors = 1.0, size_t base = 0) {
  SimPlan p{};
  p.tiles_m = (N + TILE - 1) / TILE;
  double target = sqrt((double)k * (double)N);
  if (target < k) target = k;
  int64_t ts = (int64_t)((target + TILE - 1) / TILE);
  if (ts < 1) ts = 1;
  if (exhaustive || N <= 16384 || p.tiles_m < 4 * ts) {
    p.stride = 1;
  } else {
    p.stride = (int)(p.tiles_m / ts);
  }
  p.n_sample_tiles = (p.tiles_m + p.stride - 1) / p.stride;
  p.n_slots = p.n_sample_tiles * TILE;
  if (p.stride == 1) {
    p.cap = p.n_slots;
  } else {
    const double n_sample = (double)p.n_slots;
    const double expect = (double)k * (double)N / n_sample;
    p.cap = p.n_slots + (int64_t)(4.0 * expect * survivors) + 4096;
    p.cap = (p.cap + TILE - 1) / TILE * TILE;
  }
  size_t o = base;
  p.off_val = o, o += align_up((size_t)B * p.cap * sizeof(float), 256);
  p.off_idx = o, o += align_up((size_t)B * p.cap * sizeof(int32_t), 256);
  p.off_cnt = o, o += align_up((size_t)B * CNT_STRIDE * sizeof(int32_t), 256);
  p.off_thr = o, o += align_up((size_t)B * sizeof(float), 256);
  // latency mode (B <= 32): the slices' top-k keys of the sliced threshold / select tails, [B][16 slices][128] x 8 bytes
  p.off_part = o, o += B <= 32 ? align_up((size_t)B * 16 * 128 * sizeof(unsigned long long), 256) : 0;
  p.total = o;
  return p;
}

// (the orderable keys, their 64-bit pack and the bitonic sorts: select.h)

// Four fp32 -> four bf16, stored as 8 bytes (v_cvt_pk_bf16_f32: RNE, NaN-safe): THE bf16 image of a corpus row or a query, wherever it
// is made.
__device__ __forceinline__ void store_bf16x4(uint2* dst, const float4& v) {
  union {
    __bf16 h[4];
    uint2 u;
  } o;
  o.h[0] = (__bf16)v.x, o.h[1] = (__bf16)v.y, o.h[2] = (__bf16)v.z, o.h[3] = (__bf16)v.w;
  *dst = o.u;
}

// ||row||^2 by one wave, in every lane: a lane's fmaf chain over its 16-byte pieces (lane, lane + 64, ...), then the shuffle tree.
// each(c, v) sees every piece.  The bits are a contract between row_norm2_max_kernel and prefilter_update_rows_kernel
// (include/gdr_hip.h at gdr_prefilter_update_rows): both call this.
template <class Each>
__device__ __forceinline__ float wave_row_norm2(const float* __restrict__ row, int d, int lane, Each each) {
  float ss = 0.f;
  for (int c = lane * 4; c < d; c += 256) {
    const float4 v = *reinterpret_cast<const float4*>(row + c);
    ss = fmaf(v.x, v.x, fmaf(v.y, v.y, fmaf(v.z, v.z, fmaf(v.w, v.w, ss))));
    each(c, v);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) ss += __shfl_xor(ss, off);
  return ss;
}

// Given hist[256] (LDS) find the highest bin b with  sum(hist[b..255]) >= need.
// Returns b and the count strictly above it through *above.  Every thread of the block calls it (blockDim >= 256).
// `need` is clamped to the number of keys counted (a merge input may hold fewer than k live entries).
// The suffix sums are formed inside the four waves that own the bins (shuffles, no barrier) and joined through four words
// of LDS: two workgroup barriers per call (the Hillis-Steele scan over LDS this replaces took sixteen; with up to eight
// digit passes per select that was most of the kernel's synchronisation).
__device__ __forceinline__ int find_bin(int* hist, int* scan, int& need, int* above, int* res) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int v = t < 256 ? hist[t] : 0;
  int sfx = v;  // suffix sum over this wave's 64 bins: sum of bins lane .. 63
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int u = __shfl_down(sfx, off);
    if (lane + off < 64) sfx += u;
  }
  if (t < 256 && lane == 0) scan[wave] = sfx;
  if (t == 0) res[0] = 0, res[1] = 0;
  __syncthreads();
  const int w0 = scan[0], w1 = scan[1], w2 = scan[2], w3 = scan[3];
  const int total = w0 + w1 + w2 + w3;
  if (total < need) need = total;
  if (t < 256 && need > 0) {
    const int higher = wave == 0 ? w1 + w2 + w3 : wave == 1 ? w2 + w3 : wave == 2 ? w3 : 0;
    const int mine = sfx + higher, next = mine - v;  // bins t..255 / t+1..255
    if (mine >= need && next < need) {
      res[0] = t;
      res[1] = next;
    }
  }
  __syncthreads();
  *above = res[1];
  return res[0];
}

// Block-wide min / max of 32-bit keys (red[] holds 2 * 16 words).  Result broadcast to every thread.
__device__ __forceinline__ void block_minmax(uint32_t& lo, uint32_t& hi, uint32_t* red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    lo = min(lo, (uint32_t)__shfl_xor((int)lo, off));
    hi = max(hi, (uint32_t)__shfl_xor((int)hi, off));
  }
  const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  if ((threadIdx.x & 63) == 0) red[w] = lo, red[16 + w] = hi;
  __syncthreads();
  lo = red[0], hi = red[16];
  for (int i = 1; i < nw; ++i) lo = min(lo, red[i]), hi = max(hi, red[16 + i]);
  __syncthreads();
}

// The radix passes below work on RANGE-NORMALISED keys: (key - lo) left-aligned so that the first 8-bit digit already
// spreads the live range over 256 bins.  Similarity scores share sign and exponent, so digits taken from the raw
// float bits spend two full sweeps (and ~10^4 same-address LDS atomics each) without separating anything.

// The 32-bit key (fkey) of the k-th largest of v[0 .. count), -inf entries aside; fkey(-inf) when there is nothing else.  Every
// thread of the workgroup calls it: nthr = its size as the caller knows it (a literal where the launch fixes it), hist / scan /
// res / red the caller's LDS words.  The scores are read ONCE: up to RC keys per thread stay in rk[] across the digit passes
// (every pass used to re-read them from memory — a dependent L2 round trip per sweep) and are the caller's afterwards — rk[u] is
// the key of v[tid + u * nthr], 0 for "no entry" (fkey(-inf) = 0x007fffff > 0), all 0 when count > RC * nthr: such lists are
// re-read on every pass, by loops unrolled UNROLL times (4: sim_threshold_kernel's pragma; 1: what the compiler chose for the
// pre-filter tail, which had none).  cached says which of the two it was, for a caller that goes on using rk[].
template <int UNROLL, int RC>
__device__ __forceinline__ uint32_t radix_kth_key(const float* __restrict__ v, int count, int k, int nthr, uint32_t (&rk)[RC],
                                                  bool& cached, int* hist, int* scan, int* res, uint32_t* red) {
  const int tid = threadIdx.x;
  cached = count <= RC * nthr;
#pragma unroll
  for (int u = 0; u < RC; ++u) {
    const int i = tid + u * nthr;
    rk[u] = (cached && i < count) ? fkey(v[i]) : 0u;
  }
  const uint32_t kneg = fkey(-INFINITY);
  uint32_t lo = 0xFFFFFFFFu, hi = 0u;  // range of the real scores; -inf padding slots of a ragged tile stay below it
  if (cached) {
#pragma unroll
    for (int u = 0; u < RC; ++u)
      if (rk[u] > kneg) lo = min(lo, rk[u]), hi = max(hi, rk[u]);
  } else {
#pragma unroll UNROLL
    for (int i = tid; i < count; i += nthr) {
      const float x = v[i];
      if (x > -INFINITY) {
        const uint32_t key = fkey(x);
        lo = min(lo, key), hi = max(hi, key);
      }
    }
  }
  block_minmax(lo, hi, red);
  if (hi < lo) lo = hi = kneg;  // nothing but padding
  const int nbits = hi > lo ? 32 - __clz(hi - lo) : 0;
  const int lsh = 32 - nbits;  // nbits == 0: every key equal, no pass runs
  uint32_t prefix = 0;
  int need = k;
  for (int pass = 0; 8 * pass < nbits; ++pass) {
    const int shift = 24 - 8 * pass;
    if (tid < 256) hist[tid] = 0;
    __syncthreads();
    if (cached) {
#pragma unroll
      for (int u = 0; u < RC; ++u) {
        const uint32_t raw = rk[u];
        const uint32_t key = (raw - lo) << lsh;
        const bool match = pass == 0 ? true : ((key >> (shift + 8)) == (prefix >> (shift + 8)));
        if (raw != 0u && match && raw >= lo) atomicAdd(&hist[(key >> shift) & 255u], 1);
      }
    } else {
#pragma unroll UNROLL
      for (int i = tid; i < count; i += nthr) {
        const uint32_t raw = fkey(v[i]);
        const uint32_t key = (raw - lo) << lsh;
        const bool match = pass == 0 ? true : ((key >> (shift + 8)) == (prefix >> (shift + 8)));
        if (match && raw >= lo) atomicAdd(&hist[(key >> shift) & 255u], 1);
      }
    }
    __syncthreads();
    int above;
    const int b = find_bin(hist, scan, need, &above, res);
    need -= above;
    prefix |= (uint32_t)b << shift;
    __syncthreads();
  }
  return nbits ? (prefix >> lsh) + lo : lo;
}

// ---- step 2: per-query threshold = k-th largest of the sample scores ----------------------------
// sub != null (the bf16 pre-filter below): thr[q] = value - sub[q]
__global__ __launch_bounds__(1024) void sim_threshold_kernel(const float* __restrict__ cand_val, int64_t cap,
                                                             int n_slots, int k, float* thr, int32_t* cand_cnt,
                                                             const float* __restrict__ sub) {
  __shared__ int hist[256];
  __shared__ int scan[256];
  __shared__ int res[2];
  __shared__ uint32_t red[32];
  const int q = blockIdx.x;
  uint32_t rk[8];
  bool cached;
  const uint32_t kth = radix_kth_key<4>(cand_val + (int64_t)q * cap, n_slots, k, (int)blockDim.x, rk, cached, hist, scan, res, red);
  if (threadIdx.x == 0) {
    const float t = fkey_inv(kth);
    thr[q] = sub ? t - sub[q] : t;
    cand_cnt[(int64_t)q * CNT_STRIDE] = n_slots;  // survivors of the filter pass are appended behind the sample block
  }
}

// ---- step 4 / merge: exact top-k of a candidate list, sorted ------------------------------------
// MERGE = false: entries cand_val/cand_idx[q*cap + i], i < min(cnt[q], cap); thr[q] (the k-th largest sample score,
//                at least k entries reach it) bounds the live range from below
// MERGE = true : entries vals/idx[((g*B + q)*rs + j)*es], i = g*k + j < G*k.  rs = entries per (shard, query) row (k, or
//                k+1 when a trailing status entry rides along), es = element stride (2 when vals/idx interleave as
//                {score, id} pairs).  With rs > k and `status`, status[q] = OR over shards of the trailing entry's id.
// DEEP = false: k <= 1024 — the first wave alone sorts the kpad selected keys (no workgroup barrier inside the sort).
// DEEP = true : 1024 < k <= SEL_SORT_MAX — the same passes pick the keys, the whole workgroup sorts kpad = 2048 .. 8192 of them
//                with select.h's network (16 .. 64 KiB of dynamic LDS: the launcher raises the limit).  The gather keeps its one
//                same-address LDS atomic per selected key: a per-wave ballot / prefix compaction (one atomic per wave and sweep)
//                measured the same or 1 - 2 % slower per call at k = 8192, so it was not kept.
template <bool MERGE, bool DEEP = false>
__global__ __launch_bounds__(1024) void topk_select_kernel(const float* __restrict__ vals,
                                                           const int32_t* __restrict__ idxs,
                                                           const int32_t* __restrict__ cnt, int64_t cap, int G, int B,
                                                           int k, int kpad, int32_t idx_offset,
                                                           const float* __restrict__ thr, float* out_val,
                                                           int32_t* out_idx, int32_t* __restrict__ status, int rs,
                                                           int es) {
  __shared__ int hist[256];
  __shared__ int scan[256];
  __shared__ int res[2];
  __shared__ uint32_t red[32];
  __shared__ int n_out;
  extern __shared__ __attribute__((aligned(16))) unsigned long long sortbuf[];  // kpad entries
  const int q = blockIdx.x;
  int count;
  if (MERGE) {
    count = G * k;
    if (status && rs > k && threadIdx.x == 0) {
      int32_t any = 0;
      for (int g = 0; g < G; ++g) any |= idxs[(((int64_t)g * B + q) * rs + k) * es];
      status[q] = any != 0 ? 1 : 0;
    }
  } else {
    const int c = cnt[(int64_t)q * CNT_STRIDE];  // the similarity passes' counters (common.h CNT_STRIDE)
    count = c < (int)cap ? c : (int)cap;
    if (status && threadIdx.x == 0) status[q] = c > (int)cap ? 1 : 0;  // list overflowed: result is a subset's top-k
  }
  auto addr_of = [&](int i) -> int64_t {
    if (MERGE) {
      const int g = i / k, j = i - g * k;
      return (((int64_t)g * B + q) * rs + j) * es;
    }
    return (int64_t)q * cap + i;
  };
  // The entries are read ONCE: up to RC raw keys (score key : 32 | ~id : 32; 0 = padding) per thread stay in registers across
  // the sweeps below — range, up to eight digit passes, gather — each of which used to be a dependent trip to memory per entry
  // (36 us per call at 32 queries, most of it those trips).  Longer lists (count > RC * blockDim) re-read as before.
  constexpr int RC = 16;
  const bool cached = count <= RC * (int)blockDim.x;
  auto raw_at = [&](int i) -> unsigned long long {
    const int64_t a = addr_of(i);
    const int32_t id = idxs[a];
    if (id < 0) return 0ull;
    return sel_pack(vals[a], (uint32_t)id);
  };
  unsigned long long rk[RC];
#pragma unroll
  for (int u = 0; u < RC; ++u) {
    const int i = threadIdx.x + u * (int)blockDim.x;
    rk[u] = (cached && i < count) ? raw_at(i) : 0ull;
  }
  // sweep 0: live range of the score keys
  uint32_t lo = 0xFFFFFFFFu, hi = 0u;
  if (cached) {
#pragma unroll
    for (int u = 0; u < RC; ++u)
      if (rk[u] != 0ull) {
        const uint32_t key = (uint32_t)(rk[u] >> 32);
        lo = min(lo, key), hi = max(hi, key);
      }
  } else {
#pragma unroll 4
    for (int i = threadIdx.x; i < count; i += blockDim.x) {
      const unsigned long long raw = raw_at(i);
      if (raw != 0ull) {
        const uint32_t key = (uint32_t)(raw >> 32);
        lo = min(lo, key), hi = max(hi, key);
      }
    }
  }
  block_minmax(lo, hi, red);
  if (!MERGE && thr) lo = max(lo, fkey(thr[q]));
  if (hi < lo) hi = lo;  // no valid entry at all
  const int nbits = hi > lo ? 32 - __clz(hi - lo) : 0;
  const int lsh = 32 - nbits;
  // normalised 64-bit key: (score key - lo) : nbits | ~id : 32, left-aligned; 0 = padding / below the live range
  auto norm = [&](unsigned long long raw) -> unsigned long long {
    if (raw == 0ull) return 0ull;
    const uint32_t sk = (uint32_t)(raw >> 32);
    if (sk < lo) return 0ull;
    return ((((unsigned long long)(sk - lo)) << 32) | (raw & 0xFFFFFFFFull)) << lsh;
  };
  // number of entries in the live range bounds `need` (a merge input may hold fewer than k valid entries)
  unsigned long long prefix = 0ull;
  int need = k < count ? k : count;
  int want = need;
  bool exact = false;
  for (int pass = 0; pass < 8 && !exact; ++pass) {
    const int shift = 56 - 8 * pass;
    if (threadIdx.x < 256) hist[threadIdx.x] = 0;
    __syncthreads();
    if (cached) {
#pragma unroll
      for (int u = 0; u < RC; ++u) {
        const unsigned long long key = norm(rk[u]);
        const bool match = pass == 0 ? true : ((key >> (shift + 8)) == (prefix >> (shift + 8)));
        if (match && key != 0ull) atomicAdd(&hist[(int)((key >> shift) & 255ull)], 1);
      }
    } else {
#pragma unroll 4
      for (int i = threadIdx.x; i < count; i += blockDim.x) {
        const unsigned long long key = norm(raw_at(i));
        const bool match = pass == 0 ? true : ((key >> (shift + 8)) == (prefix >> (shift + 8)));
        if (match && key != 0ull) atomicAdd(&hist[(int)((key >> shift) & 255ull)], 1);
      }
    }
    __syncthreads();
    int above;
    const int b = find_bin(hist, scan, need, &above, res);
    if (pass == 0) want = need;  // clamped to the live entries
    need -= above;
    prefix |= (unsigned long long)b << shift;
    exact = hist[b] == need;  // the whole bin is taken: the low bits need no refinement
    __syncthreads();
  }
  // gather the `want` keys >= prefix (raw keys: the sort below needs no range)
  if (threadIdx.x == 0) n_out = 0;
  for (int i = threadIdx.x; i < kpad; i += blockDim.x) sortbuf[i] = 0ull;
  __syncthreads();
  if (cached) {
#pragma unroll
    for (int u = 0; u < RC; ++u) {
      const unsigned long long key = norm(rk[u]);
      if (key >= prefix && key != 0ull) {
        const int p = atomicAdd(&n_out, 1);
        if (p < kpad) sortbuf[p] = rk[u];
      }
    }
  } else {
#pragma unroll 4
    for (int i = threadIdx.x; i < count; i += blockDim.x) {
      const unsigned long long raw = raw_at(i);
      const unsigned long long key = norm(raw);
      if (key >= prefix && key != 0ull) {
        const int p = atomicAdd(&n_out, 1);
        if (p < kpad) sortbuf[p] = raw;
      }
    }
  }
  __syncthreads();
  if (DEEP) {
    bitonic_desc(sortbuf, kpad);  // descending; every wave (kpad >= 2048 is a multiple of 2 x 16 waves), ends with a barrier
  } else {
    wave0_bitonic_desc(sortbuf, kpad);  // descending; the first wave alone, no workgroup barriers inside
    __syncthreads();
  }
  for (int i = threadIdx.x; i < k; i += blockDim.x) {
    const unsigned long long key = sortbuf[i];
    float v = -INFINITY;
    int32_t id = -1;
    if (i < want && key != 0ull) {
      v = sel_score(key);
      id = (int32_t)sel_low(key) + idx_offset;
    }
    out_val[(int64_t)q * k + i] = v;
    out_idx[(int64_t)q * k + i] = id;
  }
}

// ---- latency mode (B <= 32, the stream kernels): threshold and select SPREAD over slices (r06) -----------------------------------
// One workgroup per query left 1 .. 32 workgroups on 256 CUs for the two tails of the call (sim_threshold_kernel 22.6 us +
// topk_select_kernel 54.0 us = 29 % of a 32-query call, profiles/r05_bench_kernel_stats.csv), and most of their time was same-bin LDS
// atomics: 5 900 / 11 000 keys of one query counted into one 256-bin histogram, scores bunched just above the threshold.  Here a
// query's list is cut into NS slices, one 256-thread workgroup each: the slice radix-selects ITS top-k (the global top-k is a subset
// of the union of the slices' top-k lists), stores the keys write-through, and takes a ticket; the LAST arriver of a query loads the
// NS x k keys and selects again — then either the k-th largest score (threshold form) or sort + write (select form).  Exact, and
// deterministic: keys are distinct 64-bit values (score key : 32 | ~id : 32), a top-k set does not depend on arrival order.
// Hand-off (MI355X_MICROARCH.md, inter-workgroup visibility; the stream-K idiom of gemm_f32.hip): sc1 stores, every wave drains,
// the workgroup meets, one lane takes the ticket; the last arriver's lane 0 issues ONE agent-scope acquire, the workgroup meets, plain loads.
constexpr int SL_THREADS = 256, SL_RC = 8, SL_NS_MAX = 16, SL_KPAD_MAX = 128;
struct SelLds {
  int hist[256];
  int scan[256];
  int res[2];
  uint32_t red[32];
  int n_out, last;
};

// The `k` largest of the workgroup's register-held raw keys (0 = no entry; keys whose score key is below lo_floor do not count)
// -> outbuf[0 .. want), unsorted, zero-filled up to kpad.  Returns want = min(k, live keys).  topk_select_kernel's passes.
template <int RC>
__device__ __forceinline__ int block_select_keys(const unsigned long long (&rk)[RC], int k, int kpad, uint32_t lo_floor, SelLds& L,
                                                 unsigned long long* outbuf) {
  uint32_t lo = 0xFFFFFFFFu, hi = 0u;
#pragma unroll
  for (int u = 0; u < RC; ++u)
    if (rk[u] != 0ull) {
      const uint32_t key = (uint32_t)(rk[u] >> 32);
      lo = min(lo, key), hi = max(hi, key);
    }
  block_minmax(lo, hi, L.red);
  lo = max(lo, lo_floor);
  if (hi < lo) hi = lo;
  const int nbits = hi > lo ? 32 - __clz(hi - lo) : 0;
  const int lsh = 32 - nbits;
  auto norm = [&](unsigned long long raw) -> unsigned long long {
    if (raw == 0ull) return 0ull;
    const uint32_t sk = (uint32_t)(raw >> 32);
    if (sk < lo) return 0ull;
    return ((((unsigned long long)(sk - lo)) << 32) | (raw & 0xFFFFFFFFull)) << lsh;
  };
  unsigned long long prefix = 0ull;
  int need = k, want = k;
  bool exact = false;
  for (int pass = 0; pass < 8 && !exact; ++pass) {
    const int shift = 56 - 8 * pass;
    L.hist[threadIdx.x] = 0;
    __syncthreads();
#pragma unroll
    for (int u = 0; u < RC; ++u) {
      const unsigned long long key = norm(rk[u]);
      const bool match = pass == 0 ? true : ((key >> (shift + 8)) == (prefix >> (shift + 8)));
      if (match && key != 0ull) atomicAdd(&L.hist[(int)((key >> shift) & 255ull)], 1);
    }
    __syncthreads();
    int above;
    const int b = find_bin(L.hist, L.scan, need, &above, L.res);
    if (pass == 0) want = need;  // clamped to the live keys
    need -= above;
    prefix |= (unsigned long long)b << shift;
    exact = L.hist[b] == need;
    __syncthreads();
  }
  if (threadIdx.x == 0) L.n_out = 0;
  for (int i = threadIdx.x; i < kpad; i += SL_THREADS) outbuf[i] = 0ull;
  __syncthreads();
  if (want > 0) {
#pragma unroll
    for (int u = 0; u < RC; ++u) {
      const unsigned long long key = norm(rk[u]);
      if (key >= prefix && key != 0ull) {
        const int p = atomicAdd(&L.n_out, 1);
        if (p < kpad) outbuf[p] = rk[u];
      }
    }
  }
  __syncthreads();
  return want;
}

struct SlicedArgs {
  const float* vals;        // [B][cap]
  const int32_t* idxs;      // [B][cap]
  int32_t* cnt;             // [B][CNT_STRIDE]: [0] list length, [1] ticket of the threshold form, [2] ticket of the select form
  int64_t cap;
  int n_slots;              // threshold form: entries [0, n_slots) are the sample scores
  int k, kpad, NS;
  int32_t idx_offset;
  float* thr;               // threshold form: out; select form: in (lower bound of the live range)
  const float* sub;         // threshold form, may be null: thr[q] = value - sub[q]
  unsigned long long* part; // [B][NS][kpad]
  float* out_val;
  int32_t* out_idx;
  int32_t* status;
};

template <bool THR>
__global__ __launch_bounds__(SL_THREADS) void sim_sliced_select_kernel(const SlicedArgs a) {
  __shared__ SelLds L;
  __shared__ __attribute__((aligned(16))) unsigned long long outbuf[SL_KPAD_MAX];
  const int q = blockIdx.x / a.NS, s = blockIdx.x % a.NS, tid = threadIdx.x;
  int count;
  if (THR) {
    count = a.n_slots;
  } else {
    const int c = a.cnt[(int64_t)q * CNT_STRIDE];
    count = c < (int)a.cap ? c : (int)a.cap;
  }
  const int per = (count + a.NS - 1) / a.NS;  // <= SL_RC * SL_THREADS by the launcher's choice of NS
  const int i0 = s * per, i1 = min(count, i0 + per);
  const float* v = a.vals + (int64_t)q * a.cap;
  const int32_t* ix = a.idxs + (int64_t)q * a.cap;
  unsigned long long rk[SL_RC];
#pragma unroll
  for (int u = 0; u < SL_RC; ++u) {
    const int i = i0 + tid + u * SL_THREADS;
    unsigned long long raw = 0ull;
    if (i < i1) {
      const float x = v[i];
      if (THR) {
        if (x > -INFINITY) raw = sel_pack(x, (uint32_t)i);
      } else {
        const int32_t id = ix[i];
        if (id >= 0) raw = sel_pack(x, (uint32_t)id);
      }
    }
    rk[u] = raw;
  }
  const uint32_t floor_key = (!THR && a.thr) ? fkey(a.thr[q]) : 0u;
  block_select_keys<SL_RC>(rk, a.k, a.kpad, floor_key, L, outbuf);
  // publish this slice's keys write-through, then the ticket
  unsigned long long* mine = a.part + ((int64_t)q * a.NS + s) * a.kpad;
  if (tid < a.kpad) {
    const unsigned long long key = outbuf[tid];
    typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
    u32x2 w;
    w[0] = (unsigned int)(key & 0xFFFFFFFFull), w[1] = (unsigned int)(key >> 32);
    const __amdgpu_buffer_rsrc_t dst = __builtin_amdgcn_make_buffer_rsrc(mine, 0, a.kpad * 8, 0x00020000);
    __builtin_amdgcn_raw_buffer_store_b64(w, dst, tid * 8, 0, 16);  // aux 16 = sc1: write-through
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  int32_t* ticket = a.cnt + (int64_t)q * CNT_STRIDE + (THR ? 1 : 2);
  if (tid == 0) {
    const int t = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    L.last = t == a.NS - 1;
    if (L.last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");  // one lane: drops this CU's stale L1 lines of `part`
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
  }
  __syncthreads();
  if (!L.last) return;  // uniform
  // ---- the last arriver of query q: NS x kpad keys -> top-k
  const unsigned long long* all = a.part + (int64_t)q * a.NS * a.kpad;
  const int n_all = a.NS * a.kpad;  // <= SL_RC * SL_THREADS
#pragma unroll
  for (int u = 0; u < SL_RC; ++u) {
    const int i = tid + u * SL_THREADS;
    rk[u] = i < n_all ? all[i] : 0ull;
  }
  const int want = block_select_keys<SL_RC>(rk, a.k, a.kpad, 0u, L, outbuf);
  if (THR) {
    // the k-th largest score = the smallest selected key's score (fewer than k live entries: the smallest of all; none: -inf)
    unsigned long long m = tid < want ? outbuf[tid] : ~0ull;  // want <= kpad <= 128 <= SL_THREADS
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const unsigned long long o = __shfl_xor(m, off);
      m = o < m ? o : m;
    }
    if ((tid & 63) == 0) reinterpret_cast<unsigned long long*>(L.hist)[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) {
      const unsigned long long* w4 = reinterpret_cast<const unsigned long long*>(L.hist);
      unsigned long long mm = w4[0];
      for (int i = 1; i < SL_THREADS / 64; ++i) mm = w4[i] < mm ? w4[i] : mm;
      const float t = want > 0 ? sel_score(mm) : -INFINITY;
      a.thr[q] = a.sub ? t - a.sub[q] : t;
      a.cnt[(int64_t)q * CNT_STRIDE] = a.n_slots;  // survivors of the filter pass are appended behind the sample block
      a.cnt[(int64_t)q * CNT_STRIDE + 1] = 0;      // both tickets ready for their next use (the select form's: this call)
      a.cnt[(int64_t)q * CNT_STRIDE + 2] = 0;
    }
    return;
  }
  wave0_bitonic_desc(outbuf, a.kpad);
  __syncthreads();
  for (int i = tid; i < a.k; i += SL_THREADS) {
    const unsigned long long key = outbuf[i];
    float val = -INFINITY;
    int32_t id = -1;
    if (i < want && key != 0ull) {
      val = sel_score(key);
      id = (int32_t)sel_low(key) + a.idx_offset;
    }
    a.out_val[(int64_t)q * a.k + i] = val;
    a.out_idx[(int64_t)q * a.k + i] = id;
  }
  if (tid == 0) {
    const int c = a.cnt[(int64_t)q * CNT_STRIDE];
    if (a.status) a.status[q] = c > (int)a.cap ? 1 : 0;  // list overflowed: result is a subset's top-k
    a.cnt[(int64_t)q * CNT_STRIDE + 2] = 0;
  }
}

// slices for a list of up to `len` entries: ~1 024 entries (4 per thread) each, at most SL_NS_MAX; 0 = not served
static int sliced_ns(int64_t len, int kpad) {
  if (kpad > SL_KPAD_MAX || len > (int64_t)SL_NS_MAX * SL_RC * SL_THREADS) return 0;
  int ns = (int)((len + 1023) / 1024);
  const int need = (int)((len + SL_RC * SL_THREADS - 1) / (SL_RC * SL_THREADS));
  if (ns < need) ns = need;
  if (ns < 1) ns = 1;
  if (ns > SL_NS_MAX) ns = SL_NS_MAX;
  while ((int64_t)ns * kpad > SL_RC * SL_THREADS) --ns;  // the merge holds NS x kpad keys in registers
  return ns >= need ? ns : 0;
}

// ---- k beyond 1024 ------------------------------------------------------------------------------------------------------------
// gdr_sim_topk[_bf16], gdr_topk_merge, gdr_topk_pack and gdr_topk_merge_packed take k up to one LDS sort (select.h SEL_SORT_MAX); the
// pre-filter stops where its one-workgroup tail does (it sorts 4k band keys in LDS and rescores them in fp32).
constexpr int SIM_TOPK_MAX_K = SEL_SORT_MAX, SIM_ONE_WAVE_MAX_K = 1024, PREFILTER_MAX_K = 1024;

// The one launch of topk_select_kernel<MERGE>, one workgroup per query.  k <= 1024: the one-wave sort, `threads` lanes (the caller's:
// 1024 for a candidate list, SEL_THREADS for a merge), kpad = sel_pow2(k, 1).  1024 < k <= SIM_TOPK_MAX_K: DEEP = true, kpad = 2048 ..
// 8192 keys of dynamic LDS, DEEP_THREADS lanes whatever the caller runs below.  The merge form runs 256 threads at k <= 1024; here
// 1024 won: 0.056 / 0.106 / 0.187 ms at 1024 / 512 / 256 threads for (G, B, k) = (8, 64, 2048), 0.303 / 0.413 / 0.757 ms at k = 8192
// (16 384 keys fit 1024 threads' register cache, and the sort has 16 waves).  kpad is a multiple of 2 x 16 waves, as bitonic_desc asks.
// what / what_deep: the kernel's name in a launch error of the two forms.
constexpr int DEEP_THREADS = 1024;
template <bool MERGE>
static int launch_select(const float* vals, const int32_t* idxs, const int32_t* cnt, int64_t cap, int G, int B, int k, int32_t idx_offset,
                         const float* thr, float* out_val, int32_t* out_idx, int32_t* status, int rs, int es, int threads, const char* what,
                         const char* what_deep, hipStream_t stream) {
  if (k > SIM_ONE_WAVE_MAX_K) {
    const int kpad = sel_pow2(k, 2048);
    auto* kern = topk_select_kernel<MERGE, true>;
    if (int rc = ensure_dyn_lds(reinterpret_cast<const void*>(kern), SEL_SORT_MAX * 8, what_deep)) return rc;
    hipLaunchKernelGGL(kern, dim3(B), dim3(DEEP_THREADS), (size_t)kpad * sizeof(unsigned long long), stream, vals, idxs, cnt, cap, G, B, k,
                       kpad, idx_offset, thr, out_val, out_idx, status, rs, es);
    GDR_CHECK_LAUNCH(what_deep);
    return GDR_OK;
  }
  const int kpad = sel_pow2(k, 1);
  hipLaunchKernelGGL(topk_select_kernel<MERGE>, dim3(B), dim3(threads), kpad * sizeof(unsigned long long), stream, vals, idxs, cnt, cap, G,
                     B, k, kpad, idx_offset, thr, out_val, out_idx, status, rs, es);
  GDR_CHECK_LAUNCH(what);
  return GDR_OK;
}

// ---- GDR_SIM_LIVE_MASK: the top-k over the live rows only ---------------------------------------------------------------------
// The caller's bitmap (bit r % 32 of word r / 32 = row r is live) sits in front of the plan's scratch and is only read.  The mask
// is applied to the CANDIDATE LISTS between the existing passes, not in the epilogues that fill them: the selects already skip
// id < 0 and radix_kth_key already ignores -inf scores, so a dead entry rewritten to (-inf, -1) is padding to every kernel behind
// it.   sample -> mask [0, n_slots) -> threshold -> (fix-up) -> filter -> mask [n_slots, cnt) -> select.
// The threshold is then the k-th largest LIVE sample score: a lower bound of the k-th largest live score overall, by the argument
// at the top of this file applied to the live rows.  The filter pass still appends dead rows that reach it; the second mask drops
// them, and a list they overflow is reported through status like any other.
static size_t live_mask_bytes(int64_t N) {
  return align_up((size_t)((N + 31) / 32) * sizeof(uint32_t), 256);
}
// The bitmaps at the head of a workspace, from the call's flags: one of live_mask_bytes(N) (GDR_SIM_LIVE_MASK, read by every query:
// qstride 0) or B of them (GDR_SIM_QUERY_MASK, the gather mode included: query q's at word q * qstride).  Everything else the call
// lays out — make_plan's `base`, the gather layout — starts `bytes` in.
struct MaskHead {
  size_t bytes;     // 0 without either flag
  int64_t qstride;  // 32-bit words between two queries' bitmaps
  bool masked;
};
static MaskHead mask_head(int flags, int B, int64_t N) {
  const bool per_query = (flags & GDR_SIM_QUERY_MASK) != 0;
  MaskHead h{};
  h.masked = per_query || (flags & GDR_SIM_LIVE_MASK) != 0;
  h.bytes = h.masked ? (per_query ? (size_t)B : 1) * live_mask_bytes(N) : 0;
  h.qstride = per_query ? (int64_t)(live_mask_bytes(N) / sizeof(uint32_t)) : 0;
  return h;
}

// GDR_SIM_ROW_GATHER (sim_rows.hip): bits 8..16 of flags hold the per-query list capacity in chunks of SEL_CHUNK rows, 0 reads as 2.
constexpr int SIM_GATHER_CHUNK_BITS = 0x1FF << 8, SIM_GATHER_MAX_CHUNKS = 256;
// rows per query of a gather call; 0 = no such call (a field above 256 chunks, or a field without the flag)
static int64_t sim_gather_cap(int flags) {
  const int c = (flags & SIM_GATHER_CHUNK_BITS) >> 8;
  if (!(flags & GDR_SIM_ROW_GATHER) || c > SIM_GATHER_MAX_CHUNKS) return 0;
  return (int64_t)SEL_CHUNK * (c ? c : 2);
}

constexpr int MASK_THREADS = 256;
// GDR_SIM_QUERY_MASK is the same sequence with a bitmap PER QUERY: B bitmaps of live_mask_bytes(N) each in front of the plan, bitmap
// q at word q * qstride.  The mask pass reads list q against bitmap q (qstride = 0: the one bitmap of GDR_SIM_LIVE_MASK, the special
// case where every query's bitmap is the same), and the fix-up counts per query.  A workgroup of the mask pass works on one query
// at a time (blockIdx.y), so its bitmap reads stay inside one 40 KB region (N = 320 000) that L2 keeps.
// Entries [lo, hi) of every query's list (blockIdx.y strides the queries), hi = hi_fixed (the sample block: the counter is not set yet) or, with hi_fixed < 0,
// min(cnt[q], cap): an entry whose row is dead becomes (-inf, -1).  A thread takes four consecutive entries — lo and cap are
// multiples of four (of TILE), so a group never leaves the list — loads their ids as one int4, and touches the scores only where
// a row is dead.  Entries of a group past hi are written back as they were read.  An id outside [0, N) cannot reach the bitmap.
__global__ __launch_bounds__(MASK_THREADS) void sim_live_mask_kernel(float* __restrict__ cand_val, int32_t* __restrict__ cand_idx,
                                                                     const int32_t* __restrict__ cnt, int64_t cap, int64_t lo,
                                                                     int64_t hi_fixed, const uint32_t* __restrict__ live,
                                                                     int64_t qstride, int64_t N, int B) {
  const int64_t step = (int64_t)gridDim.x * MASK_THREADS * 4;
  for (int64_t q = blockIdx.y; q < B; q += gridDim.y) {
    int64_t hi = hi_fixed >= 0 ? hi_fixed : (int64_t)cnt[q * CNT_STRIDE];
    if (hi > cap) hi = cap;
    float* cv = cand_val + q * cap;
    int32_t* ci = cand_idx + q * cap;
    const uint32_t* lq = live + q * qstride;
    for (int64_t i = lo + ((int64_t)blockIdx.x * MASK_THREADS + threadIdx.x) * 4; i < hi; i += step) {
      int4 id = *reinterpret_cast<const int4*>(ci + i);
      auto dead = [&](int32_t r, int j) -> bool {
        if (i + j >= hi || r < 0) return false;  // past the list / padding already
        return r >= N || ((lq[r >> 5] >> (r & 31)) & 1u) == 0u;
      };
      const bool d0 = dead(id.x, 0), d1 = dead(id.y, 1), d2 = dead(id.z, 2), d3 = dead(id.w, 3);
      if (d0 || d1 || d2 || d3) {
        float4 v = *reinterpret_cast<const float4*>(cv + i);
        if (d0) v.x = -INFINITY, id.x = -1;
        if (d1) v.y = -INFINITY, id.y = -1;
        if (d2) v.z = -INFINITY, id.z = -1;
        if (d3) v.w = -INFINITY, id.w = -1;
        *reinterpret_cast<float4*>(cv + i) = v;
        *reinterpret_cast<int4*>(ci + i) = id;
      }
    }
  }
}

// Fewer than k live rows in the sample tiles: radix_kth_key clamps `need` to the entries it counted, so thr[q] came out as the
// smallest live sample score — no lower bound of anything, and the select would drop every entry below it with status 0.  The
// live sample count depends on the bitmap and the plan alone (the same for every query): one workgroup counts it and, if it is
// short, lowers every thr[q] to -inf.  The filter pass then keeps every row: either the whole corpus fits the list (exact), or the
// list overflows and status[q] = 1 sends the query to the exhaustive re-run, as for any overflow.
// qstride > 0 (GDR_SIM_QUERY_MASK): the count is a property of query q's own bitmap, so workgroup q (a grid of B) counts bitmap q and
// lowers thr[q] alone — a query with a narrow filter must not cost the others their thresholds, and a single count over any one
// bitmap would say nothing about the rest.
__global__ __launch_bounds__(256) void sim_live_thr_fixup_kernel(const uint32_t* __restrict__ live, int64_t qstride, int64_t N,
                                                                 int64_t n_sample_tiles, int stride, int k, float* __restrict__ thr,
                                                                 int B) {
  __shared__ int red[4];
  live += (int64_t)blockIdx.x * qstride;
  const int64_t n_words = (N + 31) / 32;
  int c = 0;
  for (int64_t e = threadIdx.x; e < n_sample_tiles * (TILE / 32); e += 256) {
    const int64_t w = (e / (TILE / 32)) * stride * (TILE / 32) + e % (TILE / 32);
    if (w < n_words) c += __popc(bitmap_word(live, w, N));
  }
  c = wave_sum(c);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
  __syncthreads();
  if (red[0] + red[1] + red[2] + red[3] >= k) return;
  if (qstride) {
    if (threadIdx.x == 0) thr[blockIdx.x] = -INFINITY;
    return;
  }
  for (int q = threadIdx.x; q < B; q += 256) thr[q] = -INFINITY;
}

static int launch_live_mask(const SimEpilogue& ep, const SimPlan& p, int B, int64_t lo, int64_t hi_fixed, const uint32_t* live,
                            int64_t qstride, int64_t N, hipStream_t stream) {
  const int64_t span = (hi_fixed >= 0 ? hi_fixed : p.cap) - lo;
  if (span <= 0) return GDR_OK;
  int64_t gx = (span + MASK_THREADS * 4 - 1) / (MASK_THREADS * 4);
  if (gx > 64) gx = 64;
  hipLaunchKernelGGL(sim_live_mask_kernel, dim3((unsigned)gx, (unsigned)(B < 65535 ? B : 65535)), dim3(MASK_THREADS), 0, stream, ep.cand_val,
                     ep.cand_idx, (const int32_t*)ep.cand_cnt, p.cap, lo, hi_fixed, live, qstride, N, B);
  GDR_CHECK_LAUNCH("sim_live_mask_kernel");
  return GDR_OK;
}

// ---- THE candidate-pass sequence: steps 1 - 3 of the top of this file, with the row mask between them ----------------------------
//   sample -> [mask [0, n_slots)] -> threshold -> ( [fix-up] -> filter -> [mask [n_slots, cnt)] )   (...) where p.stride > 1, [...] where
// head.masked.  Every top-k entry point over a corpus runs it, once, and differs only in what it hands in and in the tail it puts behind:
//   sim_topk_impl    D, Q as given (fp32 or bf16), stream_mode by the shape and GDR_SIM_NO_STREAM; sub = null; the sliced threshold where
//                    the stream kernels ran; then its select.
//   prefilter_impl   the bf16 image and the bf16 queries of sim_qprep_kernel; sub = eps2 (the filter pass keeps s~ >= L - 2 eps_q);
//                    never sliced; then prefilter_tail_kernel.
// ws: the workspace (the bitmaps of `head` at its start, the plan p laid out behind head.bytes).  ns_thr: the slices of the threshold, 0 =
// sim_threshold_kernel with one 1024-thread workgroup per query; sa (needed with ns_thr > 0, filled here with the lists in any case): the
// caller's SlicedArgs, its k / kpad and output side set.  ep, thr: the lists and thresholds the passes left, for the caller's tail.
static int run_candidate_passes(const void* D, const void* Q, bool bf16, bool stream_mode, int B, int64_t N, int d, const SimPlan& p,
                                const MaskHead& head, char* ws, int k, const float* sub, int ns_thr, SlicedArgs* sa, hipStream_t stream,
                                SimEpilogue& ep, float*& thr) {
  const uint32_t* live = head.masked ? reinterpret_cast<const uint32_t*>(ws) : nullptr;
  ep = SimEpilogue{};
  ep.cand_val = reinterpret_cast<float*>(ws + p.off_val);
  ep.cand_idx = reinterpret_cast<int32_t*>(ws + p.off_idx);
  ep.cand_cnt = reinterpret_cast<int32_t*>(ws + p.off_cnt);
  thr = reinterpret_cast<float*>(ws + p.off_thr);
  ep.thr = thr;
  ep.status = nullptr;  // overflow is reported per query by the caller's tail (cnt > cap)
  ep.cap = (int32_t)p.cap;
  ep.tile_stride = p.stride;
  const auto core_pass = [&](int mode) {
    ep.mode = mode;
    return stream_mode ? launch_sim_stream(D, N, Q, B, d, ep, bf16, stream) : launch_sim_gemm(D, N, Q, B, d, ep, bf16, stream);
  };
  GDR_TRY(core_pass(1));
  if (head.masked) GDR_TRY(launch_live_mask(ep, p, B, 0, p.n_slots, live, head.qstride, N, stream));  // the threshold sees allowed sample scores only
  if (sa) {
    sa->vals = ep.cand_val, sa->idxs = ep.cand_idx, sa->cnt = ep.cand_cnt, sa->cap = p.cap, sa->n_slots = (int)p.n_slots, sa->k = k;
    sa->thr = thr, sa->sub = sub, sa->part = reinterpret_cast<unsigned long long*>(ws + p.off_part);
  }
  if (ns_thr) {
    sa->NS = ns_thr;
    ProfScope prof(PROF_SELECT, 0.0, stream);
    hipLaunchKernelGGL(sim_sliced_select_kernel<true>, dim3(B * ns_thr), dim3(SL_THREADS), 0, stream, *sa);
    GDR_CHECK_LAUNCH("sim_sliced_select_kernel(threshold)");
  } else {
    // 1024 lanes per query: measured faster than 512 with twice the entries per lane (26.7 vs 37.7 us at 32 queries)
    hipLaunchKernelGGL(sim_threshold_kernel, dim3(B), dim3(1024), 0, stream, ep.cand_val, p.cap, (int)p.n_slots, k, thr, ep.cand_cnt, sub);
    GDR_CHECK_LAUNCH("sim_threshold_kernel");
  }
  if (p.stride > 1) {
    if (head.masked) {  // fewer than k allowed sample rows (per query: of query q's bitmap): thr[q] = -inf (sim_live_thr_fixup_kernel)
      hipLaunchKernelGGL(sim_live_thr_fixup_kernel, dim3(head.qstride ? B : 1), dim3(256), 0, stream, live, head.qstride, N,
                         p.n_sample_tiles, p.stride, k, thr, B);
      GDR_CHECK_LAUNCH("sim_live_thr_fixup_kernel");
    }
    GDR_TRY(core_pass(2));
    if (head.masked) GDR_TRY(launch_live_mask(ep, p, B, p.n_slots, -1, live, head.qstride, N, stream));  // the survivors, disallowed rows among them
  }
  return GDR_OK;
}

// What gdr_sim_topk[_bf16] and the two pre-filter entry points check alike, in one order (a call with several faults is refused for
// the first).  who: the message prefix.  pre (the pre-filter): D_bf16 and dnorm_max are arguments too, d % 8 == 0 and d <= 1024, k stops
// at PREFILTER_MAX_K.  d8: the rows are bf16 (d % 8 == 0 for 16-byte pieces).
static int check_search_args(const char* who, bool pre, bool d8, const void* Q, int B, const void* D, const void* D_bf16, float dnorm_max,
                             int64_t N, int d, int k, int32_t idx_offset, const float* out_val, const int32_t* out_idx,
                             const void* workspace) {
  GDR_CHECK_ARG(Q && D && (!pre || D_bf16) && out_val && out_idx && workspace, "%s: null pointer", who);
  GDR_CHECK_ARG(B > 0 && N > 0 && d > 0 && d % (d8 ? 8 : 4) == 0 && (!pre || d <= 1024), "%s: bad shape B=%d N=%lld d=%d%s", who, B,
                (long long)N, d, pre ? " (d % 8 == 0, d <= 1024)" : "");
  const int k_max = pre ? PREFILTER_MAX_K : SIM_TOPK_MAX_K;
  GDR_CHECK_ARG(k >= 1 && k <= k_max && k <= N, "%s: k=%d must be in [1, min(%d, N)]", who, k, k_max);
  GDR_CHECK_ARG(N < 0x7fffffffLL - 256, "%s: shard too large for int32 doc ids", who);
  GDR_CHECK_ARG((int64_t)idx_offset + N <= 0x7fffffffLL,
                "%s: idx_offset=%d + N=%lld leaves int32 doc ids (the largest id, idx_offset + N - 1, must be < 2^31 - 1)", who,
                (int)idx_offset, (long long)N);
  if (pre) GDR_CHECK_ARG(dnorm_max > 0.f && dnorm_max < INFINITY, "%s: dnorm_max must be the largest row norm of D (> 0, finite)", who);
  GDR_CHECK_ARG(((uintptr_t)Q & 15) == 0 && ((uintptr_t)D & 15) == 0 && (!pre || ((uintptr_t)D_bf16 & 15) == 0) && ((uintptr_t)workspace & 255) == 0,
                "%s: Q, D%s must be 16-byte and workspace 256-byte aligned", who, pre ? ", D_bf16" : "");
  return GDR_OK;
}

// The largest total(k') over k' <= k, where total(k') is the bytes of a plan of depth k' (make_plan's, or one built on it): what the
// workspace questions answer (see gdr_sim_topk_workspace_bytes for why, and for where the candidates sit).
template <class Total>
static size_t largest_plan_up_to(int64_t N, int k, Total total) {
  size_t best = total(k);
  double target = sqrt((double)k * (double)N);
  if (target < k) target = k;
  const int64_t ts_k = (int64_t)((target + TILE - 1) / TILE);
  for (int64_t ts = 1; ts <= ts_k; ++ts) {
    const double edge = (double)(ts * TILE);
    const int64_t ends[2] = {(int64_t)(edge * edge / (double)N), ts * TILE};
    for (const int64_t e : ends)
      for (int64_t kk = e - 1; kk <= e + 1; ++kk)
        if (kk >= 1 && kk < k) {
          const size_t t = total((int)kk);
          if (t > best) best = t;
        }
  }
  return best;
}

}  // namespace gdr

// The size a caller is told: the largest plan of any k' <= k, so that the answer never shrinks when k grows and a buffer sized for
// the deepest list of a caller serves its shallower ones.  make_plan itself — what a call of depth k lays out and checks its
// workspace against — is not monotone: each time a larger k lowers the sample stride by one the sample block grows by a step while
// the survivor term 4 k N / n_sample shrinks, and the sum dips by 1 - 2 %.  With the sample tile count ts fixed the plan only grows
// with k, so the maximum sits at the last k of one of the ts values up to k's: k' ~ (128 ts)^2 / N (or 128 ts once k' > N), looked
// at with its two neighbours, since the boundary comes out of a rounded square root.
extern "C" size_t gdr_sim_topk_workspace_bytes(int B, int64_t N, int d, int k, int flags) {
  (void)d;
  if (B <= 0 || N <= 0 || k <= 0) return 0;
  const bool exhaustive = (flags & GDR_SIM_EXHAUSTIVE) != 0;
  if (flags & (GDR_SIM_ROW_GATHER | gdr::SIM_GATHER_CHUNK_BITS)) {  // the B bitmaps, then the gather layout: no N, no d behind them
    const int64_t cap = gdr::sim_gather_cap(flags);
    if (cap == 0 || (flags & (GDR_SIM_QUERY_MASK | GDR_SIM_LIVE_MASK | GDR_SIM_EXHAUSTIVE)) != GDR_SIM_QUERY_MASK ||
        (cap > 2 * gdr::SEL_CHUNK && k > gdr::SIM_ONE_WAVE_MAX_K))
      return 0;  // no such call: gdr_sim_topk refuses it
    return gdr::mask_head(flags, B, N).bytes + gdr::sim_rows_workspace_bytes(B, cap, k);
  }
  if ((flags & GDR_SIM_LIVE_MASK) && (flags & GDR_SIM_QUERY_MASK)) return 0;  // no such call: gdr_sim_topk refuses the pair
  const gdr::MaskHead head = gdr::mask_head(flags, B, N);
  if (head.masked)  // the caller's row bitmap, or one per query, in front of the same plan
    return gdr_sim_topk_workspace_bytes(B, N, d, k, flags & ~(GDR_SIM_LIVE_MASK | GDR_SIM_QUERY_MASK)) + head.bytes;
  if (exhaustive) return gdr::make_plan(B, N, k, true).total;  // stride 1 whatever k: the plan does not depend on k
  return gdr::largest_plan_up_to(N, k, [&](int kk) { return gdr::make_plan(B, N, kk, false).total; });
}

namespace gdr {
__global__ __launch_bounds__(256) void cast_f32_bf16_kernel(const float4* __restrict__ in, uint2* __restrict__ out,
                                                            int64_t n4) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const float4 v = in[i];
  store_bf16x4(out + i, v);
}

static int sim_topk_impl(const void* Q, int B, const void* D, int64_t N, int d, int k, int32_t idx_offset, float* out_val,
                         int32_t* out_idx, int32_t* status, int flags, void* workspace, size_t workspace_bytes,
                         bool bf16, hipStream_t stream);
}  // namespace gdr

namespace gdr {
int launch_cast_f32_bf16(const float* in, void* out_bf16, int64_t n, hipStream_t stream) {
  if (n == 0) return GDR_OK;
  GDR_CHECK_ARG(in && out_bf16 && n >= 0 && n % 4 == 0, "cast: null pointer or n %% 4 != 0");
  GDR_CHECK_ARG(((uintptr_t)in & 15) == 0 && ((uintptr_t)out_bf16 & 7) == 0, "cast: misaligned pointer");
  if (n == 0) return GDR_OK;
  hipLaunchKernelGGL(cast_f32_bf16_kernel, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, stream,
                     reinterpret_cast<const float4*>(in), reinterpret_cast<uint2*>(out_bf16), n / 4);
  GDR_CHECK_LAUNCH("cast_f32_bf16_kernel");
  return GDR_OK;
}
}  // namespace gdr

extern "C" int gdr_cast_f32_bf16(const float* in, void* out_bf16, int64_t n, void* stream_) {
  return gdr::launch_cast_f32_bf16(in, out_bf16, n, static_cast<hipStream_t>(stream_));
}

extern "C" int gdr_sim_topk(const float* Q, int B, const float* D, int64_t N, int d, int k, int32_t idx_offset,
                            float* out_val, int32_t* out_idx, int32_t* status, int flags, void* workspace,
                            size_t workspace_bytes, void* stream_) {
  return gdr::sim_topk_impl(Q, B, D, N, d, k, idx_offset, out_val, out_idx, status, flags, workspace, workspace_bytes,
                            false, static_cast<hipStream_t>(stream_));
}

extern "C" int gdr_sim_topk_bf16(const void* Q, int B, const void* D, int64_t N, int d, int k, int32_t idx_offset,
                                 float* out_val, int32_t* out_idx, int32_t* status, int flags, void* workspace,
                                 size_t workspace_bytes, void* stream_) {
  return gdr::sim_topk_impl(Q, B, D, N, d, k, idx_offset, out_val, out_idx, status, flags, workspace, workspace_bytes,
                            true, static_cast<hipStream_t>(stream_));
}

int gdr::sim_topk_impl(const void* Q, int B, const void* D, int64_t N, int d, int k, int32_t idx_offset,
                       float* out_val, int32_t* out_idx, int32_t* status, int flags, void* workspace,
                       size_t workspace_bytes, bool bf16, hipStream_t stream) {
  if (B == 0) return GDR_OK;  // empty query batch
  GDR_TRY(check_search_args("sim_topk", false, bf16, Q, B, D, nullptr, 0.f, N, d, k, idx_offset, out_val, out_idx, workspace));
  GDR_CHECK_ARG((flags & (GDR_SIM_LIVE_MASK | GDR_SIM_QUERY_MASK)) != (GDR_SIM_LIVE_MASK | GDR_SIM_QUERY_MASK),
                "sim_topk: GDR_SIM_LIVE_MASK and GDR_SIM_QUERY_MASK name two workspace layouts: AND the live rows into the per-query "
                "bitmaps on the caller's side and pass GDR_SIM_QUERY_MASK alone");
  // GDR_SIM_ROW_GATHER: score only the rows bitmap q allows (sim_rows.hip).  No GEMM core runs, so GDR_SIM_NO_STREAM means nothing here.
  if (flags & (GDR_SIM_ROW_GATHER | SIM_GATHER_CHUNK_BITS)) {
    const int chunks = (flags & SIM_GATHER_CHUNK_BITS) >> 8;
    GDR_CHECK_ARG(flags & GDR_SIM_ROW_GATHER, "sim_topk: GDR_SIM_GATHER_CHUNKS(%d) without GDR_SIM_ROW_GATHER: bits 8..16 of flags belong to that mode", chunks);
    GDR_CHECK_ARG(!(flags & GDR_SIM_LIVE_MASK), "sim_topk: GDR_SIM_ROW_GATHER with GDR_SIM_LIVE_MASK: AND the live rows into the per-query bitmaps and "
                  "pass GDR_SIM_QUERY_MASK | GDR_SIM_ROW_GATHER");
    GDR_CHECK_ARG(flags & GDR_SIM_QUERY_MASK, "sim_topk: GDR_SIM_ROW_GATHER needs GDR_SIM_QUERY_MASK: the rows it scores are the ones the per-query bitmaps allow");
    GDR_CHECK_ARG(!(flags & GDR_SIM_EXHAUSTIVE), "sim_topk: GDR_SIM_ROW_GATHER with GDR_SIM_EXHAUSTIVE: the gather list is already every allowed row; "
                  "the exhaustive re-run of a query that allows more than its capacity is GDR_SIM_EXHAUSTIVE | GDR_SIM_QUERY_MASK");
    GDR_CHECK_ARG(chunks <= SIM_GATHER_MAX_CHUNKS, "sim_topk: GDR_SIM_ROW_GATHER: GDR_SIM_GATHER_CHUNKS(%d) must be in [0, %d] (0 = 2)", chunks, SIM_GATHER_MAX_CHUNKS);
    const int64_t cap = sim_gather_cap(flags);
    GDR_CHECK_ARG(cap <= 2 * SEL_CHUNK || k <= SIM_ONE_WAVE_MAX_K, "sim_topk: GDR_SIM_ROW_GATHER: k=%d must be <= %d with GDR_SIM_GATHER_CHUNKS(%d) > 2 "
                  "(chunks plus merge rounds; one LDS sort serves any k at 1 or 2 chunks)", k, SIM_ONE_WAVE_MAX_K, chunks);
    GDR_CHECK_ARG((int64_t)B * (cap / 16) <= 0x7fffffffLL, "sim_topk: GDR_SIM_ROW_GATHER: B=%d x %lld rows per query leaves the int32 unit list", B, (long long)cap);
    const MaskHead head = mask_head(flags, B, N);  // the B bitmaps
    const size_t required = head.bytes + sim_rows_workspace_bytes(B, cap, k);
    if (workspace_bytes < required) {
      set_error("sim_topk: workspace %zu < required %zu", workspace_bytes, required);
      return GDR_ENOSPC;
    }
    return launch_sim_rows(Q, B, D, N, d, k, idx_offset, out_val, out_idx, status, static_cast<const uint32_t*>(workspace), head.qstride, cap,
                           static_cast<char*>(workspace) + head.bytes, bf16, stream);
  }
  // GDR_SIM_LIVE_MASK: the first live_mask_bytes(N) bytes of the workspace are the caller's row bitmap (read only); the plan sits behind it.
  // GDR_SIM_QUERY_MASK: B such bitmaps, query q's at byte q * live_mask_bytes(N).
  const MaskHead head = mask_head(flags, B, N);
  const SimPlan p = make_plan(B, N, k, (flags & GDR_SIM_EXHAUSTIVE) != 0, 1.0, head.bytes);
  // A masked call is held to the size its caller was told, not to this k's own layout (which may dip below the unflagged answer,
  // see gdr_sim_topk_workspace_bytes): a buffer sized without the flag — no room reserved for the bitmap — is refused at every shape.
  const size_t required = head.masked ? gdr_sim_topk_workspace_bytes(B, N, d, k, flags) : p.total;
  if (workspace_bytes < required) {
    set_error("sim_topk: workspace %zu < required %zu", workspace_bytes, required);
    return GDR_ENOSPC;
  }
  const bool stream_mode = sim_stream_supported(B, d, bf16) && !(flags & GDR_SIM_NO_STREAM);
  static const bool sliced_on = env_flag("GDR_SIM_SLICED", true);  // A/B knob: 0 = one workgroup per query for the threshold / select tails (the r05 form)
  // the stream kernels' sample pass zeroes the tickets: only their calls may take the sliced tails
  const bool sliced = stream_mode && sliced_on && B <= 32;
  const int kpad = sel_pow2(k, 1);
  const int ns_thr = sliced ? sliced_ns(p.n_slots, kpad) : 0, ns_sel = sliced ? sliced_ns(p.cap, kpad) : 0;
  SlicedArgs sa{};  // the output side; run_candidate_passes adds the lists
  sa.kpad = kpad, sa.idx_offset = idx_offset, sa.out_val = out_val, sa.out_idx = out_idx, sa.status = status;
  SimEpilogue ep;
  float* thr;
  GDR_TRY(run_candidate_passes(D, Q, bf16, stream_mode, B, N, d, p, head, static_cast<char*>(workspace), k, nullptr, ns_thr, &sa, stream, ep, thr));
  // step 4: the exact top-k of every list, overflow (cnt > cap) to status
  if (ns_sel) {
    sa.NS = ns_sel;
    ProfScope prof(PROF_SELECT, 0.0, stream);
    hipLaunchKernelGGL(sim_sliced_select_kernel<false>, dim3(B * ns_sel), dim3(SL_THREADS), 0, stream, sa);
    GDR_CHECK_LAUNCH("sim_sliced_select_kernel(select)");
    return GDR_OK;
  }
  return launch_select<false>(ep.cand_val, ep.cand_idx, ep.cand_cnt, p.cap, 1, B, k, idx_offset, thr, out_val, out_idx, status, 0, 1, 1024,
                              "topk_select_kernel", "topk_select_kernel<deep>", stream);
}

namespace gdr {
// ------------------------------------------------------------------------------------------------------------------------------
// fp32 similarity + top-k through a bf16 PRE-FILTER (r05; B > 32): the corpus-wide pass — 2·B·N·d flop, the second largest item of
// the C2 step — runs on the bf16 MFMA path over a bf16 image of the corpus, and only a few hundred docs per query are scored in
// fp32.  The result is the top-k of the FP32 scores, exactly, for every input; the bf16 pass only decides which docs get an fp32 score:
//   * s(doc) = the fp32 score the rescoring computes, s~(doc) = the bf16-operand score (products of bf16 values are exact in fp32,
//     fp32 accumulate).  bf16 keeps 8 significand bits (1 implicit + 7 stored), so round-to-nearest-even has unit roundoff u = 2^-8
//     (r05 coded 2^-9 — half the true bound; r06 fix, tests/test_gpu_prefilter.py holds a coherent-rounding input that needs it).
//     For any summation orders:
//         |s~ - s| <= ||q||·||d||·(2u + u^2 + 2·d·2^-24·1.01) =: eps(q, d) <= eps_q := ||q||·max_doc||d||·(2^-7 + 2^-16 + d·2^-22)
//   * t~_k = k-th largest s~ over all docs.  The k docs with the largest s~ have s >= t~_k - eps, so T_k (k-th largest s) >= t~_k - eps;
//     a doc of the true top-k has s >= T_k, hence s~ >= t~_k - 2·eps.  So {s~ >= t~_k - 2 eps_q} contains the true top-k (with every doc
//     tied at T_k), and the exact select over their fp32 scores (higher score, then lower id — as the fp32 path) is the brute-force result.
//   * the sample threshold L (k-th largest s~ over the sample) is <= t~_k, so the filter pass keeps s~ >= L - 2 eps_q, a superset.
// Lists that overflow (the candidate list of the bf16 pass, or more than cap2 docs inside the 2-eps band) are flagged in status[q] like
// gdr_sim_topk's; ops.sim_topk recomputes such a query on the fp32 path.
// MASKED (gdr_sim_topk_prefilter_masked: a live-row bitmap, or one bitmap per query): the argument holds verbatim with "docs" read as
// "allowed docs" — t~_k and T_k are then the k-th largest s~ / s over the rows query q's bitmap allows, eps_q needs max ||d|| over
// those rows only (any upper bound widens the band, never breaks it), and the sample threshold L is the k-th largest ALLOWED sample
// score, which is <= the k-th largest allowed s~.  L taken over all sample rows would not do: with a query's best rows disallowed it
// lies above t~_k - 2 eps_q of the allowed rows, and the filter pass would drop docs of the answer.  So the bitmap is applied where
// gdr_sim_topk's GDR_SIM_LIVE_MASK applies it, by the same code: run_candidate_passes, which both entry points call (the mask over the
// sample block before the threshold and over the survivors behind the filter pass, the fix-up where fewer than k allowed sample rows
// leave no threshold) — and the tail below runs unchanged: radix_kth_key ignores -inf scores, the band gather skips id < 0, so a
// masked entry is padding to it.
__global__ __launch_bounds__(256) void sim_qprep_kernel(const float* __restrict__ Q, int d, float dnorm_max, __bf16* __restrict__ Q16,
                                                        float* __restrict__ eps2) {
  __shared__ float red[4];
  const int q = blockIdx.x;
  const float* row = Q + (int64_t)q * d;
  float ss = 0.f;
  for (int c = threadIdx.x * 4; c < d; c += 1024) {
    const float4 v = *reinterpret_cast<const float4*>(row + c);
    ss = fmaf(v.x, v.x, fmaf(v.y, v.y, fmaf(v.z, v.z, fmaf(v.w, v.w, ss))));
    store_bf16x4(reinterpret_cast<uint2*>(Q16 + (int64_t)q * d + c), v);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) ss += __shfl_xor(ss, off);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ss;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float nq = sqrtf(red[0] + red[1] + red[2] + red[3]) * 1.0001f;  // the norm itself is rounded: a hair of slack
    const float c = 0.0078125f + 1.52587890625e-5f + (float)d * 2.384185791015625e-7f;  // 2^-7 + 2^-16 + d * 2^-22  (u_bf16 = 2^-8)
    eps2[q] = 2.0f * nq * dnorm_max * c * 1.01f;
  }
}

// max over rows of ||D[r]||_2^2 (positive floats order like their bit patterns): one wave per row, atomicMax on the bits
__global__ __launch_bounds__(256) void row_norm2_max_kernel(const float* __restrict__ D, int64_t N, int d, unsigned* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  float best = 0.f;
  for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < N; r += (int64_t)gridDim.x * 4) {
    best = fmaxf(best, wave_row_norm2(D + r * d, d, lane, [](int, const float4&) {}));
  }
  if (lane == 0) atomicMax(out, __float_as_uint(best));
}

// The tail of the pre-filter in ONE launch per call (was four: k-th largest of the whole list, gather of the band, rescoring, exact
// select — 75 us of kernels plus three launch gaps at 32 queries): a workgroup per query
//   a. reads its candidate list once (keys cached in registers), radix-selects the k-th largest bf16-operand score t~_k,
//   b. gathers the ids of the entries inside the band s~ >= t~_k - 2 eps_q into LDS,
//   c. scores them in fp32 (a wave per candidate pair: the doc row in coalesced 16-byte pieces, q in registers),
//   d. sorts (fp32 score, ~id) keys in LDS (bitonic, all waves) and writes the first k: higher score, then lower id.
template <int RC>
__global__ __launch_bounds__(1024) void prefilter_tail_kernel(const float* __restrict__ cand_val, const int32_t* __restrict__ cand_idx,
                                                              const int32_t* __restrict__ cand_cnt, int64_t cap, int k, int cap2,
                                                              int cap2p, const float* __restrict__ eps2, const float* __restrict__ Q,
                                                              const float* __restrict__ D, int d, int32_t idx_offset,
                                                              float* __restrict__ out_val, int32_t* __restrict__ out_idx,
                                                              int32_t* __restrict__ status) {
  __shared__ int hist[256];
  __shared__ int scan[256];
  __shared__ int res[2];
  __shared__ uint32_t red[32];
  __shared__ int n_sh;
  extern __shared__ __attribute__((aligned(16))) unsigned long long pkeys[];  // [cap2p]; the ids of the band first live in its upper half
  const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c_all = cand_cnt[(int64_t)q * CNT_STRIDE], count = c_all < (int)cap ? c_all : (int)cap;
  const float* v = cand_val + (int64_t)q * cap;
  const int32_t* ix = cand_idx + (int64_t)q * cap;
  bool cached;
  uint32_t rk[RC];
  const uint32_t kneg = fkey(-INFINITY);
  const float band = fkey_inv(radix_kth_key<1>(v, count, k, 1024, rk, cached, hist, scan, res, red)) - eps2[q];  // t~_k - 2 eps_q
  // ---- b. the band's ids
  int32_t* ids = reinterpret_cast<int32_t*>(pkeys + cap2p / 2);  // [cap2p] ints in the upper half of the key array
  if (tid == 0) n_sh = 0;
  __syncthreads();
  if (cached) {
#pragma unroll
    for (int u = 0; u < RC; ++u) {
      const int i = tid + u * 1024;
      if (rk[u] > kneg && fkey_inv(rk[u]) >= band) {
        const int32_t id = ix[i];
        if (id >= 0) {
          const int p = atomicAdd(&n_sh, 1);
          if (p < cap2) ids[p] = id;
        }
      }
    }
  } else {
    for (int i = tid; i < count; i += 1024) {
      const int32_t id = ix[i];
      if (id >= 0 && v[i] >= band) {
        const int p = atomicAdd(&n_sh, 1);
        if (p < cap2) ids[p] = id;
      }
    }
  }
  __syncthreads();
  const int n_all = n_sh, n2 = n_all < cap2 ? n_all : cap2;
  if (tid == 0 && status) status[q] = (c_all > (int)cap || n_all > cap2) ? 1 : 0;
  // ---- c. fp32 scores of the band (the candidate's slot i keeps its id until its key is written: lane 0 of the owning wave does both)
  {
    constexpr int MAXP = 4;  // d <= 1024
    float4 qr[MAXP];
#pragma unroll
    for (int t = 0; t < MAXP; ++t) {
      const int col = lane * 4 + 256 * t;
      qr[t] = col < d ? *reinterpret_cast<const float4*>(Q + (int64_t)q * d + col) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float* vals = reinterpret_cast<float*>(pkeys);  // [cap2p] floats in the first quarter: disjoint from the ids
    for (int i0 = wave * 2; i0 < n2; i0 += 32) {
      const int i1 = i0 + 1 < n2 ? i0 + 1 : i0;
      const int64_t r0 = ids[i0], r1 = ids[i1];
      float4 a0[MAXP], a1[MAXP];
#pragma unroll
      for (int t = 0; t < MAXP; ++t) {
        const int col = lane * 4 + 256 * t;
        a0[t] = col < d ? *reinterpret_cast<const float4*>(D + r0 * d + col) : make_float4(0.f, 0.f, 0.f, 0.f);
        a1[t] = col < d ? *reinterpret_cast<const float4*>(D + r1 * d + col) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
      float s0 = 0.f, s1 = 0.f;
#pragma unroll
      for (int t = 0; t < MAXP; ++t) {
        s0 = fmaf(qr[t].x, a0[t].x, s0), s0 = fmaf(qr[t].y, a0[t].y, s0), s0 = fmaf(qr[t].z, a0[t].z, s0), s0 = fmaf(qr[t].w, a0[t].w, s0);
        s1 = fmaf(qr[t].x, a1[t].x, s1), s1 = fmaf(qr[t].y, a1[t].y, s1), s1 = fmaf(qr[t].z, a1[t].z, s1), s1 = fmaf(qr[t].w, a1[t].w, s1);
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) s0 += __shfl_xor(s0, off), s1 += __shfl_xor(s1, off);
      if (lane == 0) {
        vals[i0] = s0;
        if (i1 != i0) vals[i1] = s1;
      }
    }
    __syncthreads();
    // ---- d. keys, sort, first k.  Keys are built from (vals, ids) through registers: the key array overlays both
    unsigned long long mykey[4];  // cap2p <= 4096
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = tid + u * 1024;
      mykey[u] = 0ull;
      if (i < n2) mykey[u] = sel_pack(vals[i], (uint32_t)ids[i]);
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = tid + u * 1024;
      if (i < cap2p) pkeys[i] = mykey[u];
    }
    __syncthreads();
  }
  // select.h's network with a workgroup barrier behind every stage: bitonic_desc (wave-local stages) costs this kernel registers
  for (int size = 2; size <= cap2p; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = tid; t < (cap2p >> 1); t += 1024) sel_cmpx(pkeys, t, stride, size);
      __syncthreads();
    }
  }
  for (int i = tid; i < k; i += 1024) {
    const unsigned long long key = pkeys[i];
    float val = -INFINITY;
    int32_t id = -1;
    if (i < n2 && key != 0ull) {
      val = sel_score(key);
      id = (int32_t)sel_low(key) + idx_offset;
    }
    out_val[(int64_t)q * k + i] = val;
    out_idx[(int64_t)q * k + i] = id;
  }
}

static int prefilter_cap2(int k) {
  return sel_pow2(4 * k, 1024);
}
struct PrefilterPlan {
  SimPlan p;
  int cap2;
  size_t off_q16, off_eps, total;
};
// The pre-filter's filter pass keeps s~ >= L - 2 eps_q, not s~ >= L (L: the k-th largest sample score), so it appends more docs than the
// k N / n_sample that make_plan's capacity expects — 3.6 times as many at N = 2.8 M, d = 768, k = 100, where the 4x headroom of the plain
// plan left 2 of 40 queries of a Gaussian corpus with an overflowed list (status 1; 62 .. 91 k entries for 87 k slots:
// tests/test_gpu_large_offsets.py).  For Gaussian scores of deviation |q| sigma (sigma: rms doc entry, sqrt(d) sigma: rms row norm) the
// cut drops from z_L = Q^-1(k / n_sample) by
//   dz = 2 eps_q / (|q| sigma) = 2 sqrt(d) (2^-7 + 2^-16 + d 2^-22) rho,   rho = max ||D[r]|| / rms ||D[r]||,
// and the survivors grow by Q(z_L - dz) / Q(z_L).  Half of that ratio (at least 1) scales the capacity: twice the expected list.
// rho is not known to the host (dnorm_max is, the rms norm is not): 1 for a normalised corpus, 1.13 for 2.8 M Gaussian rows of 768
// entries; 1.25 is taken, so that corpora with moderately uneven norms keep the factor-two margin.  A corpus that is far from this
// model (heavy-tailed scores, one row of a huge norm) costs what it cost before: a flagged query, repaired by the caller.
static double prefilter_survivor_factor(int64_t N, int d, int k) {
  const SimPlan p0 = make_plan(1, N, k, false);
  if (p0.stride == 1) return 1.0;
  const auto Qf = [](double z) { return 0.5 * erfc(z * 0.70710678118654752); };
  const double tail = (double)k / (double)p0.n_slots;
  double lo = -8.0, hi = 8.0;  // Q is decreasing: bisect Q(z) = tail
  for (int it = 0; it < 60; ++it) {
    const double mid = 0.5 * (lo + hi);
    (Qf(mid) > tail ? lo : hi) = mid;
  }
  const double zl = 0.5 * (lo + hi);
  const double dz = 2.0 * sqrt((double)d) * (0x1p-7 + 0x1p-16 + d * 0x1p-22) * 1.25;
  const double f = 0.5 * Qf(zl - dz) / tail;
  return f > 1.0 ? f : 1.0;
}
// base: bytes in front of the plan (the caller's bitmaps of gdr_sim_topk_prefilter_masked), as make_plan's
static PrefilterPlan make_prefilter_plan(int B, int64_t N, int d, int k, size_t base = 0) {
  PrefilterPlan pp{};
  pp.p = make_plan(B, N, k, false, prefilter_survivor_factor(N, d, k), base);
  pp.cap2 = prefilter_cap2(k);
  size_t o = pp.p.total;
  pp.off_q16 = o, o += align_up((size_t)B * d * 2, 256);
  pp.off_eps = o, o += align_up((size_t)B * 4, 256);
  pp.total = o;
  return pp;
}
}  // namespace gdr

extern "C" size_t gdr_sim_topk_prefilter_workspace_bytes(int B, int64_t N, int d, int k) {
  if (B <= 0 || N <= 0 || k <= 0 || d <= 0) return 0;
  // never below what gdr_sim_topk is told for the same call (its answer is the largest plan up to k, see there) plus the bf16 queries
  // and the bands this entry point keeps beside the list
  // Nor below its own answer for any k' <= k: like make_plan, make_prefilter_plan dips (up to 2.8 % at N = 320 000, d = 768) each time a
  // larger k lowers the sample stride by one.  With the sample tile count ts fixed the list only grows with k — the survivor term is
  // max(4 k N / n_sample, 2 N Q(z_L - dz)) with z_L falling as k grows — so the maximum sits at the last k of a ts value, found as in
  // gdr_sim_topk_workspace_bytes.  Every candidate costs a bisection of erfc, several hundred of them a millisecond, and ops.sim_topk
  // asks on every call: the answers are kept (a few shapes per process).
  static std::mutex mu;
  static std::map<std::tuple<int, int64_t, int, int>, size_t> memo;
  const auto key = std::make_tuple(B, N, d, k);
  {
    std::lock_guard<std::mutex> lock(mu);
    const auto it = memo.find(key);
    if (it != memo.end()) return it->second;
  }
  const size_t own = gdr::largest_plan_up_to(N, k, [&](int kk) { return gdr::make_prefilter_plan(B, N, d, kk).total; });
  const size_t plain = gdr_sim_topk_workspace_bytes(B, N, d, k, 0) + gdr::align_up((size_t)B * d * 2, 256) + gdr::align_up((size_t)B * 4, 256);
  const size_t best = own > plain ? own : plain;
  std::lock_guard<std::mutex> lock(mu);
  if (memo.size() >= 4096) memo.clear();
  memo[key] = best;
  return best;
}

extern "C" int gdr_row_norm2_max(const float* D, int64_t N, int d, float* out_dev, void* stream_) {
  using namespace gdr;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  GDR_CHECK_ARG(D && out_dev && N > 0 && d > 0 && d % 4 == 0 && ((uintptr_t)D & 15) == 0, "row_norm2_max: bad arguments");
  if (hipMemsetAsync(out_dev, 0, 4, stream) != hipSuccess) {
    set_error("row_norm2_max: memset failed");
    return GDR_EHIP;
  }
  const int64_t blocks = (N + 3) / 4;
  hipLaunchKernelGGL(row_norm2_max_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, stream, D, N, d,
                     reinterpret_cast<unsigned*>(out_dev));
  GDR_CHECK_LAUNCH("row_norm2_max_kernel");
  return GDR_OK;
}

namespace gdr {
// gdr_sim_topk_prefilter (flags = 0) and gdr_sim_topk_prefilter_masked (flags = GDR_SIM_LIVE_MASK or GDR_SIM_QUERY_MASK: the bitmap(s) at
// the head of the workspace, the plan behind them).  With flags = 0 the launches are what they were before the masked form existed.
static int prefilter_impl(const float* Q, int B, const float* D, const void* D_bf16, float dnorm_max, int64_t N, int d, int k,
                          int32_t idx_offset, float* out_val, int32_t* out_idx, int32_t* status, int flags, void* workspace,
                          size_t workspace_bytes, hipStream_t stream) {
  if (B == 0) return GDR_OK;
  GDR_TRY(check_search_args("sim_topk_prefilter", true, true, Q, B, D, D_bf16, dnorm_max, N, d, k, idx_offset, out_val, out_idx, workspace));
  const MaskHead head = mask_head(flags, B, N);
  const PrefilterPlan pp = make_prefilter_plan(B, N, d, k, head.bytes);
  const SimPlan& p = pp.p;
  // a masked call is held to the size its caller was told (the bitmaps + the unmasked answer, never below this k's own layout)
  const size_t required = head.masked ? gdr_sim_topk_prefilter_masked_workspace_bytes(B, N, d, k, flags) : pp.total;
  if (workspace_bytes < required) {
    set_error("sim_topk_prefilter: workspace %zu < required %zu", workspace_bytes, required);
    return GDR_ENOSPC;
  }
  char* ws = static_cast<char*>(workspace);
  __bf16* Q16 = reinterpret_cast<__bf16*>(ws + pp.off_q16);
  float* eps2 = reinterpret_cast<float*>(ws + pp.off_eps);
  hipLaunchKernelGGL(sim_qprep_kernel, dim3(B), dim3(256), 0, stream, Q, d, dnorm_max, Q16, eps2);
  GDR_CHECK_LAUNCH("sim_qprep_kernel");
  // the passes over the bf16 image (B <= 32: the HBM-bound stream), the threshold lowered to L - 2 eps: the filter pass keeps a superset
  // of the band around the (yet unknown) k-th largest bf16 score
  SimEpilogue ep;
  float* thr;
  GDR_TRY(run_candidate_passes(D_bf16, Q16, true, sim_stream_supported(B, d, true), B, N, d, p, head, ws, k, eps2, 0, nullptr, stream, ep, thr));
  // the tail in one launch: k-th largest bf16-operand score, the band around it, fp32 scores of the band, exact select
  const int cap2p = sel_pow2(pp.cap2, 1024);
  if (int rc__ = ensure_dyn_lds(reinterpret_cast<const void*>(prefilter_tail_kernel<16>), cap2p * 8, "sim_topk_prefilter")) return rc__;
  hipLaunchKernelGGL(prefilter_tail_kernel<16>, dim3(B), dim3(1024), (size_t)cap2p * 8, stream, (const float*)ep.cand_val,
                     (const int32_t*)ep.cand_idx, (const int32_t*)ep.cand_cnt, p.cap, k, pp.cap2, cap2p, (const float*)eps2, Q, D, d,
                     idx_offset, out_val, out_idx, status);
  GDR_CHECK_LAUNCH("prefilter_tail_kernel");
  return GDR_OK;
}

// One wave per listed row: the row's bf16 image (the bits cast_f32_bf16_kernel gives: store_bf16x4) and its squared norm in
// row_norm2_max_kernel's order (wave_row_norm2, which both call), joined by atomicMax on the bits.  A row listed twice is written twice
// with the same bits.  Plain vector stores only.
__global__ __launch_bounds__(256) void prefilter_update_rows_kernel(const float* __restrict__ D, __bf16* __restrict__ D16, int d,
                                                                    const int32_t* __restrict__ rows, int64_t n_rows,
                                                                    unsigned* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  float best = 0.f;
  for (int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); j < n_rows; j += (int64_t)gridDim.x * 4) {
    const int64_t r = rows[j];
    if (r < 0) continue;  // no row: the upper end is the caller's to keep (the call is not told N)
    const float ss = wave_row_norm2(D + r * d, d, lane, [=](int c, const float4& v) {
      store_bf16x4(reinterpret_cast<uint2*>(D16 + r * d + c), v);
    });
    best = fmaxf(best, ss);
  }
  if (lane == 0) atomicMax(out, __float_as_uint(best));
}
}  // namespace gdr

extern "C" int gdr_sim_topk_prefilter(const float* Q, int B, const float* D, const void* D_bf16, float dnorm_max, int64_t N, int d, int k,
                                      int32_t idx_offset, float* out_val, int32_t* out_idx, int32_t* status, void* workspace,
                                      size_t workspace_bytes, void* stream_) {
  return gdr::prefilter_impl(Q, B, D, D_bf16, dnorm_max, N, d, k, idx_offset, out_val, out_idx, status, 0, workspace, workspace_bytes,
                             static_cast<hipStream_t>(stream_));
}

extern "C" size_t gdr_sim_topk_prefilter_masked_workspace_bytes(int B, int64_t N, int d, int k, int flags) {
  if (flags != GDR_SIM_LIVE_MASK && flags != GDR_SIM_QUERY_MASK) return 0;  // no such call: gdr_sim_topk_prefilter_masked refuses it
  const size_t own = gdr_sim_topk_prefilter_workspace_bytes(B, N, d, k);
  if (own == 0) return 0;
  return gdr::mask_head(flags, B, N).bytes + own;
}

extern "C" int gdr_sim_topk_prefilter_masked(const float* Q, int B, const float* D, const void* D_bf16, float dnorm_max, int64_t N, int d,
                                             int k, int32_t idx_offset, float* out_val, int32_t* out_idx, int32_t* status, int flags,
                                             void* workspace, size_t workspace_bytes, void* stream_) {
  using namespace gdr;
  GDR_CHECK_ARG(flags == GDR_SIM_LIVE_MASK || flags == GDR_SIM_QUERY_MASK,
                "sim_topk_prefilter_masked: flags=%d must be exactly GDR_SIM_LIVE_MASK (one row bitmap at the head of the workspace) or "
                "GDR_SIM_QUERY_MASK (one per query): AND the live rows into the per-query bitmaps for both; the exhaustive re-run and the "
                "gather mode are gdr_sim_topk's", flags);
  return prefilter_impl(Q, B, D, D_bf16, dnorm_max, N, d, k, idx_offset, out_val, out_idx, status, flags, workspace, workspace_bytes,
                        static_cast<hipStream_t>(stream_));
}

extern "C" int gdr_prefilter_update_rows(const float* D, void* D_bf16, int d, const int32_t* rows, int64_t n_rows, float* norm2_max_inout,
                                         void* stream_) {
  using namespace gdr;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  GDR_CHECK_ARG(d > 0 && d % 8 == 0 && n_rows >= 0, "prefilter_update_rows: bad shape d=%d (d %% 8 == 0) n_rows=%lld", d, (long long)n_rows);
  if (n_rows == 0) return GDR_OK;
  GDR_CHECK_ARG(D && D_bf16 && rows && norm2_max_inout, "prefilter_update_rows: null pointer");
  GDR_CHECK_ARG(((uintptr_t)D & 15) == 0 && ((uintptr_t)D_bf16 & 15) == 0 && ((uintptr_t)rows & 3) == 0 && ((uintptr_t)norm2_max_inout & 3) == 0,
                "prefilter_update_rows: D, D_bf16 must be 16-byte aligned");
  const int64_t blocks = (n_rows + 3) / 4;
  hipLaunchKernelGGL(prefilter_update_rows_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, stream, D,
                     static_cast<__bf16*>(D_bf16), d, rows, n_rows, reinterpret_cast<unsigned*>(norm2_max_inout));
  GDR_CHECK_LAUNCH("prefilter_update_rows_kernel");
  return GDR_OK;
}

extern "C" int gdr_topk_merge(const float* vals, const int32_t* idx, int G, int B, int k, float* out_val,
                              int32_t* out_idx, void* stream_) {
  using namespace gdr;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (B == 0) return GDR_OK;
  GDR_CHECK_ARG(vals && idx && out_val && out_idx, "topk_merge: null pointer");
  GDR_CHECK_ARG(G > 0 && B > 0 && k >= 1 && k <= SIM_TOPK_MAX_K && (int64_t)G * k <= 0x7fffffffLL,
                "topk_merge: bad shape G=%d B=%d k=%d (k in [1, %d], G * k < 2^31)", G, B, k, SIM_TOPK_MAX_K);
  return launch_select<true>(vals, idx, nullptr, 0, G, B, k, 0, nullptr, out_val, out_idx, nullptr, k, 1, SEL_THREADS,
                             "topk_select_kernel<merge>", "topk_select_kernel<merge, deep>", stream);
}

namespace gdr {
// pairs[q][j] = {score bits, id} for j < k, pairs[q][k] = {0, status[q]}: one 8-byte-per-entry message per query row
__global__ void topk_pack_kernel(const float* __restrict__ vals, const int32_t* __restrict__ idx,
                                 const int32_t* __restrict__ status, int B, int k, int2* __restrict__ pairs) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)B * (k + 1)) return;
  const int q = (int)(e / (k + 1)), j = (int)(e - (int64_t)q * (k + 1));
  int2 o;
  if (j < k) {
    o.x = __float_as_int(vals[(int64_t)q * k + j]);
    o.y = idx[(int64_t)q * k + j];
  } else {
    o.x = 0;
    o.y = status ? status[q] : 0;
  }
  pairs[e] = o;
}
}  // namespace gdr

extern "C" int gdr_topk_pack(const float* vals, const int32_t* idx, const int32_t* status, int B, int k, void* pairs,
                             void* stream_) {
  using namespace gdr;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (B == 0) return GDR_OK;
  GDR_CHECK_ARG(vals && idx && pairs, "topk_pack: null pointer");
  GDR_CHECK_ARG(B > 0 && k >= 1 && k <= SIM_TOPK_MAX_K, "topk_pack: bad shape B=%d k=%d (k in [1, %d])", B, k, SIM_TOPK_MAX_K);
  const int64_t n = (int64_t)B * (k + 1);
  hipLaunchKernelGGL(topk_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, vals, idx, status, B, k,
                     static_cast<int2*>(pairs));
  GDR_CHECK_LAUNCH("topk_pack_kernel");
  return GDR_OK;
}

extern "C" int gdr_topk_merge_packed(const void* pairs, int G, int B, int k, float* out_val, int32_t* out_idx,
                                     int32_t* out_status, void* stream_) {
  using namespace gdr;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (B == 0) return GDR_OK;
  GDR_CHECK_ARG(pairs && out_val && out_idx, "topk_merge_packed: null pointer");
  GDR_CHECK_ARG(G > 0 && B > 0 && k >= 1 && k <= SIM_TOPK_MAX_K && (int64_t)G * k <= 0x7fffffffLL,
                "topk_merge_packed: bad shape G=%d B=%d k=%d (k in [1, %d], G * k < 2^31)", G, B, k, SIM_TOPK_MAX_K);
  const float* vals = static_cast<const float*>(pairs);
  const int32_t* idx = static_cast<const int32_t*>(pairs) + 1;
  return launch_select<true>(vals, idx, nullptr, 0, G, B, k, 0, nullptr, out_val, out_idx, out_status, k + 1, 2, SEL_THREADS,
                             "topk_select_kernel<merge packed>", "topk_select_kernel<merge packed, deep>", stream);
}
