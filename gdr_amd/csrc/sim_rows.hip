// Gather top-k for narrow per-query filters (include/gdr_hip.h: GDR_SIM_ROW_GATHER of gdr_sim_topk / gdr_sim_topk_bf16).
//
// The dense masked call (sim_topk.hip) scores all N rows for every query and masks the candidate lists afterwards; a filter that
// keeps 1 % of the corpus overflows them and pays a second, exhaustive pass.  Here only the rows bitmap q allows are scored:
//
//   1. COUNT    a wave per (segment, query) popcounts its share of bitmap q (ROWS_SEGS segments per bitmap, bits past N masked).
//   2. UNITS    one workgroup: per query count_q = sum of its segments, n_q = min(count_q, cap), status[q] = count_q > cap, and the
//               exclusive prefix over the queries of ceil(n_q / ROWS_UNIT) — the flat list of workgroup units of the dot pass.
//   3. PLACE    a wave per (segment, query): its base is the sum of the query's earlier segments, inside the segment a wave scan of
//               the word popcounts places every set bit's row at ids[q][base + ...] — ascending row order, no atomics, so the list
//               is a function of the bitmap alone; positions >= cap are dropped (the first cap allowed rows stay).
//   4. DOT      a fixed grid walks the flat unit list (a query with 8 000 rows beside 511 with 300 costs its rows, not the
//               uniform grid's 512 x 8 000): a workgroup finds its unit's query by bisection of the prefix, a wave takes 4 rows,
//               every lane loads 16 bytes of each and runs one fmaf chain per row in ascending column order, then wave_sum.
//               score(q, row) is a function of the two vectors and d alone — not of B, the position, cap or the regime.
//   5. SELECT   keys sel_pack(score, row) (select.h): cap <= 2 chunks — one LDS sort per query, its width the power of two that
//               holds n_q; more — a workgroup per chunk of SEL_CHUNK positions keeps its first k, then select.h's merge rounds.
//               The keys are a strict total order, so both give the same list bit for bit.
//
// The whole sequence is stream-ordered with no host synchronisation: every grid is sized from (B, cap) alone.
#include "scan.h"
#include "select.h"

namespace gdr {

constexpr int ROWS_SEGS = 64;     // segments of one bitmap: a wave each in the count and place passes
constexpr int ROWS_UNIT = 16;     // rows per workgroup unit of the dot pass: 4 waves x 4 rows in flight (rerank.hip RR_CH)
constexpr int ROWS_GRID = 2048;   // workgroups of the dot pass: 8 per CU, 32 waves — the row loads in flight hide the latency
constexpr int ROWS_ONE_SORT = 2 * SEL_CHUNK;  // the longest list one LDS sort takes (= SEL_SORT_MAX)
static_assert(ROWS_ONE_SORT == SEL_SORT_MAX, "two chunks are one LDS sort");

// The gather layout behind the B bitmaps (base bytes): it depends on (B, cap, k) only.
struct RowsPlan {
  int nchunk;  // chunked regime: cap / SEL_CHUNK; 0 in the one-sort regime
  size_t off_ids, off_val, off_cnt, off_seg, off_unit, off_part0, off_part1, total;
};
static RowsPlan rows_plan(int B, int64_t cap, int k, size_t base) {
  RowsPlan p{};
  size_t o = base;
  p.off_ids = o, o += align_up((size_t)B * (size_t)cap * sizeof(int32_t), 256);
  p.off_val = o, o += align_up((size_t)B * (size_t)cap * sizeof(float), 256);
  p.off_cnt = o, o += align_up((size_t)B * sizeof(int32_t), 256);
  p.off_seg = o, o += align_up((size_t)B * ROWS_SEGS * sizeof(int32_t), 256);
  p.off_unit = o, o += align_up(((size_t)B + 1) * sizeof(int32_t), 256);
  p.off_part0 = p.off_part1 = o;
  if (cap > ROWS_ONE_SORT) {
    p.nchunk = (int)(cap / SEL_CHUNK);
    const int fan = sel_merge_fan(k);
    p.off_part0 = o, o += align_up((size_t)B * p.nchunk * k * sizeof(unsigned long long), 256);
    p.off_part1 = o, o += align_up((size_t)B * ((p.nchunk + fan - 1) / fan) * k * sizeof(unsigned long long), 256);
  }
  p.total = o;
  return p;
}

size_t sim_rows_workspace_bytes(int B, int64_t cap, int k) { return rows_plan(B, cap, k, 0).total; }

// words [w0, w1) of segment s
__device__ __forceinline__ void rows_segment(int s, int64_t N, int64_t& w0, int64_t& w1) {
  const int64_t n_words = (N + 31) / 32, per = (n_words + ROWS_SEGS - 1) / ROWS_SEGS;
  w0 = (int64_t)s * per < n_words ? (int64_t)s * per : n_words;
  w1 = w0 + per < n_words ? w0 + per : n_words;
}

// ---- 1: segcnt[q][s] = allowed rows of segment s of bitmap q.  Grid (ROWS_SEGS / 4, queries): a wave per segment. ---------------
__global__ __launch_bounds__(256) void rows_count_kernel(const uint32_t* __restrict__ bitmaps, int64_t qstride, int64_t N, int B,
                                                         int32_t* __restrict__ segcnt) {
  const int lane = threadIdx.x & 63, s = blockIdx.x * 4 + (threadIdx.x >> 6);
  int64_t w0, w1;
  rows_segment(s, N, w0, w1);
  for (int64_t q = blockIdx.y; q < B; q += gridDim.y) {
    const uint32_t* bm = bitmaps + q * qstride;
    int c = 0;  // <= N < 2^31
    for (int64_t w = w0 + lane; w < w1; w += 64) c += __popc(bitmap_word(bm, w, N));
    c = wave_sum(c);
    if (lane == 0) segcnt[q * ROWS_SEGS + s] = c;
  }
}

// ---- 2: counts, status and the flat unit list.  One workgroup. ---------------------------------------------------------------------
__global__ __launch_bounds__(1024) void rows_units_kernel(const int32_t* __restrict__ segcnt, int B, int cap, int32_t* __restrict__ cnt,
                                                          int32_t* __restrict__ status, int32_t* __restrict__ unit_off) {
  // scan.h's BlockScan<1024> written out around its wave scan: through the struct 10.18 - 10.27 us per launch against the parent's 10.15 - 10.20
  __shared__ int wsum[16];
  __shared__ int carry;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) carry = 0;
  __syncthreads();
  for (int q0 = 0; q0 < B; q0 += 1024) {  // workgroup-uniform
    const int q = q0 + tid;
    int units = 0;
    if (q < B) {
      const int4* sc = reinterpret_cast<const int4*>(segcnt + (int64_t)q * ROWS_SEGS);
      int total = 0;  // <= N < 2^31
#pragma unroll
      for (int j = 0; j < ROWS_SEGS / 4; ++j) {
        const int4 v = sc[j];
        total += v.x + v.y + v.z + v.w;
      }
      const int n = total < cap ? total : cap;
      cnt[q] = n;
      if (status) status[q] = total > cap ? 1 : 0;  // the list is the top-k of the first cap allowed rows
      units = (n + ROWS_UNIT - 1) / ROWS_UNIT;
    }
    const int inc = wave_scan_incl(units, lane);
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int before = carry;
    for (int w = 0; w < wave; ++w) before += wsum[w];
    if (q < B) unit_off[q] = before + inc - units;
    __syncthreads();
    if (tid == 1023) carry = before + inc;
    __syncthreads();
  }
  if (tid == 0) unit_off[B] = carry;
}

// ---- 3: ids[q][0 .. n_q) = the allowed rows of bitmap q, ascending.  Grid as rows_count_kernel. -----------------------------------
__global__ __launch_bounds__(256) void rows_place_kernel(const uint32_t* __restrict__ bitmaps, int64_t qstride, int64_t N, int B,
                                                         int64_t cap, const int32_t* __restrict__ segcnt, int32_t* __restrict__ ids) {
  const int lane = threadIdx.x & 63, s = blockIdx.x * 4 + (threadIdx.x >> 6);
  int64_t w0, w1;
  rows_segment(s, N, w0, w1);
  for (int64_t q = blockIdx.y; q < B; q += gridDim.y) {
    int64_t base = wave_sum(lane < s ? segcnt[q * ROWS_SEGS + lane] : 0);  // allowed rows in front of this segment
    const uint32_t* bm = bitmaps + q * qstride;
    int32_t* out = ids + q * cap;
    for (int64_t t0 = w0; t0 < w1 && base < cap; t0 += 64) {  // wave-uniform bounds
      const int64_t w = t0 + lane;
      uint32_t bits = w < w1 ? bitmap_word(bm, w, N) : 0u;
      const int pc = __popc(bits);
      const int inc = wave_scan_incl(pc, lane);
      const int total = __shfl(inc, 63);
      int64_t pos = base + inc - pc;
      while (bits != 0u && pos < cap) {
        out[pos++] = (int32_t)(w * 32 + (__ffs(bits) - 1));
        bits &= bits - 1u;
      }
      base += total;
    }
  }
}

// ---- 4: val[q][c] = Q[q] . D[ids[q][c]] ----------------------------------------------------------------------------------------------
// dv: 16-byte pieces of a row (fp32: d / 4 float4; bf16: d / 8 pieces of eight values, widened exactly, fp32 accumulate).
template <bool BF16>
__global__ __launch_bounds__(256) void rows_dot_kernel(const void* __restrict__ Q, const void* __restrict__ D, int dv,
                                                       const int32_t* __restrict__ ids, const int32_t* __restrict__ cnt,
                                                       const int32_t* __restrict__ unit_off, int B, int64_t cap,
                                                       float* __restrict__ val) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int total = unit_off[B];
  for (int u = blockIdx.x; u < total; u += gridDim.x) {
    int lo = 0, hi = B;  // the last query whose first unit is at or before u: queries without units own nothing
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (unit_off[mid] <= u) lo = mid;
      else hi = mid;
    }
    const int q = lo, n = cnt[q];
    const int c0 = (u - unit_off[q]) * ROWS_UNIT + wave * 4;
    if (c0 >= n) continue;  // wave-uniform
    int64_t row[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) row[i] = ids[(int64_t)q * cap + (c0 + i < n ? c0 + i : n - 1)];  // past the list: a valid row, not stored
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    if (BF16) {
      const uint4* q8 = reinterpret_cast<const uint4*>(Q) + (int64_t)q * dv;
      for (int e = lane; e < dv; e += 64) {
        const uint4 x = q8[e];
        uint4 y[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) y[i] = reinterpret_cast<const uint4*>(D)[row[i] * dv + e];
        const uint32_t xs[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const uint32_t ys[4] = {y[i].x, y[i].y, y[i].z, y[i].w};
#pragma unroll
          for (int j = 0; j < 4; ++j) {  // two bf16 per word, the lower column in the low half
            acc[i] = fmaf(__uint_as_float(xs[j] << 16), __uint_as_float(ys[j] << 16), acc[i]);
            acc[i] = fmaf(__uint_as_float(xs[j] & 0xFFFF0000u), __uint_as_float(ys[j] & 0xFFFF0000u), acc[i]);
          }
        }
      }
    } else {
      const float4* q4 = reinterpret_cast<const float4*>(Q) + (int64_t)q * dv;
      for (int e = lane; e < dv; e += 64) {
        const float4 x = q4[e];
        float4 y[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) y[i] = reinterpret_cast<const float4*>(D)[row[i] * dv + e];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          acc[i] = fmaf(x.x, y[i].x, acc[i]);
          acc[i] = fmaf(x.y, y[i].y, acc[i]);
          acc[i] = fmaf(x.z, y[i].z, acc[i]);
          acc[i] = fmaf(x.w, y[i].w, acc[i]);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float a = wave_sum(acc[i]);
      if (lane == 0 && c0 + i < n) val[(int64_t)q * cap + c0 + i] = a;
    }
  }
}

// ---- 5: the select ----------------------------------------------------------------------------------------------------------------------
// the first k of the sorted keys -> one query's row of out_val / out_idx; key 0 = no row: -inf / -1
__device__ __forceinline__ void rows_write_topk(const unsigned long long* keys, int npad, int k, int32_t idx_offset,
                                                float* __restrict__ out_val, int32_t* __restrict__ out_idx) {
  for (int i = threadIdx.x; i < k; i += blockDim.x) {
    float v = -INFINITY;
    int32_t id = -1;
    const unsigned long long key = i < npad ? keys[i] : 0ull;
    if (key != 0ull) {
      v = sel_score(key);
      id = (int32_t)sel_low(key) + idx_offset;
    }
    out_val[i] = v;
    out_idx[i] = id;
  }
}

// keys of list positions [c_lo, c_hi) of query q into LDS, zero-padded to the power of two that holds them (>= 64), sorted
__device__ __forceinline__ int rows_sort_span(const float* __restrict__ val, const int32_t* __restrict__ ids, int64_t at, int c_lo,
                                              int c_hi, unsigned long long* keys) {
  int npad = 64;
  while (npad < c_hi - c_lo) npad <<= 1;
  for (int c = threadIdx.x; c < npad; c += blockDim.x)
    keys[c] = c_lo + c < c_hi ? sel_pack(val[at + c_lo + c], (uint32_t)ids[at + c_lo + c]) : 0ull;
  __syncthreads();
  bitonic_desc(keys, npad);
  return npad;
}

// one-sort regime: a workgroup per query, dynamic LDS for cap keys
__global__ __launch_bounds__(1024) void rows_select_kernel(const float* __restrict__ val, const int32_t* __restrict__ ids,
                                                           const int32_t* __restrict__ cnt, int64_t cap, int k, int32_t idx_offset,
                                                           float* __restrict__ out_val, int32_t* __restrict__ out_idx) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long rows_keys[];
  const int q = blockIdx.x;
  const int npad = rows_sort_span(val, ids, (int64_t)q * cap, 0, cnt[q], rows_keys);
  rows_write_topk(rows_keys, npad, k, idx_offset, out_val + (int64_t)q * k, out_idx + (int64_t)q * k);
}

// chunked regime: a workgroup per (chunk of SEL_CHUNK positions, query) keeps its first k keys; part [B][nchunk][k].  A chunk past
// the query's list leaves k zero keys.
__global__ __launch_bounds__(1024) void rows_chunk_kernel(const float* __restrict__ val, const int32_t* __restrict__ ids,
                                                          const int32_t* __restrict__ cnt, int64_t cap, int k, int nchunk,
                                                          unsigned long long* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long rows_keys[];
  const int q = blockIdx.x / nchunk, chunk = blockIdx.x % nchunk, n = cnt[q];
  const int c_lo = chunk * SEL_CHUNK, c_hi = c_lo + SEL_CHUNK < n ? c_lo + SEL_CHUNK : n;
  unsigned long long* dst = part + (int64_t)blockIdx.x * k;
  if (c_lo >= n) {  // workgroup-uniform
    for (int i = threadIdx.x; i < k; i += blockDim.x) dst[i] = 0ull;
    return;
  }
  const int npad = rows_sort_span(val, ids, (int64_t)q * cap, c_lo, c_hi, rows_keys);
  for (int i = threadIdx.x; i < k; i += blockDim.x) dst[i] = i < npad ? rows_keys[i] : 0ull;
}

// the last merge round's one list per query -> its row of the result, written as rows_select_kernel writes it
struct RowsEmit {
  float* out_val;
  int32_t* out_idx;
  int32_t idx_offset;
  __device__ bool skip() const { return false; }
  __device__ void operator()(int lane, const unsigned long long* keys, int npad, int k) const {
    rows_write_topk(keys, npad, k, idx_offset, out_val + (int64_t)lane * k, out_idx + (int64_t)lane * k);
  }
};

// bitmaps: B bitmaps, qstride words apart (the head of the caller's workspace, only read); ws: the gather layout behind them.
// The arguments were validated by sim_topk_impl: cap = 4096 c, c in 1 .. 256; k <= 1024 when cap > ROWS_ONE_SORT.
int launch_sim_rows(const void* Q, int B, const void* D, int64_t N, int d, int k, int32_t idx_offset, float* out_val, int32_t* out_idx,
                    int32_t* status, const uint32_t* bitmaps, int64_t qstride, int64_t cap, void* ws_, bool bf16, hipStream_t stream) {
  const RowsPlan p = rows_plan(B, cap, k, 0);
  char* ws = static_cast<char*>(ws_);
  int32_t* ids = reinterpret_cast<int32_t*>(ws + p.off_ids);
  float* val = reinterpret_cast<float*>(ws + p.off_val);
  int32_t* cnt = reinterpret_cast<int32_t*>(ws + p.off_cnt);
  int32_t* segcnt = reinterpret_cast<int32_t*>(ws + p.off_seg);
  int32_t* unit_off = reinterpret_cast<int32_t*>(ws + p.off_unit);
  const dim3 seg_grid(ROWS_SEGS / 4, (unsigned)(B < 65535 ? B : 65535));
  hipLaunchKernelGGL(rows_count_kernel, seg_grid, dim3(256), 0, stream, bitmaps, qstride, N, B, segcnt);
  GDR_CHECK_LAUNCH("rows_count_kernel");
  hipLaunchKernelGGL(rows_units_kernel, dim3(1), dim3(1024), 0, stream, (const int32_t*)segcnt, B, (int)cap, cnt, status, unit_off);
  GDR_CHECK_LAUNCH("rows_units_kernel");
  hipLaunchKernelGGL(rows_place_kernel, seg_grid, dim3(256), 0, stream, bitmaps, qstride, N, B, cap, (const int32_t*)segcnt, ids);
  GDR_CHECK_LAUNCH("rows_place_kernel");
  {
    const int64_t max_units = (int64_t)B * (cap / ROWS_UNIT);
    const unsigned grid = (unsigned)(max_units < ROWS_GRID ? max_units : ROWS_GRID);
    ProfScope prof(PROF_RERANK, 0.0, stream);  // the row count lives on the device
    if (bf16)
      hipLaunchKernelGGL(rows_dot_kernel<true>, dim3(grid), dim3(256), 0, stream, Q, D, d / 8, (const int32_t*)ids, (const int32_t*)cnt,
                         (const int32_t*)unit_off, B, cap, val);
    else
      hipLaunchKernelGGL(rows_dot_kernel<false>, dim3(grid), dim3(256), 0, stream, Q, D, d / 4, (const int32_t*)ids, (const int32_t*)cnt,
                         (const int32_t*)unit_off, B, cap, val);
    GDR_CHECK_LAUNCH("rows_dot_kernel");
  }
  ProfScope prof(PROF_SELECT, 0.0, stream);
  if (cap <= ROWS_ONE_SORT) {
    GDR_TRY(ensure_dyn_lds(reinterpret_cast<const void*>(rows_select_kernel), SEL_SORT_MAX * 8, "sim_topk(row gather)"));
    hipLaunchKernelGGL(rows_select_kernel, dim3((unsigned)B), dim3(1024), (size_t)cap * 8, stream, (const float*)val, (const int32_t*)ids,
                       (const int32_t*)cnt, cap, k, idx_offset, out_val, out_idx);
    GDR_CHECK_LAUNCH("rows_select_kernel");
    return GDR_OK;
  }
  unsigned long long* part[2] = {reinterpret_cast<unsigned long long*>(ws + p.off_part0),
                                 reinterpret_cast<unsigned long long*>(ws + p.off_part1)};
  GDR_TRY(ensure_dyn_lds(reinterpret_cast<const void*>(sel_merge_kernel<RowsEmit>), SEL_SORT_MAX * 8, "sim_topk(row gather)"));
  hipLaunchKernelGGL(rows_chunk_kernel, dim3((unsigned)(B * p.nchunk)), dim3(1024), (size_t)SEL_CHUNK * 8, stream, (const float*)val,
                     (const int32_t*)ids, (const int32_t*)cnt, cap, k, p.nchunk, part[0]);
  GDR_CHECK_LAUNCH("rows_chunk_kernel");
  const RowsEmit emit{out_val, out_idx, idx_offset};
  return sel_merge_rounds(part, p.nchunk, k, B, 1, emit, "sel_merge_kernel<row gather>", stream);
}

}  // namespace gdr
