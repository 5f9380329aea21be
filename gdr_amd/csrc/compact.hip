// Compacting a live corpus (include/gdr_hip_compact.h): the plan (live-row bitmap -> new_id / old_id), the row mover, the id remap
// and the per-query row-bitmap remap.
//
//   PLAN    1. COUNT   a wave per tile of PLAN_TILE_WORDS bitmap words popcounts it (bits past N masked).
//           2. SCAN    ONE workgroup: the exclusive prefix of the tile counts, PLAN_SCAN_STEP tiles per step with a carry, any number
//                      of steps (N < 2^31: at most 2^19 tiles); status = (total != n_live).
//           3. PLACE   a wave per tile: per chunk of 64 words a wave scan of the word popcounts gives every word its base, then 32
//                      sweeps of 64 consecutive rows — lane l fetches its row's word and base by shuffle, its rank inside the word
//                      is a masked popcount — so new_id is written 256 contiguous bytes per instruction and old_id in ascending
//                      order without an atomic.  A position >= n_live (a wrong caller count) is never written.
//   ROWS    one kernel in three modes: out of place (src row old_id[j] -> dst row j), and for the in-place form per chunk of
//           destination rows GATHER (src row old_id[j] -> bounce row j - j0) then SCATTER (bounce row j - j0 -> dst row j), both
//           skipping the rows that stay where they are (old_id[j] == j).  A wave takes 64 / LPR rows at a time, LPR = the power of two
//           that covers a row's 16-byte (or 4-byte) units, up to 64: wide rows are swept 1 KiB per wave-instruction with four loads
//           in flight per lane, narrow rows are packed side by side in one wave.
//   IDS     out[i] = new_id[ids[i]]; negative ids kept; dead / out-of-range -> -1 and one atomicOr into the status word.
//   MASK    a wave per 64 output rows and bitmap: lane l tests bit old_id[j] of the input, one ballot is two output words.
#include "scan.h"

namespace gdr {

constexpr int PLAN_TILE_WORDS = 128;                   // bitmap words of one tile: a wave each in the count and place passes
constexpr int PLAN_TILE_ROWS = PLAN_TILE_WORDS * 32;   // 4096 rows
static_assert(PLAN_TILE_ROWS == 4096 && PLAN_TILE_WORDS % 64 == 0, "include/gdr_hip_compact.h states the tile; a wave takes whole 64-word chunks");
constexpr int PLAN_SCAN_STEP = 1024;                 // tiles per step of the one-workgroup scan
constexpr int64_t COMPACT_GRID = 2048;                 // workgroups of the memory-bound passes: 8 per CU, the rest grid-strides

static inline int64_t plan_tiles(int64_t N) { return ((N + 31) / 32 + PLAN_TILE_WORDS - 1) / PLAN_TILE_WORDS; }

// ---- plan 1: tile_cnt[t] = live rows of tile t.  256 threads = 4 tiles per workgroup. ---------------------------------------------
__global__ __launch_bounds__(256) void compact_count_kernel(const uint32_t* __restrict__ bm, int64_t N, int64_t n_tiles,
                                                            int32_t* __restrict__ tile_cnt) {
  const int lane = threadIdx.x & 63;
  const int64_t n_words = (N + 31) / 32;
  for (int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); t < n_tiles; t += (int64_t)gridDim.x * 4) {  // wave-uniform
    int c = 0;
#pragma unroll
    for (int i = 0; i < PLAN_TILE_WORDS / 64; ++i) {
      const int64_t w = t * PLAN_TILE_WORDS + i * 64 + lane;
      if (w < n_words) c += __popc(bitmap_word(bm, w, N));
    }
    c = wave_sum(c);
    if (lane == 0) tile_cnt[t] = c;
  }
}

// ---- plan 2: tile_off = exclusive prefix of tile_cnt (in place), status = total != n_live.  One workgroup. ------------------------
__global__ __launch_bounds__(PLAN_SCAN_STEP) void compact_scan_kernel(int32_t* __restrict__ tile, int64_t n_tiles, int64_t n_live,
                                                                      int32_t* __restrict__ status) {
  __shared__ int wsum[PLAN_SCAN_STEP / 64];
  __shared__ int carry;
  BlockScan<PLAN_SCAN_STEP> scan(wsum, &carry);
  for (int64_t t0 = 0; t0 < n_tiles; t0 += PLAN_SCAN_STEP) {  // workgroup-uniform
    const int64_t t = t0 + threadIdx.x;
    const int before = scan.round(t < n_tiles ? tile[t] : 0);  // every total <= N < 2^31
    if (t < n_tiles) tile[t] = before;
  }
  const int total = scan.total();
  if (threadIdx.x == 0) status[0] = (int64_t)total != n_live ? 1 : 0;
}

// ---- plan 3: new_id / old_id.  Grid as compact_count_kernel. --------------------------------------------------------------------------
__global__ __launch_bounds__(256) void compact_place_kernel(const uint32_t* __restrict__ bm, int64_t N, int64_t n_tiles, int64_t n_live,
                                                            const int32_t* __restrict__ tile_off, int32_t* __restrict__ new_id,
                                                            int32_t* __restrict__ old_id) {
  const int lane = threadIdx.x & 63;
  const int64_t n_words = (N + 31) / 32;
  for (int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); t < n_tiles; t += (int64_t)gridDim.x * 4) {  // wave-uniform
    int base = tile_off[t];
#pragma unroll 1
    for (int i = 0; i < PLAN_TILE_WORDS / 64; ++i) {
      const int64_t w0 = t * PLAN_TILE_WORDS + i * 64;
      if (w0 >= n_words) break;
      const uint32_t bits = w0 + lane < n_words ? bitmap_word(bm, w0 + lane, N) : 0u;
      const int pc = __popc(bits);
      const int inc = wave_scan_incl(pc, lane);
      const int wbase = base + inc - pc;  // live rows in front of this lane's word
#pragma unroll 4
      for (int s = 0; s < 32; ++s) {  // rows w0 * 32 + s * 64 + lane: words 2 s and 2 s + 1 of the chunk
        const int src_lane = 2 * s + (lane >> 5);
        const uint32_t wb = (uint32_t)__shfl((int)bits, src_lane);
        const int wp = __shfl(wbase, src_lane);
        const int b = lane & 31;
        const int64_t r = w0 * 32 + s * 64 + lane;
        if (r < N) {
          const bool live = (wb >> b) & 1u;
          const int pos = wp + __popc(wb & ((1u << b) - 1u));
          new_id[r] = live ? pos : -1;
          if (live && (int64_t)pos < n_live) old_id[pos] = (int32_t)r;
        }
      }
      base += __shfl(inc, 63);
    }
  }
}

// ---- the row mover ---------------------------------------------------------------------------------------------------------------------
enum { MOVE_OUT = 0, MOVE_GATHER = 1, MOVE_SCATTER = 2 };

// destination rows [j0, j0 + n); upr = units of sizeof(T) per row; lpr = lanes per row (a power of two <= 64)
template <typename T>
__global__ __launch_bounds__(256) void compact_move_kernel(const T* __restrict__ src, T* __restrict__ dst, const int32_t* __restrict__ ids,
                                                           int64_t j0, int64_t n, int64_t upr, int64_t N, int lpr, int mode) {
  const int lane = threadIdx.x & 63;
  const int rpw = 64 / lpr, sub = lane / lpr, c = lane % lpr;
  const int64_t n_groups = (n + rpw - 1) / rpw;
  for (int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); g < n_groups; g += (int64_t)gridDim.x * 4) {
    const int64_t k = g * rpw + sub;  // row inside the chunk
    if (k >= n) continue;
    const int64_t j = j0 + k, id = ids[j];
    if (id < 0 || id >= N) continue;              // moves nothing
    if (mode != MOVE_OUT && id == j) continue;    // in place: the row stays where it is
    const T* s = src + (mode == MOVE_SCATTER ? k : id) * upr;
    T* d = dst + (mode == MOVE_GATHER ? k : j) * upr;
    for (int64_t e = c; e < upr; e += 4 * (int64_t)lpr) {
      T v[4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (e + (int64_t)i * lpr < upr) v[i] = s[e + (int64_t)i * lpr];
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (e + (int64_t)i * lpr < upr) d[e + (int64_t)i * lpr] = v[i];
    }
  }
}

static int launch_move(const void* src, void* dst, const int32_t* ids, int64_t j0, int64_t n, int64_t row_bytes, int64_t N, bool vec16,
                       int mode, hipStream_t stream) {
  const int64_t upr = row_bytes / (vec16 ? 16 : 4);
  int lpr = 1;
  while (lpr < 64 && lpr < upr) lpr <<= 1;
  const int64_t groups = (n + 64 / lpr - 1) / (64 / lpr), blocks = (groups + 3) / 4;
  const dim3 grid((unsigned)(blocks < COMPACT_GRID ? blocks : COMPACT_GRID));
  if (vec16)
    hipLaunchKernelGGL(compact_move_kernel<uint4>, grid, dim3(256), 0, stream, static_cast<const uint4*>(src), static_cast<uint4*>(dst), ids,
                       j0, n, upr, N, lpr, mode);
  else
    hipLaunchKernelGGL(compact_move_kernel<uint32_t>, grid, dim3(256), 0, stream, static_cast<const uint32_t*>(src),
                       static_cast<uint32_t*>(dst), ids, j0, n, upr, N, lpr, mode);
  GDR_CHECK_LAUNCH("compact_move_kernel");
  return GDR_OK;
}

// ---- ids ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void compact_ids_kernel(const int32_t* __restrict__ new_id, int64_t N, const int32_t* ids, int32_t* out,
                                                          int64_t n, int32_t* __restrict__ status) {
  bool bad = false;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    int32_t v = ids[i];  // out may alias ids: the element is read before this lane writes it
    if (v >= 0) {
      v = (int64_t)v < N ? new_id[v] : -1;
      bad |= v < 0;
    }
    out[i] = v;
  }
  if (bad) atomicOr(status, 1);
}

// ---- per-query row bitmaps -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void compact_mask_kernel(const uint32_t* __restrict__ in, int64_t in_stride, int B, int64_t N,
                                                           const int32_t* __restrict__ old_id, int64_t n_live, uint32_t* __restrict__ out,
                                                           int64_t out_stride) {
  const int lane = threadIdx.x & 63;
  const int64_t n_groups = (n_live + 63) / 64, n_out_words = (n_live + 31) / 32;
  for (int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); g < n_groups; g += (int64_t)gridDim.x * 4) {  // wave-uniform
    const int64_t j = g * 64 + lane;
    const int64_t id = j < n_live ? old_id[j] : -1;
    const bool ok = id >= 0 && id < N;
    for (int q = blockIdx.y; q < B; q += gridDim.y) {
      const bool bit = ok && ((in[(int64_t)q * in_stride + (id >> 5)] >> (id & 31)) & 1u);
      const unsigned long long m = __ballot(bit);
      if (lane == 0) out[(int64_t)q * out_stride + 2 * g] = (uint32_t)m;
      if (lane == 32 && 2 * g + 1 < n_out_words) out[(int64_t)q * out_stride + 2 * g + 1] = (uint32_t)(m >> 32);
    }
  }
}

static inline bool ranges_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a_bytes != 0 && b_bytes != 0 && a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

}  // namespace gdr

extern "C" size_t gdr_rows_compact_plan_workspace_bytes(int64_t N) {
  using namespace gdr;
  if (N < 1 || N >= ((int64_t)1 << 31)) return 0;
  return align_up((size_t)plan_tiles(N) * sizeof(int32_t), 256);
}

extern "C" int gdr_rows_compact_plan(const int32_t* live_words, int64_t N, int64_t n_live, int32_t* out_new_id, int32_t* out_old_id,
                                     int32_t* out_status, void* workspace, size_t workspace_bytes, void* stream_) {
  using namespace gdr;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  GDR_CHECK_ARG(N >= 1 && N < ((int64_t)1 << 31), "rows_compact_plan: N=%lld must lie in [1, 2^31)", (long long)N);
  GDR_CHECK_ARG(n_live >= 0 && n_live <= N, "rows_compact_plan: n_live=%lld must lie in [0, N=%lld]", (long long)n_live, (long long)N);
  GDR_CHECK_ARG(live_words && out_new_id && out_status && workspace, "rows_compact_plan: null pointer (live_words, out_new_id, out_status, workspace)");
  GDR_CHECK_ARG(out_old_id || n_live == 0, "rows_compact_plan: out_old_id is null with n_live=%lld", (long long)n_live);
  GDR_CHECK_ARG(((uintptr_t)live_words & 3) == 0 && ((uintptr_t)out_new_id & 3) == 0 && ((uintptr_t)out_old_id & 3) == 0 &&
                    ((uintptr_t)out_status & 3) == 0 && ((uintptr_t)workspace & 3) == 0,
                "rows_compact_plan: live_words, out_new_id, out_old_id, out_status and workspace must be 4-byte aligned");
  const size_t need = gdr_rows_compact_plan_workspace_bytes(N);
  if (workspace_bytes < need) {
    set_error("rows_compact_plan: workspace too small (%zu < %zu bytes)", workspace_bytes, need);
    return GDR_ENOSPC;
  }
  const int64_t n_tiles = plan_tiles(N), blocks = (n_tiles + 3) / 4;
  const dim3 grid((unsigned)(blocks < COMPACT_GRID ? blocks : COMPACT_GRID));
  const uint32_t* bm = reinterpret_cast<const uint32_t*>(live_words);
  int32_t* tile = static_cast<int32_t*>(workspace);
  hipLaunchKernelGGL(compact_count_kernel, grid, dim3(256), 0, stream, bm, N, n_tiles, tile);
  GDR_CHECK_LAUNCH("compact_count_kernel");
  hipLaunchKernelGGL(compact_scan_kernel, dim3(1), dim3(PLAN_SCAN_STEP), 0, stream, tile, n_tiles, n_live, out_status);
  GDR_CHECK_LAUNCH("compact_scan_kernel");
  hipLaunchKernelGGL(compact_place_kernel, grid, dim3(256), 0, stream, bm, N, n_tiles, n_live, (const int32_t*)tile, out_new_id, out_old_id);
  GDR_CHECK_LAUNCH("compact_place_kernel");
  return GDR_OK;
}

extern "C" size_t gdr_rows_compact_workspace_bytes(int64_t row_bytes, int64_t chunk_rows) {
  if (row_bytes <= 0 || chunk_rows < 0) return 0;
  if (chunk_rows == 0) return (size_t)(row_bytes > GDR_COMPACT_BOUNCE_BYTES ? row_bytes : GDR_COMPACT_BOUNCE_BYTES) + 256;
  return (size_t)chunk_rows * (size_t)row_bytes + 256;
}

extern "C" int gdr_rows_compact(const void* src, void* dst, int64_t N, int64_t row_bytes, const int32_t* old_id, int64_t n_live,
                                int64_t chunk_rows, void* workspace, size_t workspace_bytes, void* stream_) {
  using namespace gdr;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  GDR_CHECK_ARG(N >= 1 && N < ((int64_t)1 << 31), "rows_compact: N=%lld must lie in [1, 2^31)", (long long)N);
  GDR_CHECK_ARG(row_bytes > 0 && row_bytes % 4 == 0, "rows_compact: row_bytes=%lld must be a positive multiple of 4", (long long)row_bytes);
  GDR_CHECK_ARG(n_live >= 0 && n_live <= N, "rows_compact: n_live=%lld must lie in [0, N=%lld]", (long long)n_live, (long long)N);
  GDR_CHECK_ARG(chunk_rows >= 0, "rows_compact: chunk_rows=%lld must not be negative (0 = the library default)", (long long)chunk_rows);
  GDR_CHECK_ARG(src && dst, "rows_compact: null pointer (src, dst)");
  GDR_CHECK_ARG(old_id || n_live == 0, "rows_compact: old_id is null with n_live=%lld", (long long)n_live);
  GDR_CHECK_ARG(((uintptr_t)src & 3) == 0 && ((uintptr_t)dst & 3) == 0 && ((uintptr_t)old_id & 3) == 0,
                "rows_compact: src, dst and old_id must be 4-byte aligned");
  const bool in_place = src == dst;
  GDR_CHECK_ARG(in_place || !ranges_overlap(src, (size_t)N * (size_t)row_bytes, dst, (size_t)n_live * (size_t)row_bytes),
                "rows_compact: dst overlaps src (the two regions must be disjoint, or dst == src for the in-place form)");
  bool vec16 = row_bytes % 16 == 0 && ((uintptr_t)src & 15) == 0 && ((uintptr_t)dst & 15) == 0;
  if (!in_place) {
    if (n_live == 0) return GDR_OK;
    return launch_move(src, dst, old_id, 0, n_live, row_bytes, N, vec16, MOVE_OUT, stream);
  }
  const size_t need = gdr_rows_compact_workspace_bytes(row_bytes, chunk_rows);
  if (!workspace || workspace_bytes < need) {
    set_error("rows_compact: workspace too small for the in-place form (%zu < %zu bytes)", workspace ? workspace_bytes : (size_t)0, need);
    return GDR_ENOSPC;
  }
  if (n_live == 0) return GDR_OK;
  int64_t chunk = chunk_rows;
  if (chunk == 0) chunk = row_bytes >= GDR_COMPACT_BOUNCE_BYTES ? 1 : GDR_COMPACT_BOUNCE_BYTES / row_bytes;
  char* bounce = reinterpret_cast<char*>(align_up((size_t)(uintptr_t)workspace, 256));  // need leaves 256 bytes for this
  for (int64_t j0 = 0; j0 < n_live; j0 += chunk) {
    const int64_t n = n_live - j0 < chunk ? n_live - j0 : chunk;
    GDR_TRY(launch_move(src, bounce, old_id, j0, n, row_bytes, N, vec16, MOVE_GATHER, stream));
    GDR_TRY(launch_move(bounce, dst, old_id, j0, n, row_bytes, N, vec16, MOVE_SCATTER, stream));
  }
  return GDR_OK;
}

extern "C" int gdr_ids_remap(const int32_t* new_id, int64_t N, const int32_t* ids, int32_t* out_ids, int64_t n, int32_t* out_status,
                             void* stream_) {
  using namespace gdr;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  GDR_CHECK_ARG(N >= 1 && N < ((int64_t)1 << 31), "ids_remap: N=%lld must lie in [1, 2^31)", (long long)N);
  GDR_CHECK_ARG(n >= 0, "ids_remap: n=%lld must not be negative", (long long)n);
  GDR_CHECK_ARG(new_id && out_status, "ids_remap: null pointer (new_id, out_status)");
  GDR_CHECK_ARG((ids && out_ids) || n == 0, "ids_remap: null pointer (ids, out_ids) with n=%lld", (long long)n);
  GDR_CHECK_ARG(((uintptr_t)new_id & 3) == 0 && ((uintptr_t)ids & 3) == 0 && ((uintptr_t)out_ids & 3) == 0 && ((uintptr_t)out_status & 3) == 0,
                "ids_remap: new_id, ids, out_ids and out_status must be 4-byte aligned");
  GDR_CHECK_ARG(ids == out_ids || !ranges_overlap(ids, (size_t)n * 4, out_ids, (size_t)n * 4),
                "ids_remap: out_ids partly overlaps ids (it may alias it exactly, or be disjoint)");
  hipError_t e = hipMemsetAsync(out_status, 0, sizeof(int32_t), stream);
  if (e != hipSuccess) {
    set_error("ids_remap: hipMemsetAsync: %s", hipGetErrorString(e));
    return GDR_EHIP;
  }
  if (n == 0) return GDR_OK;
  const int64_t blocks = (n + 255) / 256;
  hipLaunchKernelGGL(compact_ids_kernel, dim3((unsigned)(blocks < COMPACT_GRID ? blocks : COMPACT_GRID)), dim3(256), 0, stream, new_id, N, ids,
                     out_ids, n, out_status);
  GDR_CHECK_LAUNCH("compact_ids_kernel");
  return GDR_OK;
}

extern "C" int gdr_rowmask_compact(const int32_t* words_in, int64_t in_stride_words, int B, int64_t N, const int32_t* old_id, int64_t n_live,
                                   int32_t* words_out, int64_t out_stride_words, void* stream_) {
  using namespace gdr;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  GDR_CHECK_ARG(N >= 1 && N < ((int64_t)1 << 31), "rowmask_compact: N=%lld must lie in [1, 2^31)", (long long)N);
  GDR_CHECK_ARG(n_live >= 0 && n_live <= N, "rowmask_compact: n_live=%lld must lie in [0, N=%lld]", (long long)n_live, (long long)N);
  GDR_CHECK_ARG(B >= 0, "rowmask_compact: B=%d must not be negative", B);
  const int64_t w_in = (N + 31) / 32, w_out = (n_live + 31) / 32;
  GDR_CHECK_ARG(in_stride_words >= w_in, "rowmask_compact: in_stride_words=%lld is less than the %lld words of a bitmap over N rows",
                (long long)in_stride_words, (long long)w_in);
  GDR_CHECK_ARG(out_stride_words >= w_out, "rowmask_compact: out_stride_words=%lld is less than the %lld words of a bitmap over n_live rows",
                (long long)out_stride_words, (long long)w_out);
  if (B == 0 || n_live == 0) return GDR_OK;
  GDR_CHECK_ARG(words_in && words_out && old_id, "rowmask_compact: null pointer (words_in, words_out, old_id)");
  GDR_CHECK_ARG(((uintptr_t)words_in & 3) == 0 && ((uintptr_t)words_out & 3) == 0 && ((uintptr_t)old_id & 3) == 0,
                "rowmask_compact: words_in, words_out and old_id must be 4-byte aligned");
  GDR_CHECK_ARG(!ranges_overlap(words_in, ((size_t)(B - 1) * (size_t)in_stride_words + (size_t)w_in) * 4, words_out,
                                ((size_t)(B - 1) * (size_t)out_stride_words + (size_t)w_out) * 4),
                "rowmask_compact: words_out overlaps words_in (input and output must not alias)");
  const int64_t blocks = ((n_live + 63) / 64 + 3) / 4;
  const dim3 grid((unsigned)(blocks < COMPACT_GRID ? blocks : COMPACT_GRID), (unsigned)(B < 1024 ? B : 1024));
  hipLaunchKernelGGL(compact_mask_kernel, grid, dim3(256), 0, stream, reinterpret_cast<const uint32_t*>(words_in), in_stride_words, B, N,
                     old_id, n_live, reinterpret_cast<uint32_t*>(words_out), out_stride_words);
  GDR_CHECK_LAUNCH("compact_mask_kernel");
  return GDR_OK;
}
