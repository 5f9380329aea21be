// Corpus expansion: cluster centroids and the insertion of new documents into the member CSR — the device form of
// tree_embedding_calculate + tree_embedding_insert (main_models.py:154-179, 268-295).
//
//   gdr_cluster_centroids: one wave per (cluster, 256-column slice); lane l owns the float4 at column 4 * (l + 64 s).  Member
//     rows are gathered whole (1 KiB per wave-instruction), CE_ROWS of them in flight, and added in member order: with the
//     members ascending this is the reference's sum([emb[i] for i in members]) / len(members) bit for bit — sequential fp32
//     adds starting from 0 (Python's sum), then ONE correctly rounded fp32 division.  No float atomics: their sum depends on
//     arrival order.
//   gdr_cluster_insert: histogram of the targets -> one-block scan (new offsets, largest cluster) -> segmented copy of the old
//     members -> placement of the new ones by a per-cluster ticket -> per-cluster sort of each inserted tail, so that the
//     result does not depend on the order in which the tickets were taken.  Deterministic.  Cost O(N + n) while every cluster
//     receives at most CI_SORT_LDS documents; each cluster that receives more is rewritten by one ordered pass over all n inputs
//     (one block per such cluster, the blocks run side by side), so the work bound is O(N + n + n * L) with L <= n / CI_SORT_LDS
//     the number of those clusters.
//   gdr_cluster_insert, REMOVAL mode (new_target == NULL, new_ids != NULL, n_new > 0): new_ids is the strictly
//     ascending list of doc ids to take out of the CSR.  Every cluster keeps its surviving members in their order, a cluster
//     that loses all of them becomes an empty segment, an id that is a member of no cluster is ignored.  out_members still has
//     room for n_old entries; the first out_offsets[C] are written, the rest is left untouched; n_old - out_offsets[C] ids were
//     removed.  Three launches, the shape of hist / scan / copy: one wave per cluster counts its members that are in the list
//     (membership = binary search in the ascending list, no atomic at all) and stores the NEGATED count where the insert mode
//     keeps its histogram -> the same one-block scan (new offsets, largest cluster, consistency of the old offsets) -> one wave
//     per cluster walks its segment in order, RM_TILE members at a time: the ballot rank of a survivor inside its 64-member
//     chunk plus a running base is its destination.  Integers only; the result is a function of the inputs alone.  The
//     workspace is the insert mode's (per-cluster counters, nothing sized by n_old), which is why membership is tested twice.
//     Cost O(n_old log n_new); one huge cluster serialises on one wave, as in insert_copy_kernel.
#include "scan.h"

namespace gdr {
namespace {

constexpr int CE_ROWS = 8;          // member rows in flight per wave
constexpr int CE_MAX_D = 4096;      // 16 slices of 256 columns
constexpr int CI_SORT_LDS = 4096;   // inserted tails up to this size are sorted in LDS (bitonic); longer ones are compacted in order
constexpr int RM_CHUNKS = 4;        // removal: 64-member chunks one wave has in flight (their list lookups overlap)
constexpr int RM_TILE = 64 * RM_CHUNKS;

// The sum below is kmeans.hip's seq_sum written out (tests/test_gpu_kmeans.py holds the two to the same bits): through the shared function
// this kernel measured 0.25 - 0.6 % above the parent's slowest run at 334 314 x 768 rows in clusters of 12 (profiles/README.md, r30).
__global__ __launch_bounds__(256) void centroid_kernel(const float* __restrict__ D, int64_t N, int d4, int S,
                                                       const int32_t* __restrict__ offsets, const int32_t* __restrict__ members,
                                                       int64_t n_members, int C, float* __restrict__ cent,
                                                       int32_t* __restrict__ counts) {
  const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (w >= (int64_t)C * S) return;  // wave-uniform
  const int c = (int)(w / S), s = (int)(w % S);
  int64_t lo = offsets[c], hi = offsets[c + 1];
  if (lo < 0 || hi > n_members || hi < lo) lo = hi = 0;  // a malformed segment reads nothing (the caller validates)
  const int col = lane + 64 * s;                         // float4 column of this lane
  const bool on = col < d4;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  const float4* D4 = reinterpret_cast<const float4*>(D);
  int32_t mid[CE_ROWS];  // member ids of the current batch; the next batch's ids load beside its rows (one round trip per batch)
#pragma unroll
  for (int u = 0; u < CE_ROWS; ++u) mid[u] = lo + u < hi ? members[lo + u] : -1;
  for (int64_t j = lo; j < hi; j += CE_ROWS) {
    float4 x[CE_ROWS];
    bool ok[CE_ROWS];
#pragma unroll
    for (int u = 0; u < CE_ROWS; ++u) {  // every load of the batch is issued before the first add
      const int32_t m = mid[u];
      ok[u] = m >= 0 && m < N;
      x[u] = (ok[u] && on) ? D4[(int64_t)m * d4 + col] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < CE_ROWS; ++u) {
      const int64_t jn = j + CE_ROWS + u;
      mid[u] = jn < hi ? members[jn] : -1;
    }
#pragma unroll
    for (int u = 0; u < CE_ROWS; ++u) {  // member order: acc = ((x_m1 + x_m2) + ...) + x_mn
      if (ok[u]) {
        acc.x = acc.x + x[u].x;
        acc.y = acc.y + x[u].y;
        acc.z = acc.z + x[u].z;
        acc.w = acc.w + x[u].w;
      }
    }
  }
  const int cnt = (int)(hi - lo);
  if (on) {
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
    if (cnt > 0) {
      const float n = (float)cnt;  // exact: cnt < 2^24 for any cluster that fits the int32 ids
      r = make_float4(__fdiv_rn(acc.x, n), __fdiv_rn(acc.y, n), __fdiv_rn(acc.z, n), __fdiv_rn(acc.w, n));
    }
    reinterpret_cast<float4*>(cent)[(int64_t)c * d4 + col] = r;
  }
  if (s == 0 && lane == 0) counts[c] = cnt;
}

__device__ __forceinline__ int resolve_target(const int32_t* target, int64_t i, const int32_t* map, int n_map, int C) {
  int t = target[i];
  if (map) t = (t >= 0 && t < n_map) ? map[t] : -1;
  return (t >= 0 && t < C) ? t : -1;
}

__global__ __launch_bounds__(256) void insert_hist_kernel(const int32_t* __restrict__ target, int n, const int32_t* __restrict__ map,
                                                          int n_map, int C, int32_t* __restrict__ hist, int32_t* __restrict__ bad) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int c = resolve_target(target, i, map, n_map, C);
    if (c < 0) {
      atomicOr(bad, 1);
      continue;
    }
    atomicAdd(&hist[c], 1);
  }
}

// one block: new_off[c] = old_off[c] + sum_{c' < c} hist[c'], the largest new cluster, and the consistency of the old offsets.
// hist[c] is the number of documents cluster c receives, or (removal mode) minus the number it loses.
__global__ __launch_bounds__(1024) void insert_scan_kernel(const int32_t* __restrict__ old_off, const int32_t* __restrict__ hist,
                                                           int C, int64_t n_old, int32_t* __restrict__ new_off,
                                                           const int32_t* __restrict__ bad, int32_t* __restrict__ out_max) {
  __shared__ int64_t wsum[16];
  __shared__ int big[16], broken[16];
  const int t = threadIdx.x;
  const int per = (C + 1023) / 1024;
  const int c0 = t * per, c1 = min(C, c0 + per);
  int64_t sum = 0;
  int mx = 0, bk = 0;
  for (int c = c0; c < c1; ++c) {
    const int sz = old_off[c + 1] - old_off[c];
    if (sz < 0) bk = 1;
    sum += hist[c];
    mx = max(mx, sz + hist[c]);
  }
  mx = wave_max(mx), bk = wave_max(bk);
  if ((t & 63) == 0) big[t >> 6] = mx, broken[t >> 6] = bk;
  int64_t total;
  int64_t run = block_scan_once<1024>(sum, wsum, &total);  // its barrier publishes big and broken as well
  for (int c = c0; c < c1; ++c) {
    new_off[c] = (int32_t)(old_off[c] + run);
    run += hist[c];
  }
  if (t == 1023) {
    bk = (old_off[0] != 0 || old_off[C] != n_old) ? 1 : 0;
    mx = 0;
    for (int w = 0; w < 16; ++w) mx = max(mx, big[w]), bk |= broken[w];
    new_off[C] = (int32_t)(n_old + total);
    *out_max = (bk || *bad) ? -1 : mx;
  }
}

// one wave per cluster: the old members, in their order, at the start of the cluster's new segment
__global__ __launch_bounds__(256) void insert_copy_kernel(const int32_t* __restrict__ old_off, const int32_t* __restrict__ old_mem,
                                                          int C, int64_t n_old, const int32_t* __restrict__ new_off, int64_t n_total,
                                                          int32_t* __restrict__ out_mem) {
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (c >= C) return;
  const int64_t lo = old_off[c], hi = old_off[c + 1], dst = new_off[c];
  for (int64_t j = lo + lane; j < hi; j += 64) {
    const int64_t p = dst + (j - lo);
    if (j >= 0 && j < n_old && p >= 0 && p < n_total) out_mem[p] = old_mem[j];
  }
}

__global__ __launch_bounds__(256) void insert_place_kernel(const int32_t* __restrict__ new_ids, const int32_t* __restrict__ target,
                                                           int n, const int32_t* __restrict__ map, int n_map, int C,
                                                           const int32_t* __restrict__ old_off, const int32_t* __restrict__ new_off,
                                                           int32_t* __restrict__ ticket, int32_t* __restrict__ out_mem) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int c = resolve_target(target, i, map, n_map, C);
    if (c < 0) continue;
    const int slot = atomicAdd(&ticket[c], 1);
    const int64_t p = (int64_t)new_off[c] + (old_off[c + 1] - old_off[c]) + slot;
    if (p < new_off[c + 1]) out_mem[p] = new_ids[i];
  }
}

// one block per cluster: its inserted tail in ascending id order.  Tails up to CI_SORT_LDS are sorted in LDS; a longer tail
// (rare: at most n / CI_SORT_LDS clusters) is rewritten by one ordered pass over the inputs, which are ascending by contract.
__global__ __launch_bounds__(256) void insert_sort_kernel(const int32_t* __restrict__ new_ids, const int32_t* __restrict__ target,
                                                          int n, const int32_t* __restrict__ map, int n_map, int C,
                                                          const int32_t* __restrict__ old_off, const int32_t* __restrict__ new_off,
                                                          const int32_t* __restrict__ hist, int32_t* __restrict__ out_mem) {
  __shared__ int32_t s[CI_SORT_LDS];
  __shared__ int32_t wcount[4];
  const int c = blockIdx.x, t = threadIdx.x;
  const int m = hist[c];
  if (m <= 1) return;
  const int64_t base = (int64_t)new_off[c] + (old_off[c + 1] - old_off[c]);
  if (base + m > new_off[c + 1]) return;  // inconsistent input (reported through out_max)
  if (m <= CI_SORT_LDS) {
    int P = 2;
    while (P < m) P <<= 1;
    for (int i = t; i < P; i += 256) s[i] = i < m ? out_mem[base + i] : INT32_MAX;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1) {
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int i = t; i < P; i += 256) {
          const int ixj = i ^ j;
          if (ixj > i) {
            const int32_t a = s[i], b = s[ixj];
            if ((a > b) == ((i & k) == 0)) {
              s[i] = b;
              s[ixj] = a;
            }
          }
        }
        __syncthreads();
      }
    }
    for (int i = t; i < m; i += 256) out_mem[base + i] = s[i];
    return;
  }
  const int wave = t >> 6, lane = t & 63;
  int64_t written = 0;
  for (int64_t lo = 0; lo < n; lo += 256) {
    const int64_t i = lo + t;
    const bool mine = i < n && resolve_target(target, i, map, n_map, C) == c;
    const uint64_t bal = __ballot(mine);
    const int below = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) wcount[wave] = __popcll(bal);
    __syncthreads();
    int before = 0;
    for (int w = 0; w < wave; ++w) before += wcount[w];
    const int total = wcount[0] + wcount[1] + wcount[2] + wcount[3];
    if (mine && written + before + below < m) out_mem[base + written + before + below] = new_ids[i];
    written += total;
    __syncthreads();
  }
}

// removal mode: is `id` in the strictly ascending list ids[0, n)?
__device__ __forceinline__ bool in_ascending_list(const int32_t* __restrict__ ids, int n, int32_t id) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (ids[mid] < id) lo = mid + 1;
    else hi = mid;
  }
  return lo < n && ids[lo] == id;
}

// one wave per cluster: hist[c] = -(members of the cluster that are in the removal list).  No atomics.
__global__ __launch_bounds__(256) void remove_count_kernel(const int32_t* __restrict__ old_off, const int32_t* __restrict__ old_mem,
                                                           int C, int64_t n_old, const int32_t* __restrict__ ids, int n,
                                                           int32_t* __restrict__ hist) {
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (c >= C) return;  // wave-uniform
  int64_t lo = old_off[c], hi = old_off[c + 1];
  if (lo < 0 || hi > n_old || hi < lo) lo = hi = 0;  // a malformed segment reads nothing (reported through out_max)
  int gone = 0;
  for (int64_t j0 = lo; j0 < hi; j0 += RM_TILE) {
    int32_t m[RM_CHUNKS];
#pragma unroll
    for (int u = 0; u < RM_CHUNKS; ++u) {
      const int64_t j = j0 + 64 * u + lane;
      m[u] = j < hi ? old_mem[j] : 0;
    }
#pragma unroll
    for (int u = 0; u < RM_CHUNKS; ++u) gone += (j0 + 64 * u + lane < hi && in_ascending_list(ids, n, m[u])) ? 1 : 0;
  }
  gone = wave_sum(gone);
  if (lane == 0) hist[c] = -gone;
}

// one wave per cluster: the surviving members, in their order, from the start of the cluster's new segment
__global__ __launch_bounds__(256) void remove_compact_kernel(const int32_t* __restrict__ old_off, const int32_t* __restrict__ old_mem,
                                                             int C, int64_t n_old, const int32_t* __restrict__ ids, int n,
                                                             const int32_t* __restrict__ new_off, int32_t* __restrict__ out_mem) {
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (c >= C) return;  // wave-uniform
  int64_t lo = old_off[c], hi = old_off[c + 1];
  if (lo < 0 || hi > n_old || hi < lo) lo = hi = 0;
  int64_t base = new_off[c];  // next free position of the new segment (wave-uniform)
  for (int64_t j0 = lo; j0 < hi; j0 += RM_TILE) {  // every lane of the wave takes every iteration: the ballots are whole
    int32_t m[RM_CHUNKS];
    bool keep[RM_CHUNKS];
#pragma unroll
    for (int u = 0; u < RM_CHUNKS; ++u) {
      const int64_t j = j0 + 64 * u + lane;
      m[u] = j < hi ? old_mem[j] : 0;
    }
#pragma unroll
    for (int u = 0; u < RM_CHUNKS; ++u) keep[u] = j0 + 64 * u + lane < hi && !in_ascending_list(ids, n, m[u]);
#pragma unroll
    for (int u = 0; u < RM_CHUNKS; ++u) {
      const uint64_t bal = __ballot(keep[u]);
      const int64_t p = base + __popcll(bal & ((1ull << lane) - 1ull));
      if (keep[u] && p >= 0 && p < n_old) out_mem[p] = m[u];  // p <= its old position while the offsets are consistent
      base += __popcll(bal);
    }
  }
}

}  // namespace
}  // namespace gdr

extern "C" int gdr_cluster_centroids(const float* D, int64_t N, int d, const int32_t* offsets, const int32_t* members,
                                     int64_t n_members, int n_clusters, float* out_centroids, int32_t* out_counts,
                                     void* stream_) {
  using namespace gdr;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  GDR_CHECK_ARG(D && offsets && out_centroids && out_counts, "cluster_centroids: null pointer");
  GDR_CHECK_ARG(members || n_members == 0, "cluster_centroids: null members with n_members=%lld", (long long)n_members);
  GDR_CHECK_ARG(N > 0 && n_members >= 0 && n_clusters > 0, "cluster_centroids: bad size N=%lld n_members=%lld n_clusters=%d",
                (long long)N, (long long)n_members, n_clusters);
  GDR_CHECK_ARG(N < ((int64_t)1 << 31) && n_members < ((int64_t)1 << 31),
                "cluster_centroids: N=%lld / n_members=%lld do not fit int32 doc ids", (long long)N, (long long)n_members);
  GDR_CHECK_ARG(d > 0 && d % 4 == 0 && d <= CE_MAX_D, "cluster_centroids: d=%d (needs d %% 4 == 0, 4 <= d <= %d)", d, CE_MAX_D);
  GDR_CHECK_ARG(((uintptr_t)D & 15) == 0 && ((uintptr_t)out_centroids & 15) == 0,
                "cluster_centroids: D and out_centroids must be 16-byte aligned");
  const int d4 = d / 4, S = (d4 + 63) / 64;
  const int64_t waves = (int64_t)n_clusters * S;
  hipLaunchKernelGGL(centroid_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, stream, D, N, d4, S, offsets, members,
                     n_members, n_clusters, out_centroids, out_counts);
  GDR_CHECK_LAUNCH("centroid_kernel");
  return GDR_OK;
}

extern "C" size_t gdr_cluster_insert_workspace_bytes(int n_clusters) {
  if (n_clusters <= 0) return 0;
  return 2 * gdr::align_up((size_t)n_clusters * sizeof(int32_t), 256) + 256;
}

extern "C" int gdr_cluster_insert(const int32_t* offsets, const int32_t* members, int n_clusters, int64_t n_old,
                                  const int32_t* new_ids, const int32_t* new_target, int n_new, const int32_t* target_map,
                                  int n_map, int32_t* out_offsets, int32_t* out_members, int32_t* out_max, void* workspace,
                                  size_t workspace_bytes, void* stream_) {
  using namespace gdr;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  GDR_CHECK_ARG(offsets && out_offsets && out_members && out_max, "cluster_insert: null pointer");
  GDR_CHECK_ARG(members || n_old == 0, "cluster_insert: null members with n_old=%lld", (long long)n_old);
  const bool removal = new_ids && !new_target && n_new > 0;  // new_target == NULL: new_ids are the ids to take out
  GDR_CHECK_ARG((new_ids && new_target) || n_new == 0 || removal, "cluster_insert: null new_ids / new_target with n_new=%d", n_new);
  GDR_CHECK_ARG(n_clusters > 0 && n_old >= 0 && n_new >= 0, "cluster_insert: bad size n_clusters=%d n_old=%lld n_new=%d",
                n_clusters, (long long)n_old, n_new);
  GDR_CHECK_ARG(n_old + (removal ? 0 : n_new) < ((int64_t)1 << 31),
                "cluster_insert: n_old + n_new = %lld does not fit int32 doc ids", (long long)(n_old + n_new));
  GDR_CHECK_ARG(!removal || (target_map == nullptr && n_map == 0),
                "cluster_insert: removal (new_target == NULL) takes no target_map (n_map=%d)", n_map);
  GDR_CHECK_ARG(target_map == nullptr ? n_map == 0 : n_map > 0, "cluster_insert: target_map / n_map=%d disagree", n_map);
  GDR_CHECK_ARG(workspace, "cluster_insert: null workspace");
  const size_t need = gdr_cluster_insert_workspace_bytes(n_clusters);
  if (workspace_bytes < need) {
    set_error("cluster_insert: workspace %zu < %zu bytes", workspace_bytes, need);
    return GDR_ENOSPC;
  }
  char* ws = static_cast<char*>(workspace);
  const size_t hb = align_up((size_t)n_clusters * sizeof(int32_t), 256);
  int32_t* hist = reinterpret_cast<int32_t*>(ws);
  int32_t* ticket = reinterpret_cast<int32_t*>(ws + hb);
  int32_t* bad = reinterpret_cast<int32_t*>(ws + 2 * hb);
  if (hipMemsetAsync(ws, 0, need, stream) != hipSuccess) {
    set_error("cluster_insert: hipMemsetAsync failed");
    return GDR_EHIP;
  }
  if (removal) {
    const dim3 per_cluster((unsigned)((n_clusters + 3) / 4));
    hipLaunchKernelGGL(remove_count_kernel, per_cluster, dim3(256), 0, stream, offsets, members, n_clusters, n_old, new_ids, n_new,
                       hist);
    GDR_CHECK_LAUNCH("remove_count_kernel");
    hipLaunchKernelGGL(insert_scan_kernel, dim3(1), dim3(1024), 0, stream, offsets, hist, n_clusters, n_old, out_offsets, bad,
                       out_max);
    GDR_CHECK_LAUNCH("insert_scan_kernel");
    hipLaunchKernelGGL(remove_compact_kernel, per_cluster, dim3(256), 0, stream, offsets, members, n_clusters, n_old, new_ids,
                       n_new, out_offsets, out_members);
    GDR_CHECK_LAUNCH("remove_compact_kernel");
    return GDR_OK;
  }
  const unsigned gn = (unsigned)std::min<int64_t>(std::max<int64_t>((n_new + 255) / 256, 1), 2048);
  if (n_new > 0) {
    hipLaunchKernelGGL(insert_hist_kernel, dim3(gn), dim3(256), 0, stream, new_target, n_new, target_map, n_map, n_clusters, hist,
                       bad);
    GDR_CHECK_LAUNCH("insert_hist_kernel");
  }
  hipLaunchKernelGGL(insert_scan_kernel, dim3(1), dim3(1024), 0, stream, offsets, hist, n_clusters, n_old, out_offsets, bad,
                     out_max);
  GDR_CHECK_LAUNCH("insert_scan_kernel");
  hipLaunchKernelGGL(insert_copy_kernel, dim3((unsigned)((n_clusters + 3) / 4)), dim3(256), 0, stream, offsets, members, n_clusters,
                     n_old, out_offsets, n_old + n_new, out_members);
  GDR_CHECK_LAUNCH("insert_copy_kernel");
  if (n_new > 0) {
    hipLaunchKernelGGL(insert_place_kernel, dim3(gn), dim3(256), 0, stream, new_ids, new_target, n_new, target_map, n_map,
                       n_clusters, offsets, out_offsets, ticket, out_members);
    GDR_CHECK_LAUNCH("insert_place_kernel");
    hipLaunchKernelGGL(insert_sort_kernel, dim3((unsigned)n_clusters), dim3(256), 0, stream, new_ids, new_target, n_new, target_map,
                       n_map, n_clusters, offsets, out_offsets, hist, out_members);
    GDR_CHECK_LAUNCH("insert_sort_kernel");
  }
  return GDR_OK;
}
