// Hierarchical k-means docid construction: one Lloyd round over every open node of a tree level — the device
// form of Data_process/NQ_dataset/kmeans/kmeans.py's recursive clustering.  The state of a level is a CSR over nodes
// (rows int32[n] = doc ids, ascending inside a node; node_offsets int32[S+1]) and a centroid table fp32[S*k, d].
//
//   gdr_kmeans_assign: one workgroup per work item (node, first row position), KA_TILE = 128 rows, 32 per wave.  The rows are
//     gathered through rows[] into LDS in chunks of KA_KC = 64 columns (whole 256-byte pieces per row), the node's k centroids
//     beside them, and the products run on v_mfma_f32_32x32x2_f32 with the centroids in the row role: a lane ends with the scores
//     of ONE document against 16 (k <= 32) or 32 (k <= 64) centroids, so the argmax is in-lane plus one exchange with lane ^ 32.
//     A document's dot product is one fma chain over the columns in a fixed order (inside every 8 columns: 0, 4, 1, 5, 2, 6, 3,
//     7), whatever tile, node set or launch it sits in; score = dot - 0.5 |c|^2 with the half norms from halfnorm_kernel (fixed
//     order too).  Labels that differ from prev_labels are counted per node with an int atomic (order-free).
//   gdr_kmeans_partition: stable segmented counting sort of every node's rows by label.  Tiles of KP_TILE = 256 rows count their
//     labels (ballots: no atomics), ONE exclusive scan runs over the counts laid out [node][label][tile of the node], and the tiles
//     place their rows at scan value + rank inside the tile.  Nothing depends on arrival order; a child's rows stay ascending.
//   gdr_kmeans_centroids: the update step over the child CSR the partition writes — member means as a fixed-shape two-stage sum
//     (below); gdr_cluster_centroids' one sequential chain per cluster made every root round wait ~2 ms for 30 chains.
//   gdr_kmeans_seed_dist: one greedy k-means++ seeding step over the same (node, tile) work list: fp32 squared
//     distances of every row to its node's T candidates over one pinned summation tree without fma, per-tile integer potentials
//     and maxima.  The draws, the prefix sums and the argmin between the steps are torch (gdr_amd/kmeans.py).
#include "scan.h"

namespace gdr {
namespace {

constexpr int KA_TILE = 128;        // rows per assign work item: 4 waves x 32
constexpr int KA_KC = 64;           // columns staged per step
constexpr int KA_LD = KA_KC + 4;    // LDS row stride (floats): 272 B, so the 16 lanes of a ds_read_b128 group hit 16 distinct bank quads
constexpr int KP_TILE = 256;        // rows per partition work item: one per thread
constexpr int KM_MAX_K = 64;
constexpr int KM_MAX_D = 4096;      // gdr_cluster_centroids' CE_MAX_D: the update step must accept the same d

typedef float f32x16 __attribute__((ext_vector_type(16)));

// 0.5 |c|^2 of every centroid: one wave per centroid, lane l sums its float4 columns l, l + 64, ... in order, then the xor butterfly
__global__ __launch_bounds__(256) void halfnorm_kernel(const float* __restrict__ cent, int64_t n_cent, int d4, float* __restrict__ hn) {
  const int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (c >= n_cent) return;  // wave-uniform
  const float4* p = reinterpret_cast<const float4*>(cent) + c * d4;
  float acc = 0.f;
  for (int i = lane; i < d4; i += 64) {
    const float4 v = p[i];
    acc = fmaf(v.x, v.x, acc);
    acc = fmaf(v.y, v.y, acc);
    acc = fmaf(v.z, v.z, acc);
    acc = fmaf(v.w, v.w, acc);
  }
  acc = wave_sum(acc);
  if (lane == 0) hn[c] = 0.5f * acc;
}

// A work item is valid when it names a node and a row position inside that node's segment; everything a block touches is
// derived from a validated item, so a malformed list reads and writes nothing (status bit 2).
__device__ __forceinline__ bool load_item(const int32_t* work, int t, const int32_t* node_off, int S, int64_t n_rows, int& node,
                                          int& lo, int& hi, int& p0) {
  node = work[2 * t];
  p0 = work[2 * t + 1];
  if (node < 0 || node >= S) return false;
  lo = node_off[node];
  hi = node_off[node + 1];
  return lo >= 0 && hi <= n_rows && lo <= p0 && p0 < hi;
}

template <int NB>  // NB blocks of 32 centroids: k <= 32 * NB
__global__ __launch_bounds__(256) void assign_kernel(const float* __restrict__ D, int64_t N, int d4, const int32_t* __restrict__ rows,
                                                     int64_t n_rows, const int32_t* __restrict__ node_off, int S,
                                                     const float* __restrict__ cent, int k, const float* __restrict__ hn,
                                                     const int32_t* __restrict__ work, const int32_t* __restrict__ prev,
                                                     int32_t* __restrict__ labels, float* __restrict__ score,
                                                     int32_t* __restrict__ changed, int32_t* __restrict__ status) {
  __shared__ float sx[4][32][KA_LD];
  __shared__ float sc[NB * 32][KA_LD];
  int node, lo, hi, p0;
  if (!load_item(work, blockIdx.x, node_off, S, n_rows, node, lo, hi, p0)) {  // block-uniform
    if (threadIdx.x == 0) atomicOr(status, 2);
    return;
  }
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, h = l >> 5, r32 = l & 31;
  const int end = min(hi, p0 + KA_TILE);
  const float4* D4 = reinterpret_cast<const float4*>(D);
  const float4* C4 = reinterpret_cast<const float4*>(cent) + (int64_t)node * k * d4;
  // staging role: instruction u of a chunk fetches the 256-byte pieces of rows 4u .. 4u+3 of this wave (16 lanes per row)
  const int srow = l >> 4, scol = l & 15;
  int64_t rbase[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const int p = p0 + 32 * w + 4 * u + srow;
    const int32_t id = p < end ? rows[p] : -1;
    rbase[u] = (id >= 0 && id < N) ? (int64_t)id * d4 : -1;  // an id outside the corpus reads as a zero row
  }
  f32x16 acc[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[b][i] = 0.f;
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);

  // the next chunk's pieces are fetched into registers while the MFMAs of the current one run
  float4 x[8], cv[2 * NB];
  auto fetch = [&](int c4) {
    const bool col_ok = c4 + scol < d4;
#pragma unroll
    for (int u = 0; u < 8; ++u) x[u] = (rbase[u] >= 0 && col_ok) ? D4[rbase[u] + c4 + scol] : zero4;
#pragma unroll
    for (int i = 0; i < 2 * NB; ++i) {
      const int j = (tid + 256 * i) >> 4;  // centroid 0 .. 32 NB - 1; its column piece is scol as well
      cv[i] = (j < k && col_ok) ? C4[(int64_t)j * d4 + c4 + scol] : zero4;
    }
  };
  fetch(0);
  for (int c4 = 0; c4 < d4; c4 += KA_KC / 4) {
#pragma unroll
    for (int u = 0; u < 8; ++u) *reinterpret_cast<float4*>(&sx[w][4 * u + srow][4 * scol]) = x[u];
#pragma unroll
    for (int i = 0; i < 2 * NB; ++i) *reinterpret_cast<float4*>(&sc[(tid + 256 * i) >> 4][4 * scol]) = cv[i];
    __syncthreads();
    if (c4 + KA_KC / 4 < d4) fetch(c4 + KA_KC / 4);
#pragma unroll
    for (int s = 0; s < KA_KC / 8; ++s) {
      // lane (r32, h) supplies columns 8 s + 4 h + e of document r32 (B) and of centroid r32 (A) to the e-th MFMA
      const float4 b = *reinterpret_cast<const float4*>(&sx[w][r32][8 * s + 4 * h]);
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        const float4 a = *reinterpret_cast<const float4*>(&sc[32 * nb + r32][8 * s + 4 * h]);
        acc[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc[nb], 0, 0, 0);
        acc[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc[nb], 0, 0, 0);
        acc[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc[nb], 0, 0, 0);
        acc[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc[nb], 0, 0, 0);
      }
    }
    __syncthreads();
  }

  // accumulator register g of lane (r32, h): document r32 of the wave, centroid 32 nb + (g & 3) + 8 (g >> 2) + 4 h — ascending in g
  float best = -INFINITY;
  int bi = INT32_MAX;
  const float* hn_node = hn + (int64_t)node * k;
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      const int j = 32 * nb + (g & 3) + 8 * (g >> 2) + 4 * h;
      if (j < k) {
        const float sco = acc[nb][g] - hn_node[j];
        if (sco > best) {  // strict: a tie keeps the lower centroid
          best = sco;
          bi = j;
        }
      }
    }
  }
  const float ob = __shfl_xor(best, 32);
  const int oi = __shfl_xor(bi, 32);
  if (ob > best || (ob == best && oi < bi)) {
    best = ob;
    bi = oi;
  }
  if (bi == INT32_MAX) bi = 0;  // every score NaN: centroid 0, as an argmax over NaNs gives
  const int p = p0 + 32 * w + r32;
  const bool mine = h == 0 && p < end;
  bool diff = false;
  if (mine) {
    diff = prev ? prev[p] != bi : true;
    labels[p] = bi;
    score[p] = best;
  }
  const int n_diff = __popcll(__ballot(diff));
  if (l == 0 && n_diff) atomicAdd(&changed[node], n_diff);
}

struct PartItem {
  int node, lo, hi, p0, q, ntiles, first;  // tile q of the node's ntiles; `first` = index of the node's tile 0 in the work list
};
__device__ __forceinline__ bool load_part_item(const int32_t* work, int t, int n_work, const int32_t* node_off, int S, int64_t n_rows,
                                               PartItem& it) {
  if (!load_item(work, t, node_off, S, n_rows, it.node, it.lo, it.hi, it.p0)) return false;
  if ((it.p0 - it.lo) % KP_TILE) return false;
  it.q = (it.p0 - it.lo) / KP_TILE;
  it.ntiles = (it.hi - it.lo + KP_TILE - 1) / KP_TILE;
  it.first = t - it.q;
  return it.first >= 0 && it.first + it.ntiles <= n_work;
}

// rank of a thread's row among the rows of its tile that carry the same label and come before it, and the tile's label counts
// in cnt[0][lab] .. — ballots only: the result is a function of the labels, not of any arrival order
__device__ __forceinline__ int tile_rank(int lab, int k, int32_t (*cnt)[KM_MAX_K]) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  int rank = 0;
  for (int j = 0; j < k; ++j) {
    const uint64_t bal = __ballot(lab == j);
    if (lane == 0) cnt[wave][j] = __popcll(bal);
    if (lab == j) rank = __popcll(bal & ((1ull << lane) - 1ull));
  }
  __syncthreads();
  if (lab >= 0)
    for (int w2 = 0; w2 < wave; ++w2) rank += cnt[w2][lab];
  return rank;
}

__global__ __launch_bounds__(256) void part_hist_kernel(const int32_t* __restrict__ labels, int64_t n_rows,
                                                        const int32_t* __restrict__ node_off, int S, int k,
                                                        const int32_t* __restrict__ work, int n_work, int32_t* __restrict__ hist,
                                                        int32_t* __restrict__ status) {
  __shared__ int32_t cnt[4][KM_MAX_K];
  PartItem it;
  if (!load_part_item(work, blockIdx.x, n_work, node_off, S, n_rows, it)) {
    if (threadIdx.x == 0) atomicOr(status, 2);
    return;
  }
  const int p = it.p0 + threadIdx.x;
  int lab = p < min(it.hi, it.p0 + KP_TILE) ? labels[p] : -1;
  if (lab >= k || (lab < 0 && p < min(it.hi, it.p0 + KP_TILE))) {
    atomicOr(status, 1);
    lab = -1;
  }
  tile_rank(lab, k, cnt);
  const int j = threadIdx.x;
  if (j < k) hist[(int64_t)k * it.first + (int64_t)j * it.ntiles + it.q] = cnt[0][j] + cnt[1][j] + cnt[2][j] + cnt[3][j];
}

// one block: exclusive scan of m int32 counts in place (m = n_work * k < 2^31, total <= n_rows < 2^31)
__global__ __launch_bounds__(1024) void part_scan_kernel(int32_t* __restrict__ a, int64_t m) {
  __shared__ int32_t wsum[16];
  const int t = threadIdx.x;
  const int64_t per = (m + 1023) / 1024, i0 = t * per, i1 = min(m, i0 + per);
  int32_t sum = 0;
  for (int64_t i = i0; i < i1; ++i) sum += a[i];
  int32_t run = block_scan_once<1024>(sum, wsum);
  for (int64_t i = i0; i < i1; ++i) {
    const int32_t c = a[i];
    a[i] = run;
    run += c;
  }
}

__global__ __launch_bounds__(256) void part_place_kernel(const int32_t* __restrict__ rows, const int32_t* __restrict__ labels,
                                                         int64_t n_rows, const int32_t* __restrict__ node_off, int S, int k,
                                                         const int32_t* __restrict__ work, int n_work,
                                                         const int32_t* __restrict__ base, int32_t* __restrict__ out_rows,
                                                         int32_t* __restrict__ child_off) {
  __shared__ int32_t cnt[4][KM_MAX_K];
  PartItem it;
  if (!load_part_item(work, blockIdx.x, n_work, node_off, S, n_rows, it)) return;  // reported by part_hist_kernel
  const int p = it.p0 + threadIdx.x;
  const bool in = p < min(it.hi, it.p0 + KP_TILE);
  int lab = in ? labels[p] : -1;
  if (lab >= k) lab = -1;
  const int rank = tile_rank(lab, k, cnt);
  const int64_t e0 = (int64_t)k * it.first;  // the node's first scan entry: its children start at the node's own `lo`
  const int32_t b0 = base[e0];
  if (lab >= 0) {
    const int64_t pos = (int64_t)it.lo + (base[e0 + (int64_t)lab * it.ntiles + it.q] - b0) + rank;
    if (pos >= it.lo && pos < it.hi) out_rows[pos] = rows[p];
  }
  const int j = threadIdx.x;
  if (it.q == 0 && j < k) child_off[(int64_t)it.node * k + j] = it.lo + (base[e0 + (int64_t)j * it.ntiles] - b0);
}

__global__ void part_tail_kernel(const int32_t* __restrict__ node_off, int S, int k, int32_t* __restrict__ child_off) {
  if (threadIdx.x == 0 && blockIdx.x == 0) child_off[(int64_t)S * k] = node_off[S];
}

// ---- update step: member means as a fixed-shape two-stage sum ------------------------------------------------------------
// A child's members are cut into chunks of KC_CHUNK, counted from the child's own start; a chunk is summed member after member
// (fp32, from 0), the chunk sums are added in chunk order, then ONE correctly rounded division.  The result is a function of the
// child's member list alone; for a child of <= KC_CHUNK members it is gdr_cluster_centroids' sequential sum bit for bit.
// Stage 1 runs one wave per (slot of KC_CHUNK row positions, 256-column slice) and sums every chunk that STARTS in its slot: at most
// one later chunk of the child that reaches into the slot (two children cannot both straddle the slot's first position), and chunk 0
// of every child that starts in it — of which only the last can be longer than a chunk.  So partial[2 slot + (chunk 0 ? 1 : 0)]
// holds each long child's chunk sums without any index structure.
constexpr int KC_CHUNK = 256;
// rows[a] .. rows[b - 1] of D4 at this lane's column, added in that order from 0; 8 rows in flight, every load of a batch issued before the
// first add, the next batch's ids loaded beside the current rows — centroid_kernel's loop (cluster_insert.hip), written out there
__device__ __forceinline__ float4 seq_sum(const float4* __restrict__ D4, int64_t N, int d4, int col, bool on,
                                          const int32_t* __restrict__ rows, int a, int b) {
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  int32_t mid[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) mid[u] = a + u < b ? rows[a + u] : -1;
  for (int j = a; j < b; j += 8) {
    float4 x[8];
    bool ok[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int32_t m = mid[u];
      ok[u] = m >= 0 && m < N;
      x[u] = (ok[u] && on) ? D4[(int64_t)m * d4 + col] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) mid[u] = b - j > 8 + u ? rows[j + 8 + u] : -1;  // no j + 8 + u past INT_MAX
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (ok[u]) {
        acc.x = acc.x + x[u].x;
        acc.y = acc.y + x[u].y;
        acc.z = acc.z + x[u].z;
        acc.w = acc.w + x[u].w;
      }
    }
  }
  return acc;
}

__device__ __forceinline__ float4 div4(float4 a, float n) {
  return make_float4(__fdiv_rn(a.x, n), __fdiv_rn(a.y, n), __fdiv_rn(a.z, n), __fdiv_rn(a.w, n));
}

__global__ __launch_bounds__(256) void cent_chunk_kernel(const float* __restrict__ D, int64_t N, int d4, int S,
                                                         const int32_t* __restrict__ off, const int32_t* __restrict__ rows, int n,
                                                         int C, float* __restrict__ cent, float* __restrict__ partial) {
  const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int n_slots = (n + KC_CHUNK - 1) / KC_CHUNK;
  if (w >= (int64_t)n_slots * S) return;  // wave-uniform
  const int g = (int)(w / S), s = (int)(w % S);
  const int col = lane + 64 * s;
  const bool on = col < d4;
  const float4* D4 = reinterpret_cast<const float4*>(D);
  const int P = g * KC_CHUNK;
  int lo_c = 0, hi_c = C;  // the last child whose offset is <= P: the one that holds position P
  while (hi_c - lo_c > 1) {
    const int mid = (lo_c + hi_c) >> 1;
    if (off[mid] <= P) lo_c = mid; else hi_c = mid;
  }
  for (int c = lo_c; c < C; ++c) {
    const int lo = off[c], hi = off[c + 1];
    if (lo < 0 || hi < lo || hi > n) break;  // a malformed CSR reads nothing further
    if (lo >= P + KC_CHUNK) break;
    if (hi == lo) continue;
    const int start = lo >= P ? lo : lo + (P - lo + KC_CHUNK - 1) / KC_CHUNK * KC_CHUNK;
    if (start >= hi || start >= P + KC_CHUNK) continue;
    const float4 acc = seq_sum(D4, N, d4, col, on, rows, start, min(start + KC_CHUNK, hi));
    if (!on) continue;
    if (hi - lo <= KC_CHUNK)
      reinterpret_cast<float4*>(cent)[(int64_t)c * d4 + col] = div4(acc, (float)(hi - lo));
    else
      reinterpret_cast<float4*>(partial)[((int64_t)2 * g + (start == lo ? 1 : 0)) * d4 + col] = acc;
  }
}

__global__ __launch_bounds__(256) void cent_final_kernel(int d4, int S, const int32_t* __restrict__ off, int n, int C,
                                                         const float* __restrict__ partial, float* __restrict__ cent,
                                                         int32_t* __restrict__ counts) {
  const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (w >= (int64_t)C * S) return;  // wave-uniform
  const int c = (int)(w / S), s = (int)(w % S);
  const int col = lane + 64 * s;
  int lo = off[c], hi = off[c + 1];
  if (lo < 0 || hi < lo || hi > n) lo = hi = 0;
  const int cnt = hi - lo;
  if (s == 0 && lane == 0) counts[c] = cnt;
  if (col >= d4) return;
  float4* out = reinterpret_cast<float4*>(cent) + (int64_t)c * d4 + col;
  if (cnt == 0) {
    *out = make_float4(0.f, 0.f, 0.f, 0.f);
  } else if (cnt > KC_CHUNK) {
    const float4* P4 = reinterpret_cast<const float4*>(partial);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int i = 0, st = lo; st < hi; ++i, st += KC_CHUNK) {
      const float4 v = P4[((int64_t)2 * (st / KC_CHUNK) + (i == 0 ? 1 : 0)) * d4 + col];
      acc.x = acc.x + v.x;
      acc.y = acc.y + v.y;
      acc.z = acc.z + v.z;
      acc.w = acc.w + v.w;
    }
    *out = div4(acc, (float)cnt);
  }
}

// ---- k-means++ seeding: one greedy step over every node of a level (include/gdr_hip_kmeans_seed.h) -------------------------------
// d2(x, c) = sum_j (x_j - c_j)^2 with every operation rounded on its own (no fma) and ONE summation tree per (row, centre): lane j of
// the 16 lanes of a row takes the 16-byte pieces j, j + 16, ... in order (inside a piece x, y, z, w; a chain from 0), then the xor
// butterfly 8, 4, 2, 1.  A work item is KS_TILE = 128 row positions: 16 rows per pass, 8 passes kept in registers so that a lane
// fetches its pieces of the T candidate rows once per 8 rows.  The potentials are integers (order-free): floor(v * 2^(22 - e)).
constexpr int KS_TILE = 128;
constexpr int KS_MAX_T = 6;  // 2 + floor(ln 64)

__device__ __forceinline__ void sq_acc(float& acc, const float4 x, const float4 c) {
#pragma clang fp contract(off)
  float t = x.x - c.x;
  acc = acc + t * t;
  t = x.y - c.y;
  acc = acc + t * t;
  t = x.z - c.z;
  acc = acc + t * t;
  t = x.w - c.w;
  acc = acc + t * t;
}

__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}

template <int T>
__global__ __launch_bounds__(256) void seed_dist_kernel(const float* __restrict__ D, int64_t N, int d4, const int32_t* __restrict__ rows,
                                                        int64_t n_rows, const int32_t* __restrict__ node_off, int S,
                                                        const int32_t* __restrict__ work, const int32_t* __restrict__ cand,
                                                        const float* __restrict__ d2, const int32_t* __restrict__ e_node,
                                                        float* __restrict__ out_d2, long long* __restrict__ out_pot,
                                                        float* __restrict__ out_max, int32_t* __restrict__ status) {
  __shared__ long long s_pot[4][T];
  __shared__ float s_max[4][T];
  int node, lo, hi, p0;
  if (!load_item(work, blockIdx.x, node_off, S, n_rows, node, lo, hi, p0)) {  // block-uniform
    if (threadIdx.x == 0) atomicOr(status, 2);
    return;
  }
  const int tid = threadIdx.x, g = tid >> 4, j = tid & 15;
  const int end = min(hi, p0 + KS_TILE);
  const float4* D4 = reinterpret_cast<const float4*>(D);
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  int64_t xb[8], cb[T];
  bool has[T];
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const int p = p0 + 16 * u + g;
    const int32_t id = p < end ? rows[p] : -1;
    xb[u] = (id >= 0 && id < N) ? (int64_t)id * d4 : -1;  // an id outside the corpus reads as a zero row
  }
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const int32_t id = cand[(int64_t)node * T + t];
    has[t] = id >= 0;  // a negative candidate: the column is the current d2
    cb[t] = (id >= 0 && id < N) ? (int64_t)id * d4 : -1;
  }
  float acc[8][T];
#pragma unroll
  for (int u = 0; u < 8; ++u)
#pragma unroll
    for (int t = 0; t < T; ++t) acc[u][t] = 0.f;
  for (int c = j; c < d4; c += 16) {
    float4 cv[T], x[8];
#pragma unroll
    for (int t = 0; t < T; ++t) cv[t] = cb[t] >= 0 ? D4[cb[t] + c] : zero4;
#pragma unroll
    for (int u = 0; u < 8; ++u) x[u] = xb[u] >= 0 ? D4[xb[u] + c] : zero4;
#pragma unroll
    for (int u = 0; u < 8; ++u)
#pragma unroll
      for (int t = 0; t < T; ++t) sq_acc(acc[u][t], x[u], cv[t]);
  }
#pragma unroll
  for (int m = 8; m >= 1; m >>= 1)
#pragma unroll
    for (int u = 0; u < 8; ++u)
#pragma unroll
      for (int t = 0; t < T; ++t) acc[u][t] = add_rn(acc[u][t], __shfl_xor(acc[u][t], m));

  // lane j < T of a row's 16 lanes owns column j: it stores the column and sums its weights over the lane's 8 rows
  const int e = max(-1000, min(1000, e_node[node]));
  const double scale = __longlong_as_double((long long)(1045 - e) << 52);  // 2^(22 - e)
  long long pot = 0;
  float mx = 0.f;
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const int p = p0 + 16 * u + g;
    if (p < end) {
      const float cur = d2[p];
#pragma unroll
      for (int t = 0; t < T; ++t) {
        if (j == t) {
          const float v = has[t] ? fminf(cur, acc[u][t]) : cur;
          out_d2[(int64_t)p * T + t] = v;
          pot += (long long)fmin((double)v * scale, 4194303.0);  // v >= 0: the conversion truncates = floor; v >= 2^e saturates
          mx = fmaxf(mx, v);
        }
      }
    }
  }
  pot += __shfl_xor(pot, 16);
  pot += __shfl_xor(pot, 32);
  mx = fmaxf(mx, __shfl_xor(mx, 16));
  mx = fmaxf(mx, __shfl_xor(mx, 32));
  if ((tid & 63) < T) {
    s_pot[tid >> 6][tid & 63] = pot;
    s_max[tid >> 6][tid & 63] = mx;
  }
  __syncthreads();
  if (tid < T) {
    out_pot[(int64_t)blockIdx.x * T + tid] = s_pot[0][tid] + s_pot[1][tid] + s_pot[2][tid] + s_pot[3][tid];
    out_max[(int64_t)blockIdx.x * T + tid] = fmaxf(fmaxf(s_max[0][tid], s_max[1][tid]), fmaxf(s_max[2][tid], s_max[3][tid]));
  }
}

}  // namespace
}  // namespace gdr

extern "C" int gdr_kmeans_assign_tile(void) { return gdr::KA_TILE; }
extern "C" int gdr_kmeans_partition_tile(void) { return gdr::KP_TILE; }

extern "C" size_t gdr_kmeans_assign_workspace_bytes(int n_nodes, int k) {
  if (n_nodes <= 0 || k <= 0) return 0;
  return gdr::align_up((size_t)n_nodes * (size_t)k * sizeof(float), 256);
}

extern "C" int gdr_kmeans_assign(const float* D, int64_t N, int d, const int32_t* rows, int64_t n_rows, const int32_t* node_offsets,
                                 int n_nodes, const float* centroids, int k, const int32_t* work, int n_work,
                                 const int32_t* prev_labels, int32_t* out_labels, float* out_score, int32_t* out_changed,
                                 int32_t* out_status, void* workspace, size_t workspace_bytes, void* stream_) {
  using namespace gdr;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  GDR_CHECK_ARG(D && rows && node_offsets && centroids && work && out_labels && out_score && out_changed && out_status,
                "kmeans_assign: null pointer");
  GDR_CHECK_ARG(N > 0 && N < ((int64_t)1 << 31), "kmeans_assign: N=%lld does not fit int32 doc ids", (long long)N);
  GDR_CHECK_ARG(n_rows > 0 && n_rows < ((int64_t)1 << 31) && n_nodes > 0 && n_work > 0,
                "kmeans_assign: bad size n_rows=%lld n_nodes=%d n_work=%d", (long long)n_rows, n_nodes, n_work);
  GDR_CHECK_ARG(d > 0 && d % 4 == 0 && d <= KM_MAX_D, "kmeans_assign: d=%d (needs d %% 4 == 0, 4 <= d <= %d)", d, KM_MAX_D);
  GDR_CHECK_ARG(k >= 2 && k <= KM_MAX_K, "kmeans_assign: k=%d (needs 2 <= k <= %d)", k, KM_MAX_K);
  GDR_CHECK_ARG((int64_t)n_nodes * k < ((int64_t)1 << 31), "kmeans_assign: n_nodes * k = %lld does not fit int32",
                (long long)n_nodes * k);
  GDR_CHECK_ARG(((uintptr_t)D & 15) == 0 && ((uintptr_t)centroids & 15) == 0, "kmeans_assign: D and centroids must be 16-byte aligned");
  GDR_CHECK_ARG(workspace, "kmeans_assign: null workspace");
  const size_t need = gdr_kmeans_assign_workspace_bytes(n_nodes, k);
  if (workspace_bytes < need) {
    set_error("kmeans_assign: workspace %zu < %zu bytes", workspace_bytes, need);
    return GDR_ENOSPC;
  }
  float* hn = static_cast<float*>(workspace);
  const int d4 = d / 4;
  if (hipMemsetAsync(out_changed, 0, (size_t)n_nodes * sizeof(int32_t), stream) != hipSuccess ||
      hipMemsetAsync(out_status, 0, sizeof(int32_t), stream) != hipSuccess) {
    set_error("kmeans_assign: hipMemsetAsync failed");
    return GDR_EHIP;
  }
  const int64_t n_cent = (int64_t)n_nodes * k;
  hipLaunchKernelGGL(halfnorm_kernel, dim3((unsigned)((n_cent + 3) / 4)), dim3(256), 0, stream, centroids, n_cent, d4, hn);
  GDR_CHECK_LAUNCH("kmeans halfnorm_kernel");
  if (k <= 32)
    hipLaunchKernelGGL(assign_kernel<1>, dim3((unsigned)n_work), dim3(256), 0, stream, D, N, d4, rows, n_rows, node_offsets, n_nodes,
                       centroids, k, hn, work, prev_labels, out_labels, out_score, out_changed, out_status);
  else
    hipLaunchKernelGGL(assign_kernel<2>, dim3((unsigned)n_work), dim3(256), 0, stream, D, N, d4, rows, n_rows, node_offsets, n_nodes,
                       centroids, k, hn, work, prev_labels, out_labels, out_score, out_changed, out_status);
  GDR_CHECK_LAUNCH("kmeans assign_kernel");
  return GDR_OK;
}

extern "C" size_t gdr_kmeans_partition_workspace_bytes(int n_work, int k) {
  if (n_work <= 0 || k <= 0) return 0;
  return gdr::align_up((size_t)n_work * (size_t)k * sizeof(int32_t), 256);
}

extern "C" int gdr_kmeans_partition(const int32_t* rows, const int32_t* labels, int64_t n_rows, const int32_t* node_offsets,
                                    int n_nodes, int k, const int32_t* work, int n_work, int32_t* out_rows,
                                    int32_t* out_child_offsets, int32_t* out_status, void* workspace, size_t workspace_bytes,
                                    void* stream_) {
  using namespace gdr;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  GDR_CHECK_ARG(rows && labels && node_offsets && work && out_rows && out_child_offsets && out_status,
                "kmeans_partition: null pointer");
  GDR_CHECK_ARG(n_rows > 0 && n_rows < ((int64_t)1 << 31) && n_nodes > 0 && n_work > 0,
                "kmeans_partition: bad size n_rows=%lld n_nodes=%d n_work=%d", (long long)n_rows, n_nodes, n_work);
  GDR_CHECK_ARG(k >= 2 && k <= KM_MAX_K, "kmeans_partition: k=%d (needs 2 <= k <= %d)", k, KM_MAX_K);
  GDR_CHECK_ARG((int64_t)n_nodes * k < ((int64_t)1 << 31) - 1 && (int64_t)n_work * k < ((int64_t)1 << 31),
                "kmeans_partition: n_nodes * k or n_work * k does not fit int32");
  GDR_CHECK_ARG(workspace, "kmeans_partition: null workspace");
  const size_t need = gdr_kmeans_partition_workspace_bytes(n_work, k);
  if (workspace_bytes < need) {
    set_error("kmeans_partition: workspace %zu < %zu bytes", workspace_bytes, need);
    return GDR_ENOSPC;
  }
  int32_t* hist = static_cast<int32_t*>(workspace);
  const int64_t m = (int64_t)n_work * k;
  // a node no work item covers keeps -1 in its child offsets; an item that fails validation leaves its scan entries at 0
  if (hipMemsetAsync(hist, 0, need, stream) != hipSuccess || hipMemsetAsync(out_status, 0, sizeof(int32_t), stream) != hipSuccess ||
      hipMemsetAsync(out_child_offsets, 0xFF, ((size_t)n_nodes * k + 1) * sizeof(int32_t), stream) != hipSuccess) {
    set_error("kmeans_partition: hipMemsetAsync failed");
    return GDR_EHIP;
  }
  hipLaunchKernelGGL(part_hist_kernel, dim3((unsigned)n_work), dim3(256), 0, stream, labels, n_rows, node_offsets, n_nodes, k, work,
                     n_work, hist, out_status);
  GDR_CHECK_LAUNCH("kmeans part_hist_kernel");
  hipLaunchKernelGGL(part_scan_kernel, dim3(1), dim3(1024), 0, stream, hist, m);
  GDR_CHECK_LAUNCH("kmeans part_scan_kernel");
  hipLaunchKernelGGL(part_place_kernel, dim3((unsigned)n_work), dim3(256), 0, stream, rows, labels, n_rows, node_offsets, n_nodes, k,
                     work, n_work, hist, out_rows, out_child_offsets);
  GDR_CHECK_LAUNCH("kmeans part_place_kernel");
  hipLaunchKernelGGL(part_tail_kernel, dim3(1), dim3(64), 0, stream, node_offsets, n_nodes, k, out_child_offsets);
  GDR_CHECK_LAUNCH("kmeans part_tail_kernel");
  return GDR_OK;
}

extern "C" size_t gdr_kmeans_centroids_workspace_bytes(int64_t n_rows, int d) {
  if (n_rows <= 0 || d <= 0) return 0;
  return gdr::align_up((size_t)2 * (size_t)((n_rows + gdr::KC_CHUNK - 1) / gdr::KC_CHUNK) * (size_t)d * sizeof(float), 256);
}

extern "C" int gdr_kmeans_centroids(const float* D, int64_t N, int d, const int32_t* child_offsets, const int32_t* rows,
                                    int64_t n_rows, int n_children, float* out_centroids, int32_t* out_counts, void* workspace,
                                    size_t workspace_bytes, void* stream_) {
  using namespace gdr;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  GDR_CHECK_ARG(D && child_offsets && rows && out_centroids && out_counts, "kmeans_centroids: null pointer");
  GDR_CHECK_ARG(N > 0 && N < ((int64_t)1 << 31) && n_rows > 0 && n_rows < ((int64_t)1 << 31) && n_children > 0,
                "kmeans_centroids: bad size N=%lld n_rows=%lld n_children=%d", (long long)N, (long long)n_rows, n_children);
  GDR_CHECK_ARG(d > 0 && d % 4 == 0 && d <= KM_MAX_D, "kmeans_centroids: d=%d (needs d %% 4 == 0, 4 <= d <= %d)", d, KM_MAX_D);
  GDR_CHECK_ARG(((uintptr_t)D & 15) == 0 && ((uintptr_t)out_centroids & 15) == 0 && ((uintptr_t)workspace & 15) == 0,
                "kmeans_centroids: D, out_centroids and workspace must be 16-byte aligned");
  GDR_CHECK_ARG(workspace, "kmeans_centroids: null workspace");
  const size_t need = gdr_kmeans_centroids_workspace_bytes(n_rows, d);
  if (workspace_bytes < need) {
    set_error("kmeans_centroids: workspace %zu < %zu bytes", workspace_bytes, need);
    return GDR_ENOSPC;
  }
  const int d4 = d / 4, S = (d4 + 63) / 64;
  const int64_t slots = (n_rows + KC_CHUNK - 1) / KC_CHUNK;
  float* partial = static_cast<float*>(workspace);
  hipLaunchKernelGGL(cent_chunk_kernel, dim3((unsigned)((slots * S + 3) / 4)), dim3(256), 0, stream, D, N, d4, S, child_offsets, rows,
                     (int)n_rows, n_children, out_centroids, partial);
  GDR_CHECK_LAUNCH("kmeans cent_chunk_kernel");
  hipLaunchKernelGGL(cent_final_kernel, dim3((unsigned)(((int64_t)n_children * S + 3) / 4)), dim3(256), 0, stream, d4, S,
                     child_offsets, (int)n_rows, n_children, partial, out_centroids, out_counts);
  GDR_CHECK_LAUNCH("kmeans cent_final_kernel");
  return GDR_OK;
}

extern "C" int gdr_kmeans_seed_tile(void) { return gdr::KS_TILE; }

// the step keeps no scratch: every partial it forms is one of its outputs
extern "C" size_t gdr_kmeans_seed_workspace_bytes(int n_nodes, int n_work, int n_trials) { return 0; }

extern "C" int gdr_kmeans_seed_dist(const float* D, int64_t N, int d, const int32_t* rows, int64_t n_rows, const int32_t* node_offsets,
                                    int n_nodes, const int32_t* work, int n_work, const int32_t* cand, int n_trials, const float* d2,
                                    const int32_t* e, float* out_cand_d2, int64_t* out_pot, float* out_max, int32_t* out_status,
                                    void* workspace, size_t workspace_bytes, void* stream_) {
  using namespace gdr;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  GDR_CHECK_ARG(D && rows && node_offsets && work && cand && d2 && e && out_cand_d2 && out_pot && out_max && out_status,
                "kmeans_seed_dist: null pointer");
  GDR_CHECK_ARG(N > 0 && N < ((int64_t)1 << 31), "kmeans_seed_dist: N=%lld does not fit int32 doc ids", (long long)N);
  GDR_CHECK_ARG(n_rows > 0 && n_rows < ((int64_t)1 << 31) && n_nodes > 0 && n_work > 0,
                "kmeans_seed_dist: bad size n_rows=%lld n_nodes=%d n_work=%d", (long long)n_rows, n_nodes, n_work);
  GDR_CHECK_ARG(d > 0 && d % 4 == 0 && d <= KM_MAX_D, "kmeans_seed_dist: d=%d (needs d %% 4 == 0, 4 <= d <= %d)", d, KM_MAX_D);
  GDR_CHECK_ARG(n_trials >= 1 && n_trials <= KS_MAX_T, "kmeans_seed_dist: n_trials=%d (needs 1 <= n_trials <= %d)", n_trials, KS_MAX_T);
  GDR_CHECK_ARG(((uintptr_t)D & 15) == 0, "kmeans_seed_dist: D must be 16-byte aligned");
  (void)workspace;
  (void)workspace_bytes;
  if (hipMemsetAsync(out_status, 0, sizeof(int32_t), stream) != hipSuccess) {
    set_error("kmeans_seed_dist: hipMemsetAsync failed");
    return GDR_EHIP;
  }
  const int d4 = d / 4;
  long long* pot = reinterpret_cast<long long*>(out_pot);
#define GDR_SEED_LAUNCH(T)                                                                                                          \
  hipLaunchKernelGGL(seed_dist_kernel<T>, dim3((unsigned)n_work), dim3(256), 0, stream, D, N, d4, rows, n_rows, node_offsets, n_nodes, \
                     work, cand, d2, e, out_cand_d2, pot, out_max, out_status)
  switch (n_trials) {
    case 1: GDR_SEED_LAUNCH(1); break;
    case 2: GDR_SEED_LAUNCH(2); break;
    case 3: GDR_SEED_LAUNCH(3); break;
    case 4: GDR_SEED_LAUNCH(4); break;
    case 5: GDR_SEED_LAUNCH(5); break;
    default: GDR_SEED_LAUNCH(6); break;
  }
#undef GDR_SEED_LAUNCH
  GDR_CHECK_LAUNCH("kmeans seed_dist_kernel");
  return GDR_OK;
}
