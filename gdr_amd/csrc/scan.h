// Device helpers of the integer "plan" kernels (count -> scan -> place): THE wave scan, THE one-workgroup exclusive prefix in its two
// forms, and THE masked word of a row bitmap.  Every such kernel of the library goes through these; workgroups are one-dimensional.
//
//   round form        the workgroup walks its items NT at a time (thread t owns item base + t): BlockScan<NT>::round per step, a carry
//                     between the steps (rows_units_kernel, sim_rows.hip, is this loop written out: it measured slower through the struct)
//   single-shot form  thread t owns ceil(n / NT) CONSECUTIVE items and sums them itself: block_scan_once over the NT thread sums, one barrier
//
// NOT copies of these, and not to be folded in (different algorithms):
//   - find_bin's SUFFIX scan over the radix histogram (sim_topk.hip);
//   - the ballot + popcount ranks: beam.hip's select, sim_stream.hip's list appends, kmeans.hip's tile_rank, cluster_insert.hip's
//     remove_compact_kernel and insert_sort_kernel — a rank among set predicate bits, not a prefix of counts;
//   - the float butterflies that pin a rounding (add_rn) or carry a (value, index) pair: kmeans.hip's argmax exchange and seeding
//     sums, beam.hip's and sim_topk.hip's paired maxima.
#pragma once
#include "common.h"

namespace gdr {

// inclusive prefix over the 64 lanes of a wave (every lane must call it); lane = threadIdx.x & 63, which every caller holds already
template <typename T>
__device__ __forceinline__ T wave_scan_incl(T v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T t = __shfl_up(v, o);
    if (lane >= o) v += t;
  }
  return v;
}

// Round form.  The caller owns the LDS: wsum[NT / 64] and one carry word.  EVERY thread of the workgroup calls round() the same number
// of times (a workgroup-uniform trip count): it holds barriers.  round(v) = the sum of every value handed in before this thread's —
// all earlier rounds, and the lower threads of this one.  Two barriers per round: the carry a round leaves is ordered before its next
// read by the next round's first barrier (or by that of total(), the sum of everything scanned), and nobody rewrites wsum before the second.
template <int NT>
struct BlockScan {
  int *wsum, *carry;
  __device__ __forceinline__ BlockScan(int* wsum_, int* carry_) : wsum(wsum_), carry(carry_) {
    if (threadIdx.x == 0) *carry = 0;
  }
  __device__ __forceinline__ int round(int v) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int inc = wave_scan_incl(v, lane);
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int before = *carry;
    for (int w = 0; w < wave; ++w) before += wsum[w];
    __syncthreads();
    if (tid == NT - 1) *carry = before + inc;
    return before + inc - v;
  }
  __device__ __forceinline__ int total() {
    __syncthreads();
    return *carry;
  }
};

// Single-shot form: `part` is this thread's own sum; returns the sum of the lower threads' parts; *total (if asked for) = the
// workgroup's.  One barrier (every thread calls it once); wsum[NT / 64] is the caller's LDS, and whatever else the caller stored
// before the call is visible after it.
template <int NT, typename T>
__device__ __forceinline__ T block_scan_once(T part, T* wsum, T* total = nullptr) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const T inc = wave_scan_incl(part, lane);
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  T before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < NT / 64; ++w) {
    if (w < wave) before += wsum[w];
    all += wsum[w];
  }
  if (total) *total = all;
  return before + inc - part;
}

// word w of a bitmap over N rows; bits past N in the last word are ignored
__device__ __forceinline__ uint32_t bitmap_word(const uint32_t* __restrict__ bm, int64_t w, int64_t N) {
  uint32_t bits = bm[w];
  const int64_t rem = N - w * 32;
  if (rem < 32) bits &= (1u << rem) - 1u;
  return bits;
}

}  // namespace gdr
