// Ranking by sorted 64-bit keys, shared by the similarity top-k (sim_topk.hip), the in-cluster rerank (rerank.hip) and the
// beam step's top-2R (beam.hip).  One recipe: a float score becomes an order-preserving 32-bit key, packed as
// key << 32 | ~low word (a position, a doc id, a flat beam * vocab index) — distinct keys, so their order is total: higher
// score first, then the lower low word — the keys are bitonic-sorted in LDS, descending, and the first k unpacked.  Key 0 is
// "no entry": it sorts behind every live key (fkey(-inf) = 0x007fffff > 0).
// Lists too long for one LDS sort are cut into chunks of SEL_CHUNK positions whose first `keep` keys are merged in rounds
// (sel_merge_kernel / sel_merge_rounds): the top-k of a list is the top-k of the union of its pieces' top-k whatever the cut,
// so the chunked form returns what one larger sort would, bit for bit.
#pragma once
#include "common.h"

namespace gdr {

constexpr int SEL_SORT_MAX = 8192;  // keys of one LDS sort: 64 KiB
constexpr int SEL_CHUNK = 4096;     // positions per chunk workgroup of a chunked select: 32 KiB of keys, two 1024-thread workgroups per CU
constexpr int SEL_MAX_KEEP = 2 * GDR_MAX_BEAMS;  // the longest partial list: the beam step's 2R (the rerank keeps k <= GDR_MAX_BEAMS)
static_assert(SEL_MAX_KEEP <= SEL_CHUNK && SEL_SORT_MAX / SEL_MAX_KEEP >= 2,
              "a chunk keeps `keep` keys; a merge round must shrink the list count");

// sort width: the power of two >= n, at least `least` (a wave's 64 keys unless the caller says otherwise)
static inline int sel_pow2(int n, int least = 64) {
  int p = least;
  while (p < n) p <<= 1;
  return p;
}
// partial lists of `keep` keys one merge workgroup sorts
static inline int sel_merge_fan(int keep) { return SEL_SORT_MAX / keep > 2 ? SEL_SORT_MAX / keep : 2; }

// ---- keys ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t fkey(float v) {
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float fkey_inv(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
__device__ __forceinline__ unsigned long long sel_pack(float score, uint32_t low) {
  return ((unsigned long long)fkey(score) << 32) | (unsigned long long)(0xFFFFFFFFu - low);
}
__device__ __forceinline__ float sel_score(unsigned long long key) { return fkey_inv((uint32_t)(key >> 32)); }
__device__ __forceinline__ uint32_t sel_low(unsigned long long key) { return 0xFFFFFFFFu - (uint32_t)(key & 0xFFFFFFFFull); }

// ---- the sort ------------------------------------------------------------------------------------------------------------
// LDS operations of one wave execute in order: between steps that only exchange data inside a wave this wave-level barrier
// (plus fences for the compiler) is all the synchronisation needed.
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Compare-exchange of pair t of a bitonic stage: descending where bit `size` of the lower index is clear (size 0: everywhere).
__device__ __forceinline__ void sel_cmpx(unsigned long long* keys, int t, int stride, int size) {
  const int lo = (t / stride) * (stride << 1) + (t % stride), hi = lo + stride;
  const bool desc = ((lo & size) == 0);
  const unsigned long long x = keys[lo], y = keys[hi];
  if ((x < y) == desc) keys[lo] = y, keys[hi] = x;
}

// Bitonic sort of n 64-bit keys in LDS (n a power of two >= 64, a multiple of 2 * the workgroup's waves), descending, by the
// whole workgroup.  Barrier contract: the caller has a workgroup barrier behind its last store to keys[]; the routine ends with
// one, so the caller reads the result at once.  A wave owns a block of n / nwaves consecutive keys: every stage whose pairs stay
// inside a block costs a wave barrier only, so of the 66 stages of a 2048-key sort on 16 waves only the ones with
// stride >= 64 cost a workgroup barrier pair.  nthr: the workgroup's size, for a caller that knows it as a literal.
// bitonic_stages is the network without the closing barrier, for a caller that joins another path in front of one barrier
// (beam_topk_kernel: a closing barrier in each of its two branches measured 0.85 us per step slower at 100 beams).
__device__ __forceinline__ void bitonic_stages(unsigned long long* keys, int n, int nthr) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int epw = n / (nthr >> 6);
  for (int size = 2; size <= n; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      if (2 * stride <= epw) {
        for (int p = lane; p < (epw >> 1); p += 64) sel_cmpx(keys, (epw >> 1) * wave + p, stride, size);
        wave_sync();
      } else {
        __syncthreads();
        for (int t = tid; t < (n >> 1); t += nthr) sel_cmpx(keys, t, stride, size);
        __syncthreads();
      }
    }
  }
}
__device__ __forceinline__ void bitonic_desc(unsigned long long* keys, int n, int nthr) {
  bitonic_stages(keys, n, nthr);
  __syncthreads();
}
__device__ __forceinline__ void bitonic_desc(unsigned long long* keys, int n) { bitonic_desc(keys, n, (int)blockDim.x); }

// The same sort of kpad <= 1024 keys by the FIRST WAVE alone: its 28 .. 55 stages need no workgroup barrier (one before, one
// after — the callers').
__device__ __forceinline__ void wave0_bitonic_desc(unsigned long long* buf, int kpad) {
  if (threadIdx.x >= 64) return;
  for (int size = 2; size <= kpad; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = threadIdx.x; t < (kpad >> 1); t += 64) sel_cmpx(buf, t, stride, size);
      wave_sync();
    }
  }
}

// ---- merge rounds of a chunked select ----------------------------------------------------------------------------------------
// A "lane" is one independent ranking (the beam step: a query; the rerank: an (alpha slot, query) pair); its partial lists lie
// [lane][n][keep], sorted.  One round: a workgroup per (group of up to `fan` consecutive lists, lane) sorts the group's keys
// (fan * keep <= SEL_SORT_MAX) and files the first `keep` into dst [lane][n_out][keep]; the round that is left with one list per
// lane (n_out == 1, dst == nullptr) hands the sorted keys to emit(lane, keys, npad, keep) instead.  emit.skip() ends a workgroup
// before it reads anything.  Grid: x = inner lanes, y = groups, z = outer lanes (lane = outer * inner count + inner).
template <class Emit>
__global__ __launch_bounds__(1024) void sel_merge_kernel(const unsigned long long* __restrict__ src, int n_in, int fan, int n_out,
                                                         int keep, int npad, unsigned long long* __restrict__ dst, Emit emit) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long sel_keys[];  // [npad]
  if (emit.skip()) return;  // workgroup-uniform
  const int g = blockIdx.y, lane = blockIdx.z * gridDim.x + blockIdx.x;
  const int tid = threadIdx.x, nthr = blockDim.x;
  const int lists = n_in - g * fan < fan ? n_in - g * fan : fan;
  const int cnt = lists * keep;  // <= npad
  const unsigned long long* in = src + ((int64_t)lane * n_in + (int64_t)g * fan) * keep;
  for (int t = tid; t < npad; t += nthr) sel_keys[t] = t < cnt ? in[t] : 0ull;
  __syncthreads();
  bitonic_desc(sel_keys, npad);
  if (dst == nullptr) {
    emit(lane, sel_keys, npad, keep);
    return;
  }
  unsigned long long* o = dst + ((int64_t)lane * n_out + g) * keep;
  for (int i = tid; i < keep; i += nthr) o[i] = sel_keys[i];
}

// The rounds: part[0] holds n_in lists per lane, the rounds alternate between part[0] and part[1] until one list is left.
// lanes = lanes_z * lanes_x, split as the caller's grid limits ask (z <= 65535).  The caller has raised this instantiation's
// dynamic LDS limit to SEL_SORT_MAX * 8 (ensure_dyn_lds); `what` names the caller's launch in an error message.
template <class Emit>
static int sel_merge_rounds(unsigned long long* const part[2], int n_in, int keep, int lanes_x, int lanes_z, const Emit& emit,
                            const char* what, hipStream_t stream) {
  const int fan = sel_merge_fan(keep);
  int from = 0;
  do {
    const int n_out = (n_in + fan - 1) / fan;
    const int npad = sel_pow2((n_in < fan ? n_in : fan) * keep);
    hipLaunchKernelGGL(sel_merge_kernel<Emit>, dim3((unsigned)lanes_x, (unsigned)n_out, (unsigned)lanes_z), dim3(npad >= 2048 ? 1024 : 256),
                       (size_t)npad * 8, stream, part[from], n_in, fan, n_out, keep, npad, n_out == 1 ? nullptr : part[from ^ 1], emit);
    GDR_CHECK_LAUNCH(what);
    n_in = n_out;
    from ^= 1;
  } while (n_in > 1);
  return GDR_OK;
}

}  // namespace gdr
