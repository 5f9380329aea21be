// Non-GEMM layer kernels for gfx950 around the attention (attention.hip): embedding gathers, the ragged-batch plan and its row
// moves, T5 RMS norm, LayerNorm, L2 normalize.
//
// All of them are HBM-bound: a wave per row, 16-byte coalesced global accesses, wave64 shuffle reductions.
#include <math.h>

#include <stdlib.h>

#include "layers.h"
#include "scan.h"

namespace gdr {

// ------------------------------------------------------------------------------------------ embed
__global__ __launch_bounds__(256) void embed_kernel(const float* __restrict__ table, const int64_t* __restrict__ ids,
                                                    int64_t rows, int d4, int vocab, float* __restrict__ out) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  int64_t id = ids[row];
  id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
  const float4* src = reinterpret_cast<const float4*>(table) + id * d4;
  float4* dst = reinterpret_cast<float4*>(out) + row * d4;
  for (int c = threadIdx.x & 63; c < d4; c += 64) dst[c] = src[c];
}

int launch_embed(const float* table, const int64_t* ids, int64_t rows, int d, int vocab, float* out,
                 hipStream_t stream) {
  GDR_CHECK_ARG(d % 4 == 0, "embed: d %% 4 != 0");
  if (rows == 0) return GDR_OK;
  hipLaunchKernelGGL(embed_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, table, ids, rows, d / 4,
                     vocab, out);
  GDR_CHECK_LAUNCH("embed_kernel");
  return GDR_OK;
}

// ------------------------------------------------------------------------------------------ ragged batches
// Planning a ragged batch, two small kernels: (1) a wave per mask row: length + prefix test (B/4 workgroups — one workgroup
// walking 512 rows of dependent loads took 43 us); (2) one workgroup: exclusive scan of the lengths and the total.  The
// row map is written by (3), again a wave per sequence.
__global__ __launch_bounds__(256) void pack_len_kernel(const int64_t* __restrict__ mask, int B, int L,
                                                       int32_t* __restrict__ seq_len) {
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (b >= B) return;
  int cnt = 0, last = -1;
  for (int j = lane; j < L; j += 64) {
    const bool on = mask[(int64_t)b * L + j] != 0;
    cnt += on ? 1 : 0;
    last = on ? j : last;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {  // sum and max in one butterfly (the parent's code: every kernel of the C2 step but pack_scan is)
    cnt += __shfl_xor(cnt, o);
    last = max(last, __shfl_xor(last, o));
  }
  if (lane == 0) seq_len[b] = (cnt > 0 && last + 1 == cnt) ? cnt : L;   // a non-empty prefix of ones, else keep all
}

__global__ __launch_bounds__(1024) void pack_scan_kernel(int B, const int32_t* __restrict__ seq_len,
                                                         int32_t* __restrict__ seq_off, int64_t* __restrict__ rows_total) {
  __shared__ int wsum[16];
  __shared__ int carry;
  BlockScan<1024> scan(wsum, &carry);
  for (int base = 0; base < B; base += 1024) {  // workgroup-uniform
    const int b = base + threadIdx.x;
    const int before = scan.round(b < B ? seq_len[b] : 0);
    if (b < B) seq_off[b] = before;
  }
  const int total = scan.total();
  if (threadIdx.x == 0) {
    seq_off[B] = total;
    *rows_total = total;
  }
}

__global__ __launch_bounds__(256) void pack_rows_kernel(int B, int L, const int32_t* __restrict__ seq_len,
                                                        const int32_t* __restrict__ seq_off, int32_t* __restrict__ row_src) {
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (b >= B) return;
  const int o = seq_off[b], n = seq_len[b];
  for (int j = lane; j < n; j += 64) row_src[o + j] = b * L + j;
}

int launch_pack_plan(const int64_t* mask, int B, int L, int32_t* seq_len, int32_t* seq_off, int32_t* row_src,
                     int64_t* rows_total, hipStream_t stream) {
  GDR_CHECK_ARG(mask && seq_len && seq_off && row_src && rows_total, "pack_plan: null pointer");
  GDR_CHECK_ARG((int64_t)B * L < 0x7fffffffLL, "pack_plan: batch too large");
  const unsigned g = (unsigned)((B + 3) / 4);
  hipLaunchKernelGGL(pack_len_kernel, dim3(g), dim3(256), 0, stream, mask, B, L, seq_len);
  GDR_CHECK_LAUNCH("pack_len_kernel");
  hipLaunchKernelGGL(pack_scan_kernel, dim3(1), dim3(1024), 0, stream, B, seq_len, seq_off, rows_total);
  GDR_CHECK_LAUNCH("pack_scan_kernel");
  hipLaunchKernelGGL(pack_rows_kernel, dim3(g), dim3(256), 0, stream, B, L, seq_len, seq_off, row_src);
  GDR_CHECK_LAUNCH("pack_rows_kernel");
  return GDR_OK;
}

__global__ __launch_bounds__(256) void embed_packed_kernel(const float* __restrict__ table, const int64_t* __restrict__ ids,
                                                           const int32_t* __restrict__ row_src,
                                                           const int64_t* __restrict__ rows_dev, int d4, int vocab,
                                                           float* __restrict__ out) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= *rows_dev) return;
  int64_t id = ids[row_src[row]];
  id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
  const float4* src = reinterpret_cast<const float4*>(table) + id * d4;
  float4* dst = reinterpret_cast<float4*>(out) + row * d4;
  for (int c = threadIdx.x & 63; c < d4; c += 64) dst[c] = src[c];
}

int launch_embed_packed(const float* table, const int64_t* ids, const int32_t* row_src, const int64_t* rows_dev,
                        int64_t max_rows, int d, int vocab, float* out, hipStream_t stream) {
  GDR_CHECK_ARG(d % 4 == 0, "embed: d %% 4 != 0");
  if (max_rows == 0) return GDR_OK;
  hipLaunchKernelGGL(embed_packed_kernel, dim3((unsigned)((max_rows + 3) / 4)), dim3(256), 0, stream, table, ids, row_src,
                     rows_dev, d / 4, vocab, out);
  GDR_CHECK_LAUNCH("embed_packed_kernel");
  return GDR_OK;
}

// Two gathers by the same token id in one launch: out[row] = table[id] (d4 float4) and out2[row] = table2[id] (e4 float4) — the
// embedding row and block 0's q/k/v row of the token table (encoder.hip).  Same id, same clamp as embed_packed_kernel.
__global__ __launch_bounds__(256) void embed_packed2_kernel(const float* __restrict__ table, const float* __restrict__ table2,
                                                            const int64_t* __restrict__ ids, const int32_t* __restrict__ row_src,
                                                            const int64_t* __restrict__ rows_dev, int d4, int e4, int vocab,
                                                            float* __restrict__ out, float* __restrict__ out2) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= *rows_dev) return;
  int64_t id = ids[row_src[row]];
  id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
  const float4* src2 = reinterpret_cast<const float4*>(table2) + id * e4;
  float4* dst2 = reinterpret_cast<float4*>(out2) + row * e4;
  for (int c = threadIdx.x & 63; c < e4; c += 64) dst2[c] = src2[c];
  const float4* src = reinterpret_cast<const float4*>(table) + id * d4;
  float4* dst = reinterpret_cast<float4*>(out) + row * d4;
  for (int c = threadIdx.x & 63; c < d4; c += 64) dst[c] = src[c];
}

int launch_embed_packed2(const float* table, const float* table2, const int64_t* ids, const int32_t* row_src,
                         const int64_t* rows_dev, int64_t max_rows, int d, int e, int vocab, float* out, float* out2,
                         hipStream_t stream) {
  GDR_CHECK_ARG(d % 4 == 0 && e % 4 == 0, "embed: d %% 4 != 0");
  if (max_rows == 0) return GDR_OK;
  hipLaunchKernelGGL(embed_packed2_kernel, dim3((unsigned)((max_rows + 3) / 4)), dim3(256), 0, stream, table, table2, ids,
                     row_src, rows_dev, d / 4, e / 4, vocab, out, out2);
  GDR_CHECK_LAUNCH("embed_packed2_kernel");
  return GDR_OK;
}

// SCATTER = false: dst[i] = src[map[i]];  SCATTER = true: dst[map[i]] = src[i]   (rows of d4 float4), i < n or *n_dev;
// dst rows are dst_ld4 float4 apart (= d4: dense)
template <bool SCATTER>
__global__ __launch_bounds__(256) void move_rows_kernel(const float* __restrict__ src, const int32_t* __restrict__ map,
                                                        int64_t n, const int64_t* __restrict__ n_dev, int d4,
                                                        float* __restrict__ dst, int64_t dst_ld4) {
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n_dev) n = *n_dev;
  if (i >= n) return;
  const int64_t m = map[i];
  const float4* s = reinterpret_cast<const float4*>(src) + (SCATTER ? i : m) * d4;
  float4* o = reinterpret_cast<float4*>(dst) + (SCATTER ? m : i) * dst_ld4;
  for (int c = threadIdx.x & 63; c < d4; c += 64) o[c] = s[c];
}

int launch_gather_rows(const float* src, const int32_t* idx, int n, int d, float* dst, hipStream_t stream) {
  GDR_CHECK_ARG(d % 4 == 0, "gather_rows: d %% 4 != 0");
  if (n == 0) return GDR_OK;
  hipLaunchKernelGGL(move_rows_kernel<false>, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, stream, src, idx, (int64_t)n,
                     (const int64_t*)nullptr, d / 4, dst, (int64_t)(d / 4));
  GDR_CHECK_LAUNCH("gather_rows");
  return GDR_OK;
}

// dst[idx[i]] = src[i] for i < n: rows of d floats out of a dense src into rows of dst that are ldd floats apart
int launch_scatter_rows_strided(const float* src, const int32_t* idx, int n, int d, float* dst, int64_t ldd, hipStream_t stream) {
  GDR_CHECK_ARG(d % 4 == 0 && ldd % 4 == 0 && ldd >= d && ((uintptr_t)dst & 15) == 0, "scatter_rows: bad row width / stride / alignment");
  if (n == 0) return GDR_OK;
  hipLaunchKernelGGL(move_rows_kernel<true>, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, stream, src, idx, (int64_t)n,
                     (const int64_t*)nullptr, d / 4, dst, ldd / 4);
  GDR_CHECK_LAUNCH("scatter_rows_strided");
  return GDR_OK;
}

int launch_scatter_rows(const float* src, const int32_t* row_src, const int64_t* rows_dev, int64_t max_rows, int d,
                        float* dst, hipStream_t stream) {
  GDR_CHECK_ARG(d % 4 == 0, "scatter_rows: d %% 4 != 0");
  if (max_rows == 0) return GDR_OK;
  hipLaunchKernelGGL(move_rows_kernel<true>, dim3((unsigned)((max_rows + 3) / 4)), dim3(256), 0, stream, src, row_src,
                     max_rows, rows_dev, d / 4, dst, (int64_t)(d / 4));
  GDR_CHECK_LAUNCH("scatter_rows");
  return GDR_OK;
}

__global__ __launch_bounds__(256) void zero_dead_rows_kernel(float* __restrict__ x, const int32_t* __restrict__ seq_len,
                                                             int64_t rows, int L, int d4) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int b = (int)(row / L), j = (int)(row - (int64_t)b * L);
  if (j < seq_len[b]) return;
  float4* o = reinterpret_cast<float4*>(x) + row * d4;
  for (int c = threadIdx.x & 63; c < d4; c += 64) o[c] = make_float4(0.f, 0.f, 0.f, 0.f);
}

int launch_zero_dead_rows(float* x, const int32_t* seq_len, int B, int L, int d, hipStream_t stream) {
  GDR_CHECK_ARG(d % 4 == 0, "zero_dead_rows: d %% 4 != 0");
  const int64_t rows = (int64_t)B * L;
  if (rows == 0) return GDR_OK;
  hipLaunchKernelGGL(zero_dead_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, x, seq_len, rows, L, d / 4);
  GDR_CHECK_LAUNCH("zero_dead_rows_kernel");
  return GDR_OK;
}

// ------------------------------------------------------------------------------------------ norms
template <bool BF16OUT>
__global__ __launch_bounds__(256) void rmsnorm_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                      float* __restrict__ y, int64_t rows, int d4, float eps,
                                                      float* __restrict__ pooled, int pool_every,
                                                      const int64_t* __restrict__ rows_dev, uint2* __restrict__ y16 = nullptr,
                                                      int planes_ld = 0) {
  // planes_ld != 0 (the split-bf16 form, r06): y16 receives the row as three bf16 planes [hi | mid | lo] (row stride planes_ld
  // elements, plane stride d) instead of one rounded image, and y may be null (the fp32 copy is not written)
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (rows_dev) rows = *rows_dev;
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  const float4* xr = reinterpret_cast<const float4*>(x) + row * d4;
  // the row stays in registers between the two passes (d <= 2048: 8 float4 per lane; wider rows are read twice as before): the
  // second read was an L1 / L2 round trip on a kernel that is a chain of round trips (23 us for 76 MB at 12 308 rows)
  constexpr int MAXC = 8;
  const bool in_regs = d4 <= 64 * MAXC;
  float4 xv[MAXC];
  float ss = 0.f;
  if (in_regs) {
#pragma unroll
    for (int i = 0; i < MAXC; ++i) {
      const int c = lane + 64 * i;
      xv[i] = c < d4 ? xr[c] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int i = 0; i < MAXC; ++i)
      if (lane + 64 * i < d4) ss += xv[i].x * xv[i].x + xv[i].y * xv[i].y + xv[i].z * xv[i].z + xv[i].w * xv[i].w;
  } else {
    for (int c = lane; c < d4; c += 64) {
      const float4 v = xr[c];
      ss += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
    }
  }
  ss = wave_sum(ss);
  const RowDivisor over(sqrtf(ss / (float)(d4 * 4) + eps));
  float4* yr = reinterpret_cast<float4*>(y) + row * d4;
  float4* pr = (pooled && row % pool_every == 0) ? reinterpret_cast<float4*>(pooled) + (row / pool_every) * d4
                                                  : nullptr;
  const float4* wr = reinterpret_cast<const float4*>(w);
  auto emit = [&](int c, const float4 v) {
    const float4 g = wr[c];
    float4 o;
    o.x = g.x * over(v.x), o.y = g.y * over(v.y), o.z = g.z * over(v.z), o.w = g.w * over(v.w);
    if (BF16OUT) {
      (reinterpret_cast<uint2*>(y) + row * d4)[c] = pack_bf16x4(o.x, o.y, o.z, o.w);
    } else {
      if (y) yr[c] = o;
      if (pr) pr[c] = o;
      if (y16 && planes_ld > 0) {  // bf16 x 3 planes [hi | mid | lo]
        __bf16* pl = reinterpret_cast<__bf16*>(y16) + row * planes_ld + 4 * c;
        const float v4[4] = {o.x, o.y, o.z, o.w};
        union {
          __bf16 h[4];
          uint2 u;
        } hi, mid, lo;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          hi.h[j] = (__bf16)v4[j];
          const float r1 = v4[j] - (float)hi.h[j];
          mid.h[j] = (__bf16)r1;
          lo.h[j] = (__bf16)(r1 - (float)mid.h[j]);
        }
        *reinterpret_cast<uint2*>(pl) = hi.u;
        *reinterpret_cast<uint2*>(pl + 4 * d4) = mid.u;
        *reinterpret_cast<uint2*>(pl + 8 * d4) = lo.u;
      } else if (y16 && planes_ld < 0) {  // fp16 x 2 planes [hi | (x - hi) * 2^11], row stride -planes_ld
        _Float16* pl = reinterpret_cast<_Float16*>(y16) + row * (int64_t)(-planes_ld) + 4 * c;
        const float v4[4] = {o.x, o.y, o.z, o.w};
        union {
          _Float16 h[4];
          uint2 u;
        } hi, lo;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          hi.h[j] = (_Float16)v4[j];
          lo.h[j] = (_Float16)((v4[j] - (float)hi.h[j]) * 2048.0f);
        }
        *reinterpret_cast<uint2*>(pl) = hi.u;
        *reinterpret_cast<uint2*>(pl + 4 * d4) = lo.u;
      } else if (y16) {
        (y16 + row * d4)[c] = pack_bf16x4(o.x, o.y, o.z, o.w);  // the same values, rounded: a bf16 linear's operand
      }
    }
  };
  if (in_regs) {
#pragma unroll
    for (int i = 0; i < MAXC; ++i)
      if (lane + 64 * i < d4) emit(lane + 64 * i, xv[i]);
  } else {
    for (int c = lane; c < d4; c += 64) emit(c, xr[c]);
  }
}

int launch_rmsnorm(const float* x, const float* w, float* y, int64_t rows, int d, float eps, float* pooled,
                   int pool_every, hipStream_t stream, void* y16) {
  GDR_CHECK_ARG(d % 4 == 0, "rmsnorm: d %% 4 != 0");
  if (rows == 0) return GDR_OK;
  hipLaunchKernelGGL(rmsnorm_kernel<false>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, x, w, y, rows, d / 4, eps,
                     pooled, pool_every > 0 ? pool_every : 1, (const int64_t*)nullptr, static_cast<uint2*>(y16));
  GDR_CHECK_LAUNCH("rmsnorm_kernel");
  return GDR_OK;
}

int launch_rmsnorm_dev(const float* x, const float* w, float* y, const int64_t* rows_dev, int64_t max_rows, int d, float eps,
                       hipStream_t stream, void* y16) {
  GDR_CHECK_ARG(d % 4 == 0, "rmsnorm: d %% 4 != 0");
  if (max_rows == 0) return GDR_OK;
  hipLaunchKernelGGL(rmsnorm_kernel<false>, dim3((unsigned)((max_rows + 3) / 4)), dim3(256), 0, stream, x, w, y, max_rows,
                     d / 4, eps, (float*)nullptr, 1, rows_dev, static_cast<uint2*>(y16));
  GDR_CHECK_LAUNCH("rmsnorm_kernel(dev rows)");
  return GDR_OK;
}

// y (nullable) fp32 rows; planes: bf16 [rows, ld] rows = [hi | mid | lo] of the normed row (split-bf16 operand); rows_dev may be null
int launch_rmsnorm_planes(const float* x, const float* w, float* y, void* planes, int64_t ld, const int64_t* rows_dev, int64_t max_rows,
                          int d, float eps, hipStream_t stream, int f16x2) {
  GDR_CHECK_ARG(d % 4 == 0 && ld >= (f16x2 ? 2 : 3) * (int64_t)d && ld % 4 == 0, "rmsnorm(planes): d %% 4 != 0 or the plane row is too short");
  if (max_rows == 0) return GDR_OK;
  hipLaunchKernelGGL(rmsnorm_kernel<false>, dim3((unsigned)((max_rows + 3) / 4)), dim3(256), 0, stream, x, w, y, max_rows, d / 4, eps,
                     (float*)nullptr, 1, rows_dev, static_cast<uint2*>(planes), f16x2 ? -(int)ld : (int)ld);
  GDR_CHECK_LAUNCH("rmsnorm_kernel(planes)");
  return GDR_OK;
}

int launch_rmsnorm_bf16(const float* x, const float* w, void* y_bf16, int64_t rows, int d, float eps, hipStream_t stream) {
  GDR_CHECK_ARG(d % 4 == 0, "rmsnorm: d %% 4 != 0");
  if (rows == 0) return GDR_OK;
  hipLaunchKernelGGL(rmsnorm_kernel<true>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, x, w,
                     static_cast<float*>(y_bf16), rows, d / 4, eps, (float*)nullptr, 1, (const int64_t*)nullptr);
  GDR_CHECK_LAUNCH("rmsnorm_kernel<bf16>");
  return GDR_OK;
}

int launch_rmsnorm_bf16_dev(const float* x, const float* w, void* y_bf16, const int64_t* rows_dev, int64_t max_rows, int d,
                            float eps, hipStream_t stream) {
  GDR_CHECK_ARG(d % 4 == 0, "rmsnorm: d %% 4 != 0");
  if (max_rows == 0) return GDR_OK;
  hipLaunchKernelGGL(rmsnorm_kernel<true>, dim3((unsigned)((max_rows + 3) / 4)), dim3(256), 0, stream, x, w,
                     static_cast<float*>(y_bf16), max_rows, d / 4, eps, (float*)nullptr, 1, rows_dev);
  GDR_CHECK_LAUNCH("rmsnorm_kernel<bf16>(dev rows)");
  return GDR_OK;
}

// y = x / max(||x||_2, eps) per row: torch.nn.functional.normalize(rep, dim=-1) of DensePooler (dense.py:24-25)
__global__ __launch_bounds__(256) void l2_normalize_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t rows,
                                                           int d, float eps) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  const float* xr = x + row * d;
  float ss = 0.f;
  for (int c = lane; c < d; c += 64) ss += xr[c] * xr[c];
  const float nrm = fmaxf(sqrtf(wave_sum(ss)), eps);
  for (int c = lane; c < d; c += 64) y[row * d + c] = xr[c] / nrm;
}

__global__ __launch_bounds__(256) void layernorm_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                        const float* __restrict__ b, float* __restrict__ y,
                                                        int64_t rows, int d4, float eps,
                                                        const float* __restrict__ addv,
                                                        const int64_t* __restrict__ rows_dev, uint2* __restrict__ y16,
                                                        int f16x2_ld = 0) {
  // f16x2_ld != 0 (the fp16 x 2 split form, r06): y16 receives the row as plane rows [fp16 hi | fp16 (y - hi) * 2^11] of f16x2_ld elements
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (rows_dev) rows = *rows_dev;
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  const float4* xr = reinterpret_cast<const float4*>(x) + row * d4;
  const float inv_d = 1.0f / (float)(d4 * 4);
  const float4* av = reinterpret_cast<const float4*>(addv);
  auto ld = [&](int c) {
    float4 v = xr[c];
    if (av) {
      const float4 t = av[c];
      v.x += t.x, v.y += t.y, v.z += t.z, v.w += t.w;
    }
    return v;
  };
  float s = 0.f;
  for (int c = lane; c < d4; c += 64) {
    const float4 v = ld(c);
    s += v.x + v.y + v.z + v.w;
  }
  const float mean = wave_sum(s) * inv_d;
  float ss = 0.f;
  for (int c = lane; c < d4; c += 64) {
    const float4 v = ld(c);
    const float a0 = v.x - mean, a1 = v.y - mean, a2 = v.z - mean, a3 = v.w - mean;
    ss += a0 * a0 + a1 * a1 + a2 * a2 + a3 * a3;
  }
  const float rstd = 1.0f / sqrtf(wave_sum(ss) * inv_d + eps);
  float4* yr = reinterpret_cast<float4*>(y) + row * d4;
  const float4* wr = reinterpret_cast<const float4*>(w);
  const float4* br = reinterpret_cast<const float4*>(b);
  for (int c = lane; c < d4; c += 64) {
    const float4 v = ld(c), g = wr[c], bb = br[c];
    float4 o;
    o.x = (v.x - mean) * rstd * g.x + bb.x, o.y = (v.y - mean) * rstd * g.y + bb.y;
    o.z = (v.z - mean) * rstd * g.z + bb.z, o.w = (v.w - mean) * rstd * g.w + bb.w;
    yr[c] = o;
    if (y16 && f16x2_ld) {
      _Float16* pl = reinterpret_cast<_Float16*>(y16) + row * (int64_t)f16x2_ld + 4 * c;
      const float v4[4] = {o.x, o.y, o.z, o.w};
      union {
        _Float16 h[4];
        uint2 u;
      } hi, lo;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        hi.h[j] = (_Float16)v4[j];
        lo.h[j] = (_Float16)((v4[j] - (float)hi.h[j]) * 2048.0f);
      }
      *reinterpret_cast<uint2*>(pl) = hi.u;
      *reinterpret_cast<uint2*>(pl + 4 * d4) = lo.u;
    } else if (y16) {
      (y16 + row * d4)[c] = pack_bf16x4(o.x, o.y, o.z, o.w);
    }
  }
}

// y = LN(LN(x; w1, b1) + addv; w2, b2) — the adaptor's norm1 -> (+ the constant single-key cross-attention output) -> norm2
// (nn.TransformerDecoderLayer, post-LN; modeling_t5.py:1241-1244) in ONE pass: the row stays in registers between the two
// norms instead of going through memory and a second launch.  Same expressions and reduction order as two layernorm_kernel
// launches: bit-identical.  d <= 2048.
__global__ __launch_bounds__(256) void layernorm2_kernel(const float* __restrict__ x, const float* __restrict__ w1,
                                                         const float* __restrict__ b1, const float* __restrict__ w2,
                                                         const float* __restrict__ b2, const float* __restrict__ addv,
                                                         float* __restrict__ y, int64_t rows, int d4, float eps,
                                                         const int64_t* __restrict__ rows_dev, uint2* __restrict__ y16) {
  constexpr int MAXC = 8;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (rows_dev) rows = *rows_dev;
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  const float inv_d = 1.0f / (float)(d4 * 4);
  const float4* xr = reinterpret_cast<const float4*>(x) + row * d4;
  float4 v[MAXC];
#pragma unroll
  for (int i = 0; i < MAXC; ++i) {
    const int c = lane + 64 * i;
    v[i] = c < d4 ? xr[c] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  const float4* wr[2] = {reinterpret_cast<const float4*>(w1), reinterpret_cast<const float4*>(w2)};
  const float4* br[2] = {reinterpret_cast<const float4*>(b1), reinterpret_cast<const float4*>(b2)};
  const float4* av = reinterpret_cast<const float4*>(addv);
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    if (pass == 1 && av) {
#pragma unroll
      for (int i = 0; i < MAXC; ++i) {
        const int c = lane + 64 * i;
        if (c < d4) {
          const float4 t = av[c];
          v[i].x += t.x, v[i].y += t.y, v[i].z += t.z, v[i].w += t.w;
        }
      }
    }
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < MAXC; ++i)
      if (lane + 64 * i < d4) s += v[i].x + v[i].y + v[i].z + v[i].w;
    const float mean = wave_sum(s) * inv_d;
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < MAXC; ++i)
      if (lane + 64 * i < d4) {
        const float a0 = v[i].x - mean, a1 = v[i].y - mean, a2 = v[i].z - mean, a3 = v[i].w - mean;
        ss += a0 * a0 + a1 * a1 + a2 * a2 + a3 * a3;
      }
    const float rstd = 1.0f / sqrtf(wave_sum(ss) * inv_d + eps);
#pragma unroll
    for (int i = 0; i < MAXC; ++i) {
      const int c = lane + 64 * i;
      if (c < d4) {
        const float4 g = wr[pass][c], bb = br[pass][c];
        float4 o;
        o.x = (v[i].x - mean) * rstd * g.x + bb.x, o.y = (v[i].y - mean) * rstd * g.y + bb.y;
        o.z = (v[i].z - mean) * rstd * g.z + bb.z, o.w = (v[i].w - mean) * rstd * g.w + bb.w;
        v[i] = o;
      }
    }
  }
  float4* yr = reinterpret_cast<float4*>(y) + row * d4;
#pragma unroll
  for (int i = 0; i < MAXC; ++i) {
    const int c = lane + 64 * i;
    if (c < d4) {
      yr[c] = v[i];
      if (y16) (y16 + row * d4)[c] = pack_bf16x4(v[i].x, v[i].y, v[i].z, v[i].w);
    }
  }
}

// returns 1 when d is too wide for the one-pass form (the caller runs two layernorm launches)
int launch_layernorm2(const float* x, const float* w1, const float* b1, const float* w2, const float* b2, const float* addv, float* y,
                      const int64_t* rows_dev, int64_t max_rows, int d, float eps, hipStream_t stream, void* y16) {
  GDR_CHECK_ARG(d % 4 == 0, "layernorm: d %% 4 != 0");
  if (d > 2048) return 1;
  if (max_rows == 0) return GDR_OK;
  hipLaunchKernelGGL(layernorm2_kernel, dim3((unsigned)((max_rows + 3) / 4)), dim3(256), 0, stream, x, w1, b1, w2, b2, addv, y,
                     max_rows, d / 4, eps, rows_dev, static_cast<uint2*>(y16));
  GDR_CHECK_LAUNCH("layernorm2_kernel");
  return GDR_OK;
}

int launch_layernorm(const float* x, const float* w, const float* b, float* y, int64_t rows, int d, float eps,
                     const float* addv, hipStream_t stream, void* y16, int f16x2_ld) {
  GDR_CHECK_ARG(d % 4 == 0 && (f16x2_ld == 0 || (y16 && f16x2_ld >= 2 * d && f16x2_ld % 4 == 0)), "layernorm: d %% 4 != 0 or a bad plane row");
  if (rows == 0) return GDR_OK;
  hipLaunchKernelGGL(layernorm_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, x, w, b, y, rows, d / 4,
                     eps, addv, (const int64_t*)nullptr, static_cast<uint2*>(y16), f16x2_ld);
  GDR_CHECK_LAUNCH("layernorm_kernel");
  return GDR_OK;
}

int launch_layernorm_dev(const float* x, const float* w, const float* b, float* y, const int64_t* rows_dev, int64_t max_rows,
                         int d, float eps, const float* addv, hipStream_t stream, void* y16, int f16x2_ld) {
  GDR_CHECK_ARG(d % 4 == 0 && (f16x2_ld == 0 || (y16 && f16x2_ld >= 2 * d && f16x2_ld % 4 == 0)), "layernorm: d %% 4 != 0 or a bad plane row");
  if (max_rows == 0) return GDR_OK;
  hipLaunchKernelGGL(layernorm_kernel, dim3((unsigned)((max_rows + 3) / 4)), dim3(256), 0, stream, x, w, b, y, max_rows, d / 4,
                     eps, addv, rows_dev, static_cast<uint2*>(y16), f16x2_ld);
  GDR_CHECK_LAUNCH("layernorm_kernel(dev rows)");
  return GDR_OK;
}

}  // namespace gdr

extern "C" int gdr_t5_layer_norm(const float* x, const float* w, float* y, int64_t rows, int d, float eps, void* stream_) {
  using namespace gdr;
  GDR_CHECK_ARG(x && w && y && rows >= 0 && d > 0 && d % 4 == 0, "t5_layer_norm: bad arguments (d %% 4 == 0)");
  return launch_rmsnorm(x, w, y, rows, d, eps, nullptr, 1, static_cast<hipStream_t>(stream_));
}

extern "C" int gdr_l2_normalize(const float* x, float* y, int64_t rows, int d, float eps, void* stream_) {
  using namespace gdr;
  GDR_CHECK_ARG(x && y && rows >= 0 && d > 0, "l2_normalize: bad arguments");
  if (rows == 0) return GDR_OK;
  hipLaunchKernelGGL(l2_normalize_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, static_cast<hipStream_t>(stream_), x, y,
                     rows, d, eps);
  GDR_CHECK_LAUNCH("l2_normalize_kernel");
  return GDR_OK;
}
