/* gdr_hip_prefilter_mask.h — part of the C ABI of libgdr_hip.so; include/gdr_hip.h includes it, so `#include "gdr_hip.h"` declares
 * everything below.  The conventions (return codes, streams, alignment, gdr_last_error) are gdr_hip.h's; gdr_abi_version() stays 9:
 * these are additions, no existing entry point changed.
 *
 * THE PRE-FILTERED CORPUS SEARCH OVER LIVE ROWS AND PER-QUERY FILTERS
 *
 * gdr_sim_topk_prefilter_masked is gdr_sim_topk_prefilter's contract applied to the ALLOWED rows: row q of the result is the top-k of
 * the FP32 scores over the rows query q's bitmap allows, for every input; ties: the higher score in the total order of the fp32 bits,
 * then the lower id; ids = row + idx_offset; where fewer than k rows are allowed the tail of the list is -inf / -1 (an empty bitmap
 * gives k such entries).  The values are the fp32 dot products the unmasked call computes: the score of (query, row) depends on the two
 * vectors and d alone, so the list equals gdr_sim_topk_prefilter over the matrix of the allowed rows (and their bf16 image), ids mapped
 * back, bit for bit.
 *   flags: exactly GDR_SIM_LIVE_MASK (one bitmap for every query) or exactly GDR_SIM_QUERY_MASK (one bitmap per query).  Anything else —
 *     0, both flags, GDR_SIM_EXHAUSTIVE, GDR_SIM_NO_STREAM, GDR_SIM_ROW_GATHER, the chunk bits — is GDR_EINVAL before any launch, and
 *     gdr_sim_topk_prefilter_masked_workspace_bytes answers 0 for it.  (Live rows AND per-query filters: AND them into the per-query
 *     bitmaps on the caller's side, as for gdr_sim_topk.)
 *   Input layout: the bitmap(s) sit at the head of `workspace` in gdr_sim_topk's format: M = align_up(4 * ceil(N / 32), 256) bytes, bit
 *     r % 32 of int32 word r / 32 set = row r is allowed; GDR_SIM_QUERY_MASK: B of them, bitmap q at byte q * M.  The library only reads
 *     that region; bits past N and the padding up to M are ignored; its own scratch starts behind it.
 *     gdr_sim_topk_prefilter_masked_workspace_bytes = the bitmaps + gdr_sim_topk_prefilter_workspace_bytes(B, N, d, k) (so it never
 *     shrinks where that one does not); a smaller workspace is GDR_ENOSPC before any launch.
 *   status[q] = 1 where query q's candidate list or its band overflowed: the list is then the top-k of a subset, and the caller re-runs
 *     the query with gdr_sim_topk under GDR_SIM_EXHAUSTIVE plus the same mask (gdr_amd.ops.sim_topk does).  That includes a query with
 *     fewer than k allowed rows inside the sampled tiles of a corpus that takes a filter pass: the sample gives it no threshold, the
 *     filter pass keeps every row and the list overflows.  A disallowed row that reaches the threshold takes a slot of the list until
 *     the second mask pass drops it, so narrow filters overflow as they do in gdr_sim_topk (NARROW FILTERS there; the gather mode
 *     serves them).
 *   dnorm_max: ANY upper bound of ||D[r]||_2 over the allowed rows (> 0, finite).  The largest norm over all rows (what
 *     gdr_row_norm2_max gives) is one; so is a bound that has only grown while rows were rewritten (gdr_prefilter_update_rows).  A
 *     looser bound widens the band that is rescored in fp32 — more work, an earlier status 1 — and never breaks exactness.
 *   Limits: gdr_sim_topk_prefilter's — d % 8 == 0, d <= 1024, 1 <= k <= min(1024, N), idx_offset + N <= 2^31 - 1, Q / D / D_bf16 16-byte
 *     and workspace 256-byte aligned.  Stream-ordered and capturable, no host synchronisation: a captured call replayed after the
 *     bitmap in the workspace was rewritten follows the new bitmap.
 *   Sequence (one implementation with gdr_sim_topk_prefilter, whose launches and results are what they were): query prep, the sample
 *     pass over the bf16 image, the mask pass over the sample block, the threshold (k-th largest ALLOWED sample score - 2 eps_q), and
 *     where the plan has a filter pass: the fix-up (fewer than k allowed sample rows: -inf; per query for GDR_SIM_QUERY_MASK), the filter
 *     pass, the mask pass over the survivors; then the unchanged tail.  Three small launches more than the unmasked call; why the band
 *     still holds the answer: csrc/sim_topk.hip above sim_qprep_kernel.
 *   Measured at N = 320 000, d = 768, k = 100 (tools/bench_prefilter_mask.py, profiles/r24_prefilter_mask_bench.jsonl) against gdr_sim_topk
 *     with the same mask: 512 queries 2.07 -> 0.79 ms with every row or 99 % of the rows allowed, 2.16 -> 0.92 ms with 50 %, live mask and
 *     per-query bitmaps alike; at 32 queries it is NOT faster (0.25 -> 0.27 ms), as the unmasked pre-filter is not at that batch. */
#ifndef GDR_HIP_PREFILTER_MASK_H
#define GDR_HIP_PREFILTER_MASK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

size_t gdr_sim_topk_prefilter_masked_workspace_bytes(int B, int64_t N, int d, int k, int flags);
int gdr_sim_topk_prefilter_masked(const float* Q, int B, const float* D, const void* D_bf16, float dnorm_max, int64_t N, int d, int k,
                                  int32_t idx_offset, float* out_val, int32_t* out_idx, int32_t* status, int flags, void* workspace,
                                  size_t workspace_bytes, void* stream);

/* Row-wise upkeep of the bf16 image: for each of the n_rows ids in `rows` (device int32, each in [0, rows of D): the call is not told
 * N, the range is the caller's to keep; a negative id is skipped) row r of D_bf16 becomes the round-to-nearest-even image of row r of
 * D — the bits gdr_cast_f32_bf16 gives.  norm2_max_inout (device float) is NOT zeroed: it is raised (atomicMax on the bits) to the
 * largest squared norm among the listed rows, each computed exactly as gdr_row_norm2_max computes it, so after a call that lists the
 * row of the largest norm it equals a full gdr_row_norm2_max, and otherwise it stays an upper bound as long as it was one.  An id may
 * repeat.  d % 8 == 0; n_rows == 0 is a no-op; D and D_bf16 16-byte aligned.  Stream-ordered, capturable. */
int gdr_prefilter_update_rows(const float* D, void* D_bf16, int d, const int32_t* rows, int64_t n_rows, float* norm2_max_inout,
                              void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GDR_HIP_PREFILTER_MASK_H */
