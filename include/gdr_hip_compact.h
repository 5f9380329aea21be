/* gdr_hip_compact.h — part of the C ABI of libgdr_hip.so; include/gdr_hip.h includes it, so `#include "gdr_hip.h"` declares
 * everything below.  The conventions (return codes, streams, gdr_last_error) are gdr_hip.h's: every pointer is a device pointer,
 * the library allocates nothing, the calls are stream-ordered with no host synchronisation and capturable, all byte offsets are
 * 64-bit.  gdr_abi_version() stays 9: these are additions, no existing entry point changed.
 *
 * COMPACTING A LIVE CORPUS: DROP THE DEAD ROWS, RENUMBER THE DOCUMENTS
 *
 * A corpus whose documents were removed (GDR_SIM_LIVE_MASK's bitmap marks the live rows) keeps paying for the dead rows in every
 * search.  The four calls below make "the matrix of the live rows, ids mapped" the corpus in place: a PLAN turns the bitmap into
 * the two id maps, the ROW MOVER compacts any row-major table through it, and two small calls renumber what holds document ids
 * (id lists, per-query row bitmaps).  No float atomics anywhere; every output is a function of the inputs alone.
 *
 * gdr_rows_compact_plan
 *   live_words: a bitmap in GDR_SIM_LIVE_MASK's format (bit r % 32 of int32 word r / 32 set = row r is live; ceil(N / 32) words are
 *     read, bits past N in the last word are ignored).
 *   out_new_id int32[N]: the new row of old row r, or -1 for a dead row.  out_old_id int32[n_live]: the live rows, ascending (may
 *     be NULL when n_live == 0).  The map is monotone: the live rows keep their order.
 *   n_live is the CALLER's count of live rows (ops.LiveRows.count is kept on the host): it sizes out_old_id, so nothing has to be
 *     read back.  out_status[0] = 0 on success, 1 when the bitmap's popcount is not n_live: nothing is then written past
 *     out_old_id[n_live) and the outputs are invalid.
 *   Limits: 1 <= N < 2^31, 0 <= n_live <= N.  Method: a wave per tile of 4096 rows popcounts it, ONE workgroup scans the tile counts
 *     (1024 tiles per step, any number of steps: any N), a wave per tile places its rows in ascending order, writing 256 contiguous
 *     bytes per instruction.  Three launches.  gdr_rows_compact_plan_workspace_bytes(N) = the tile offsets (0 for N outside the
 *     limits); a smaller workspace is GDR_ENOSPC before any launch.
 *
 * gdr_rows_compact
 *   dst row j = src row old_id[j] for j < n_live; rows >= n_live of dst are not written.  src / dst: N (resp. at least n_live) rows of
 *   row_bytes bytes, row-major, any element type; row_bytes % 4 == 0.  Lanes move 16 bytes each when row_bytes % 16 == 0 and both
 *   bases are 16-byte aligned, otherwise 4 bytes (the bases must be 4-byte aligned).  old_id is what the plan emits: strictly
 *   ascending, so old_id[j] >= j.  An id outside [0, N) moves nothing.
 *   dst != src: the regions must not overlap (an overlap of [src, src + N rows) with [dst, dst + n_live rows) is GDR_EINVAL); ONE
 *     gather launch; workspace may be NULL and chunk_rows is not used.
 *   dst == src: stable compaction in place with bounded extra memory.  The destination rows are taken in ascending chunks of
 *     chunk_rows; each chunk's sources are gathered into a bounce buffer in the workspace, and a second, stream-ordered launch copies
 *     the bounce buffer to the destination.  Why that is exact for every bitmap: a chunk's destination [j0, j1) can only overlap its
 *     OWN sources (old_id[j] >= j >= j0), which are already in the bounce buffer when it is written; it can never overlap a LATER
 *     chunk's sources, which are all >= j1.  The leading rows with old_id[j] == j are neither read nor written.
 *   chunk_rows == 0 selects the library default: as many rows as fit GDR_COMPACT_BOUNCE_BYTES = 64 MiB (at least one row) — a fixed
 *     size that does not depend on N.
 *   gdr_rows_compact_workspace_bytes(row_bytes, chunk_rows) = chunk_rows * row_bytes + 256 (the bounce buffer is aligned inside the
 *     workspace, which may start anywhere); with chunk_rows == 0: max(GDR_COMPACT_BOUNCE_BYTES, row_bytes) + 256.  Non-decreasing in
 *     row_bytes for a fixed chunk_rows and in chunk_rows >= 1; 0 for row_bytes <= 0 or chunk_rows < 0.  In place, a smaller
 *     workspace is GDR_ENOSPC before any launch.
 *
 * gdr_ids_remap
 *   out_ids[i] = new_id[ids[i]] for i < n.  A negative id stays as it is (the -1 padding of result lists).  An id >= N, or one whose
 *   row is dead (new_id = -1), becomes -1 and ORs 1 into out_status[0] (an integer atomic: order-free); the call clears that word
 *   first.  out_ids may alias ids exactly (each element is read and written by the same lane).
 *
 * gdr_rowmask_compact
 *   Remaps B per-query bitmaps (ops.QueryRows' format: bitmap q at words_in + q * in_stride_words, over N rows) through the
 *   compaction: bit j of output bitmap q = bit old_id[j] of input bitmap q (an id outside [0, N) reads as 0).  The bits past n_live
 *   in the last written word are 0; words past ceil(n_live / 32) of an output bitmap are not written.  A wave per 64 output rows:
 *   lane l tests its source bit, one ballot yields two output words.  Input and output must not overlap (GDR_EINVAL where the two
 *   ranges show it).  in_stride_words >= ceil(N / 32), out_stride_words >= ceil(n_live / 32).
 *
 * Measured on one MI355X at N = 320 000, d = 768 fp32 (983 MB; tools/bench_compact.py, profiles/r26_compact_bench.jsonl):
 *   the in-place move alone at 50 % dead, ms by MiB of bounce buffer, two runs: 16 -> 1.25 / 1.95, 32 -> 0.74 / 1.08, 64 -> 0.51 / 0.68,
 *     128 -> 0.43 / 0.52, 256 -> 0.41 / 0.45 (1 MiB: 9.1 / 14.4): 64 MiB is the last doubling that saves a third — the default;
 *   plan + in-place move: 1.23 ms with 10 % of the rows dead, 0.72 ms with 50 %, 0.22 ms with 90 %, 0.62 ms with one dead block of
 *     50 % (437 - 721 GB/s of rows moved; the traffic is four times that) against 0.48 / 0.35 / 0.23 / 0.36 ms for
 *     D[live].contiguous() plus a host remap of the CSR, which needs a second corpus of the live rows (844 / 469 / 93 / 469 MiB)
 *     where this needs 64 MiB: the in-place form is NOT faster, it is smaller;
 *   GDRRetriever.search, masked over N rows before -> over the compacted corpus after: 512 queries 2.14 -> 1.93 ms (10 % dead),
 *     2.21 -> 1.22 ms (50 %), 16.6 -> 0.42 ms (90 %: the masked search overflows and re-runs exhaustively); 32 queries 0.310 -> 0.302,
 *     0.309 -> 0.235, 1.79 -> 0.165 ms. */
#ifndef GDR_HIP_COMPACT_H
#define GDR_HIP_COMPACT_H

#include <stddef.h>
#include <stdint.h>

#define GDR_COMPACT_BOUNCE_BYTES 67108864 /* the bounce buffer of chunk_rows == 0: 64 MiB */

#ifdef __cplusplus
extern "C" {
#endif

size_t gdr_rows_compact_plan_workspace_bytes(int64_t N);
int gdr_rows_compact_plan(const int32_t* live_words, int64_t N, int64_t n_live, int32_t* out_new_id, int32_t* out_old_id,
                          int32_t* out_status, void* workspace, size_t workspace_bytes, void* stream);

size_t gdr_rows_compact_workspace_bytes(int64_t row_bytes, int64_t chunk_rows);
int gdr_rows_compact(const void* src, void* dst, int64_t N, int64_t row_bytes, const int32_t* old_id, int64_t n_live,
                     int64_t chunk_rows, void* workspace, size_t workspace_bytes, void* stream);

int gdr_ids_remap(const int32_t* new_id, int64_t N, const int32_t* ids, int32_t* out_ids, int64_t n, int32_t* out_status, void* stream);

int gdr_rowmask_compact(const int32_t* words_in, int64_t in_stride_words, int B, int64_t N, const int32_t* old_id, int64_t n_live,
                        int32_t* words_out, int64_t out_stride_words, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GDR_HIP_COMPACT_H */
