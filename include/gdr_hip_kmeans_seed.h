/* gdr_hip_kmeans_seed.h — part of the C ABI of libgdr_hip.so; include/gdr_hip.h includes it, so `#include "gdr_hip.h"` declares
 * everything below.  The conventions (return codes, streams, gdr_last_error) are gdr_hip.h's: every pointer is a device pointer,
 * the library allocates nothing, the calls are stream-ordered with no host synchronisation and capturable.  gdr_abi_version()
 * stays 9: these are additions, no existing entry point changed.
 *
 * K-MEANS++ SEEDING OF THE HIERARCHICAL DOCID BUILD: ONE GREEDY STEP OVER EVERY NODE OF A LEVEL
 *
 * gdr_amd.kmeans.build_docids(init="k-means++") seeds every split with sklearn's greedy k-means++ rule (T = 2 + floor(ln k)
 * candidates per step drawn in proportion to the squared distance to the nearest chosen centre, the one with the smallest potential
 * kept), made deterministic and order-free (tests/kmeans_pp_ref.py restates it in numpy): distances are fp32 with a
 * pinned summation tree, potentials and prefix sums are integers.  The draws, the prefix sums and the argmin stay with the caller;
 * this call is the pass over the rows.
 *
 * The level is gdr_kmeans_assign's: rows int32[n_rows] (doc ids, ascending inside a node), node_offsets int32[n_nodes + 1], and a
 * work list int32[n_work, 2] of (node, first row position) for every tile of gdr_kmeans_seed_tile() = 128 row positions.
 *
 * gdr_kmeans_seed_dist
 *   cand int32[n_nodes, n_trials]: the candidate doc ids of every node; a negative id means "no candidate".
 *   d2 fp32[n_rows]: every row's squared distance to its nearest chosen centre (+inf before the first centre).
 *   e int32[n_nodes]: the node's exponent, with every d2 of the node < 2^e (frexp of the node's largest d2).
 *   out_cand_d2 fp32[n_rows, n_trials]: min(d2[p], dist2(row p, candidate t of p's node)); the column of a negative candidate is d2[p].
 *   out_pot int64[n_work, n_trials]: per tile, the sum over its rows of weight(out_cand_d2[p, t], e[node]).
 *   out_max fp32[n_work, n_trials]: per tile, the largest out_cand_d2[p, t] (0 if all are 0).
 *   out_status int32[1]: cleared first; bit 2 (value 2) when a work item names no node or a position outside its node — such an item
 *     reads and writes nothing else.
 *
 *   dist2(x, c) = sum_j (x_j - c_j)^2 in fp32, every subtraction, multiplication and addition rounded on its own (no fma; denormals
 *   are kept), over ONE summation tree: the row is cut into pieces of 4 columns; partial sum l (0 <= l < 16) starts at 0 and takes the
 *   pieces l, l + 16, l + 32, ... in order, inside a piece the columns in order (acc = acc + t * t, t = x_j - c_j); then
 *   s8[l] = p[l] + p[l + 8] (l < 8), s4[l] = s8[l] + s8[l + 4], s2[l] = s4[l] + s4[l + 2], dist2 = s2[0] + s2[1].  It is a function of
 *   the row and the candidate alone — not of the tile, the node set or the launch — is never negative, and is exactly 0 for the
 *   candidate itself and its duplicates.  A doc id outside [0, N) (row or non-negative candidate) reads as a zero row.
 *
 *   weight(v, e) = floor(min(v * 2^(22 - e), 2^22 - 1)): an exact integer < 2^22 for 0 <= v < 2^e; a larger v (+inf included)
 *   saturates.  With n_rows < 2^31 every sum of weights is < 2^53: integer accumulation, the same in any order.
 *
 *   Limits: those of gdr_kmeans_assign (d % 4 == 0, d <= 4096, N and n_rows < 2^31) and 1 <= n_trials <= 6 (k <= 64).  D must be
 *   16-byte aligned.  gdr_kmeans_seed_workspace_bytes(...) is 0 today: the per-tile partials are outputs, reduced by the caller, so
 *   the step keeps no scratch (workspace may be NULL); the query exists so that a caller sizes this call like every other one.
 *   One launch, no atomics on data (the status word is an integer OR).  The pass reads the level's rows once: memory-bound. */
#ifndef GDR_HIP_KMEANS_SEED_H
#define GDR_HIP_KMEANS_SEED_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int gdr_kmeans_seed_tile(void);
size_t gdr_kmeans_seed_workspace_bytes(int n_nodes, int n_work, int n_trials);
int gdr_kmeans_seed_dist(const float* D, int64_t N, int d, const int32_t* rows, int64_t n_rows, const int32_t* node_offsets,
                         int n_nodes, const int32_t* work, int n_work, const int32_t* cand, int n_trials, const float* d2,
                         const int32_t* e, float* out_cand_d2, int64_t* out_pot, float* out_max, int32_t* out_status,
                         void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GDR_HIP_KMEANS_SEED_H */
