"""Inputs and expected lists for the width sweep of the similarity top-k (tests/test_sim_widths_host.py checks them on the host,
tests/test_gpu_sim_widths.py runs them): gdr_sim_topk, gdr_sim_topk_bf16 and gdr_sim_topk_prefilter take any width d with d % 4 == 0
(fp32) or d % 8 == 0 (bf16, pre-filter), and six contraction paths with width code of their own stand behind that.  No test lives here.

EXACT inputs (the idiom of tests/test_gpu_sim_deep_k.py, with a range that follows the width): Q and D hold integers drawn
uniformly from [-R, R], R = min(127, floor(sqrt(2^23 / d))).  Then d R^2 <= 2^23: every product and every partial sum is an integer
below 2^24, every fp32 score is exact in any summation order, every component (|x| <= 127 < 2^8) is exact in bf16 — so the fp32
paths, the bf16 paths and the pre-filter all owe ONE list, np.lexsort((ids, -scores))[:k] on the integer scores, compared with
torch.equal.  The range is wide on purpose: at d = 4 the scores still spread over +-64 516, so ties at the cut stay rare and no
candidate list overflows (shown from the inputs alone by the host test, with plan() below).

Ties are planted, so that the rule "higher score, then lower id" decides some rank of every list: query 0 is the row of the largest
norm among the first 100 rows, and that row has a copy 50 rows on (no other of those rows can reach its score: Cauchy-Schwarz), so
query 0 has a tie at ranks 0 / 1 of both one-pass shapes; its best row over the whole corpus has a copy 10 007 rows on.

FLOAT inputs: rows of unit norm whose first and last 16-byte pieces together carry half of the squared norm, so that a dropped or
doubled end piece moves a score by tenths, not by 1e-3."""
import functools
import math

import numpy as np
import torch

B_MAX = 129
N_BIG, K_BIG = 20_001, 10                       # the two-pass plan: 157 row tiles, the last one holds 33 rows
ONE_PASS = ((130, 130), (100, 7))               # k == N with two rows in the second tile; less than one tile
SHAPES = ((N_BIG, K_BIG),) + ONE_PASS
TILE = 128

F32_TILED = (4, 8, 28, 32, 36, 60, 64, 100, 132, 1028)
F32_STREAM = tuple(range(128, 1025, 128))       # B <= 32: the fp32 stream kernels (ring over d / 32 groups)
BF16_GENERIC = (8, 24, 40, 72, 136, 1032)       # d % 64 != 0: the generic core
BF16_GLDS = (64, 192, 320, 1088)                # d % 64 == 0: the LDS-DMA core
BF16_STREAM = tuple(range(256, 2049, 256))      # B <= 32: the bf16 stream kernels (ring over d / 64 groups); the LDS-DMA core above
PREFILTER = (8, 40, 72, 256, 264, 520, 1016, 1024)
PREFILTER_B = (7, 40)
PREFILTER_K100 = (264, 1016)
DEEP_WIDTHS = {"fp32": (36, 896), "bf16": (1032, 2048)}     # k = 1 and k = 100 run here only
EXTRA_WIDTH = {"fp32": 36, "bf16": 72}                      # the idx_offset and the SIM_EXHAUSTIVE call
FLOAT_WIDTHS = {"fp32": (36, 896, 1028), "bf16": (72, 1792, 2048), "prefilter": (264, 1016)}
FLOAT_B = (7, 40)
RERANK_WIDTHS = (4, 36, 260, 1028)


def widths(corpus):
    return F32_TILED + F32_STREAM if corpus == "fp32" else BF16_GENERIC + BF16_GLDS + BF16_STREAM


def stream_eligible(corpus, d):
    """csrc/sim_stream.hip sim_stream_supported, for B <= 32"""
    return (d % 128 == 0 and d <= 1024) if corpus == "fp32" else (d % 256 == 0 and d <= 2048)


def batches(corpus, d):
    """(B, with SIM_NO_STREAM) of the calls at width d: the latency mode with and without its stream kernels, then the tiled core at
    one below, at and one past its 128-query column tile; a width the stream kernels do not take runs B = 7 and B = 129 only."""
    if stream_eligible(corpus, d):
        return [(b, ns) for b in (1, 7, 32) for ns in (False, True)] + [(33, False), (128, False), (129, False)]
    return [(7, False), (129, False)]


def radius(d):
    return min(127, math.isqrt(2 ** 23 // d))


@functools.lru_cache(maxsize=2)
def ints(d):
    """(Q fp32 [B_MAX, d], D fp32 [N_BIG, d]) of integers in [-radius(d), radius(d)], ties planted (module docstring)."""
    R = radius(d)
    g = np.random.default_rng(1000 + d)
    Q = g.integers(-R, R + 1, size=(B_MAX, d)).astype(np.float32)
    D = g.integers(-R, R + 1, size=(N_BIG, d)).astype(np.float32)
    a = int(np.argmax((D[:100].astype(np.int64) ** 2).sum(1)))
    D[(a + 50) % 100] = D[a]
    Q[0] = D[a]
    best = int(np.argmax(D.astype(np.float64) @ Q[0].astype(np.float64)))
    D[100 + (best + 10_007) % (N_BIG - 100)] = D[best]
    return Q, D


@functools.lru_cache(maxsize=2)
def int_scores(d):
    """int64 [B_MAX, N_BIG].  The float64 product is exact (integers below 2^24 < 2^53 at every step), so its cast is the integer product."""
    Q, D = ints(d)
    return np.rint(Q.astype(np.float64) @ D.astype(np.float64).T).astype(np.int64)


def topk_by_rule(s, k):
    """s: integer scores int64 [B, N], |s| < 2^24, N < 2^15.  (values int64 [B, k], ids int64 [B, k]): higher score, then lower id —
    np.lexsort((ids, -s[q]))[:k] for every q, through one key  -s * 2^15 + id  (the host test holds it against the lexsort)."""
    B, N = s.shape
    assert N < 2 ** 15 and np.abs(s).max() < 2 ** 24
    key = -s * 2 ** 15 + np.arange(N, dtype=np.int64)[None, :]
    if k < N:
        part = np.argpartition(key, k - 1, axis=1)[:, :k]
    else:
        part = np.tile(np.arange(N), (B, 1))
    order = np.take_along_axis(part, np.argsort(np.take_along_axis(key, part, 1), axis=1), 1)
    return np.take_along_axis(s, order, 1), order


@functools.lru_cache(maxsize=None)
def expected(d, N, k):
    """(values fp32 [B_MAX, k], ids int32 [B_MAX, k]) over the first N rows of ints(d)[1], as torch tensors.  Left unchanged by the tests."""
    v, i = topk_by_rule(int_scores(d)[:, :N], k)
    return torch.from_numpy(v.astype(np.float32)), torch.from_numpy(i.astype(np.int32))


def plan(N, k, exhaustive=False, survivors=1.0):
    """What one gdr_sim_topk call of depth k lays out (include/gdr_hip.h at gdr_sim_topk_workspace_bytes; csrc/sim_topk.hip make_plan):
    (sample stride in tiles of 128 rows, sample slots, list capacity per query).  A corpus of at most 16 384 rows, or of fewer than four
    sample blocks, or a SIM_EXHAUSTIVE call, is its own sample (stride 1).  Otherwise about sqrt(k N) rows are sampled, and the list holds
    the sample block, 4 x the k N / n_sample survivors expected (x `survivors`: the pre-filter's wider cut), and 4096.
    N = 20 001, k = 10: (39, 640, 6016).  The one restatement of the rule in the tests: the search suites import it."""
    tiles = -(-N // TILE)
    ts = max(1, int((max(math.sqrt(float(k) * float(N)), float(k)) + TILE - 1) / TILE))
    if exhaustive or N <= 16384 or tiles < 4 * ts:
        n = tiles * TILE
        return 1, n, n
    stride = tiles // ts
    slots = -(-tiles // stride) * TILE
    cap = slots + int(4.0 * (float(k) * float(N) / float(slots)) * survivors) + 4096
    return stride, slots, -(-cap // TILE) * TILE


def in_sample_tile(N, stride):
    """bool [N]: row r sits in a sample tile (tile index % stride == 0)"""
    return (np.arange(N) // TILE) % stride == 0


def sample_rows(N, stride):
    """the rows of the tiles t with t % stride == 0"""
    return np.nonzero(in_sample_tile(N, stride))[0]


def survivors(s, N, k):
    """per query of s [B, N]: how many rows score at least the k-th best SAMPLED row (every entry a call can append to the list)"""
    stride, _, _ = plan(N, k)
    thr = np.sort(s[:, sample_rows(N, stride)], axis=1)[:, -k]
    return (s >= thr[:, None]).sum(1), thr


def prefilter_eps2(Q, D):
    """2 eps_q of include/gdr_hip.h at gdr_sim_topk_prefilter, float64 [B], with the 2 % of slack the kernel adds (csrc/sim_topk.hip
    sim_qprep_kernel: 1.01, 1.0001 and the 1e-6 of ops.PrefilteredCorpus)"""
    d = Q.shape[1]
    nq = np.linalg.norm(Q.astype(np.float64), axis=1)
    return 2.0 * nq * np.linalg.norm(D.astype(np.float64), axis=1).max() * (2.0 ** -7 + 2.0 ** -16 + d * 2.0 ** -22) * 1.02


# ---- float inputs -----------------------------------------------------------------------------------------------------------------
FLOAT_N, FLOAT_K = N_BIG, K_BIG


def end_weighted(n, d, piece, seed):
    """fp32 [n, d], rows of unit norm: the first `piece` and the last `piece` columns carry a quarter of the squared norm each, the
    columns between them the other half.  piece: the elements of 16 bytes (4 fp32, 8 bf16)."""
    g = np.random.default_rng(seed)
    x = g.standard_normal((n, d))
    if d <= 2 * piece:                            # no middle (the rerank's d = 4): plain unit rows
        return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    for lo, hi, w in ((0, piece, 0.25), (piece, d - piece, 0.5), (d - piece, d, 0.25)):
        x[:, lo:hi] *= np.sqrt(w) / np.linalg.norm(x[:, lo:hi], axis=1, keepdims=True)
    return x.astype(np.float32)


@functools.lru_cache(maxsize=2)
def floats(kind, d):
    """(Q fp32 [40, d], D fp32 [FLOAT_N, d]); kind: "fp32", "bf16" or "prefilter" (fp32 rows, fp32 pieces)"""
    piece = 8 if kind == "bf16" else 4
    return end_weighted(max(FLOAT_B), d, piece, 7000 + d), end_weighted(FLOAT_N, d, piece, 8000 + d)


def float_reference(kind, d):
    """(Q64, D64, scores float64 [40, N]): the operands the kernels multiply — bf16-rounded for a bf16 corpus (the device rounds the
    queries too) — and their float64 product"""
    Q, D = floats(kind, d)
    if kind == "bf16":
        Q64, D64 = torch.from_numpy(Q).bfloat16().double().numpy(), torch.from_numpy(D).bfloat16().double().numpy()
    else:
        Q64, D64 = Q.astype(np.float64), D.astype(np.float64)
    return Q64, D64, Q64 @ D64.T


def float_tolerance(kind, d, Q64, D64):
    """The larger of the project's tolerance (1e-4 for fp32 scores, 1e-5 for bf16 operands against the rounded operands: products of
    bf16 values are exact in fp32, only the sum rounds) and the a-priori band of an fp32 sum of d products in any order,
    (2 d + 8) 2^-24 max|q| max|d|.  From the inputs alone."""
    band = (2 * d + 8) * 2.0 ** -24 * np.linalg.norm(Q64, axis=1).max() * np.linalg.norm(D64, axis=1).max()
    return max(1e-5 if kind == "bf16" else 1e-4, band), band


def float_topk(s, k):
    """float64 scores [B, N] -> (values [B, k], ids [B, k]), descending, lower id first among equals"""
    order = np.stack([np.lexsort((np.arange(s.shape[1]), -s[q]))[:k] for q in range(s.shape[0])])
    return np.take_along_axis(s, order, 1), order


# ---- rerank -----------------------------------------------------------------------------------------------------------------------
def rerank_case(d, seed=5):
    """B = 3 queries, R = 4 clusters of 5 to 40 candidates each, in the one-CSR layout; rows and queries end-weighted as above (queries
    scaled to 0.9: scores inside +-0.9, away from the saturation of tanh)."""
    B, R, N = 3, 4, 2_000
    g = np.random.default_rng(seed + d)
    D = end_weighted(N, d, 4, 9000 + d)
    Q = end_weighted(B, d, 4, 9500 + d) * np.float32(0.9)
    sizes = g.integers(5, 41, size=(B, R))
    sizes[0, 0], sizes[B - 1, R - 1] = 5, 40
    mem = [g.choice(N, size=int(sizes[b].sum()), replace=False).astype(np.int64).tolist() for b in range(B)]
    offsets = np.concatenate([[0], np.cumsum(sizes.reshape(-1))]).astype(np.int32)
    ids = np.concatenate([np.asarray(m) for m in mem]).astype(np.int32)
    beam = np.sort(g.standard_normal((B, R)).astype(np.float32) - 6, axis=1)[:, ::-1].copy()
    return dict(B=B, R=R, Q=Q, D=D, sizes=sizes, mem=mem, offsets=offsets, ids=ids, beam=beam, alphas=[0.0, 1.0], k=10)
