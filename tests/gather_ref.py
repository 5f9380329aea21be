"""Host restatement (numpy) of gdr_sim_topk's gather mode (GDR_SIM_ROW_GATHER): a query's bitmap gives its allowed
row ids in ascending order, cut at the capacity; the list is live_ref.topk over exactly those rows."""
import numpy as np

import live_ref

CHUNK = 4096


def cap_of(chunks):
    """Rows per query for the chunk field c: 4096 c, 0 reads as 2."""
    return CHUNK * (chunks if chunks else 2)


def rows_of(words, N, cap):
    """(ascending allowed row ids cut at cap, how many rows the bitmap allows): words int32 [>= ceil(N / 32)], bits past N ignored."""
    w = np.asarray(words).view(np.uint32)[:(N + 31) // 32]
    bits = ((w[:, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool).reshape(-1)[:N]
    rows = np.nonzero(bits)[0]
    return rows[:cap], int(rows.size)


def topk(S, allowed, k, cap, idx_offset=0):
    """S: fp64 scores [B, N]; allowed: bool [B, N].  (values fp64 [B, k], ids int64 [B, k], status int [B])."""
    S = np.asarray(S, np.float64)
    B, N = S.shape
    vals, ids, status = np.full((B, k), -np.inf), np.full((B, k), -1, np.int64), np.zeros(B, np.int64)
    for q in range(B):
        rows, count = rows_of(live_ref.pack(allowed[q]), N, cap)
        keep = np.zeros(N, bool)
        keep[rows] = True
        v, i = live_ref.topk(S[q:q + 1], keep, k, idx_offset)
        vals[q], ids[q], status[q] = v[0], i[0], int(count > cap)
    return vals, ids, status
