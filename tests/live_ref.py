"""Host restatement (numpy) of the corpus search over live rows: what tests/test_live_search_host.py checks
against hand-written cases and tests/test_gpu_live_search.py checks gdr_sim_topk's GDR_SIM_LIVE_MASK mode against."""
import numpy as np


def pack(live):
    """bool [n] -> int32 [ceil(n / 32)]: bit r % 32 of word r // 32 is row r."""
    live = np.asarray(live, dtype=bool).reshape(-1)
    bits = np.zeros(-(-live.size // 32) * 32, dtype=np.uint32)
    bits[:live.size] = live
    return (bits.reshape(-1, 32) << np.arange(32, dtype=np.uint32)).sum(1, dtype=np.uint64).astype(np.uint32).view(np.int32)


def mask_bytes(N):
    """Bytes of one row bitmap at the head of a masked call's workspace (csrc/sim_topk.hip live_mask_bytes): its words, up to 256."""
    return (4 * ((N + 31) // 32) + 255) // 256 * 256


class FixedWorkspace:
    """An ops.Workspace stand-in that hands out one buffer of a fixed size: what a captured graph needs (no allocation on replay)."""

    def __init__(self, buf):
        self.buf = buf

    def get(self, nbytes):
        assert nbytes <= self.buf.numel()
        return self.buf


def scores(Q, D):
    """fp64 scores [B, N] of the operands as given (a bf16 corpus is passed in already rounded)."""
    return np.asarray(Q, np.float64) @ np.asarray(D, np.float64).T


def topk(S, live, k, idx_offset=0):
    """(values fp64 [B, k], ids int64 [B, k]): per row of the score matrix S the k best LIVE columns, higher score first, then
    the lower id; where fewer than k columns are live the tail is -inf / -1."""
    S = np.asarray(S, np.float64)
    rows = np.nonzero(np.asarray(live, dtype=bool).reshape(-1))[0]
    B = S.shape[0]
    vals = np.full((B, k), -np.inf)
    ids = np.full((B, k), -1, dtype=np.int64)
    for b in range(B):
        s = S[b, rows]
        order = np.lexsort((rows, -s))[:k]                          # last key first: score descending, then id ascending
        vals[b, :order.size] = s[order]
        ids[b, :order.size] = rows[order] + idx_offset
    return vals, ids
