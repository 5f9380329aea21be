"""Host restatement (numpy) of corpus expansion — the reference's tree_embedding_calculate + tree_embedding_insert
(main_models.py:154-179, 268-295) with the rules of DESIGN.md §8: what tests/test_expand_host.py checks against the reference's
golden (g14) and tests/test_gpu_expand.py checks the device kernels against at scale."""
import numpy as np


def centroids(D, offsets, members):
    """(fp32[C, d], int32[C]): every cluster's members in ascending order, added one after another in fp32 starting from 0
    (Python's sum), then one fp32 division by the count.  An empty cluster: a zero row, count 0."""
    D = np.asarray(D, dtype=np.float32)
    C = len(offsets) - 1
    cent = np.zeros((C, D.shape[1]), np.float32)
    counts = np.diff(np.asarray(offsets)).astype(np.int32)
    for c in range(C):
        mem = np.sort(np.asarray(members[offsets[c]:offsets[c + 1]], dtype=np.int64))
        if mem.size == 0:
            continue
        acc = np.zeros(D.shape[1], np.float32)
        for m in mem:
            acc = acc + D[m]
        cent[c] = acc / np.float32(mem.size)
    return cent, counts


def assign(X, cent, counts, chunk=2048, choice=None):
    """(cluster int32[n], fp64 top-2 gap [n], fp64 error band [n]): the argmax of the fp64 scores over the non-empty
    clusters, ties to the lower index.  The band 2·d·2^-24·|x|·max|c| bounds the difference between an fp32 dot product and the
    exact one, so a device choice whose fp64 score lies within it of the maximum is a correct fp32 argmax.
    choice (cluster indices [n], optional): also returns, per row, whether that choice is non-empty and lies within the band.
    Rows are scored `chunk` at a time (one [chunk, C] fp64 block, top-2 by partition)."""
    X = np.asarray(X)
    live = np.nonzero(np.asarray(counts) > 0)[0]
    C = np.asarray(cent, np.float64)[live]
    pos = np.full(len(counts), -1, np.int64)
    pos[live] = np.arange(live.size)
    n, d = X.shape
    best = np.empty(n, np.int64)
    gap = np.full(n, np.inf)
    ok = np.empty(n, bool)
    band = 2 * d * 2.0 ** -24 * np.linalg.norm(np.asarray(X, np.float64), axis=1) * np.linalg.norm(C, axis=1).max()
    for lo in range(0, n, chunk):
        s = np.asarray(X[lo:lo + chunk], np.float64) @ C.T
        r = np.arange(s.shape[0])
        best[lo:lo + chunk] = np.argmax(s, axis=1)
        top = s[r, best[lo:lo + chunk]]
        if live.size > 1:
            t2 = np.partition(s, -2, axis=1)
            gap[lo:lo + chunk] = t2[:, -1] - t2[:, -2]
        if choice is not None:
            p = pos[np.asarray(choice[lo:lo + chunk], np.int64)]
            ok[lo:lo + chunk] = (p >= 0) & (s[r, np.maximum(p, 0)] >= top - band[lo:lo + chunk])
    out = (live[best].astype(np.int32), gap, band)
    return out + (ok,) if choice is not None else out


def merge(offsets, members, new_ids, targets):
    """(offsets int32[C+1], members int32[N+n]): every cluster keeps its members in order, followed by the ids it received in
    ascending order."""
    C = len(offsets) - 1
    new_ids = np.asarray(new_ids, np.int64)
    targets = np.asarray(targets, np.int64)
    order = np.lexsort((new_ids, targets))
    ids_s, tg_s = new_ids[order], targets[order]
    cut = np.searchsorted(tg_s, np.arange(C + 1))
    offs, mem = [0], []
    for c in range(C):
        seg = list(members[offsets[c]:offsets[c + 1]]) + list(ids_s[cut[c]:cut[c + 1]])
        mem.extend(seg)
        offs.append(offs[-1] + len(seg))
    return np.asarray(offs, np.int32), np.asarray(mem, np.int32)


def as_sets(offsets, members):
    return [frozenset(int(x) for x in members[offsets[c]:offsets[c + 1]]) for c in range(len(offsets) - 1)]


def pairwise_sum(rows):
    """A pairwise (tree) fp32 sum of the rows — what a reduction that ignores the member order would compute."""
    rows = list(rows)
    while len(rows) > 1:
        rows = [rows[i] + rows[i + 1] if i + 1 < len(rows) else rows[i] for i in range(0, len(rows), 2)]
    return rows[0]
