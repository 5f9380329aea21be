"""Numpy restatement of the k-means++ seeding of gdr_amd.kmeans.build_docids(init="k-means++") (DESIGN.md §9a;
include/gdr_hip_kmeans_seed.h) — sklearn's greedy k-means++ rule (T = 2 + floor(ln k) candidates per step, the one with the smallest
potential kept), made deterministic and order-free: fp32 distances over one pinned summation tree, integer weights, potentials and
prefix sums, draws from the integer hash of tests/kmeans_ref.py.  The device agrees with it bit for bit on every input; Lloyd from
the seeds is tests/kmeans_ref.py's.  No sklearn, no torch.
"""
import math

import numpy as np

import kmeans_ref as kr

W_BITS = 22
W_MAX = float((1 << W_BITS) - 1)


def n_trials(k):
    """Candidates per greedy step: sklearn's 2 + int(log(k))."""
    return 2 + int(math.floor(math.log(k)))


def dist2(X, c):
    """fp32 squared distances of the rows X fp32[m, d] to c fp32[d], every operation rounded on its own, over the pinned tree:
    partial sum l of 16 takes the 4-column pieces l, l + 16, ... in order (columns in order inside a piece), then the halving adds
    8, 4, 2, 1 (s[l] = s[l] + s[l + h]).  Zero padding to a multiple of 64 columns adds +0 terms: the bits do not change."""
    X = np.asarray(X, np.float32)
    c = np.asarray(c, np.float32)
    m, d = X.shape
    P = -(-d // 64)
    Xp = np.zeros((m, P * 64), np.float32)
    cp = np.zeros((P * 64,), np.float32)
    Xp[:, :d], cp[:d] = X, c
    Xp, cp = Xp.reshape(m, P, 16, 4), cp.reshape(P, 16, 4)
    acc = np.zeros((m, 16), np.float32)
    for p in range(P):
        for j in range(4):
            t = Xp[:, p, :, j] - cp[p, :, j]
            acc = acc + t * t
    for h in (8, 4, 2, 1):
        acc = acc[:, :h] + acc[:, h:2 * h]
    assert acc.dtype == np.float32
    return acc[:, 0]


def exponent(dmax):
    """e with dmax < 2^e: frexp's exponent (0 for dmax = 0)."""
    return int(np.frexp(np.float32(dmax))[1])


def weights(v, e):
    """floor(min(v * 2^(22 - e), 2^22 - 1)) as int64: exact integers < 2^22 for 0 <= v < 2^e; a larger v (+inf) saturates."""
    s = np.ldexp(np.asarray(v, np.float32).astype(np.float64), W_BITS - int(e))
    return np.floor(np.minimum(s, W_MAX)).astype(np.int64)


def draw(seed, restart, level, first_id, step, trial):
    """53-bit integer of (node, step, trial): splitmix64(splitmix64(prefix(seed, restart, level) ^ the node's smallest doc id) ^
    (step << 8 | trial)) >> 11 — it does not depend on which other nodes share the level."""
    a = kr.splitmix64(kr.mix_prefix(seed, restart, level) ^ int(first_id))
    return kr.splitmix64(a ^ ((int(step) << 8) | int(trial))) >> 11


def threshold(u, pot):
    """floor(u * 2^-53 * pot) (one float64 multiplication rounds), kept below pot."""
    return min(int(np.floor((np.float64(u) * 2.0 ** -53) * np.float64(pot))), int(pot) - 1)


def step_columns(X, ids, cand_ids, d2, e):
    """One greedy step of a node as gdr_kmeans_seed_dist forms it: (cand_d2 fp32[m, T], potentials int64[T], maxima fp32[T]).
    A negative candidate leaves d2 in its column; an id outside the corpus (row or candidate) reads as a zero row."""
    X = np.asarray(X, np.float32)
    N, d = X.shape
    ids = np.asarray(ids, np.int64)
    ok = (ids >= 0) & (ids < N)
    Xn = np.where(ok[:, None], X[np.where(ok, ids, 0)], np.float32(0))
    cols = []
    for cid in cand_ids:
        if cid < 0:
            cols.append(np.asarray(d2, np.float32).copy())
            continue
        c = X[cid] if cid < N else np.zeros(d, np.float32)
        cols.append(np.minimum(np.asarray(d2, np.float32), dist2(Xn, c)))
    cd = np.stack(cols, 1)
    pots = np.array([weights(cd[:, t], e).sum() for t in range(cd.shape[1])], np.int64)
    return cd, pots, cd.max(0)


def seed_node(X, ids, k, seed, restart, level, trace=None):
    """Doc ids of the k initial centres of one node (ids ascending).  m <= k: the hashed rule (kmeans_ref.init_rows).  Otherwise
    the first centre is the member with the smallest key; step j = 1 .. k - 1 draws T candidates (the first position whose inclusive
    prefix sum of the integer weights exceeds the threshold) and keeps the one with the smallest potential (ties to the lower
    trial); a node whose potential is 0 takes centre j from the hashed (key, id) order.  trace (a list) receives per step
    (potential before the step, candidate ids, candidate potentials, chosen id)."""
    X = np.asarray(X, np.float32)
    ids = np.asarray(ids, np.int64)
    m = len(ids)
    hashed = kr.init_rows(ids, k, seed, restart, level)
    if m <= k:
        return hashed
    T = n_trials(k)
    Xn = X[ids]
    chosen = [int(hashed[0])]
    d2 = dist2(Xn, X[chosen[0]])
    for step in range(1, k):
        e = exponent(d2.max())
        cs = np.cumsum(weights(d2, e))
        pot = int(cs[-1])
        if pot == 0:
            chosen.append(int(hashed[step]))
            if trace is not None:
                trace.append((0, [], [], chosen[-1]))
            continue
        pos = [int(np.searchsorted(cs, threshold(draw(seed, restart, level, ids[0], step, t), pot), side="right")) for t in range(T)]
        cd, pots, _mx = step_columns(X, ids, ids[pos], d2, e)
        b = int(np.argmin(pots))                                  # the first minimum: ties to the lower trial
        chosen.append(int(ids[pos[b]]))
        d2 = cd[:, b]
        if trace is not None:
            trace.append((pot, ids[pos].tolist(), pots.tolist(), chosen[-1]))
    return np.array(chosen, np.int64)


def seed_level(X, rows, node_offsets, k, seed, restart, level):
    """The seeds of every node of a level, int64[S, k]: each node by itself."""
    return np.stack([seed_node(X, rows[node_offsets[s]:node_offsets[s + 1]], k, seed, restart, level)
                     for s in range(len(node_offsets) - 1)])


def split_node(X, ids, k, seed, level, max_iter, n_init, init_centroids=None, on_round=None, on_restart=None, trace=None):
    """kmeans_ref.split_node with k-means++ seeds: the restart with the smallest inertia (ties to the lower restart), then rule 6."""
    Xn = np.asarray(X[ids], np.float64)
    best = None
    for r in range(1 if init_centroids is not None else n_init):
        tr = [] if trace is not None else None
        C0 = init_centroids if init_centroids is not None else np.asarray(X[seed_node(X, ids, k, seed, r, level, tr)], np.float64)
        if trace is not None:
            trace.append((level, int(ids[0]), r, tr))
        lab, _C, inertia, _rounds = kr.lloyd(Xn, C0, max_iter, (lambda t, g, l, r=r: on_round(r, t, g, l)) if on_round else None)
        if on_restart:
            on_restart(r, inertia)
        if best is None or inertia < best[1]:
            best = (lab, inertia)
    lab, inertia = best
    if len(ids) > 1 and (lab == lab[0]).all():
        lab = np.arange(len(ids)) % k
    return lab, inertia


def build(X, k, c, seed=7, max_iter=300, n_init=1, max_depth=None, init_centroids=None, on_round=None, on_restart=None, stats=None,
          trace=None):
    """kmeans_ref.build with k-means++ seeds.  trace (a list) receives (level, the node's smallest doc id, restart, the steps of
    seed_node) for every seeded split, in depth-first order."""
    X = np.asarray(X)
    total = [0.0]

    def split_labels(ids, level, path):
        lab, inertia = split_node(
            X, ids, k, seed, level, max_iter, n_init, init_centroids if level == 0 else None,
            (lambda r, t, g, l: on_round(path, r, t, g, l)) if on_round else None,
            (lambda r, i: on_restart(path, r, i)) if on_restart else None, trace)
        total[0] += inertia
        return lab

    out = kr.assemble_ids(X.shape[0], k, c, split_labels, max_depth)
    if stats is not None:
        stats["inertia"] = total[0]
    return out
